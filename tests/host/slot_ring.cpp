// tests/host/slot_ring.cpp -- the slot hand-out of concurrent batch calls (graphik_amd/csrc/gik_slots.h) without a
// device: 8 threads take and hand back the slots of a ring of 3, a few thousand rounds each, with a "previous launch
// has completed" answer that flips pseudo-randomly.  More threads than slots: the in_use / yield branch runs all
// the time.  Exits non-zero if a slot is ever held twice at once, if a take does not return (the driver's time limit),
// or if a slot handed back without a launch comes out pending.  tests/test_slot_ring.py runs it plain and under the
// thread sanitizer, which also checks that the slot fields are only touched by the owner or under the mutex.
#include "gik_slots.h"

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace {

constexpr int RING = 3, THREADS = 8, ROUNDS = 4000;

struct Slot {
  int done = 0;      // stands for the event: 0 until the first user "creates" it, then index + 1
  bool pending = false;
  bool in_use = false;
};

std::vector<Slot> g_slots(RING);
unsigned g_next = 0;
std::mutex g_mu;

// What the test knows next to the slots.  g_guarded / g_completed are touched like the slots themselves: by the
// owner, or under g_mu by the completion test (which take_slot calls under the lock).
std::atomic<int> g_holders[RING];
bool g_guarded[RING];      // a launch of this slot was handed back covered by an event that has not been seen complete
bool g_completed[RING];    // the completion test has just said yes for this slot
std::atomic<long> g_takes{0}, g_failures{0}, g_asked{0}, g_uncovered{0};

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "slot_ring: line %d: %s\n", __LINE__, #cond);   \
      ++g_failures;                                                        \
    }                                                                      \
  } while (0)

uint32_t next_random(uint32_t &s) {      // xorshift32
  s ^= s << 13;
  s ^= s >> 17;
  s ^= s << 5;
  return s;
}

uint32_t g_flip = 2463534242u;      // (under g_mu)
bool completed(int done) {
  const int i = done - 1;
  ++g_asked;
  CHECK(i >= 0 && i < RING && g_guarded[i]);      // only a pending slot is asked about, and pending means a covered launch
  const bool yes = next_random(g_flip) & 1;
  if (yes) g_completed[i] = true;
  return yes;
}

void worker(int id) {
  uint32_t rng = 88172645u + 7919u * (uint32_t)id;
  for (int round = 0; round < ROUNDS; ++round) {
    gik::SlotLease<Slot> lease(g_mu);
    Slot &s = lease.take(g_slots, g_next, (unsigned)RING, completed);
    ++g_takes;
    const int i = (int)(&s - g_slots.data());
    CHECK(g_holders[i].fetch_add(1) == 0);      // nobody else holds it
    CHECK(s.in_use);
    bool pending = s.pending;
    CHECK(!pending || g_guarded[i]);                           // pending only behind a launch that was covered by an event
    CHECK(!(g_guarded[i] && !pending) || g_completed[i]);      // ... and handed out as idle only once that launch had completed
    g_completed[i] = false;
    if (!s.done) s.done = i + 1;
    const uint32_t r = next_random(rng);
    if (pending && (r & 3) == 0) s.pending = pending = false;      // (the owner waited for the previous launch itself)
    g_guarded[i] = pending;
    if (r & 4) std::this_thread::yield();      // between hand-out and launch
    if ((r >> 3) % 3) {      // launched and recorded; else an error return: nothing new is pending
      lease.covered_by_event();
      g_guarded[i] = true;
    } else {
      ++g_uncovered;
    }
    CHECK(g_holders[i].fetch_sub(1) == 1);
  }
}

}  // namespace

int main() {
  std::vector<std::thread> threads;
  for (int id = 0; id < THREADS; ++id) threads.emplace_back(worker, id);
  for (std::thread &t : threads) t.join();
  CHECK(g_takes == (long)THREADS * ROUNDS);      // every take returned
  for (const Slot &s : g_slots) CHECK(!s.in_use && s.done);
  CHECK(g_asked > 0 && g_uncovered > 0);
  std::printf("slot_ring: %ld takes, %ld completion tests, %ld hand-backs without a launch, %ld failures\n", g_takes.load(),
              g_asked.load(), g_uncovered.load(), g_failures.load());
  return g_failures ? 1 : 0;
}
