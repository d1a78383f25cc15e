// graphik_amd/csrc/gik_slots.h -- hand-out of a handle's mutable slots to concurrent batch calls: the ring of
// work-queue counters and the pool of time-slicing workspaces (gik_template in gik_host.hip).  Plain C++17, no HIP:
// the "previous launch has completed" test is a callable, so tests/host/slot_ring.cpp runs the protocol without a device.
//
// A slot has `done` (the event recorded behind the launch that used it last; null until its first user creates it),
// `pending` (`done` may not have completed yet) and `in_use` (handed to a call that has not given it back).  The lock
// covers the hand-out and the hand-back only: waiting for a slot's previous user, growing its workspace and the launch
// happen outside it, on a slot marked in_use -- only its owner touches it.
#pragma once

#include <mutex>
#include <thread>

namespace gik {

// The slot used last if the launch that used it has completed -- a sequence of calls then keeps ONE workspace warm
// instead of growing all of the pool --, else the next one that no other call holds.  `completed(slot.done)` is asked
// under the lock, about a pending slot only.
template <typename Slots, typename Completed>
int take_slot(std::mutex &mu, Slots &slots, unsigned &next, unsigned n, Completed &&completed) {
  for (;;) {
    {
      std::lock_guard<std::mutex> lock(mu);
      const unsigned last = (next + n - 1) % n;
      auto &ls = slots[last];
      if (!ls.in_use && ls.done && (!ls.pending || completed(ls.done))) {
        ls.pending = false;
        ls.in_use = true;
        return (int)last;
      }
      for (unsigned k = 0; k < n; ++k) {
        const unsigned i = (next + k) % n;
        if (!slots[i].in_use) {
          slots[i].in_use = true;
          next = (i + 1) % n;
          return (int)i;
        }
      }
    }
    std::this_thread::yield();      // every slot is between hand-out and launch in some other thread
  }
}

// Holds a slot until the end of the call.  It goes back "pending" only if the caller says that a recorded event
// covers its launch; error paths hand it back too (no launch: nothing new is pending).
template <typename Slot>
class SlotLease {
 public:
  explicit SlotLease(std::mutex &mu) : mu_(mu) {}
  SlotLease(const SlotLease &) = delete;
  SlotLease &operator=(const SlotLease &) = delete;
  ~SlotLease() {
    if (!slot_) return;
    std::lock_guard<std::mutex> lock(mu_);
    slot_->in_use = false;
    if (covered_) slot_->pending = true;
  }
  template <typename Slots, typename Completed>
  Slot &take(Slots &slots, unsigned &next, unsigned n, Completed &&completed) {
    slot_ = &slots[take_slot(mu_, slots, next, n, completed)];
    return *slot_;
  }
  Slot *get() const { return slot_; }
  void covered_by_event() { covered_ = true; }

 private:
  std::mutex &mu_;
  Slot *slot_ = nullptr;
  bool covered_ = false;
};

}  // namespace gik
