// tests/host/walk_digest.h -- what the anch_*_walk programs print as "digest": a 64-bit FNV-1a over the bit patterns of
// every value of their random sweep, least significant byte first.  A NaN is hashed as one fixed word, not by its payload.
// The Python tests that run the walks hold the digests of the commit before the pair functions became one (c11b7a7).
#pragma once

#include <cstdint>
#include <cstring>

struct WalkDigest {
  uint64_t h = 0xcbf29ce484222325ull;
  void add(double x) {
    uint64_t w;
    std::memcpy(&w, &x, sizeof w);
    if (x != x) w = 0x7ff8000000000000ull;
    for (int i = 0; i < 8; ++i) h = (h ^ ((w >> (8 * i)) & 0xffu)) * 0x100000001b3ull;
  }
};
