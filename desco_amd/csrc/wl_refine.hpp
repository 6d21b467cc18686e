// The hash chain of the colour refinement, for both sides of the compiler: the gfx950 kernel (wl_refine_dev.hip) and the
// host twin (wl_refine.cpp).  Definitions: include/desco_hip.h, "COLOUR REFINEMENT".  Everything is uint64 arithmetic
// with wrap-around, so the two sides agree bit for bit whatever order they add in.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DESCO_WL_HD __host__ __device__ __forceinline__
#define DESCO_WL_UNROLL _Pragma("unroll")
#else
#define DESCO_WL_HD inline
#define DESCO_WL_UNROLL
#endif

namespace desco {
namespace wl {

constexpr uint64_t kG = 0x9E3779B97F4A7C15ull;
constexpr int kMaxSlots = 4;

DESCO_WL_HD uint64_t mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// what a row sends to its readers and to the segment's pool
DESCO_WL_HD uint64_t message(uint64_t colour) { return mix(colour + kG); }

// the new colour of a row of colour c whose SLOT sums are ms[0 .. slots): the slots are pooled by group first
DESCO_WL_HD uint64_t update(uint64_t c, const uint64_t* ms, const int* group, int slots) {
  uint64_t h = mix(c + kG);
DESCO_WL_UNROLL
  for (int g = 0; g < kMaxSlots; ++g) {
    if (g >= slots) break;
    uint64_t m = 0;
DESCO_WL_UNROLL
    for (int s = 0; s < kMaxSlots; ++s)
      if (s < slots && group[s] == g) m += ms[s];
    h = mix(h ^ (m + (uint64_t)(g + 1) * kG));
  }
  return h;
}

DESCO_WL_HD uint64_t signature(bool anchored, uint64_t anchor_colour, uint64_t pool) {
  return anchored ? mix(mix(anchor_colour + kG) ^ (pool + kG)) : mix(pool + kG);
}

}  // namespace wl
}  // namespace desco
