// The decision chain of the sampled counts (RAND-ESU), for both sides of the compiler: the gfx950 kernel
// (sampled_counts_dev.hip) and the host twin (sampled_counts.cpp).  Definitions: include/desco_hip.h, "SAMPLED COUNTS".
//
// Whether u is kept as node number d (1-based; d = 2 .. kmax) of the sequence (s_0 .. s_{d-2}, u) is a function of
// (seed, replica index, graph index, s_0 .. s_{d-2}, u) alone:
//   h_1 = w0 | w1 << 32,  w = Philox4x32-10(counter = {s_0, lo32(graph), lo32(replica), kTag}, key = seed)
//   h_d = mix(h_{d-1} ^ (uint64(u + 1) * G))                       (mix and G of wl_refine.hpp)
//   keep iff (h_d >> 32) < thr[d],  thr[d] in 0 .. 2^32 (2^32: always)
// Everything is integer arithmetic with wrap-around, so the two sides agree bit for bit.
#pragma once
#include <stdint.h>

#include "null_model.hpp"
#include "wl_refine.hpp"

namespace desco {
namespace sampled {

constexpr uint32_t kTag = 0x53414D50u;               // "SAMP": keeps the counters apart from the null model's
constexpr uint64_t kAlways = (uint64_t)1 << 32;      // the threshold of probability 1
constexpr int kKmaxHost = 6;

// h_1 of the root s0 (local id) of graph `graph` in replica `replica` (both already offset by their bases)
DESCO_NM_HD uint64_t root_hash(uint64_t seed, uint32_t graph, uint32_t replica, uint32_t s0) {
  uint32_t c[4] = {s0, graph, replica, kTag};
  null_model::philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (uint64_t)c[0] | (uint64_t)c[1] << 32;
}

// h_d from h_{d-1} and the candidate u (local id)
DESCO_NM_HD uint64_t step(uint64_t h, int u) { return wl::mix(h ^ ((uint64_t)(uint32_t)(u + 1) * wl::kG)); }

DESCO_NM_HD bool keep(uint64_t h, uint64_t thr) { return (h >> 32) < thr; }

}  // namespace sampled
}  // namespace desco
