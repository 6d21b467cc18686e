// The limits and device workspaces of the clique census, for both sides of the compiler: the gfx950 kernels and their
// entry points (clique_census_dev.hip), the host twin (clique_census.cpp) and any host code that sizes a launch.  The
// limits are DESCO_PEEL_DEV_MAX_WORDS, DESCO_CLIQUE_DEV_MAX_OUT and DESCO_CLIQUE_MAX_K (include/desco_hip.h, "CLIQUE
// CENSUS"); the host twins have none but the last.
//
// The peel kernel keeps one graph of n nodes and m undirected edges in LDS, in 32-bit words:
//   control  3        flag and minimum of a pass (one spare)
//   rowptr   n + 1    local CSR offsets
//   entry    2 m      one word per CSR entry: the local neighbour id
//   degree   n        the remaining degree of a live node; -1 - pass for a node that left in that pass
// The census kernel gives every wave, for a launch bound max_out on the out-degree, in bytes:
//   rows     8 max_out                 the 64-bit adjacency row of every out-neighbour
//   nodes    4 max_out (8-aligned)     their global ids
//   stacks   16 * 64 * max_out         per lane and depth: the candidate set and the set still to branch on
//   tallies  8 (max_out + 1) kmax      the root's and the out-neighbours' columns, flushed once per root
// Python mirrors both formulas (desco_amd/cliques.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DESCO_CC_HD __host__ __device__ __forceinline__
#else
#define DESCO_CC_HD inline
#endif

namespace desco {
namespace clique_census {

constexpr int kMaxK = 64;          // DESCO_CLIQUE_MAX_K
constexpr int kDevMaxOut = 64;     // DESCO_CLIQUE_DEV_MAX_OUT
constexpr int kLdsBytes = 160 * 1024;
constexpr int kSlices = 8;         // workgroups per graph of the census launch: their waves share the graph's roots

DESCO_CC_HD int64_t peel_words(int64_t n, int64_t m) { return 2 * n + 2 * m + 8; }

DESCO_CC_HD int64_t wave_bytes(int64_t max_out, int64_t kmax) {
  return 8 * max_out + ((4 * max_out + 7) & ~(int64_t)7) + 16 * 64 * max_out + 8 * (max_out + 1) * kmax;
}

// waves per workgroup of a census launch: 4, or as many as 160 KiB of LDS hold
DESCO_CC_HD int waves_per_group(int64_t max_out, int64_t kmax) {
  const int64_t fit = kLdsBytes / wave_bytes(max_out, kmax);
  return fit >= 4 ? 4 : fit >= 2 ? 2 : 1;
}

}  // namespace clique_census
}  // namespace desco
