// The device workspace of the k-core / k-truss decomposition, for both sides of the compiler: the gfx950 kernel and its
// entry point (core_truss_dev.hip) and any host code that sizes a launch.  The limit on it is
// DESCO_CORE_TRUSS_DEV_MAX_WORDS (include/desco_hip.h, "CORE / TRUSS"); the host twin (core_truss.cpp) has none.
//
// The kernel keeps one graph of n nodes and m undirected edges in LDS, in 32-bit words:
//   control  3        flag, minimum and count of a peel pass
//   rowptr   n + 1    local CSR offsets
//   entry    2 m      one word per CSR entry: local neighbour id | local edge row << 16 (both below 2^16)
//   ends     m        one word per edge: u | v << 16, u < v
//   peel     max(3 m, n)   truss peel: support, state and frontier, one word per edge each;
//                          core peel (which runs first, in the same words): the remaining degree of every node
// Python mirrors the formula (desco_amd/decomposition.py, workspace_words).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DESCO_CT_HD __host__ __device__ __forceinline__
#else
#define DESCO_CT_HD inline
#endif

namespace desco {
namespace core_truss {

DESCO_CT_HD int64_t workspace_words(int64_t n, int64_t m) { return n + 4 + 3 * m + (3 * m > n ? 3 * m : n); }

}  // namespace core_truss
}  // namespace desco
