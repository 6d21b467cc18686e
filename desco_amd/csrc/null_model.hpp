// The degree-preserving null model's chain, as the host twin (null_model.cpp) and the gfx950 kernel
// (null_model_dev.hip) share it.  See include/desco_hip.h, "NULL MODEL".
//
// One chain per (graph, replica): attempt t of graph g (index graph_base + g) and replica r (index replica_base + r)
// draws
//   w = Philox4x32-10(counter = {lo32(t), hi32(t), lo32(graph_base + g), lo32(replica_base + r)},
//                     key = {lo32(seed), hi32(seed)})
//   i = (uint64(w0) * m) >> 32,  j = (uint64(w1) * m) >> 32,  flip = w2 & 1
// over the m edge slots of the graph.  The Philox is the one of common_device.hpp (Salmon et al., SC'11, the
// Random123 constants), restated here for both sides of the compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DESCO_NM_HD __host__ __device__ __forceinline__
#else
#define DESCO_NM_HD inline
#endif

namespace desco {
namespace null_model {

struct Draw {
  uint32_t i, j, flip;
};

DESCO_NM_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0;
    const uint32_t h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  c[0] = c0, c[1] = c1, c[2] = c2, c[3] = c3;
}

// attempt t of the chain (graph, replica) over m slots, 1 <= m < 2^32
DESCO_NM_HD Draw draw(uint64_t seed, uint32_t graph, uint32_t replica, uint64_t t, uint32_t m) {
  uint32_t c[4] = {(uint32_t)t, (uint32_t)(t >> 32), graph, replica};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return Draw{(uint32_t)(((uint64_t)c[0] * m) >> 32), (uint32_t)(((uint64_t)c[1] * m) >> 32), c[2] & 1u};
}

// Device workspace, in 32-bit words, of a graph with n nodes and m edges: the adjacency bitset, n rows of
// ceil(n / 32) | 1 words (an odd stride: lanes that walk consecutive rows start on different LDS banks), and one word
// per edge slot (a | b << 16)
DESCO_NM_HD int64_t row_words(int64_t n) { return ((n + 31) >> 5) | 1; }
DESCO_NM_HD int64_t workspace_words(int64_t n, int64_t m) { return n * row_words(n) + m; }

}  // namespace null_model
}  // namespace desco
