// Shared by the exact ground-truth enumerators.  Host side, header-only: the class-table offsets, the pair-bit
// convention of adjacency masks, the query-edge reader, one graph's adjacency bitset rows, and THE host ESU walk
// (groundtruth.cpp and groundtruth_label.cpp are visitors over it; groundtruth_match.cpp uses the bitset rows).
// The device walk is groundtruth_esu_dev.hpp.
#pragma once
#include <stdint.h>

#include <new>
#include <string>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/desco_hip.h"
#include "common_host.hpp"

namespace desco {

// class table of the device enumerators: for k = 2..5 nodes the 2^(k(k-1)/2) adjacency masks start at ESU_OFF[k]
constexpr int ESU_KMAX_DEV = 5, ESU_ENTRIES = 1098;
constexpr int ESU_OFF[ESU_KMAX_DEV + 2] = {0, 0, 0, 2, 10, 74, ESU_ENTRIES};
// class table of the 6-node device enumerator (groundtruth6_dev.hip): the same blocks, then the 2^15 masks of 6 nodes
constexpr int ESU6_KMAX = 6, ESU6_ENTRIES = 33866, ESU6_MAXQ = 142;      // 142 = 1 + 2 + 6 + 21 + 112 classes
constexpr int ESU6_OFF[ESU6_KMAX + 2] = {0, 0, 0, 2, 10, 74, ESU_ENTRIES, ESU6_ENTRIES};

inline int pair_bit(int a, int b) { return b * (b - 1) / 2 + a; }   // a < b

// Adjacency mask of query q (k nodes) from its edge list.  Returns 0, or DESCO_EINVAL with "<who>: bad query edge".
inline int query_mask(const char* who, const int32_t* q_edge_ptr, const int32_t* q_edges, int q, int k,
                      uint32_t* mask) {
  uint32_t m = 0;
  for (int e = q_edge_ptr[q]; e < q_edge_ptr[q + 1]; ++e) {
    int a = q_edges[2 * e], b = q_edges[2 * e + 1];
    if (a == b || a < 0 || b < 0 || a >= k || b >= k)
      return fail(DESCO_EINVAL, (std::string(who) + ": bad query edge").c_str());
    if (a > b) { const int t = a; a = b; b = t; }
    m |= 1u << pair_bit(a, b);
  }
  *mask = m;
  return 0;
}

// One graph of a CSR graph set with its adjacency bitset rows (n x words; node ids local to the graph).
struct GraphBits {
  int64_t base = 0, n = 0;
  int words = 0;
  std::vector<uint64_t> bits;
  void build(const int64_t* graph_ptr, int64_t g, const int64_t* rowptr, const int32_t* col) {
    base = graph_ptr[g];
    n = graph_ptr[g + 1] - base;
    words = (int)((n + 63) / 64);
    bits.assign((size_t)n * words, 0);
    for (int64_t u = 0; u < n; ++u)
      for (int64_t e = rowptr[base + u]; e < rowptr[base + u + 1]; ++e) {
        const int w = (int)(col[e] - base);
        bits[(size_t)u * words + (w >> 6)] |= (uint64_t)1 << (w & 63);
      }
  }
  bool adj(int a, int b) const { return bits[(size_t)a * words + (b >> 6)] >> (b & 63) & 1; }
  // induced adjacency mask of sub[0..k-1]
  uint32_t mask_of(const int* sub, int k) const {
    uint32_t m = 0;
    for (int b = 1; b < k; ++b)
      for (int a = 0; a < b; ++a)
        if (adj(sub[a], sub[b])) m |= 1u << pair_bit(a, b);
    return m;
  }
};

constexpr int ESU_KMAX_HOST = 6;

// ESU: every connected node subset of 2..kmax nodes is visited exactly once, rooted at its largest id v = sub[0].
template <class Visitor>
struct EsuWalk {
  const GraphBits& g;
  const int64_t* rowptr;
  const int32_t* col;
  int kmax;
  Visitor& visit;
  std::vector<uint8_t> seen;

  void extend(int* sub, int nsub, std::vector<int>& ext, int v) {
    if (nsub > 1) visit(g, sub, nsub, v);
    if (nsub == kmax) return;
    std::vector<int> newly, ext2;
    while (!ext.empty()) {
      const int w = ext.back();
      ext.pop_back();
      newly.clear();
      const int64_t gw = g.base + w;
      for (int64_t e = rowptr[gw]; e < rowptr[gw + 1]; ++e) {
        const int u = (int)(col[e] - g.base);
        if (u >= v) break;                       // rows sorted ascending; only ids below the root
        if (!seen[u]) {
          seen[u] = 1;
          newly.push_back(u);
        }
      }
      ext2 = ext;
      ext2.insert(ext2.end(), newly.begin(), newly.end());
      sub[nsub] = w;
      extend(sub, nsub + 1, ext2, v);
      for (int u : newly) seen[u] = 0;
    }
  }

  void graph() {
    seen.assign((size_t)g.n, 0);
    int sub[ESU_KMAX_HOST];
    std::vector<int> ext;
    for (int v = 0; v < (int)g.n; ++v) {
      ext.clear();
      seen[v] = 1;
      const int64_t gv = g.base + v;
      for (int64_t e = rowptr[gv]; e < rowptr[gv + 1]; ++e) {
        const int u = (int)(col[e] - g.base);
        if (u >= v) break;
        seen[u] = 1;
        ext.push_back(u);
      }
      const std::vector<int> marked = ext;
      sub[0] = v;
      extend(sub, 1, ext, v);
      for (int u : marked) seen[u] = 0;
      seen[v] = 0;
    }
  }
};

// The walk over every graph.  OpenMP over graphs; every thread gets its own visitor from make_visitor() and calls it as
// visit(graph, sub, k, v) for every subset.  A graph's subsets are visited by one thread, in one order, so a visitor
// that writes only that graph's output rows gives a result that does not depend on the number of threads.
// Returns false when memory ran out.
template <class MakeVisitor>
bool esu_enumerate_graphs(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr, const int32_t* col,
                          int kmax, int num_threads, MakeVisitor make_visitor) {
#ifdef _OPENMP
  const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
  (void)num_threads;
#endif
  bool oom = false;
#pragma omp parallel num_threads(nt)
  {
    auto visit = make_visitor();
    GraphBits g;
    EsuWalk<decltype(visit)> walk{g, rowptr, col, kmax, visit, {}};
#pragma omp for schedule(dynamic, 1)
    for (int64_t i = 0; i < num_graphs; ++i) try {
      g.build(graph_ptr, i, rowptr, col);
      walk.graph();
    } catch (const std::bad_alloc&) {
#pragma omp atomic write
      oom = true;
    }
  }
  return !oom;
}

}  // namespace desco
