// THE device ESU walk of the exact ground-truth kernels (gt_count_kernel, go_count_kernel and ge_count_kernel in
// groundtruth_dev.hip, gtl_count_kernel in groundtruth_label_dev.hip, g6_count_kernel in groundtruth6_dev.hip): each
// kernel is a visitor over it.
//
// Enumeration: ESU without extension lists.  In ESU a node u enters the extension set when the FIRST subset node
// adjacent to it is added, and choices are made in list order; with key(u) = (insertion index of that first
// neighbour, position of u in its adjacency row) this is exactly "chosen nodes have strictly increasing keys".  So a
// level is two nested loops over the adjacency rows of the subset's nodes, starting behind the previous key, and a
// candidate is taken iff it is below the root, not in the subset and adjacent to no earlier subset node -- the same
// adjacency bits then extend the induced-subgraph mask.  No per-thread lists: the subset (<= 5 nodes, <= 6 for a
// visitor that asks for it: esu_kmax below), the mask and the loop cursors live in registers (levels are
// template-unrolled).
//
// Work item = one CSR entry (v, u0) with u0 < v: the subtree of subsets whose first chosen node is u0, handled by
// ONE WAVE: the candidates for the next node (the rest of v's row, then u0's row) are dealt round-robin to the 64
// lanes and every lane walks the deeper levels of its candidates on its own.  (One thread per item left the launch
// waiting for the few items rooted at hubs, whose subtrees grow with the cube of the degree.)
//
// A visitor V supplies what differs between the kernels:
//   V::Path    value carried down the levels of one path (EsuNone, or the labelled kernel's running label sum)
//   V::Level   value of one candidate loop (EsuNone, or the orbit kernel's run), closed when the loop ends
//   push<NS>(path, u)                 the path value with u as node number NS
//   found<K>(S, u, mask, path, level) the K-subset S[0..K-2] + u with induced mask `mask` was found
//   close<NS>(S, level)               the loop that chose node number NS of S[0..NS-1] has ended
// A visitor that declares `static constexpr bool kWithEntry = true` (the edge-orbit kernel) is told where a candidate
// was found and gets the path value when a loop ends; it supplies, in place of push and close,
//   push_at<NS>(path, S, u, ab, ci, e)  ab = adjacency bits of u to S[0..NS-1]; e = the CSR entry (S[ci], u)
//   close_at<NS>(S, path, level)        path = the path value of S[0..NS-1]
// A visitor that declares `static constexpr bool kWithVeto = true` (the sampling kernel, sampled_counts_dev.hip) may
// drop a candidate with its whole subtree: it supplies
//   keep<K>(path)                       path = the pushed path value of the K-subset; false: neither found nor descended
#pragma once
#include <type_traits>

#include "common_device.hpp"
#include "groundtruth_esu.hpp"

namespace desco {

constexpr int ESU_KMAX = ESU_KMAX_DEV;

struct EsuNone {};

// the graph of one work item
struct EsuGraph {
  const int64_t* rowptr;
  const int32_t* col;
  const unsigned long long* bits;    // this graph's bitset rows
  int64_t base;                      // its first node
  int words, lv, kmax;               // words per row, the root (local id), largest subset
};

// groundtruth_dev.hip: zero `bits` and build the per-graph adjacency bitset rows from the CSR (the first kernel of
// every device enumerator).  Returns 0 or a hipError_t with the message set.
int gt_build_bitsets(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, const int32_t* node_graph,
                     const int64_t* bit_off, uint64_t* bits, int64_t num_words, int64_t num_nodes,
                     int64_t num_entries, void* stream, const char* who);

__device__ __forceinline__ int64_t esu_row_of_entry(const int64_t* __restrict__ rowptr, int64_t n, int64_t e) {
  int64_t lo = 0, hi = n;            // last row with rowptr[row] <= e
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rowptr[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// the graph of the entry's row v (kmax is the caller's)
__device__ __forceinline__ EsuGraph esu_graph_of(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col,
                                                 const int32_t* node_graph, const int64_t* bit_off,
                                                 const unsigned long long* bits, int64_t v, int kmax) {
  const int g = node_graph[v];
  EsuGraph c;
  c.rowptr = rowptr;
  c.col = col;
  c.base = graph_ptr[g];
  c.words = (int)((graph_ptr[g + 1] - c.base + 63) >> 6);
  c.bits = bits + bit_off[g];
  c.lv = (int)(v - c.base);
  c.kmax = kmax;
  return c;
}

__device__ __forceinline__ unsigned esu_adj(const EsuGraph& g, int a, int b) {
  return (unsigned)(g.bits[(int64_t)a * g.words + (b >> 6)] >> (b & 63)) & 1u;
}

template <class V, class = void>
struct esu_with_entry : std::false_type {};
template <class V>
struct esu_with_entry<V, std::void_t<decltype(V::kWithEntry)>> : std::true_type {};

template <class V, class = void>
struct esu_with_veto : std::false_type {};
template <class V>
struct esu_with_veto<V, std::void_t<decltype(V::kWithVeto)>> : std::true_type {};

// the walk's depth: a visitor that declares `static constexpr int kMax = 6` (groundtruth6_dev.hip) is walked to six
// nodes, its S has kMax entries and its masks up to kMax (kMax - 1) / 2 bits; one that declares nothing is walked to
// ESU_KMAX_DEV = 5
template <class V, class = void>
struct esu_kmax : std::integral_constant<int, ESU_KMAX> {};
template <class V>
struct esu_kmax<V, std::void_t<decltype(V::kMax)>> : std::integral_constant<int, V::kMax> {};

template <int NS, class V>
__device__ __forceinline__ typename V::Path esu_push(V& vis, const int (&S)[esu_kmax<V>::value], typename V::Path path, int u,
                                                     unsigned ab, int ci, int64_t e) {
  if constexpr (esu_with_entry<V>::value) return vis.template push_at<NS>(path, S, u, ab, ci, e);
  else return vis.template push<NS>(path, u);
}

template <int NS, class V>
__device__ __forceinline__ void esu_close(V& vis, const int (&S)[esu_kmax<V>::value], typename V::Path path,
                                          typename V::Level& level) {
  if constexpr (esu_with_entry<V>::value) vis.template close_at<NS>(S, path, level);
  else vis.template close<NS>(S, level);
}

template <int NS, class V>
__device__ void esu_extend(const EsuGraph& g, V& vis, const int (&S)[esu_kmax<V>::value], unsigned mask, typename V::Path path,
                           int ci0, int cp0);

// candidate at position e of the adjacency row (starting at r0) of S[ci] for node number NS of the subset: taken iff
// it is below the root, new, and adjacent to no subset node before S[ci].  Returns false when the row has passed the
// root's id (rows ascend: nothing further qualifies).
template <int NS, class V>
__device__ __forceinline__ bool esu_try(const EsuGraph& g, V& vis, const int (&S)[esu_kmax<V>::value], unsigned mask,
                                        typename V::Path path, int ci, int64_t r0, int64_t e,
                                        typename V::Level& level) {
  const int u = (int)(g.col[e] - g.base);
  if (u >= g.lv) return false;
  unsigned ab = 0;
  bool in_s = false;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    in_s |= u == S[j];
    ab |= esu_adj(g, S[j], u) << j;
  }
  if (in_s || (ab & ((1u << ci) - 1u))) return true;     // u entered the extension set earlier
  const unsigned m2 = mask | (ab << (NS * (NS - 1) / 2));
  const typename V::Path p2 = esu_push<NS>(vis, S, path, u, ab, ci, e);
  if constexpr (esu_with_veto<V>::value) {
    if (!vis.template keep<NS + 1>(p2)) return true;
  }
  vis.template found<NS + 1>(S, u, m2, p2, level);
  constexpr int KM = esu_kmax<V>::value;
  if constexpr (NS + 1 < KM) {
    if (NS + 1 < g.kmax) {
      int S2[KM];
#pragma unroll
      for (int j = 0; j < KM; ++j) S2[j] = j < NS ? S[j] : 0;
      S2[NS] = u;
      esu_extend<NS + 1>(g, vis, S2, m2, p2, ci, (int)(e - r0) + 1);
    }
  }
  return true;
}

// choose node number NS of the subset (S[0..NS-1] chosen, induced mask `mask`); candidates start at key (ci0, cp0)
template <int NS, class V>
__device__ void esu_extend(const EsuGraph& g, V& vis, const int (&S)[esu_kmax<V>::value], unsigned mask, typename V::Path path,
                           int ci0, int cp0) {
  typename V::Level level{};
#pragma unroll
  for (int ci = 0; ci < NS; ++ci) {
    if (ci < ci0) continue;
    const int64_t r0 = g.rowptr[g.base + S[ci]], r1 = g.rowptr[g.base + S[ci] + 1];
    for (int64_t e = r0 + (ci == ci0 ? cp0 : 0); e < r1; ++e)
      if (!esu_try<NS>(g, vis, S, mask, path, ci, r0, e, level)) break;
  }
  esu_close<NS>(vis, S, path, level);
}

// The wave's part of the item (v, u0) at CSR entry e: the candidates for the third node -- v's row behind u0, then
// u0's row; position p -> lane p % 64 -- and everything below them.  `path` is the path value of {v, u0}.
template <class V>
__device__ __forceinline__ void esu_wave_walk(const EsuGraph& g, V& vis, int64_t v, int64_t e, int u0, int lane,
                                              typename V::Path path) {
  if (g.kmax <= 2) return;
  const int S[esu_kmax<V>::value] = {g.lv, u0};      // (the other entries are 0)
  const int64_t v0 = g.rowptr[v], v1 = g.rowptr[v + 1];
  const int64_t w0 = g.rowptr[g.base + u0], w1 = g.rowptr[g.base + u0 + 1];
  const int64_t rest = v1 - (e + 1), total = rest + (w1 - w0);
  typename V::Level level{};           // the lane's 3-node subsets: they share S[0] and S[1]
  for (int64_t p = lane; p < total; p += 64) {
    if (p < rest)
      esu_try<2>(g, vis, S, 1u, path, 0, v0, e + 1 + p, level);
    else
      esu_try<2>(g, vis, S, 1u, path, 1, w0, w0 + (p - rest), level);
  }
  esu_close<2>(vis, S, path, level);
}

}  // namespace desco
