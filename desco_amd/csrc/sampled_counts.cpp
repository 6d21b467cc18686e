// Sampled canonical counts, the host twin (C ABI: desco_sampled_counts): RAND-ESU over the KEY-ORDERED tree of the
// device walk.  Definitions: include/desco_hip.h, "SAMPLED COUNTS"; the decision chain: sampled_counts.hpp.
//
// The host's exact walk (groundtruth_esu.hpp, EsuWalk) pops its extension list from the back and so builds another tree
// over the same subsets; which subsets survive a sampled walk depends on the tree, so this file restates the device
// walk (groundtruth_esu_dev.hpp, esu_try / esu_extend) in plain C++: a tree node is a sequence (s_0 = v, s_1, ..), its
// children are the candidates u < v outside S whose key -- (index i of the first member of S adjacent to u, position of
// u in s_i's row) -- is larger than the key of the last member, in key order.  Up to 6 nodes.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "groundtruth_esu.hpp"
#include "sampled_counts.hpp"

namespace {

using desco::GraphBits;
using desco::pair_bit;
namespace sc = desco::sampled;

constexpr int KMAX = sc::kKmaxHost;
// class table: for k = 2..6 nodes the 2^(k(k-1)/2) adjacency masks start at OFF[k] (the device table's offsets, then 6)
constexpr int OFF[KMAX + 2] = {0, 0, 0, 2, 10, 74, 1098, 1098 + 32768};

struct Walk {
  const GraphBits& g;
  const int64_t* rowptr;
  const int32_t* col;
  const int16_t* table;
  const uint64_t* thr;
  int kmax, Q, lv;
  int64_t* out;                      // the root's row
  int S[KMAX];

  // choose node number ns of the subset (S[0..ns-1] chosen, induced mask `mask`, path hash h); candidates start at
  // key (ci0, cp0)
  void extend(int ns, uint32_t mask, uint64_t h, int ci0, int cp0) {
    for (int ci = ci0; ci < ns; ++ci) {
      const int64_t r0 = rowptr[g.base + S[ci]], r1 = rowptr[g.base + S[ci] + 1];
      for (int64_t e = r0 + (ci == ci0 ? cp0 : 0); e < r1; ++e) {
        const int u = (int)(col[e] - g.base);
        if (u >= lv) break;                          // rows ascend: nothing further is below the root
        uint32_t ab = 0;
        bool in_s = false;
        for (int j = 0; j < ns; ++j) {
          in_s |= u == S[j];
          ab |= (uint32_t)g.adj(S[j], u) << j;
        }
        if (in_s || (ab & ((1u << ci) - 1u))) continue;          // u entered the extension set earlier
        const uint64_t h2 = sc::step(h, u);
        if (!sc::keep(h2, thr[ns + 1])) continue;                // dropped with its whole subtree
        const uint32_t m2 = mask | (ab << (ns * (ns - 1) / 2));
        const int q = table[OFF[ns + 1] + m2];
        if (q >= 0) out[q] += 1;
        if (ns + 1 < kmax && ns + 1 < KMAX) {
          S[ns] = u;
          extend(ns + 1, m2, h2, ci, (int)(e - r0) + 1);
        }
      }
    }
  }
};

}  // namespace

extern "C" int desco_sampled_counts(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                    const int32_t* col, const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                    const int32_t* q_edges, int num_queries, int kmax, const int64_t* thr,
                                    uint64_t seed, int64_t graph_base, int64_t replica_base, int num_replicas,
                                    int per_graph, int num_threads, int64_t* out) {
  const char* who = "desco_sampled_counts";
  if (num_replicas < 0) return desco::fail(DESCO_EINVAL, "desco_sampled_counts: num_replicas must not be negative");
  if (num_graphs < 0 || num_queries < 0 || graph_base < 0 || replica_base < 0)
    return desco::fail(DESCO_EINVAL, "desco_sampled_counts: negative count or base");
  if (num_graphs == 0 || num_queries == 0 || num_replicas == 0) return 0;
  if (!graph_ptr || !rowptr || !q_nodes || !q_edge_ptr || !thr || !out)
    return desco::fail(DESCO_EINVAL, "desco_sampled_counts: null pointer");
  if (kmax < 2 || kmax > KMAX) return desco::fail(DESCO_EINVAL, "desco_sampled_counts: kmax must be 2..6");
  if (per_graph != 0 && per_graph != 1)
    return desco::fail(DESCO_EINVAL, "desco_sampled_counts: per_graph must be 0 or 1");
  if (num_queries > 32767) return desco::fail(DESCO_EINVAL, "desco_sampled_counts: too many queries");
  uint64_t t[KMAX + 1] = {0};
  for (int d = 2; d <= kmax; ++d) {
    if (thr[d] < 0 || thr[d] > (int64_t)sc::kAlways)
      return desco::fail(DESCO_EINVAL, "desco_sampled_counts: a threshold is outside 0..2^32");
    t[d] = (uint64_t)thr[d];
  }
  const int64_t total = graph_ptr[num_graphs];
  if (total < 0 || (total > 0 && rowptr[total] > 0 && !col))
    return desco::fail(DESCO_EINVAL, "desco_sampled_counts: null pointer");
  try {
    std::vector<int16_t> table((size_t)OFF[KMAX + 1], -1);
    for (int q = 0; q < num_queries; ++q) {
      const int k = q_nodes[q];
      if (k < 2 || k > kmax)
        return desco::fail(DESCO_EINVAL, "desco_sampled_counts: queries must have 2..kmax nodes");
      uint32_t m = 0;
      if (const int rc = desco::query_mask(who, q_edge_ptr, q_edges, q, k, &m)) return rc;
      int perm[KMAX];                                  // every relabeling of the query is a mask of its class
      for (int i = 0; i < k; ++i) perm[i] = i;
      bool clash = false;
      do {
        uint32_t r = 0;
        for (int b = 1; b < k; ++b)
          for (int a = 0; a < b; ++a)
            if (m >> pair_bit(a, b) & 1)
              r |= 1u << pair_bit(std::min(perm[a], perm[b]), std::max(perm[a], perm[b]));
        int16_t& slot = table[OFF[k] + r];
        clash |= slot >= 0 && slot != q;
        slot = (int16_t)q;
      } while (std::next_permutation(perm, perm + k));
      if (clash) return desco::fail(DESCO_EINVAL, "desco_sampled_counts: two queries are isomorphic");
    }
    const size_t rows = per_graph ? (size_t)num_graphs : (size_t)total;
    std::memset(out, 0, sizeof(int64_t) * (size_t)num_replicas * rows * (size_t)num_queries);
#ifdef _OPENMP
    const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
    (void)num_threads;
#endif
    bool oom = false;
    const int64_t R = num_replicas, items = num_graphs * R;
#pragma omp parallel num_threads(nt)
    {
      GraphBits g;
      int64_t built = -1;                              // the graph whose bitset rows g holds
#pragma omp for schedule(dynamic, 1)
      for (int64_t i = 0; i < items; ++i) try {
        const int64_t gi = i / R, r = i - gi * R;
        if (built != gi) {
          g.build(graph_ptr, gi, rowptr, col);
          built = gi;
        }
        Walk w{g, rowptr, col, table.data(), t, kmax, num_queries, 0, nullptr, {0}};
        for (int v = 0; v < (int)g.n; ++v) {
          w.lv = v;
          w.S[0] = v;
          w.out = out + ((size_t)r * rows + (size_t)(per_graph ? gi : g.base + v)) * (size_t)num_queries;
          w.extend(1, 0u, sc::root_hash(seed, (uint32_t)(graph_base + gi), (uint32_t)(replica_base + r), (uint32_t)v),
                   0, 0);
        }
      } catch (const std::bad_alloc&) {
#pragma omp atomic write
        oom = true;
      }
    }
    if (oom) return desco::fail(DESCO_ENOMEM, "desco_sampled_counts: out of memory");
    return 0;
  } catch (const std::bad_alloc&) {
    return desco::fail(DESCO_ENOMEM, "desco_sampled_counts: out of memory");
  }
}
