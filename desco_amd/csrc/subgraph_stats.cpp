// Host twin of subgraph_stats_dev.hip (C ABI: desco_subgraph_stats), see include/desco_hip.h.
//
// Per node set M (ascending global ids of one graph): H = G[M], C = its largest connected component (a tie goes to the
// component holding the smallest id), and of C the seven exact quantities the data-set statistics are derived from --
// members |M|, n, m, diameter, sum of d(s,t) over ordered pairs, triangles (int64) and the clustering sum (fp64).
//
// The induced adjacency is a local CSR (every neighbour of a member bisected in the sorted member list); components by
// a queue BFS; then one queue BFS per source of C, with one distance array per thread: memory is O(|M| + edges) per
// thread, never |M|^2.  Sets run in parallel (OpenMP, dynamic); a set above kInnerSet members runs alone with the
// OpenMP loop over its sources instead, so that one huge set does not leave the other threads idle.
//
// The clustering sum is formed the way the device kernel forms it, so that the two agree to the bit: term i (local id
// i in M; 0 outside C or for degree < 2) = (2 T(i)) / (d (d - 1)), one correctly rounded division of two exact
// integers, summed by the balanced pairwise tree over local ids (leaf i and leaf i + s meet at stride s = 1, 2, 4, ..).
// Missing leaves are +0.0 and x + 0.0 = x, so the tree's result does not depend on the power of two it is padded to.
#include <algorithm>
#include <cstdint>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/desco_hip.h"
#include "common_host.hpp"

namespace {

constexpr int64_t kInnerSet = 4096;   // sets above this many members: OpenMP over sources inside the set

struct SetStats {
  int64_t v[6] = {0, 0, 0, 0, 0, 0};   // members, n, m, diameter, dist_sum, triangles
  double clustering_sum = 0.0;
};

// BFS from `src` over the local CSR; dist must be all -1 on entry and is restored through `queue` on exit
inline void bfs_source(const std::vector<int64_t>& ptr, const std::vector<int32_t>& adj, int32_t src,
                       std::vector<int32_t>& dist, std::vector<int32_t>& queue, int64_t& ecc, int64_t& sum) {
  size_t head = 0;
  queue.clear();
  queue.push_back(src);
  dist[src] = 0;
  ecc = 0;
  sum = 0;
  while (head < queue.size()) {
    const int32_t u = queue[head++];
    const int32_t du = dist[u];
    for (int64_t e = ptr[u]; e < ptr[u + 1]; ++e) {
      const int32_t w = adj[e];
      if (dist[w] < 0) {
        dist[w] = du + 1;
        sum += du + 1;
        ecc = du + 1;
        queue.push_back(w);
      }
    }
  }
  for (int32_t u : queue) dist[u] = -1;
}

SetStats set_stats(const int64_t* rowptr, const int32_t* col, const int32_t* mem, int64_t m, int inner_threads) {
  SetStats r;
  r.v[0] = m;
  if (m == 0) return r;
  // local CSR of the induced subgraph
  std::vector<int64_t> ptr(m + 1, 0);
  std::vector<int32_t> adj;
  for (int64_t i = 0; i < m; ++i) {
    const int64_t v = mem[i];
    for (int64_t e = rowptr[v]; e < rowptr[v + 1]; ++e) {
      const int32_t* p = std::lower_bound(mem, mem + m, col[e]);
      if (p != mem + m && *p == col[e]) adj.push_back((int32_t)(p - mem));
    }
    ptr[i + 1] = (int64_t)adj.size();
  }
  // components, labelled by their smallest local id; the largest wins, the first of equals
  std::vector<int32_t> comp(m, -1), queue;
  queue.reserve(m);
  int32_t best = 0;
  int64_t best_size = 0;
  for (int64_t s = 0; s < m; ++s) {
    if (comp[s] >= 0) continue;
    queue.clear();
    queue.push_back((int32_t)s);
    comp[s] = (int32_t)s;
    for (size_t head = 0; head < queue.size(); ++head) {
      const int32_t u = queue[head];
      for (int64_t e = ptr[u]; e < ptr[u + 1]; ++e)
        if (comp[adj[e]] < 0) {
          comp[adj[e]] = (int32_t)s;
          queue.push_back(adj[e]);
        }
    }
    if ((int64_t)queue.size() > best_size) {
      best_size = (int64_t)queue.size();
      best = (int32_t)s;
    }
  }
  std::vector<int32_t> members;   // local ids of C, ascending
  members.reserve(best_size);
  for (int64_t i = 0; i < m; ++i)
    if (comp[i] == best) members.push_back((int32_t)i);
  const int64_t n = best_size;
  // edges, triangles, clustering terms
  int64_t deg_sum = 0, tri2_sum = 0;
  int64_t leaves = 1;
  while (leaves < m) leaves <<= 1;
  std::vector<double> term(leaves, 0.0);
  for (int32_t i : members) {
    const int64_t d = ptr[i + 1] - ptr[i];
    deg_sum += d;
    int64_t tri2 = 0;          // sum over neighbours j of |N(i) & N(j)| = 2 T(i)
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
      const int32_t j = adj[e];
      int64_t a = ptr[i], b = ptr[j];
      while (a < ptr[i + 1] && b < ptr[j + 1]) {
        if (adj[a] < adj[b])
          ++a;
        else if (adj[a] > adj[b])
          ++b;
        else
          ++tri2, ++a, ++b;
      }
    }
    tri2_sum += tri2;
    if (d >= 2) term[i] = (double)tri2 / ((double)d * (double)(d - 1));
  }
  for (int64_t s = 1; s < leaves; s <<= 1)
    for (int64_t i = 0; i + s < leaves; i += 2 * s) term[i] += term[i + s];
  // distances
  int64_t diameter = 0, dist_sum = 0;
#ifdef _OPENMP
#pragma omp parallel num_threads(inner_threads) if (inner_threads > 1)
#endif
  {
    std::vector<int32_t> dist(m, -1), q;
    q.reserve(n);
    int64_t my_diam = 0, my_sum = 0;
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 16) nowait
#endif
    for (int64_t k = 0; k < n; ++k) {
      int64_t ecc, sum;
      bfs_source(ptr, adj, members[k], dist, q, ecc, sum);
      my_diam = std::max(my_diam, ecc);
      my_sum += sum;
    }
#ifdef _OPENMP
#pragma omp critical(desco_subgraph_stats_merge)
#endif
    {
      diameter = std::max(diameter, my_diam);
      dist_sum += my_sum;
    }
  }
  r.v[1] = n;
  r.v[2] = deg_sum / 2;
  r.v[3] = diameter;
  r.v[4] = dist_sum;
  r.v[5] = tri2_sum / 6;
  r.clustering_sum = term[0];
  return r;
}

}  // namespace

extern "C" int desco_subgraph_stats(const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                                    const int64_t* set_ptr, const int32_t* set_nodes, int64_t num_sets, int num_threads,
                                    int64_t* out_i64, double* out_f64) {
  if (num_sets < 0 || num_nodes < 0) return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: negative num_sets or num_nodes");
  if (num_sets == 0) return 0;
  if (!rowptr) return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: rowptr is null");
  if (!set_ptr) return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: set_ptr is null");
  if (!out_i64) return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: out_i64 is null");
  if (!out_f64) return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: out_f64 is null");
  if (set_ptr[0] < 0) return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: set_ptr is not monotone from 0");
  for (int64_t s = 0; s < num_sets; ++s)
    if (set_ptr[s + 1] < set_ptr[s]) return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: set_ptr is not monotone");
  if (set_ptr[num_sets] > set_ptr[0] && !set_nodes)
    return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: set_nodes is null");
  if (rowptr[num_nodes] > rowptr[0] && !col) return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: col is null");
  for (int64_t s = 0; s < num_sets; ++s)
    for (int64_t k = set_ptr[s]; k < set_ptr[s + 1]; ++k) {
      if (set_nodes[k] < 0 || set_nodes[k] >= num_nodes)
        return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: set_nodes holds an id outside the graph");
      if (k > set_ptr[s] && set_nodes[k] <= set_nodes[k - 1])
        return desco::fail(DESCO_EINVAL, "desco_subgraph_stats: a set is not strictly ascending");
    }
  int nt = 1;
#ifdef _OPENMP
  nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#endif
  (void)num_threads;
  auto store = [&](int64_t s, const SetStats& r) {
    for (int k = 0; k < 6; ++k) out_i64[6 * s + k] = r.v[k];
    out_f64[s] = r.clustering_sum;
  };
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 8) num_threads(nt)
#endif
  for (int64_t s = 0; s < num_sets; ++s) {
    const int64_t m = set_ptr[s + 1] - set_ptr[s];
    if (m <= kInnerSet) store(s, set_stats(rowptr, col, set_nodes + set_ptr[s], m, 1));
  }
  for (int64_t s = 0; s < num_sets; ++s) {
    const int64_t m = set_ptr[s + 1] - set_ptr[s];
    if (m > kInnerSet) store(s, set_stats(rowptr, col, set_nodes + set_ptr[s], m, nt));
  }
  return 0;
}
