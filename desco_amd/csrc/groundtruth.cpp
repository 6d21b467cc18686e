// Exact canonical ground-truth counts (C ABI: desco_canonical_counts), SURVEY.md 8f row N1.
//
// count[v][q] = number of node subsets S with max(S) = v whose INDUCED subgraph is isomorphic to
// query q -- what the reference obtains by running networkx VF2 (MatchSubgraphWorker,
// workload.py:327-348: one match per automorphism, keyed by max(vmap.keys())) and dividing by the
// query's symmetry factor (data.py:61-67).  Written from that definition with the ESU enumeration
// (every connected node subset of size <= kmax is visited exactly once, rooted at its maximum id)
// and an isomorphism-class lookup over induced adjacency bitmasks (<= 6 nodes -> <= 15 bits).
// The walk is groundtruth_esu.hpp's; this file holds its canonical, orbit and edge-orbit visitors and their tables.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "groundtruth_esu.hpp"

namespace {

using desco::ESU_ENTRIES;
using desco::ESU_OFF;
using desco::GraphBits;
using desco::pair_bit;
constexpr int KMAX = desco::ESU_KMAX_HOST;
constexpr int ORB_KMAX = desco::ESU_KMAX_DEV;     // orbit counts and the device class table: queries of 2..5 nodes

// canonical form of every adjacency mask on k nodes: minimum over all relabelings
std::vector<uint16_t> canon_table(int k) {
  const int nb = k * (k - 1) / 2;
  std::vector<uint16_t> tab((size_t)1 << nb, 0xffff);
  std::vector<int> perm(k);
  for (int i = 0; i < k; ++i) perm[i] = i;
  std::vector<std::vector<int>> perms;
  do perms.push_back(perm);
  while (std::next_permutation(perm.begin(), perm.end()));
  for (uint32_t m = 0; m < ((uint32_t)1 << nb); ++m) {
    uint32_t best = 0xffffffffu;
    for (const auto& p : perms) {
      uint32_t r = 0;
      for (int b = 1; b < k; ++b)
        for (int a = 0; a < b; ++a)
          if (m >> pair_bit(a, b) & 1) {
            const int x = std::min(p[a], p[b]), y = std::max(p[a], p[b]);
            r |= 1u << pair_bit(x, y);
          }
      best = std::min(best, r);
    }
    tab[m] = (uint16_t)best;
  }
  return tab;
}

struct Classifier {
  // for size k: map canonical mask -> list of query indices
  std::vector<std::vector<int>> by_mask[KMAX + 1];
  std::vector<uint16_t> canon[KMAX + 1];
  bool used[KMAX + 1] = {false};
};

// canonical counts: the subset counts for its root v, in the columns of the queries of its class
struct CanonicalVisitor {
  const Classifier& cl;
  int64_t* out;
  int num_q;
  void operator()(const GraphBits& g, const int* sub, int k, int v) const {
    if (!cl.used[k]) return;
    for (int q : cl.by_mask[k][cl.canon[k][g.mask_of(sub, k)]]) out[(g.base + v) * num_q + q] += 1;
  }
};

// orbit counts: the subset counts for every member, in the column of the member's position (desco_orbit_table)
struct OrbitVisitor {
  const int16_t* table;
  int64_t* out;
  int num_cols;
  void operator()(const GraphBits& g, const int* sub, int k, int) const {
    const int16_t* row = table + (size_t)(ESU_OFF[k] + g.mask_of(sub, k)) * ORB_KMAX;
    if (row[0] < 0) return;
    for (int i = 0; i < k; ++i) out[(g.base + sub[i]) * num_cols + row[i]] += 1;
  }
};

// the mask of every relabeling p of the k-node mask m (position a becomes position p[a]), in std::next_permutation
// order from the identity: f(image, p)
template <class F>
void for_each_relabeling(int k, uint32_t m, F f) {
  int perm[KMAX];
  for (int i = 0; i < k; ++i) perm[i] = i;
  do {
    uint32_t r = 0;
    for (int b = 1; b < k; ++b)
      for (int a = 0; a < b; ++a)
        if (m >> pair_bit(a, b) & 1) r |= 1u << pair_bit(std::min(perm[a], perm[b]), std::max(perm[a], perm[b]));
    f(r, perm);
  } while (std::next_permutation(perm, perm + k));
}

}  // namespace

extern "C" int desco_canonical_counts(const int64_t* graph_ptr, int64_t num_graphs,
                                      const int64_t* rowptr, const int32_t* col,
                                      const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                      const int32_t* q_edges, int num_queries, int num_threads,
                                      int64_t* out) {
  if (!graph_ptr || !rowptr || !q_nodes || !q_edge_ptr || !out || num_graphs < 0 || num_queries < 0)
    return desco::fail(DESCO_EINVAL, "desco_canonical_counts: bad argument");
  try {
    Classifier cl;
    int kmax = 0;
    for (int q = 0; q < num_queries; ++q) {
      const int k = q_nodes[q];
      if (k < 2 || k > KMAX)
        return desco::fail(DESCO_EINVAL, "desco_canonical_counts: queries must have 2..6 nodes");
      kmax = std::max(kmax, k);
      if (!cl.used[k]) {
        cl.used[k] = true;
        cl.canon[k] = canon_table(k);
        cl.by_mask[k].assign((size_t)1 << (k * (k - 1) / 2), {});
      }
      uint32_t m = 0;
      if (const int rc = desco::query_mask("desco_canonical_counts", q_edge_ptr, q_edges, q, k, &m)) return rc;
      cl.by_mask[k][cl.canon[k][m]].push_back(q);
    }
    const int64_t total = graph_ptr[num_graphs];
    std::memset(out, 0, sizeof(int64_t) * (size_t)total * (size_t)num_queries);
    if (num_queries == 0) return 0;
    if (!desco::esu_enumerate_graphs(graph_ptr, num_graphs, rowptr, col, kmax, num_threads,
                                     [&] { return CanonicalVisitor{cl, out, num_queries}; }))
      return desco::fail(DESCO_ENOMEM, "desco_canonical_counts: out of memory");
    return 0;
  } catch (const std::bad_alloc&) {
    return desco::fail(DESCO_ENOMEM, "desco_canonical_counts: out of memory");
  }
}

// HOST helper: the class table the device kernel (groundtruth_dev.hip, gt_count_kernel) reads.
extern "C" int desco_canonical_class_table(const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                           const int32_t* q_edges, int num_queries, int16_t* table,
                                           int* kmax_out) {
  if (!q_nodes || !q_edge_ptr || !table || !kmax_out || num_queries < 0 || num_queries > 32)
    return desco::fail(DESCO_EINVAL, "desco_canonical_class_table: bad argument (at most 32 queries)");
  for (int i = 0; i < ESU_ENTRIES; ++i) table[i] = -1;
  int kmax = 0;
  for (int q = 0; q < num_queries; ++q) {
    const int k = q_nodes[q];
    if (k < 2 || k > ORB_KMAX)
      return desco::fail(DESCO_EINVAL, "desco_canonical_class_table: the device path takes queries of 2..5 nodes");
    kmax = std::max(kmax, k);
    uint32_t m = 0;
    if (const int rc = desco::query_mask("desco_canonical_class_table", q_edge_ptr, q_edges, q, k, &m)) return rc;
    bool clash = false;                              // every relabeling of the query is a mask of its class
    for_each_relabeling(k, m, [&](uint32_t r, const int*) {
      int16_t& slot = table[ESU_OFF[k] + r];
      clash |= slot >= 0 && slot != q;
      slot = (int16_t)q;
    });
    if (clash) return desco::fail(DESCO_EINVAL, "desco_canonical_class_table: two queries are isomorphic");
  }
  *kmax_out = kmax;
  return 0;
}

// HOST helper: the class table of the 6-node device kernel (groundtruth6_dev.hip, g6_count_kernel): the table above
// with the block of the 2^15 masks of 6 nodes behind it (ESU6_OFF), queries of 2..6 nodes, at most 142.
extern "C" int desco_canonical_class_table6(const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                            const int32_t* q_edges, int num_queries, int16_t* table,
                                            int* kmax_out) {
  if (!q_nodes || !q_edge_ptr || !table || !kmax_out || num_queries < 0 || num_queries > desco::ESU6_MAXQ)
    return desco::fail(DESCO_EINVAL, "desco_canonical_class_table6: bad argument (at most 142 queries)");
  for (int i = 0; i < desco::ESU6_ENTRIES; ++i) table[i] = -1;
  int kmax = 0;
  for (int q = 0; q < num_queries; ++q) {
    const int k = q_nodes[q];
    if (k < 2 || k > desco::ESU6_KMAX)
      return desco::fail(DESCO_EINVAL, "desco_canonical_class_table6: queries must have 2..6 nodes");
    kmax = std::max(kmax, k);
    uint32_t m = 0;
    if (const int rc = desco::query_mask("desco_canonical_class_table6", q_edge_ptr, q_edges, q, k, &m)) return rc;
    bool clash = false;                              // every relabeling of the query (720 for 6 nodes) is a mask of its class
    for_each_relabeling(k, m, [&](uint32_t r, const int*) {
      int16_t& slot = table[desco::ESU6_OFF[k] + r];
      clash |= slot >= 0 && slot != q;
      slot = (int16_t)q;
    });
    if (clash) return desco::fail(DESCO_EINVAL, "desco_canonical_class_table6: two queries are isomorphic");
  }
  *kmax_out = kmax;
  return 0;
}

// ---- orbit counts (graphlet degree vectors) ---------------------------------------------------------------------------
// orbit[v][(q,o)] = #{S containing v : G[S] isomorphic to q by a map that takes v into orbit o of Aut(q)}.  The orbits
// of a query are those of its automorphism group on the node positions, numbered in ascending order of their smallest
// member; the columns are the queries in the given order and, inside a query, its orbits in order.
//
// HOST helper: table[1098][5], for k = 2..5 and every adjacency mask on k nodes (the class table's convention and
// offsets) the output column of every position i < k of the subset, or -1 where the mask's class was not asked for.
extern "C" int desco_orbit_table(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                                 int num_queries, int16_t* table, int* num_columns, int* kmax_out) {
  if (!q_nodes || !q_edge_ptr || !table || !num_columns || !kmax_out || num_queries < 0)
    return desco::fail(DESCO_EINVAL, "desco_orbit_table: bad argument");
  for (int i = 0; i < ESU_ENTRIES * ORB_KMAX; ++i) table[i] = -1;
  int kmax = 0, cols = 0;
  std::vector<int16_t> owner(ESU_ENTRIES, -1);
  for (int q = 0; q < num_queries; ++q) {
    const int k = q_nodes[q];
    if (k < 2 || k > ORB_KMAX) return desco::fail(DESCO_EINVAL, "desco_orbit_table: orbit counts take queries of 2..5 nodes");
    if (q >= 32767) return desco::fail(DESCO_EINVAL, "desco_orbit_table: too many queries");
    kmax = std::max(kmax, k);
    uint32_t m = 0;
    if (const int rc = desco::query_mask("desco_orbit_table", q_edge_ptr, q_edges, q, k, &m)) return rc;
    uint32_t reach = 1;                              // positions reachable from position 0
    for (int it = 0; it < k; ++it)
      for (int b = 1; b < k; ++b)
        for (int a = 0; a < b; ++a)
          if ((m >> pair_bit(a, b) & 1) && ((reach >> a | reach >> b) & 1)) reach |= 1u << a | 1u << b;
    if (reach != (1u << k) - 1) return desco::fail(DESCO_EINVAL, "desco_orbit_table: a query is not connected");
    // every relabeling p of the query (position a becomes subset position p[a]); those that keep the mask are Aut(q)
    int orbit_min[ORB_KMAX];
    for (int i = 0; i < k; ++i) orbit_min[i] = i;
    std::vector<uint32_t> images;
    std::vector<int> perms;
    for_each_relabeling(k, m, [&](uint32_t r, const int* perm) {
      images.push_back(r);
      perms.insert(perms.end(), perm, perm + k);
      if (r == m)
        for (int i = 0; i < k; ++i) orbit_min[i] = std::min(orbit_min[i], perm[i]);   // (Aut is a group: min is exact)
    });
    int orbit_of[ORB_KMAX], n_orb = 0;               // numbered in ascending order of the smallest member
    for (int i = 0; i < k; ++i)
      if (orbit_min[i] == i) orbit_of[i] = n_orb++;
    for (int i = 0; i < k; ++i) orbit_of[i] = orbit_of[orbit_min[i]];
    if (cols + n_orb > 32767) return desco::fail(DESCO_EINVAL, "desco_orbit_table: too many columns");
    for (size_t t = 0; t < images.size(); ++t) {
      const int slot = ESU_OFF[k] + (int)images[t];
      if (owner[slot] >= 0 && owner[slot] != q)
        return desco::fail(DESCO_EINVAL, "desco_orbit_table: two queries are isomorphic");
      owner[slot] = (int16_t)q;
      for (int a = 0; a < k; ++a) table[(size_t)slot * ORB_KMAX + perms[t * k + a]] = (int16_t)(cols + orbit_of[a]);
    }
    cols += n_orb;
  }
  *num_columns = cols;
  *kmax_out = kmax;
  return 0;
}

// HOST: out[v][column] int64 [num_nodes][num_columns of desco_orbit_table], every found subset adds 1 to k cells.
extern "C" int desco_orbit_counts(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                  const int32_t* col, const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                  const int32_t* q_edges, int num_queries, int num_threads, int64_t* out) {
  if (!graph_ptr || !rowptr || !q_nodes || !q_edge_ptr || !out || num_graphs < 0 || num_queries < 0)
    return desco::fail(DESCO_EINVAL, "desco_orbit_counts: bad argument");
  try {
    std::vector<int16_t> table((size_t)ESU_ENTRIES * ORB_KMAX);
    int cols = 0, kmax = 0;
    if (const int rc = desco_orbit_table(q_nodes, q_edge_ptr, q_edges, num_queries, table.data(), &cols, &kmax))
      return rc;
    std::memset(out, 0, sizeof(int64_t) * (size_t)graph_ptr[num_graphs] * (size_t)cols);
    if (cols == 0) return 0;
    if (!desco::esu_enumerate_graphs(graph_ptr, num_graphs, rowptr, col, kmax, num_threads,
                                     [&] { return OrbitVisitor{table.data(), out, cols}; }))
      return desco::fail(DESCO_ENOMEM, "desco_orbit_counts: out of memory");
    return 0;
  } catch (const std::bad_alloc&) {
    return desco::fail(DESCO_ENOMEM, "desco_orbit_counts: out of memory");
  }
}
// ---- edge orbit counts (edge graphlet degree vectors) -----------------------------------------------------------------
// eorb[e][(q,o)] = #{connected S containing both ends of e : G[S] isomorphic to q by a map that takes e into edge orbit
// o}.  The edge orbits of a query are those of Aut(q) on its edge set; edges are ordered by pair_bit and the orbits
// numbered in ascending order of their smallest member.  Rows: the CSR entries (v, u) with u < v, in CSR order.
//
// HOST helper: table[1098][10], for k = 2..5, every adjacency mask on k nodes and every pair bit p of k nodes the output
// column of that pair when the mask's class was asked for and the pair is an edge of the mask, else -1.
namespace {
constexpr int EORB_PAIRS = ORB_KMAX * (ORB_KMAX - 1) / 2;
}

extern "C" int desco_edge_orbit_table(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                                      int num_queries, int16_t* table, int* num_columns, int* kmax_out) {
  if (!q_nodes || !q_edge_ptr || !table || !num_columns || !kmax_out || num_queries < 0)
    return desco::fail(DESCO_EINVAL, "desco_edge_orbit_table: bad argument");
  for (int i = 0; i < ESU_ENTRIES * EORB_PAIRS; ++i) table[i] = -1;
  int kmax = 0, cols = 0;
  std::vector<int16_t> owner(ESU_ENTRIES, -1);
  for (int q = 0; q < num_queries; ++q) {
    const int k = q_nodes[q];
    if (k < 2 || k > ORB_KMAX)
      return desco::fail(DESCO_EINVAL, "desco_edge_orbit_table: edge orbit counts take queries of 2..5 nodes");
    if (q >= 32767) return desco::fail(DESCO_EINVAL, "desco_edge_orbit_table: too many queries");
    kmax = std::max(kmax, k);
    uint32_t m = 0;
    if (const int rc = desco::query_mask("desco_edge_orbit_table", q_edge_ptr, q_edges, q, k, &m)) return rc;
    uint32_t reach = 1;                              // positions reachable from position 0
    for (int it = 0; it < k; ++it)
      for (int b = 1; b < k; ++b)
        for (int a = 0; a < b; ++a)
          if ((m >> pair_bit(a, b) & 1) && ((reach >> a | reach >> b) & 1)) reach |= 1u << a | 1u << b;
    if (reach != (1u << k) - 1) return desco::fail(DESCO_EINVAL, "desco_edge_orbit_table: a query is not connected");
    // every relabeling p of the query; the pair (a, b) becomes the pair bit image[pair_bit(a, b)] of the subset.  Those
    // that keep the mask are Aut(q): they permute the query's edges.
    const int nb = k * (k - 1) / 2;
    int orbit_min[EORB_PAIRS];
    for (int p = 0; p < nb; ++p) orbit_min[p] = p;
    std::vector<uint32_t> images;
    std::vector<int> pair_images;
    for_each_relabeling(k, m, [&](uint32_t r, const int* perm) {
      images.push_back(r);
      for (int b = 1; b < k; ++b)
        for (int a = 0; a < b; ++a) {
          const int to = pair_bit(std::min(perm[a], perm[b]), std::max(perm[a], perm[b]));
          pair_images.push_back(to);                 // (pushed in pair-bit order: b outer, a inner)
          if (r == m) orbit_min[pair_bit(a, b)] = std::min(orbit_min[pair_bit(a, b)], to);   // (a group: min is exact)
        }
    });
    int orbit_of[EORB_PAIRS], n_orb = 0;             // over the edges only, ascending smallest member
    for (int p = 0; p < nb; ++p)
      if ((m >> p & 1) && orbit_min[p] == p) orbit_of[p] = n_orb++;
    for (int p = 0; p < nb; ++p)
      if (m >> p & 1) orbit_of[p] = orbit_of[orbit_min[p]];
    if (cols + n_orb > 32767) return desco::fail(DESCO_EINVAL, "desco_edge_orbit_table: too many columns");
    for (size_t t = 0; t < images.size(); ++t) {
      const int slot = ESU_OFF[k] + (int)images[t];
      if (owner[slot] >= 0 && owner[slot] != q)
        return desco::fail(DESCO_EINVAL, "desco_edge_orbit_table: two queries are isomorphic");
      owner[slot] = (int16_t)q;
      for (int p = 0; p < nb; ++p)
        if (m >> p & 1) table[(size_t)slot * EORB_PAIRS + pair_images[t * nb + p]] = (int16_t)(cols + orbit_of[p]);
    }
    cols += n_orb;
  }
  *num_columns = cols;
  *kmax_out = kmax;
  return 0;
}

namespace {

// edge orbit counts: the subset counts for every edge among its members, in the column of the edge's pair
// (desco_edge_orbit_table).  The row of the edge {x, y}, x > y: the lower entries (ids below the row's node) come first
// in a CSR row, so it is the number of lower entries in the rows before x plus the position of y in row x -- found by
// bisection, or for a graph of at most EORB_DENSE_MAX nodes read from a dense n x n table filled when the walk enters
// the graph (rows relative to the graph's first; the walk visits a graph's subsets in one go, on one thread).
constexpr int64_t EORB_DENSE_MAX = 1024;

struct EdgeOrbitVisitor {
  const int16_t* table;
  const int64_t* rowptr;
  const int32_t* col;
  const int64_t* lower_start;                        // [N + 1] lower entries in the rows before a node
  int64_t* out;
  int num_cols;
  std::vector<int32_t> dense;                        // [n][n] of the graph at dense_base, where it is small
  int64_t dense_base = -1, dense_n = 0;

  void enter(const GraphBits& g) {
    dense_base = g.base;
    dense_n = g.n <= EORB_DENSE_MAX ? g.n : 0;
    if (dense_n == 0) return;
    if (dense.size() < (size_t)(g.n * g.n)) dense.resize((size_t)(g.n * g.n));    // (only cells of edges are read)
    for (int64_t x = 0; x < g.n; ++x) {
      const int64_t r0 = rowptr[g.base + x];
      for (int64_t e = r0; e < rowptr[g.base + x + 1] && col[e] < g.base + x; ++e) {
        const int64_t y = col[e] - g.base;
        dense[x * g.n + y] = dense[y * g.n + x] = (int32_t)(lower_start[g.base + x] + (e - r0) - lower_start[g.base]);
      }
    }
  }
  int64_t edge_row(const GraphBits& g, int x, int y) const {
    if (dense_n) return lower_start[g.base] + dense[(size_t)x * g.n + y];
    if (x < y) std::swap(x, y);
    const int32_t* first = col + rowptr[g.base + x];
    const int32_t* last = col + rowptr[g.base + x + 1];
    return lower_start[g.base + x] + (std::lower_bound(first, last, (int32_t)(g.base + y)) - first);
  }
  void operator()(const GraphBits& g, const int* sub, int k, int) {
    if (g.base != dense_base) enter(g);
    const int16_t* row = table + (size_t)(ESU_OFF[k] + g.mask_of(sub, k)) * EORB_PAIRS;
    for (int b = 1; b < k; ++b)
      for (int a = 0; a < b; ++a) {
        const int column = row[pair_bit(a, b)];
        if (column >= 0) out[edge_row(g, sub[a], sub[b]) * num_cols + column] += 1;
      }
  }
};

}  // namespace

// HOST: out[edge][column] int64 [number of entries (v, u) with u < v][num_columns of desco_edge_orbit_table].
extern "C" int desco_edge_orbit_counts(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                       const int32_t* col, const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                       const int32_t* q_edges, int num_queries, int num_threads, int64_t* out) {
  if (!graph_ptr || !rowptr || !q_nodes || !q_edge_ptr || !out || num_graphs < 0 || num_queries < 0)
    return desco::fail(DESCO_EINVAL, "desco_edge_orbit_counts: bad argument");
  try {
    std::vector<int16_t> table((size_t)ESU_ENTRIES * EORB_PAIRS);
    int cols = 0, kmax = 0;
    if (const int rc = desco_edge_orbit_table(q_nodes, q_edge_ptr, q_edges, num_queries, table.data(), &cols, &kmax))
      return rc;
    const int64_t total = graph_ptr[num_graphs];
    if (total > 0 && rowptr[total] > 0 && !col)
      return desco::fail(DESCO_EINVAL, "desco_edge_orbit_counts: bad argument");
    std::vector<int64_t> lower_start((size_t)total + 1, 0);
    for (int64_t v = 0; v < total; ++v) {
      int64_t e = rowptr[v];
      while (e < rowptr[v + 1] && col[e] < v) ++e;
      lower_start[v + 1] = lower_start[v] + (e - rowptr[v]);
    }
    std::memset(out, 0, sizeof(int64_t) * (size_t)lower_start[total] * (size_t)cols);
    if (cols == 0 || lower_start[total] == 0) return 0;
    if (!desco::esu_enumerate_graphs(graph_ptr, num_graphs, rowptr, col, kmax, num_threads, [&] {
          return EdgeOrbitVisitor{table.data(), rowptr, col, lower_start.data(), out, cols, {}, -1, 0};
        }))
      return desco::fail(DESCO_ENOMEM, "desco_edge_orbit_counts: out of memory");
    return 0;
  } catch (const std::bad_alloc&) {
    return desco::fail(DESCO_ENOMEM, "desco_edge_orbit_counts: out of memory");
  }
}
