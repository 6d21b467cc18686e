// Exact canonical ground-truth counts (C ABI: desco_canonical_counts), SURVEY.md 8f row N1.
//
// count[v][q] = number of node subsets S with max(S) = v whose INDUCED subgraph is isomorphic to
// query q -- what the reference obtains by running networkx VF2 (MatchSubgraphWorker,
// workload.py:327-348: one match per automorphism, keyed by max(vmap.keys())) and dividing by the
// query's symmetry factor (data.py:61-67).  Written from that definition with the ESU enumeration
// (every connected node subset of size <= kmax is visited exactly once, rooted at its maximum id)
// and an isomorphism-class lookup over induced adjacency bitmasks (<= 6 nodes -> <= 15 bits).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/desco_hip.h"
#include "common_host.hpp"

namespace {

constexpr int KMAX = 6;

inline int pair_bit(int a, int b) { return b * (b - 1) / 2 + a; }   // a < b

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

struct Ctx {
  int64_t base, n;
  const int64_t* rowptr;
  const int32_t* col;
  int kmax;
  const std::vector<uint16_t>* canon;               // [k] -> table
  const std::vector<std::vector<int>>* cls2q;       // [k][canonical mask] -> query ids (flattened below)
  const std::vector<int32_t>* qlist;                 // per k: offsets into qids
  std::vector<uint64_t> bits;                        // adjacency bitset rows (n x words)
  int words;
  std::vector<uint8_t> seen;
  int64_t* out;
  int num_q;
  const int16_t* orbit = nullptr;                    // orbit table (desco_orbit_table) or null: canonical counts
  bool adj(int a, int b) const { return bits[(size_t)a * words + (b >> 6)] >> (b & 63) & 1; }
};

struct Classifier {
  // for size k: map canonical mask -> list of query indices
  std::vector<std::vector<int>> by_mask[KMAX + 1];
  std::vector<uint16_t> canon[KMAX + 1];
  bool used[KMAX + 1] = {false};
};

// class-table offsets of the device enumerator: the masks of k nodes start at ORB_OFF[k] (k = 2..5)
constexpr int ORB_KMAX = 5, ORB_ENTRIES = 1098;
constexpr int ORB_OFF[ORB_KMAX + 2] = {0, 0, 0, 2, 10, 74, ORB_ENTRIES};

void classify(const Ctx& c, const Classifier& cl, const int* sub, int k, int v) {
  if (!c.orbit && !cl.used[k]) return;
  uint32_t m = 0;
  for (int b = 1; b < k; ++b)
    for (int a = 0; a < b; ++a)
      if (c.adj(sub[a], sub[b])) m |= 1u << pair_bit(a, b);
  if (c.orbit) {                                     // orbit counts: every member, by the column of its position
    if (k < 2) return;
    const int16_t* row = c.orbit + (size_t)(ORB_OFF[k] + m) * ORB_KMAX;
    if (row[0] < 0) return;
    for (int i = 0; i < k; ++i) c.out[(c.base + sub[i]) * c.num_q + row[i]] += 1;
    return;
  }
  const auto& lst = cl.by_mask[k][cl.canon[k][m]];
  for (int q : lst) c.out[(c.base + v) * c.num_q + q] += 1;
}

void extend(Ctx& c, const Classifier& cl, int* sub, int nsub, std::vector<int>& ext, int v) {
  classify(c, cl, sub, nsub, v);
  if (nsub == c.kmax) return;
  std::vector<int> newly, ext2;
  while (!ext.empty()) {
    const int w = ext.back();
    ext.pop_back();
    newly.clear();
    const int64_t gw = c.base + w;
    for (int64_t e = c.rowptr[gw]; e < c.rowptr[gw + 1]; ++e) {
      const int u = (int)(c.col[e] - c.base);
      if (u >= v) break;                       // rows sorted ascending; only ids below the root
      if (!c.seen[u]) {
        c.seen[u] = 1;
        newly.push_back(u);
      }
    }
    ext2 = ext;
    ext2.insert(ext2.end(), newly.begin(), newly.end());
    sub[nsub] = w;
    extend(c, cl, sub, nsub + 1, ext2, v);
    for (int u : newly) c.seen[u] = 0;
  }
}

// ESU over every graph (OpenMP over graphs: a graph's rows are written by one thread only, so the result does not
// depend on the number of threads).  `orbit` null: canonical counts through `cl`; else orbit counts through the table.
void enumerate_graphs(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr, const int32_t* col,
                      const Classifier& cl, const int16_t* orbit, int kmax, int num_cols, int num_threads,
                      int64_t* out) {
#ifdef _OPENMP
  const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
  const int nt = 1;
  (void)num_threads;
#endif
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
  for (int64_t g = 0; g < num_graphs; ++g) {
    Ctx c;
    c.base = graph_ptr[g];
    c.n = graph_ptr[g + 1] - c.base;
    c.rowptr = rowptr;
    c.col = col;
    c.kmax = kmax;
    c.out = out;
    c.num_q = num_cols;
    c.orbit = orbit;
    c.words = (int)((c.n + 63) / 64);
    c.bits.assign((size_t)c.n * c.words, 0);
    for (int64_t u = 0; u < c.n; ++u)
      for (int64_t e = rowptr[c.base + u]; e < rowptr[c.base + u + 1]; ++e) {
        const int w = (int)(col[e] - c.base);
        c.bits[(size_t)u * c.words + (w >> 6)] |= (uint64_t)1 << (w & 63);
      }
    c.seen.assign((size_t)c.n, 0);
    int sub[KMAX];
    std::vector<int> ext;
    for (int v = 0; v < (int)c.n; ++v) {
      ext.clear();
      c.seen[v] = 1;
      const int64_t gv = c.base + v;
      for (int64_t e = rowptr[gv]; e < rowptr[gv + 1]; ++e) {
        const int u = (int)(col[e] - c.base);
        if (u >= v) break;
        c.seen[u] = 1;
        ext.push_back(u);
      }
      std::vector<int> marked = ext;
      sub[0] = v;
      extend(c, cl, sub, 1, ext, v);
      for (int u : marked) c.seen[u] = 0;
      c.seen[v] = 0;
    }
  }
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
      for (int e = q_edge_ptr[q]; e < q_edge_ptr[q + 1]; ++e) {
        int a = q_edges[2 * e], b = q_edges[2 * e + 1];
        if (a == b || a < 0 || b < 0 || a >= k || b >= k)
          return desco::fail(DESCO_EINVAL, "desco_canonical_counts: bad query edge");
        if (a > b) std::swap(a, b);
        m |= 1u << pair_bit(a, b);
      }
      cl.by_mask[k][cl.canon[k][m]].push_back(q);
    }
    const int64_t total = graph_ptr[num_graphs];
    std::memset(out, 0, sizeof(int64_t) * (size_t)total * (size_t)num_queries);
    if (num_queries == 0) return 0;
    enumerate_graphs(graph_ptr, num_graphs, rowptr, col, cl, nullptr, kmax, num_queries, num_threads, out);
    return 0;
  } catch (const std::bad_alloc&) {
    return desco::fail(DESCO_ENOMEM, "desco_canonical_counts: out of memory");
  }
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
  for (int i = 0; i < ORB_ENTRIES * ORB_KMAX; ++i) table[i] = -1;
  int kmax = 0, cols = 0;
  std::vector<int16_t> owner(ORB_ENTRIES, -1);
  for (int q = 0; q < num_queries; ++q) {
    const int k = q_nodes[q];
    if (k < 2 || k > ORB_KMAX) return desco::fail(DESCO_EINVAL, "desco_orbit_table: orbit counts take queries of 2..5 nodes");
    if (q >= 32767) return desco::fail(DESCO_EINVAL, "desco_orbit_table: too many queries");
    kmax = std::max(kmax, k);
    uint32_t m = 0;
    for (int e = q_edge_ptr[q]; e < q_edge_ptr[q + 1]; ++e) {
      int a = q_edges[2 * e], b = q_edges[2 * e + 1];
      if (a == b || a < 0 || b < 0 || a >= k || b >= k)
        return desco::fail(DESCO_EINVAL, "desco_orbit_table: bad query edge");
      if (a > b) std::swap(a, b);
      m |= 1u << pair_bit(a, b);
    }
    uint32_t reach = 1;                              // positions reachable from position 0
    for (int it = 0; it < k; ++it)
      for (int b = 1; b < k; ++b)
        for (int a = 0; a < b; ++a)
          if ((m >> pair_bit(a, b) & 1) && ((reach >> a | reach >> b) & 1)) reach |= 1u << a | 1u << b;
    if (reach != (1u << k) - 1) return desco::fail(DESCO_EINVAL, "desco_orbit_table: a query is not connected");
    // every relabeling p of the query (position a becomes subset position p[a]); those that keep the mask are Aut(q)
    int perm[ORB_KMAX], orbit_min[ORB_KMAX];
    for (int i = 0; i < k; ++i) perm[i] = orbit_min[i] = i;
    std::vector<uint32_t> images;
    std::vector<int> perms;
    do {
      uint32_t r = 0;
      for (int b = 1; b < k; ++b)
        for (int a = 0; a < b; ++a)
          if (m >> pair_bit(a, b) & 1) r |= 1u << pair_bit(std::min(perm[a], perm[b]), std::max(perm[a], perm[b]));
      images.push_back(r);
      perms.insert(perms.end(), perm, perm + k);
      if (r == m)
        for (int i = 0; i < k; ++i) orbit_min[i] = std::min(orbit_min[i], perm[i]);   // (Aut is a group: min is exact)
    } while (std::next_permutation(perm, perm + k));
    int orbit_of[ORB_KMAX], n_orb = 0;               // numbered in ascending order of the smallest member
    for (int i = 0; i < k; ++i)
      if (orbit_min[i] == i) orbit_of[i] = n_orb++;
    for (int i = 0; i < k; ++i) orbit_of[i] = orbit_of[orbit_min[i]];
    if (cols + n_orb > 32767) return desco::fail(DESCO_EINVAL, "desco_orbit_table: too many columns");
    for (size_t t = 0; t < images.size(); ++t) {
      const int slot = ORB_OFF[k] + (int)images[t];
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
    std::vector<int16_t> table((size_t)ORB_ENTRIES * ORB_KMAX);
    int cols = 0, kmax = 0;
    if (const int rc = desco_orbit_table(q_nodes, q_edge_ptr, q_edges, num_queries, table.data(), &cols, &kmax))
      return rc;
    std::memset(out, 0, sizeof(int64_t) * (size_t)graph_ptr[num_graphs] * (size_t)cols);
    if (cols == 0) return 0;
    enumerate_graphs(graph_ptr, num_graphs, rowptr, col, Classifier(), table.data(), kmax, cols, num_threads, out);
    return 0;
  } catch (const std::bad_alloc&) {
    return desco::fail(DESCO_ENOMEM, "desco_orbit_counts: out of memory");
  }
}
