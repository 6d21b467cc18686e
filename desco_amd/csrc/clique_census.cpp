// Host twins of clique_census_dev.hip (C ABI: desco_peel_order, desco_clique_census), see include/desco_hip.h, "CLIQUE
// CENSUS".  OpenMP over graphs; a graph has one owner, so the tallies are plain sums.
//   peel    level-synchronous core peel with a frontier: the nodes of remaining degree <= k at the start of a pass leave
//           together and take one from each neighbour; the next frontier of the level is whoever fell to <= k; when it is
//           empty the level rises to the smallest live degree.  O(m + levels * n).  key = the index of the pass.
//   census  pivoting on the subgraph induced by every root's out-neighbours: multi-word bitset rows, one candidate set per
//           recursion depth, Pascal rows mod 2^64 up to the largest out-degree (columns 0 .. 64).  No branch is cut, so
//           omega is exact for any kmax.
#include <algorithm>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/desco_hip.h"
#include "clique_census.hpp"
#include "common_host.hpp"

namespace {

using desco::clique_census::kMaxK;

// what is wrong with the rows of the graph on nodes [n0, n1), or nullptr (rowptr is monotone by now)
const char* check_graph(const int64_t* rowptr, const int32_t* col, int64_t n0, int64_t n1) {
  for (int64_t v = n0; v < n1; ++v) {
    for (int64_t e = rowptr[v]; e < rowptr[v + 1]; ++e) {
      const int64_t u = col[e];
      if (u < n0 || u >= n1) return "col holds an id outside the node's graph";
      if (u == v) return "col holds a loop";
      if (e > rowptr[v] && col[e - 1] >= u) return "a row is not strictly ascending (unsorted)";
    }
  }
  for (int64_t v = n0; v < n1; ++v)            // (the ids are in range by now)
    for (int64_t e = rowptr[v]; e < rowptr[v + 1]; ++e) {
      const int32_t* r0 = col + rowptr[col[e]];
      const int32_t* r1 = col + rowptr[col[e] + 1];
      if (!std::binary_search(r0, r1, (int32_t)v)) return "the adjacency is asymmetric";
    }
  return nullptr;
}

int fail_named(const char* who, const char* what) {
  const std::string m = std::string(who) + ": " + what;
  return desco::fail(DESCO_EINVAL, m.c_str());
}

// the checks desco_core_truss makes, under the name `who`; 0, or the code of the failure that was reported
int check_set(const char* who, const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, int64_t num_graphs,
              int nt) {
  if (!graph_ptr) return fail_named(who, "graph_ptr is null");
  if (!rowptr) return fail_named(who, "rowptr is null");
  if (graph_ptr[0] != 0) return fail_named(who, "graph_ptr does not start at 0");
  for (int64_t g = 0; g < num_graphs; ++g)
    if (graph_ptr[g + 1] < graph_ptr[g]) return fail_named(who, "graph_ptr is not monotone");
  const int64_t N = graph_ptr[num_graphs];
  if (N > INT32_MAX) return fail_named(who, "more than 2^31 - 1 nodes");
  if (rowptr[0] != 0) return fail_named(who, "rowptr does not start at 0");
  for (int64_t v = 0; v < N; ++v)              // (before any row is read: monotone offsets end within col's E entries)
    if (rowptr[v + 1] < rowptr[v]) return fail_named(who, "rowptr is not monotone");
  const int64_t E = rowptr[N];
  if (E > INT32_MAX) return fail_named(who, "more than 2^31 - 1 adjacency entries");
  if (E > 0 && !col) return fail_named(who, "col is null");
  const char* bad = nullptr;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 8) num_threads(nt)
#endif
  for (int64_t g = 0; g < num_graphs; ++g) {
    const char* why = check_graph(rowptr, col, graph_ptr[g], graph_ptr[g + 1]);
    if (why) {
#ifdef _OPENMP
#pragma omp critical(desco_clique_census_bad)
#endif
      bad = why;
    }
  }
  (void)nt;
  return bad ? fail_named(who, bad) : 0;
}

int thread_count(int num_threads) {
#ifdef _OPENMP
  return num_threads > 0 ? num_threads : omp_get_max_threads();
#else
  (void)num_threads;
  return 1;
#endif
}

struct PeelScratch {
  std::vector<int32_t> deg, front, next;
};

// pass index (key) and level (core, may be null) of every node of the graph on [n0, n0 + n); both point at the graph's
// first node
void peel(const int64_t* rowptr, const int32_t* col, int64_t n0, int64_t n, PeelScratch& s, int32_t* key, int32_t* core) {
  s.deg.resize((size_t)n);
  for (int64_t v = 0; v < n; ++v) s.deg[v] = (int32_t)(rowptr[n0 + v + 1] - rowptr[n0 + v]);
  int64_t left = n;
  int32_t k = 0, pass = 0;
  s.front.clear();
  while (left > 0) {
    if (s.front.empty()) {                     // a new level: the smallest live degree, and everybody at or below it
      int32_t lo = INT32_MAX;
      for (int64_t v = 0; v < n; ++v)
        if (s.deg[v] >= 0) lo = std::min(lo, s.deg[v]);
      k = std::max(k, lo);
      for (int64_t v = 0; v < n; ++v)
        if (s.deg[v] >= 0 && s.deg[v] <= k) s.front.push_back((int32_t)v);
    }
    for (const int32_t v : s.front) {          // the pass: all of them leave on the degrees of its start
      key[v] = pass;
      if (core) core[v] = k;
      s.deg[v] = -1;
    }
    s.next.clear();
    for (const int32_t v : s.front)
      for (int64_t e = rowptr[n0 + v]; e < rowptr[n0 + v + 1]; ++e) {
        const int32_t u = (int32_t)(col[e] - n0);
        if (s.deg[u] < 0) continue;
        if (s.deg[u]-- == k + 1) s.next.push_back(u);          // falls to the level exactly once
      }
    left -= (int64_t)s.front.size();
    s.front.swap(s.next);
    ++pass;
  }
}

struct CensusScratch {
  PeelScratch peel;
  std::vector<int32_t> key;                    // of the graph, when none was given
  std::vector<int32_t> pos;                    // local node -> index among the root's out-neighbours, or -1
  std::vector<int32_t> out;                    // the root's out-neighbours, local ids ascending
  std::vector<uint64_t> rows, sets;            // d rows and d + 2 candidate sets of W words
  std::vector<int32_t> held, piv;
  std::vector<uint64_t> binom;                 // (rows_built) x (kMaxK + 1), mod 2^64
  int64_t rows_built = 0;
  // the walk's view of the current root
  int W = 0, kmax = 0;
  int32_t omega = 0;
  uint64_t* root_col = nullptr;                // the graph's tallies [kmax]
  uint64_t* node_col = nullptr;                // node_cliques of the graph's first node, or null
  int64_t root = 0;

  void pascal(int64_t top) {                   // rows 0 .. top
    if (top < rows_built) return;
    binom.resize((size_t)(top + 1) * (kMaxK + 1), 0);
    for (int64_t n = rows_built; n <= top; ++n) {
      uint64_t* r = binom.data() + n * (kMaxK + 1);
      const uint64_t* above = n ? r - (kMaxK + 1) : nullptr;
      r[0] = 1;
      for (int j = 1; j <= kMaxK; ++j) r[j] = above ? above[j] + above[j - 1] : 0;
    }
    rows_built = top + 1;
  }
  uint64_t C(int64_t n, int64_t j) const { return n < 0 || j < 0 || j > kMaxK ? 0 : binom[(size_t)n * (kMaxK + 1) + j]; }

  void leaf() {
    const int r = 1 + (int)held.size(), p = (int)piv.size();
    omega = std::max(omega, r + p);
    for (int k = r; k <= std::min(r + p, kmax); ++k) {
      const uint64_t c = C(p, k - r);
      root_col[k - 1] += c;
      if (!node_col) continue;
      node_col[root * kmax + k - 1] += c;
      for (const int32_t h : held) node_col[(int64_t)out[h] * kmax + k - 1] += c;
      if (k > r) {
        const uint64_t c2 = C(p - 1, k - r - 1);
        for (const int32_t q : piv) node_col[(int64_t)out[q] * kmax + k - 1] += c2;
      }
    }
  }

  void walk(int depth) {
    uint64_t* P = sets.data() + (size_t)depth * W;
    int u = -1, best = -1;
    for (int w = 0; w < W; ++w)
      for (uint64_t bits = P[w]; bits; bits &= bits - 1) {
        const int i = w * 64 + __builtin_ctzll(bits);
        const uint64_t* r = rows.data() + (size_t)i * W;
        int c = 0;
        for (int x = 0; x < W; ++x) c += __builtin_popcountll(P[x] & r[x]);
        if (c > best) best = c, u = i;
      }
    if (u < 0) return leaf();
    uint64_t* child = P + W;
    const uint64_t* ru = rows.data() + (size_t)u * W;
    for (int x = 0; x < W; ++x) child[x] = P[x] & ru[x];
    piv.push_back(u);
    walk(depth + 1);
    piv.pop_back();
    P[u >> 6] &= ~(uint64_t(1) << (u & 63));
    for (int w = 0; w < W; ++w)
      for (uint64_t bits = P[w] & ~ru[w]; bits; bits &= bits - 1) {
        const int i = w * 64 + __builtin_ctzll(bits);
        const uint64_t* ri = rows.data() + (size_t)i * W;
        for (int x = 0; x < W; ++x) child[x] = P[x] & ri[x];
        held.push_back(i);
        walk(depth + 1);
        held.pop_back();
        P[w] &= ~(uint64_t(1) << (i & 63));
      }
  }
};

// the census of the graph on nodes [n0, n0 + n) under key (of the graph's nodes)
void census(const int64_t* rowptr, const int32_t* col, const int32_t* key, int64_t n0, int64_t n, int kmax,
            CensusScratch& s, uint64_t* graph_col, uint64_t* node_col, int32_t* omega) {
  auto after = [&](int64_t u, int64_t v) { return key[u] > key[v] || (key[u] == key[v] && u > v); };      // local ids
  s.kmax = kmax, s.omega = 0, s.root_col = graph_col, s.node_col = node_col;
  s.pos.assign((size_t)n, -1);
  for (int64_t v = 0; v < n; ++v) {
    s.out.clear();
    for (int64_t e = rowptr[n0 + v]; e < rowptr[n0 + v + 1]; ++e)
      if (after(col[e] - n0, v)) s.out.push_back((int32_t)(col[e] - n0));
    const int d = (int)s.out.size();
    const int W = std::max((d + 63) / 64, 1);
    s.W = W, s.root = v;
    s.pascal(d);
    s.rows.assign((size_t)d * W, 0);
    s.sets.assign((size_t)(d + 2) * W, 0);
    for (int i = 0; i < d; ++i) s.pos[s.out[i]] = i;
    for (int i = 0; i < d; ++i) {
      const int64_t w = n0 + s.out[i];
      for (int64_t e = rowptr[w]; e < rowptr[w + 1]; ++e) {
        const int32_t j = s.pos[col[e] - n0];
        if (j >= 0) s.rows[(size_t)i * W + (j >> 6)] |= uint64_t(1) << (j & 63);
      }
    }
    for (int i = 0; i < d; ++i) s.sets[i >> 6] |= uint64_t(1) << (i & 63);
    s.held.clear(), s.piv.clear();
    s.walk(0);
    for (int i = 0; i < d; ++i) s.pos[s.out[i]] = -1;
  }
  if (omega) *omega = s.omega;
}

}  // namespace

extern "C" int desco_peel_order(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, int64_t num_graphs,
                                int num_threads, int32_t* key_out, int32_t* core_out) {
  const char* who = "desco_peel_order";
  if (num_graphs < 0) return fail_named(who, "negative num_graphs");
  if (num_graphs == 0) return 0;
  const int nt = thread_count(num_threads);
  if (const int rc = check_set(who, graph_ptr, rowptr, col, num_graphs, nt)) return rc;
  if (graph_ptr[num_graphs] > 0 && !key_out) return fail_named(who, "key_out is null");
  bool no_memory = false;
#ifdef _OPENMP
#pragma omp parallel num_threads(nt)
#endif
  {
    PeelScratch s;
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 4)
#endif
    for (int64_t g = 0; g < num_graphs; ++g) {
      try {
        peel(rowptr, col, graph_ptr[g], graph_ptr[g + 1] - graph_ptr[g], s, key_out + graph_ptr[g],
             core_out ? core_out + graph_ptr[g] : nullptr);
      } catch (const std::bad_alloc&) {
#ifdef _OPENMP
#pragma omp atomic write
#endif
        no_memory = true;
      }
    }
  }
  if (no_memory) return desco::fail(DESCO_ENOMEM, "desco_peel_order: out of memory for a graph's peel");
  return 0;
}

extern "C" int desco_clique_census(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col,
                                   int64_t num_graphs, const int32_t* key, int kmax, int num_threads,
                                   int64_t* graph_cliques, int64_t* node_cliques, int32_t* omega) {
  const char* who = "desco_clique_census";
  if (num_graphs < 0) return fail_named(who, "negative num_graphs");
  if (kmax < 1 || kmax > DESCO_CLIQUE_MAX_K) return fail_named(who, "kmax is outside 1..DESCO_CLIQUE_MAX_K (64)");
  if (num_graphs == 0) return 0;
  const int nt = thread_count(num_threads);
  if (const int rc = check_set(who, graph_ptr, rowptr, col, num_graphs, nt)) return rc;
  const int64_t N = graph_ptr[num_graphs];
  if (key)
    for (int64_t v = 0; v < N; ++v)
      if (key[v] < 0) return fail_named(who, "key holds a negative value");
  if (!graph_cliques && !node_cliques && !omega) return 0;
  bool no_memory = false;
#ifdef _OPENMP
#pragma omp parallel num_threads(nt)
#endif
  {
    CensusScratch s;
    std::vector<uint64_t> totals((size_t)kmax);
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1)
#endif
    for (int64_t g = 0; g < num_graphs; ++g) {
      const int64_t n0 = graph_ptr[g], n = graph_ptr[g + 1] - n0;
      try {
        const int32_t* k = key ? key + n0 : nullptr;
        if (!k) {
          s.key.resize((size_t)n);
          peel(rowptr, col, n0, n, s.peel, s.key.data(), nullptr);
          k = s.key.data();
        }
        std::fill(totals.begin(), totals.end(), 0);
        uint64_t* nodes = node_cliques ? reinterpret_cast<uint64_t*>(node_cliques) + n0 * kmax : nullptr;
        if (nodes) std::fill(nodes, nodes + n * kmax, 0);
        census(rowptr, col, k, n0, n, kmax, s, totals.data(), nodes, omega ? omega + g : nullptr);
        if (graph_cliques) std::copy(totals.begin(), totals.end(), reinterpret_cast<uint64_t*>(graph_cliques) + g * kmax);
      } catch (const std::bad_alloc&) {
#ifdef _OPENMP
#pragma omp atomic write
#endif
        no_memory = true;
      }
    }
  }
  if (no_memory) return desco::fail(DESCO_ENOMEM, "desco_clique_census: out of memory for a graph's census");
  return 0;
}
