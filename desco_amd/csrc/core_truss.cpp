// Host twin of core_truss_dev.hip (C ABI: desco_core_truss), see include/desco_hip.h, "CORE / TRUSS".
//
// k-core and k-truss decomposition of every graph of a set, OpenMP over graphs.  Both decompositions are unique -- they
// do not depend on the order in which nodes or edges of a level are peeled -- so this sequential peel and the kernel's
// parallel one return the same integers.
//   core   Batagelj-Zaversnik: the nodes bucket-sorted by remaining degree, O(n + m).
//   truss  the support of an edge by merging the two sorted rows; then level by level: the live edges of support
//          <= k - 2 are queued; a popped edge gets truss number k and every triangle it still closes (both other edges
//          not popped yet) is destroyed, which takes one from the support of the two others and queues one that falls
//          to the level; an empty queue raises k to the smallest live support + 2.
#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/desco_hip.h"
#include "common_host.hpp"

namespace {

struct Scratch {
  std::vector<int32_t> deg, pos, vert, bin;              // core
  std::vector<int32_t> eid, ea, eb, sup, queue;          // truss: edge row of every entry, ends, support
  std::vector<uint8_t> state;                            // 0 live, 1 queued, 2 popped
};

// core numbers of the graph on nodes [n0, n0 + n) into core[n0 ..]
void core_peel(const int64_t* rowptr, const int32_t* col, int64_t n0, int64_t n, Scratch& s, int32_t* core) {
  s.deg.resize((size_t)n), s.pos.resize((size_t)n), s.vert.resize((size_t)n);
  int32_t md = 0;
  for (int64_t v = 0; v < n; ++v) {
    s.deg[v] = (int32_t)(rowptr[n0 + v + 1] - rowptr[n0 + v]);
    md = std::max(md, s.deg[v]);
  }
  s.bin.assign((size_t)md + 2, 0);
  for (int64_t v = 0; v < n; ++v) ++s.bin[s.deg[v] + 1];
  for (int32_t d = 0; d <= md; ++d) s.bin[d + 1] += s.bin[d];          // bin[d] = first position of degree d
  {
    std::vector<int32_t>& next = s.queue;
    next.assign(s.bin.begin(), s.bin.end());
    for (int64_t v = 0; v < n; ++v) {
      s.pos[v] = next[s.deg[v]]++;
      s.vert[s.pos[v]] = (int32_t)v;
    }
  }
  for (int64_t i = 0; i < n; ++i) {
    const int32_t v = s.vert[i];
    core[n0 + v] = s.deg[v];
    for (int64_t e = rowptr[n0 + v]; e < rowptr[n0 + v + 1]; ++e) {
      const int32_t u = (int32_t)(col[e] - n0);
      if (s.deg[u] > s.deg[v]) {                                        // move u to the front of its bucket, one down
        const int32_t du = s.deg[u], pu = s.pos[u], pw = s.bin[du], w = s.vert[pw];
        if (u != w) s.pos[u] = pw, s.vert[pw] = u, s.pos[w] = pu, s.vert[pu] = w;
        ++s.bin[du];
        --s.deg[u];
      }
    }
  }
}

// support and truss numbers of the graph on nodes [n0, n0 + n): rows [r0, r0 + m) of support / truss (either may be null)
void truss_peel(const int64_t* rowptr, const int32_t* col, int64_t n0, int64_t n, Scratch& s, int32_t* support,
                int32_t* truss) {
  const int64_t e0 = rowptr[n0], m = (rowptr[n0 + n] - e0) / 2, r0 = e0 / 2;
  if (m == 0) return;
  s.eid.resize((size_t)(2 * m)), s.ea.resize((size_t)m), s.eb.resize((size_t)m), s.sup.assign((size_t)m, 0);
  int32_t k = 0;
  for (int64_t v = 0; v < n; ++v)                        // the lower entries (v, u), u < v, in CSR order are the rows
    for (int64_t e = rowptr[n0 + v]; e < rowptr[n0 + v + 1] && col[e] - n0 < v; ++e)
      s.eid[e - e0] = k, s.ea[k] = (int32_t)(col[e] - n0), s.eb[k] = (int32_t)v, ++k;
  for (int64_t v = 0; v < n; ++v)                        // an upper entry (v, u), u > v, takes the row of its twin (u, v)
    for (int64_t e = rowptr[n0 + v + 1] - 1; e >= rowptr[n0 + v] && col[e] - n0 > v; --e) {
      const int32_t* r = col + rowptr[col[e]];
      s.eid[e - e0] = s.eid[(std::lower_bound(r, col + rowptr[col[e] + 1], (int32_t)(n0 + v)) - col) - e0];
    }
  // calls f(edge of (a, w), edge of (b, w)) for every common neighbour w of a and b
  auto triangles = [&](int32_t a, int32_t b, auto&& f) {
    int64_t i = rowptr[n0 + a], i1 = rowptr[n0 + a + 1], j = rowptr[n0 + b], j1 = rowptr[n0 + b + 1];
    while (i < i1 && j < j1) {
      const int32_t x = col[i], y = col[j];
      if (x == y) f(s.eid[i - e0], s.eid[j - e0]);
      i += x <= y;
      j += y <= x;
    }
  };
  for (int64_t e = 0; e < m; ++e) triangles(s.ea[e], s.eb[e], [&](int32_t, int32_t) { ++s.sup[e]; });
  if (support) std::copy(s.sup.begin(), s.sup.end(), support + r0);
  if (!truss) return;
  s.state.assign((size_t)m, 0);
  s.queue.clear();
  int64_t left = m;
  int32_t level = 2;
  while (left > 0) {
    int32_t lo = INT32_MAX;
    for (int64_t e = 0; e < m; ++e)
      if (s.state[e] == 0) lo = std::min(lo, s.sup[e]);
    level = std::max(level, lo + 2);
    for (int64_t e = 0; e < m; ++e)
      if (s.state[e] == 0 && s.sup[e] <= level - 2) s.state[e] = 1, s.queue.push_back((int32_t)e);
    for (size_t q = 0; q < s.queue.size(); ++q) {
      const int32_t e = s.queue[q];
      truss[r0 + e] = level;
      triangles(s.ea[e], s.eb[e], [&](int32_t e1, int32_t e2) {
        if (s.state[e1] == 2 || s.state[e2] == 2) return;              // the triangle went with an earlier edge
        for (const int32_t x : {e1, e2})
          if (--s.sup[x] <= level - 2 && s.state[x] == 0) s.state[x] = 1, s.queue.push_back(x);
      });
      s.state[e] = 2;
    }
    left -= (int64_t)s.queue.size();
    s.queue.clear();
  }
}

// what is wrong with the rows of the graph on nodes [n0, n1), or nullptr (rowptr is monotone by now)
const char* check_graph(const int64_t* rowptr, const int32_t* col, int64_t n0, int64_t n1) {
  for (int64_t v = n0; v < n1; ++v) {
    for (int64_t e = rowptr[v]; e < rowptr[v + 1]; ++e) {
      const int64_t u = col[e];
      if (u < n0 || u >= n1) return "desco_core_truss: col holds an id outside the node's graph";
      if (u == v) return "desco_core_truss: col holds a loop";
      if (e > rowptr[v] && col[e - 1] >= u) return "desco_core_truss: a row is not strictly ascending (unsorted)";
    }
  }
  for (int64_t v = n0; v < n1; ++v)            // (the ids are in range by now)
    for (int64_t e = rowptr[v]; e < rowptr[v + 1]; ++e) {
      const int32_t* r0 = col + rowptr[col[e]];
      const int32_t* r1 = col + rowptr[col[e] + 1];
      if (!std::binary_search(r0, r1, (int32_t)v)) return "desco_core_truss: the adjacency is asymmetric";
    }
  return nullptr;
}

}  // namespace

extern "C" int desco_core_truss(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col,
                                int64_t num_graphs, int num_threads, int32_t* core_out, int32_t* truss_out,
                                int32_t* support_out) {
  if (num_graphs < 0) return desco::fail(DESCO_EINVAL, "desco_core_truss: negative num_graphs");
  if (num_graphs == 0) return 0;
  if (!graph_ptr) return desco::fail(DESCO_EINVAL, "desco_core_truss: graph_ptr is null");
  if (!rowptr) return desco::fail(DESCO_EINVAL, "desco_core_truss: rowptr is null");
  if (graph_ptr[0] != 0) return desco::fail(DESCO_EINVAL, "desco_core_truss: graph_ptr does not start at 0");
  for (int64_t g = 0; g < num_graphs; ++g)
    if (graph_ptr[g + 1] < graph_ptr[g]) return desco::fail(DESCO_EINVAL, "desco_core_truss: graph_ptr is not monotone");
  const int64_t N = graph_ptr[num_graphs];
  if (N > INT32_MAX) return desco::fail(DESCO_EINVAL, "desco_core_truss: more than 2^31 - 1 nodes");
  if (rowptr[0] != 0) return desco::fail(DESCO_EINVAL, "desco_core_truss: rowptr does not start at 0");
  for (int64_t v = 0; v < N; ++v)              // (before any row is read: monotone offsets end within col's E entries)
    if (rowptr[v + 1] < rowptr[v]) return desco::fail(DESCO_EINVAL, "desco_core_truss: rowptr is not monotone");
  const int64_t E = rowptr[N];
  if (E > INT32_MAX) return desco::fail(DESCO_EINVAL, "desco_core_truss: more than 2^31 - 1 adjacency entries");
  if (E > 0 && !col) return desco::fail(DESCO_EINVAL, "desco_core_truss: col is null");
  int nt = 1;
#ifdef _OPENMP
  nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#endif
  (void)num_threads;
  const char* bad = nullptr;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 8) num_threads(nt)
#endif
  for (int64_t g = 0; g < num_graphs; ++g) {
    const char* why = check_graph(rowptr, col, graph_ptr[g], graph_ptr[g + 1]);
    if (why) {
#ifdef _OPENMP
#pragma omp critical(desco_core_truss_bad)
#endif
      bad = why;
    }
  }
  if (bad) return desco::fail(DESCO_EINVAL, bad);
  if (!core_out && !truss_out && !support_out) return 0;

  bool no_memory = false;
#ifdef _OPENMP
#pragma omp parallel num_threads(nt)
#endif
  {
    Scratch s;
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 4)
#endif
    for (int64_t g = 0; g < num_graphs; ++g) {
      const int64_t n0 = graph_ptr[g], n = graph_ptr[g + 1] - n0;
      try {
        if (core_out) core_peel(rowptr, col, n0, n, s, core_out);
        if (truss_out || support_out) truss_peel(rowptr, col, n0, n, s, support_out, truss_out);
      } catch (const std::bad_alloc&) {
#ifdef _OPENMP
#pragma omp atomic write
#endif
        no_memory = true;
      }
    }
  }
  if (no_memory) return desco::fail(DESCO_ENOMEM, "desco_core_truss: out of memory for a graph's peel");
  return 0;
}
