// Host twin of null_model_dev.hip (C ABI: desco_null_model_rewire, desco_null_model_draw), see include/desco_hip.h.
//
// Degree-preserving null model: every (graph, replica) pair is one sequential Markov chain of double edge switches
// whose draws come from a counter-based generator (null_model.hpp), so that a chain has exactly one result whoever
// runs it.  Chains run in parallel (OpenMP, dynamic); a chain keeps its graph's adjacency as bitset rows over local
// node ids and its edge slots as two int32 arrays, and at the end reads the new rows off the bitset, ascending.
#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/desco_hip.h"
#include "common_host.hpp"
#include "null_model.hpp"

namespace {

using desco::null_model::Draw;

struct Scratch {
  std::vector<uint64_t> bits;
  std::vector<int32_t> sa, sb;
};

// one chain; returns the accepted switches.  out = the graph's entries of one replica's col (global ids)
int32_t run_chain(const int64_t* rowptr, const int32_t* col, int64_t n0, int64_t n, uint64_t seed, uint32_t graph,
                  uint32_t replica, int64_t swaps_per_edge, Scratch& s, int32_t* out_col) {
  const int64_t e0 = rowptr[n0], e1 = rowptr[n0 + n];
  const int64_t m = (e1 - e0) / 2;
  if (m < 2 || swaps_per_edge == 0) {
    std::copy(col + e0, col + e1, out_col + e0);
    return 0;
  }
  const int64_t W = (n + 63) >> 6;
  s.bits.assign((size_t)(n * W), 0ull);
  s.sa.resize((size_t)m);
  s.sb.resize((size_t)m);
  int64_t k = 0;
  for (int64_t v = 0; v < n; ++v)
    for (int64_t e = rowptr[n0 + v]; e < rowptr[n0 + v + 1]; ++e) {
      const int64_t u = col[e] - n0;
      s.bits[v * W + (u >> 6)] |= 1ull << (u & 63);
      if (u < v) s.sa[k] = (int32_t)u, s.sb[k] = (int32_t)v, ++k;
    }
  auto has = [&](int64_t x, int64_t y) { return (s.bits[x * W + (y >> 6)] >> (y & 63)) & 1ull; };
  auto flip_pair = [&](int64_t x, int64_t y) {
    s.bits[x * W + (y >> 6)] ^= 1ull << (y & 63);
    s.bits[y * W + (x >> 6)] ^= 1ull << (x & 63);
  };
  const uint64_t T = (uint64_t)swaps_per_edge * (uint64_t)m;
  int32_t accepted = 0;
  for (uint64_t t = 0; t < T; ++t) {
    const Draw d = desco::null_model::draw(seed, graph, replica, t, (uint32_t)m);
    if (d.i == d.j) continue;
    const int32_t a = s.sa[d.i], b = s.sb[d.i];
    int32_t c = s.sa[d.j], dd = s.sb[d.j];
    if (d.flip) std::swap(c, dd);
    if (a == dd || c == b || has(a, dd) || has(c, b)) continue;
    flip_pair(a, b);
    flip_pair(c, dd);
    flip_pair(a, dd);
    flip_pair(c, b);
    s.sa[d.i] = a, s.sb[d.i] = dd;
    s.sa[d.j] = c, s.sb[d.j] = b;
    ++accepted;
  }
  for (int64_t v = 0; v < n; ++v) {
    int32_t* o = out_col + rowptr[n0 + v];
    for (int64_t w = 0; w < W; ++w) {
      uint64_t x = s.bits[v * W + w];
      while (x) {
        *o++ = (int32_t)(n0 + w * 64 + __builtin_ctzll(x));
        x &= x - 1;
      }
    }
  }
  return accepted;
}

// what is wrong with graph g's rows, or nullptr
const char* check_graph(const int64_t* rowptr, const int32_t* col, int64_t n0, int64_t n1) {
  for (int64_t v = n0; v < n1; ++v) {
    if (rowptr[v + 1] < rowptr[v]) return "desco_null_model_rewire: rowptr is not monotone";
    for (int64_t e = rowptr[v]; e < rowptr[v + 1]; ++e) {
      const int64_t u = col[e];
      if (u < n0 || u >= n1) return "desco_null_model_rewire: col holds an id outside the node's graph";
      if (u == v) return "desco_null_model_rewire: col holds a loop";
      if (e > rowptr[v] && col[e - 1] >= u) return "desco_null_model_rewire: a row is not strictly ascending (unsorted)";
    }
  }
  for (int64_t v = n0; v < n1; ++v)            // (the rows are in range and monotone by now)
    for (int64_t e = rowptr[v]; e < rowptr[v + 1]; ++e) {
      const int32_t* r0 = col + rowptr[col[e]];
      const int32_t* r1 = col + rowptr[col[e] + 1];
      if (!std::binary_search(r0, r1, (int32_t)v)) return "desco_null_model_rewire: the adjacency is asymmetric";
    }
  return nullptr;
}

}  // namespace

extern "C" int desco_null_model_draw(uint64_t seed, int64_t graph, int64_t replica, uint64_t t, int64_t m,
                                     int64_t* out) {
  if (!out) return desco::fail(DESCO_EINVAL, "desco_null_model_draw: out is null");
  if (m < 1 || m > (int64_t)UINT32_MAX) return desco::fail(DESCO_EINVAL, "desco_null_model_draw: m outside 1..2^32-1");
  const Draw d = desco::null_model::draw(seed, (uint32_t)graph, (uint32_t)replica, t, (uint32_t)m);
  out[0] = d.i, out[1] = d.j, out[2] = d.flip;
  return 0;
}

extern "C" int desco_null_model_rewire(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col,
                                       int64_t num_graphs, int64_t graph_base, int replicas, int64_t replica_base,
                                       int64_t swaps_per_edge, uint64_t seed, int num_threads, int32_t* col_out,
                                       int32_t* accepted) {
  if (num_graphs < 0 || replicas < 0)
    return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: negative num_graphs or replicas");
  if (swaps_per_edge < 0) return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: swaps_per_edge is negative");
  if (graph_base < 0 || replica_base < 0)
    return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: negative graph_base or replica_base");
  if (num_graphs == 0 || replicas == 0) return 0;
  if (!graph_ptr) return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: graph_ptr is null");
  if (!rowptr) return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: rowptr is null");
  if (!accepted) return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: accepted is null");
  if (graph_ptr[0] != 0) return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: graph_ptr does not start at 0");
  for (int64_t g = 0; g < num_graphs; ++g)
    if (graph_ptr[g + 1] < graph_ptr[g])
      return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: graph_ptr is not monotone");
  const int64_t N = graph_ptr[num_graphs];
  if (N > INT32_MAX) return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: more than 2^31 - 1 nodes");
  if (rowptr[0] != 0) return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: rowptr does not start at 0");
  const int64_t E = rowptr[N];
  if (E < 0) return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: rowptr is not monotone");
  if (E > 0 && !col) return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: col is null");
  if (E > 0 && !col_out) return desco::fail(DESCO_EINVAL, "desco_null_model_rewire: col_out is null");
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
    if (!why) {
      const int64_t m = (rowptr[graph_ptr[g + 1]] - rowptr[graph_ptr[g]]) / 2;
      if (m > (int64_t)UINT32_MAX)
        why = "desco_null_model_rewire: a graph has 2^32 edges or more";
      else if (m > 0 && swaps_per_edge > INT64_MAX / m)
        why = "desco_null_model_rewire: swaps_per_edge * m is beyond 2^63 attempts";
    }
    if (why) {
#ifdef _OPENMP
#pragma omp critical(desco_null_model_bad)
#endif
      bad = why;
    }
  }
  if (bad) return desco::fail(DESCO_EINVAL, bad);

  const int64_t chains = num_graphs * (int64_t)replicas;
  bool no_memory = false;
#ifdef _OPENMP
#pragma omp parallel num_threads(nt)
#endif
  {
    Scratch s;
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1)
#endif
    for (int64_t c = 0; c < chains; ++c) {
      const int64_t g = c / replicas, r = c % replicas;
      try {
        accepted[r * num_graphs + g] =
            run_chain(rowptr, col, graph_ptr[g], graph_ptr[g + 1] - graph_ptr[g], seed, (uint32_t)(graph_base + g),
                      (uint32_t)(replica_base + r), swaps_per_edge, s, col_out + r * E);
      } catch (const std::bad_alloc&) {
#ifdef _OPENMP
#pragma omp atomic write
#endif
        no_memory = true;
      }
    }
  }
  if (no_memory) return desco::fail(DESCO_ENOMEM, "desco_null_model_rewire: out of memory for a graph's adjacency bitset");
  return 0;
}
