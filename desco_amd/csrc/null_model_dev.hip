// Device side of the degree-preserving null model (C ABI: desco_null_model_rewire_dev), see include/desco_hip.h.
// Bit-identical to the host twin (null_model.cpp): the chain is defined sequentially (null_model.hpp) and this kernel
// reproduces it exactly.
//
// One workgroup of ONE wavefront per chain (graph, replica).  The chain's state sits in the wave's LDS workspace, sized
// by the launch's largest graph: the adjacency bitset (n rows of ceil(n / 32) | 1 words) and one word per edge slot
// (a | b << 16; node ids are local and below 2^16 because the bitset has to fit).
//
//   build   lane per node: sets the bits of its own row (plain LDS stores, the row is its own) and counts its entries
//           (v, u) with u < v; a wave prefix sum gives the node's first slot, which is the CSR order of those entries.
//   chain   SPECULATIVE BATCHES of 64 attempts: lane l draws attempt t0 + l and evaluates it against the state at batch
//           start.  An accepted earlier lane l' INTERFERES with lane l when it wrote one of l's two slots, or when one
//           of the two pairs that l tests is among the two pairs l' removes and the two it adds.  The accepted lanes are
//           walked in ascending order (their draws broadcast with v_readlane), every later lane compares, and a ballot
//           keeps l*, the first lane interfered with; the walk stops once it reaches l*.  Every lane below l* saw exactly
//           the state the sequential chain would have shown it, so the accepted ones among them are applied -- slot
//           words by plain LDS stores (no two share a slot), bitset words by LDS and/or (no two touch the same pair,
//           but they may share a word) -- and the next batch starts at t0 + l*.  Lane 0 is never interfered with, so a
//           batch advances by at least one attempt.  Flagging more than strictly needed (a lane that rejects on its
//           draw alone) only shortens a batch; it cannot change the result.
//   output  lane per node: reads its row off the bitset, ascending, into col_out.
//
// The kernel guards itself: a graph whose workspace exceeds the launch's, whose entries leave the graph, or whose lower
// and upper entries do not pair up gets accepted = -1 and nothing else written.  Every LDS index is below the workspace
// by construction (slot indices are < m from the draw, node ids are checked at build).  No global atomics: a chain has
// one owner.
#include "common_device.hpp"
#include "null_model.hpp"

namespace desco {

struct NullModelArgs {
  const int64_t* graph_ptr;   // [num_graphs + 1]
  const int64_t* rowptr;      // [num_nodes + 1]
  const int32_t* col;         // global ids
  const int64_t* graph_ids;   // [num_ids] the graphs of this launch, or null: all of them
  int64_t num_graphs, num_edges;
  int64_t ws_words;           // LDS words of the launch
  uint32_t graph_base, replica_base;
  int replicas;
  int64_t swaps_per_edge;
  uint64_t seed;
  int32_t* col_out;           // [replicas][num_edges]
  int32_t* accepted;          // [replicas][num_graphs]
};

__device__ __forceinline__ uint32_t pair_key(uint32_t x, uint32_t y) { return x < y ? (x << 16) | y : (y << 16) | x; }

__device__ __forceinline__ uint32_t lane_value(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

__global__ __launch_bounds__(64) void null_model_kernel(NullModelArgs p) {
  extern __shared__ uint32_t nm_lds[];
  const int lane = threadIdx.x;
  const int64_t chain = blockIdx.x;
  const int64_t k = chain / p.replicas;
  const int r = (int)(chain % p.replicas);
  const int64_t g = p.graph_ids ? p.graph_ids[k] : k;
  if (g < 0 || g >= p.num_graphs) return;                     // (wave-uniform) a bad id: nothing to write to
  const int64_t n0 = p.graph_ptr[g], n = p.graph_ptr[g + 1] - n0;
  int32_t* __restrict__ acc_out = p.accepted + (int64_t)r * p.num_graphs + g;
  if (n <= 0) {
    if (lane == 0) *acc_out = n == 0 ? 0 : -1;
    return;
  }
  const int64_t e0 = p.rowptr[n0], e1 = p.rowptr[n0 + n];
  const int64_t m = (e1 - e0) >> 1;
  const int S = (int)null_model::row_words(n);
  if (e1 < e0 || ((e1 - e0) & 1) || n > 65535 || null_model::workspace_words(n, m) > p.ws_words) {
    if (lane == 0) *acc_out = -1;                               // (wave-uniform) not this launch's: no LDS is touched
    return;
  }
  const int32_t* __restrict__ col = p.col;
  int32_t* __restrict__ out = p.col_out + (int64_t)r * p.num_edges;
  if (m < 2 || p.swaps_per_edge == 0) {                         // unchanged
    for (int64_t e = e0 + lane; e < e1; e += 64) out[e] = col[e];
    if (lane == 0) *acc_out = 0;
    return;
  }
  uint32_t* bits = nm_lds;
  uint32_t* slot = nm_lds + n * S;
  const int nn = (int)n, mm = (int)m;

  // ---- build -------------------------------------------------------------------------------------------------------
  for (int q = lane; q < nn * S; q += 64) bits[q] = 0u;
  __syncthreads();
  int bad = 0, first = 0;
  for (int base = 0; base < nn; base += 64) {
    const int v = base + lane;
    int lower = 0;
    if (v < nn)
      for (int64_t e = p.rowptr[n0 + v]; e < p.rowptr[n0 + v + 1]; ++e) {
        const int64_t u = (int64_t)col[e] - n0;
        if (u < 0 || u >= n || u == v) {
          bad = 1;
          continue;
        }
        bits[v * S + (int)(u >> 5)] |= 1u << (u & 31);
        lower += u < v;
      }
    int incl = lower;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int x = __shfl_up(incl, o, 64);
      if (lane >= o) incl += x;
    }
    int q = first + incl - lower;
    if (v < nn)
      for (int64_t e = p.rowptr[n0 + v]; e < p.rowptr[n0 + v + 1]; ++e) {
        const int64_t u = (int64_t)col[e] - n0;
        if (u >= 0 && u < v) {
          if (q < mm) slot[q] = (uint32_t)u | ((uint32_t)v << 16);
          ++q;
        }
      }
    first += __shfl(incl, 63, 64);
  }
  bad |= first != mm;
  if (__ballot(bad)) {                                          // (one wave: the ballot is the whole workgroup's)
    if (lane == 0) *acc_out = -1;
    return;
  }
  __syncthreads();

  // ---- chain -------------------------------------------------------------------------------------------------------
  const uint64_t T = (uint64_t)p.swaps_per_edge * (uint64_t)m;
  const uint32_t gid = p.graph_base + (uint32_t)g, rid = p.replica_base + (uint32_t)r;
  uint64_t t0 = 0;
  int accepted = 0;
  while (t0 < T) {
    const uint64_t t = t0 + (uint64_t)lane;
    const null_model::Draw d = null_model::draw(p.seed, gid, rid, t, (uint32_t)mm);
    const uint32_t si = slot[d.i], sj = slot[d.j];
    const uint32_t a = si & 0xffffu, b = si >> 16;
    const uint32_t c = d.flip ? sj >> 16 : sj & 0xffffu, dd = d.flip ? sj & 0xffffu : sj >> 16;
    bool ok = t < T && d.i != d.j && a != dd && c != b;
    const uint32_t w1 = bits[a * S + (dd >> 5)], w2 = bits[c * S + (b >> 5)];
    ok = ok && !((w1 >> (dd & 31)) & 1u) && !((w2 >> (b & 31)) & 1u);
    const uint32_t p1 = pair_key(a, dd), p2 = pair_key(c, b), r1 = pair_key(a, b), r2 = pair_key(c, dd);

    uint64_t rem = __ballot(ok);
    const uint64_t okmask = rem;
    int lstar = 64;                                             // the first lane an accepted earlier lane interferes with
    while (rem) {
      const int lp = __builtin_amdgcn_readfirstlane(__ffsll((long long)rem) - 1);
      rem &= rem - 1;
      if (lp + 1 >= lstar) break;                               // no lane between lp and l*
      const uint32_t qi = lane_value(d.i, lp), qj = lane_value(d.j, lp);
      const uint32_t q1 = lane_value(p1, lp), q2 = lane_value(p2, lp), q3 = lane_value(r1, lp), q4 = lane_value(r2, lp);
      const bool hit = lane > lp && (d.i == qi || d.i == qj || d.j == qi || d.j == qj ||
                                     p1 == q1 || p1 == q2 || p1 == q3 || p1 == q4 ||
                                     p2 == q1 || p2 == q2 || p2 == q3 || p2 == q4);
      const uint64_t h = __ballot(hit);
      if (h) lstar = min(lstar, __ffsll((long long)h) - 1);
    }
    __syncthreads();                                            // every read of the batch is behind us
    if (ok && lane < lstar) {
      slot[d.i] = a | (dd << 16);
      slot[d.j] = c | (b << 16);
      atomicAnd(&bits[a * S + (b >> 5)], ~(1u << (b & 31)));
      atomicAnd(&bits[b * S + (a >> 5)], ~(1u << (a & 31)));
      atomicAnd(&bits[c * S + (dd >> 5)], ~(1u << (dd & 31)));
      atomicAnd(&bits[dd * S + (c >> 5)], ~(1u << (c & 31)));
      atomicOr(&bits[a * S + (dd >> 5)], 1u << (dd & 31));
      atomicOr(&bits[dd * S + (a >> 5)], 1u << (a & 31));
      atomicOr(&bits[c * S + (b >> 5)], 1u << (b & 31));
      atomicOr(&bits[b * S + (c >> 5)], 1u << (c & 31));
    }
    accepted += __popcll(lstar >= 64 ? okmask : okmask & ((1ull << lstar) - 1ull));
    t0 += (uint64_t)lstar;
    __syncthreads();
  }

  // ---- output ------------------------------------------------------------------------------------------------------
  for (int v = lane; v < nn; v += 64) {
    const int64_t o0 = p.rowptr[n0 + v], deg = p.rowptr[n0 + v + 1] - o0;
    int64_t cnt = 0;
    for (int w = 0; w < S; ++w) {
      uint32_t x = bits[v * S + w];
      while (x) {
        const int u = w * 32 + __ffs((int)x) - 1;
        x &= x - 1;
        if (cnt < deg) out[o0 + cnt] = (int32_t)(n0 + u);
        ++cnt;
      }
    }
  }
  if (lane == 0) *acc_out = accepted;
}

}  // namespace desco

using namespace desco;

extern "C" int desco_null_model_rewire_dev(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col,
                                           int64_t num_graphs, int64_t num_edges, const int64_t* graph_ids,
                                           int64_t num_ids, int64_t max_words, int64_t graph_base, int replicas,
                                           int64_t replica_base, int64_t swaps_per_edge, uint64_t seed,
                                           int32_t* col_out, int32_t* accepted, desco_stream_t stream) {
  if (num_graphs < 0 || num_ids < 0 || replicas < 0 || num_edges < 0)
    return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: negative num_graphs, num_ids, num_edges or replicas");
  if (swaps_per_edge < 0) return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: swaps_per_edge is negative");
  if (graph_base < 0 || replica_base < 0)
    return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: negative graph_base or replica_base");
  if (max_words < 0) return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: negative max_words");
  if (!graph_ids) num_ids = num_graphs;
  if (num_ids == 0 || replicas == 0) return 0;
  if (max_words > DESCO_NULL_MODEL_DEV_MAX_WORDS)
    return fail(DESCO_EINVAL,
                "desco_null_model_rewire_dev: a graph's workspace, n * (ceil(n / 32) | 1) + m words, exceeds "
                "DESCO_NULL_MODEL_DEV_MAX_WORDS (40960); use desco_null_model_rewire for it");
  if (max_words > 0 && swaps_per_edge > INT64_MAX / max_words)                 // (m <= max_words)
    return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: swaps_per_edge * m is beyond 2^63 attempts");
  if (num_ids > INT32_MAX / replicas)
    return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: num_ids * replicas is above 2^31 - 1 chains");
  if (!graph_ptr) return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: graph_ptr is null");
  if (!rowptr) return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: rowptr is null");
  if (!accepted) return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: accepted is null");
  if (num_edges > 0 && !col) return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: col is null");
  if (num_edges > 0 && !col_out) return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: col_out is null");
  if (mis8(graph_ptr) || mis8(rowptr) || mis8(graph_ids))
    return fail(DESCO_EINVAL, "desco_null_model_rewire_dev: a 64-bit array is not 8-byte aligned");
  const hipError_t e = size_dynamic_lds<null_model_kernel>(4 * DESCO_NULL_MODEL_DEV_MAX_WORDS);
  if (e != hipSuccess) return fail((int)e, "desco_null_model_rewire_dev: cannot size LDS");
  NullModelArgs a;
  a.graph_ptr = graph_ptr, a.rowptr = rowptr, a.col = col, a.graph_ids = graph_ids;
  a.num_graphs = num_graphs, a.num_edges = num_edges;
  a.ws_words = (max_words + 3) & ~(int64_t)3;
  a.graph_base = (uint32_t)graph_base, a.replica_base = (uint32_t)replica_base;
  a.replicas = replicas, a.swaps_per_edge = swaps_per_edge, a.seed = seed;
  a.col_out = col_out, a.accepted = accepted;
  hipLaunchKernelGGL(null_model_kernel, dim3((unsigned)(num_ids * replicas)), dim3(64), (size_t)(4 * a.ws_words),
                     (hipStream_t)stream, a);
  return launch_status("desco_null_model_rewire_dev");
}
