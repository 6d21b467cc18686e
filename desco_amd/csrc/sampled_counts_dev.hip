// Sampled canonical counts on the GPU (C ABI: desco_sampled_counts_dev): RAND-ESU (Wernicke 2006) over the shared
// device walk.  Definitions: include/desco_hip.h, "SAMPLED COUNTS"; the decision chain: sampled_counts.hpp.
//
//   tally[r][v][q] = #{ KEPT node subsets S : max(S) = v, G[S] connected and of class q }   in replica r
//
// The kernel is the exact census kernel (groundtruth_dev.hip, gt_count_kernel) with a visitor that vetoes candidates:
// a child of the tree is kept with a probability that depends only on its depth, a dropped child goes with its whole
// subtree.  One wave per (CSR entry (v, u0) with u0 < v, replica); a dropped u0 ends the wave before it reads
// anything else -- that early exit, not the thinner deep levels, is where the time goes away.  Matches are tallied in
// an LDS column per thread, reduced over the wave and flushed with one 64-bit atomic per non-zero class -- into the
// root's row, or with per_graph into its graph's row, so that graph-level tallies never exist per node.  Integer adds
// commute: the result equals the host twin's bit for bit and does not change from call to call.
#include "groundtruth_esu_dev.hpp"
#include "sampled_counts.hpp"

namespace desco {

constexpr int SC_MAXQ = 32, SC_THREADS = 256, SC_WAVES = SC_THREADS / 64;
__device__ __constant__ int SC_OFF_DEV[ESU_KMAX + 2] = {ESU_OFF[0], ESU_OFF[1], ESU_OFF[2], ESU_OFF[3],
                                                        ESU_OFF[4], ESU_OFF[5], ESU_OFF[6]};

struct ScArgs {
  const int64_t* graph_ptr;
  const int64_t* rowptr;
  const int32_t* col;
  const int32_t* node_graph;
  const int64_t* bit_off;
  const unsigned long long* bits;
  const int16_t* cls;                // [1098] query index of the mask's isomorphism class, or -1
  int kmax, Q, per_graph;
  int64_t num_nodes, num_graphs, num_entries, num_replicas;
  unsigned long long thr[ESU_KMAX + 1];              // thr[d], d = 2 .. kmax: 0 .. 2^32
  unsigned long long seed;
  int64_t graph_base, replica_base;
  unsigned long long* out;           // [R][N][Q], or per_graph: [R][G][Q]
};

struct ScVisitor {
  static constexpr bool kWithVeto = true;
  using Path = unsigned long long;   // h of the sequence
  using Level = EsuNone;
  const int16_t* cls;
  unsigned* cnt;                     // this thread's LDS column (stride SC_THREADS)
  const ScArgs& a;
  template <int K>
  __device__ __forceinline__ void classify(unsigned mask) const {
    const int q = cls[SC_OFF_DEV[K] + mask];
    if (q >= 0) atomicAdd(cnt + q * SC_THREADS, 1u);
  }
  template <int NS>
  __device__ __forceinline__ Path push(Path h, int u) const { return sampled::step(h, u); }
  template <int K>
  __device__ __forceinline__ bool keep(Path h) const { return sampled::keep(h, a.thr[K]); }
  template <int K>
  __device__ __forceinline__ void found(const int (&)[ESU_KMAX], int, unsigned mask, Path, Level&) const {
    classify<K>(mask);
  }
  template <int NS>
  __device__ __forceinline__ void close(const int (&)[ESU_KMAX], Level&) const {}
};

// esu_row_of_entry by the whole wave: the last row with rowptr[row] <= e, 64 probes a step (3 dependent loads for 2^18
// rows where the bisection takes 18).  Most waves of a thin schedule end right after their level-2 decision, so their
// time is this search.  All 64 lanes call it with the same arguments.
__device__ __forceinline__ int64_t sc_row_of_entry(const int64_t* __restrict__ rowptr, int64_t n, int64_t e, int lane) {
  int64_t lo = 0, hi = n;            // the row is in [lo, hi), rowptr[lo] <= e
  while (hi - lo > 1) {
    const int64_t step = (hi - lo + 63) >> 6, idx = lo + lane * step;
    const bool below = idx < hi && rowptr[idx] <= e;         // true for the first k lanes, k >= 1 (lane 0 probes lo)
    const int k = __popcll(__ballot(below));
    lo += (k - 1) * step;
    hi = lo + step < hi ? lo + step : hi;
  }
  return lo;
}

__global__ __launch_bounds__(SC_THREADS) void sc_count_kernel(ScArgs a) {
  __shared__ unsigned cnt[SC_MAXQ * SC_THREADS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t w = (int64_t)blockIdx.x * SC_WAVES + (tid >> 6);             // one wave per (entry, replica)
  if (w >= a.num_entries * a.num_replicas) return;   // (no barrier below: columns are private)
  const int64_t e = w / a.num_replicas, r = w - e * a.num_replicas;
  const int64_t v = sc_row_of_entry(a.rowptr, a.num_nodes, e, lane);
  const int g = a.node_graph[v];
  const int64_t base = a.graph_ptr[g];
  const int u0 = (int)(a.col[e] - base);
  const int lv = (int)(v - base);
  if (u0 >= lv) return;                              // the root is the maximum of its subsets
  const unsigned long long h1 = sampled::root_hash(a.seed, (uint32_t)(a.graph_base + g),
                                                   (uint32_t)(a.replica_base + r), (uint32_t)lv);
  const unsigned long long h2 = sampled::step(h1, u0);
  if (!sampled::keep(h2, a.thr[2])) return;          // (wave-uniform) the item's subtree goes
  for (int q = 0; q < a.Q; ++q) cnt[q * SC_THREADS + tid] = 0;
  const EsuGraph c = esu_graph_of(a.graph_ptr, a.rowptr, a.col, a.node_graph, a.bit_off, a.bits, v, a.kmax);
  ScVisitor vis{a.cls, cnt + tid, a};
  if (lane == 0) vis.classify<2>(1u);
  esu_wave_walk(c, vis, v, e, u0, lane, h2);
  unsigned long long* out = a.out + (a.per_graph ? r * a.num_graphs + g : r * a.num_nodes + v) * a.Q;
  for (int q = 0; q < a.Q; ++q) {
    unsigned long long n = cnt[q * SC_THREADS + tid];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0 && n) atomicAdd(out + q, n);
  }
}

}  // namespace desco

using namespace desco;

extern "C" int desco_sampled_counts_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                        const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                        const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                        int64_t num_words, const int16_t* cls, int kmax, int num_queries,
                                        const int64_t* thr, uint64_t seed, int64_t graph_base, int64_t replica_base,
                                        int num_replicas, int per_graph, int64_t* out, desco_stream_t stream) {
  if (num_replicas < 0) return fail(DESCO_EINVAL, "desco_sampled_counts_dev: num_replicas must not be negative");
  if (num_nodes == 0 || num_queries == 0 || num_replicas == 0) return 0;
  if (!graph_ptr || !rowptr || !node_graph || !bit_off || !bits || !cls || !thr || !out ||
      (num_entries > 0 && !col))
    return fail(DESCO_EINVAL, "desco_sampled_counts_dev: null pointer");
  if (num_graphs < 0 || num_nodes < 0 || num_entries < 0 || num_words < 0 || graph_base < 0 || replica_base < 0)
    return fail(DESCO_EINVAL, "desco_sampled_counts_dev: negative count or base");
  if (kmax < 2 || kmax > ESU_KMAX) return fail(DESCO_EINVAL, "desco_sampled_counts_dev: kmax must be 2..5");
  if ((per_graph != 0 && per_graph != 1) || (per_graph && num_graphs == 0))
    return fail(DESCO_EINVAL, "desco_sampled_counts_dev: per_graph must be 0 or 1 (1: with num_graphs > 0)");
  if (num_queries < 0 || num_queries > SC_MAXQ)
    return fail(DESCO_EINVAL, "desco_sampled_counts_dev: num_queries must be 1..32");
  ScArgs a{};
  for (int d = 2; d <= kmax; ++d) {
    if (thr[d] < 0 || thr[d] > (int64_t)sampled::kAlways)
      return fail(DESCO_EINVAL, "desco_sampled_counts_dev: a threshold is outside 0..2^32");
    a.thr[d] = (unsigned long long)thr[d];
  }
  const int64_t max_items = (int64_t)INT32_MAX * SC_WAVES;
  if (num_entries > max_items / num_replicas)
    return fail(DESCO_EINVAL, "desco_sampled_counts_dev: too many work items (entries x replicas) for one grid");
  if (num_nodes > INT64_MAX / 8 / num_queries / num_replicas)
    return fail(DESCO_EINVAL, "desco_sampled_counts_dev: the output is too large");
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = per_graph ? num_graphs : num_nodes;
  if (hipMemsetAsync(out, 0, (size_t)num_replicas * rows * num_queries * 8, s) != hipSuccess)
    return launch_status("desco_sampled_counts_dev: memset");
  if (const int rc = gt_build_bitsets(graph_ptr, rowptr, col, node_graph, bit_off, bits, num_words, num_nodes,
                                      num_entries, stream, "desco_sampled_counts_dev"))
    return rc;
  if (num_entries == 0) return 0;
  a.graph_ptr = graph_ptr;
  a.rowptr = rowptr;
  a.col = col;
  a.node_graph = node_graph;
  a.bit_off = bit_off;
  a.bits = reinterpret_cast<const unsigned long long*>(bits);
  a.cls = cls;
  a.kmax = kmax;
  a.Q = num_queries;
  a.num_nodes = num_nodes;
  a.num_graphs = num_graphs;
  a.per_graph = per_graph;
  a.num_entries = num_entries;
  a.num_replicas = num_replicas;
  a.seed = seed;
  a.graph_base = graph_base;
  a.replica_base = replica_base;
  a.out = reinterpret_cast<unsigned long long*>(out);
  const int64_t blocks = (num_entries * num_replicas + SC_WAVES - 1) / SC_WAVES;
  hipLaunchKernelGGL(sc_count_kernel, dim3((unsigned)blocks), dim3(SC_THREADS), 0, s, a);
  return launch_status("desco_sampled_counts_dev");
}
