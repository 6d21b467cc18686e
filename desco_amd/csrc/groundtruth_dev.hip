// Exact canonical ground-truth counts on the GPU (C ABI: desco_canonical_counts_dev), SURVEY.md 8f
// row N1.  Same definition as the host enumerator (groundtruth.cpp):
//
//   count[v][q] = #{ node subsets S : max(S) = v, G[S] connected and isomorphic to query q }
//
// i.e. what the reference gets from networkx VF2 (MatchSubgraphWorker, workload.py:327-348, keyed by
// max(vmap.keys())) divided by the query's symmetry factor (data.py:61-67).
//
// Enumeration: ESU without extension lists.  In ESU a node u enters the extension set when the
// FIRST subset node adjacent to it is added, and choices are made in list order; with
// key(u) = (insertion index of that first neighbour, position of u in its adjacency row) this is
// exactly "chosen nodes have strictly increasing keys".  So a level is two nested loops over the
// adjacency rows of the subset's nodes, starting behind the previous key, and a candidate is taken
// iff it is below the root, not in the subset and adjacent to no earlier subset node -- the same
// adjacency bits then extend the induced-subgraph mask.  No per-thread lists: the subset (<= 5
// nodes), the mask and the loop cursors live in registers (levels are template-unrolled).
//
// Work item = one CSR entry (v, u0) with u0 < v: the subtree of subsets whose first chosen node is
// u0, handled by ONE WAVE: the candidates for the next node (the rest of v's row, then u0's row) are
// dealt round-robin to the 64 lanes and every lane walks the deeper levels of its candidates on its
// own.  (One thread per item left the launch waiting for the few items rooted at hubs, whose
// subtrees grow with the cube of the degree.)  Matches are tallied in an LDS column per thread
// (ds_add_u32, conflict-free), reduced over the wave and flushed with one 64-bit atomic per (item,
// query).  Adjacency tests read per-graph bitset rows (built by a
// first kernel from the CSR).  Integer work, bit-exact against the host enumerator.
#include "common_device.hpp"
#include "groundtruth_label.hpp"

namespace desco {

constexpr int GT_MAXQ = 32, GT_THREADS = 256, GT_KMAX = 5;
// class table: for k nodes the 2^(k(k-1)/2) adjacency masks start at GT_OFF[k]
__device__ __constant__ int GT_OFF_DEV[GT_KMAX + 2] = {0, 0, 0, 2, 10, 74, 1098};
static const int GT_OFF[GT_KMAX + 2] = {0, 0, 0, 2, 10, 74, 1098};

struct GtArgs {
  const int64_t* graph_ptr;
  const int64_t* rowptr;
  const int32_t* col;
  const int32_t* node_graph;
  const int64_t* bit_off;            // [G] first bitset word of graph g
  unsigned long long* bits;
  const int16_t* cls;                // [1098] query index of the mask's isomorphism class, or -1
  int kmax, Q;
  int64_t num_nodes, num_entries;
  unsigned long long* out;           // [N][Q]
};

__device__ __forceinline__ int64_t gt_row_of_entry(const int64_t* __restrict__ rowptr, int64_t n,
                                                   int64_t e) {
  int64_t lo = 0, hi = n;            // last row with rowptr[row] <= e
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rowptr[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(GT_THREADS) void gt_bits_kernel(GtArgs a) {
  const int64_t e = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x;
  if (e >= a.num_entries) return;
  const int64_t v = gt_row_of_entry(a.rowptr, a.num_nodes, e);
  const int g = a.node_graph[v];
  const int64_t base = a.graph_ptr[g];
  const int words = (int)((a.graph_ptr[g + 1] - base + 63) >> 6);
  const int u = (int)(a.col[e] - base);
  atomicOr(a.bits + a.bit_off[g] + (v - base) * words + (u >> 6), 1ull << (u & 63));
}

struct GtCtx {
  const int64_t* rowptr;
  const int32_t* col;
  const unsigned long long* bits;    // this graph's rows
  const int16_t* cls;
  int64_t base;
  int words, lv, kmax;
  unsigned* cnt;                     // this thread's LDS column (stride GT_THREADS)
};

__device__ __forceinline__ unsigned gt_adj(const GtCtx& c, int a, int b) {
  return (unsigned)(c.bits[(int64_t)a * c.words + (b >> 6)] >> (b & 63)) & 1u;
}

template <int K>
__device__ __forceinline__ void gt_classify(const GtCtx& c, unsigned mask) {
  const int q = c.cls[GT_OFF_DEV[K] + mask];
  if (q >= 0) atomicAdd(c.cnt + q * GT_THREADS, 1u);
}

template <int NS>
__device__ void gt_extend(const GtCtx& c, const int (&S)[GT_KMAX], unsigned mask, int ci0, int cp0);

// candidate at position e of the adjacency row (starting at r0) of S[ci] for node number NS of the
// subset: taken iff it is below the root, new, and adjacent to no subset node before S[ci].
// Returns false when the row has passed the root's id (rows ascend: nothing further qualifies).
template <int NS>
__device__ __forceinline__ bool gt_try(const GtCtx& c, const int (&S)[GT_KMAX], unsigned mask, int ci,
                                       int64_t r0, int64_t e) {
  const int u = (int)(c.col[e] - c.base);
  if (u >= c.lv) return false;
  unsigned ab = 0;
  bool in_s = false;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    in_s |= u == S[j];
    ab |= gt_adj(c, S[j], u) << j;
  }
  if (in_s || (ab & ((1u << ci) - 1u))) return true;     // u entered the extension set earlier
  const unsigned m2 = mask | (ab << (NS * (NS - 1) / 2));
  gt_classify<NS + 1>(c, m2);
  if constexpr (NS + 1 < GT_KMAX) {
    if (NS + 1 < c.kmax) {
      int S2[GT_KMAX];
#pragma unroll
      for (int j = 0; j < GT_KMAX; ++j) S2[j] = j < NS ? S[j] : 0;
      S2[NS] = u;
      gt_extend<NS + 1>(c, S2, m2, ci, (int)(e - r0) + 1);
    }
  }
  return true;
}

// choose node number NS of the subset (S[0..NS-1] chosen, induced mask `mask`); candidates start at
// key (ci0, cp0)
template <int NS>
__device__ void gt_extend(const GtCtx& c, const int (&S)[GT_KMAX], unsigned mask, int ci0, int cp0) {
#pragma unroll
  for (int ci = 0; ci < NS; ++ci) {
    if (ci < ci0) continue;
    const int64_t r0 = c.rowptr[c.base + S[ci]], r1 = c.rowptr[c.base + S[ci] + 1];
    for (int64_t e = r0 + (ci == ci0 ? cp0 : 0); e < r1; ++e)
      if (!gt_try<NS>(c, S, mask, ci, r0, e)) break;
  }
}

__global__ __launch_bounds__(GT_THREADS) void gt_count_kernel(GtArgs a) {
  __shared__ unsigned cnt[GT_MAXQ * GT_THREADS];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int q = 0; q < a.Q; ++q) cnt[q * GT_THREADS + tid] = 0;
  const int64_t e = (int64_t)blockIdx.x * (GT_THREADS / 64) + (tid >> 6);     // one wave per entry
  if (e >= a.num_entries) return;                  // (no barrier below: columns are private)
  const int64_t v = gt_row_of_entry(a.rowptr, a.num_nodes, e);
  const int g = a.node_graph[v];
  GtCtx c;
  c.rowptr = a.rowptr;
  c.col = a.col;
  c.cls = a.cls;
  c.base = a.graph_ptr[g];
  c.words = (int)((a.graph_ptr[g + 1] - c.base + 63) >> 6);
  c.bits = a.bits + a.bit_off[g];
  c.lv = (int)(v - c.base);
  c.kmax = a.kmax;
  c.cnt = cnt + tid;
  const int u0 = (int)(a.col[e] - c.base);
  if (u0 >= c.lv) return;                          // the root is the maximum of its subsets
  const int S[GT_KMAX] = {c.lv, u0, 0, 0, 0};
  if (lane == 0) gt_classify<2>(c, 1u);
  if (c.kmax > 2) {
    // candidates for the third node: v's row behind u0, then u0's row; position p -> lane p % 64
    const int64_t v0 = a.rowptr[v], v1 = a.rowptr[v + 1];
    const int64_t w0 = a.rowptr[c.base + u0], w1 = a.rowptr[c.base + u0 + 1];
    const int64_t rest = v1 - (e + 1), total = rest + (w1 - w0);
    for (int64_t p = lane; p < total; p += 64) {
      if (p < rest)
        gt_try<2>(c, S, 1u, 0, v0, e + 1 + p);
      else
        gt_try<2>(c, S, 1u, 1, w0, w0 + (p - rest));
    }
  }
  for (int q = 0; q < a.Q; ++q) {
    unsigned long long n = cnt[q * GT_THREADS + tid];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0 && n) atomicAdd(a.out + v * a.Q + q, n);
  }
}

// ---- orbit counts (graphlet degree vectors): C ABI desco_orbit_counts_dev ---------------------------------------------
//   out[v][column] = #{connected subsets S containing v whose induced subgraph is a requested query, v in the position
//   orbit that the column stands for}; orb[(GT_OFF[k] + mask) * 5 + i] = the column of subset position i, or -1.
// The enumeration is the one above (same items, same lanes, same order); it is repeated here, not shared through a
// template, so that the canonical kernel's code stays what it was.  What differs is the tally: a subset of k nodes
// updates k rows.  Adds that share a destination are summed on chip first:
//   * S[0] = v and S[1] = u0 belong to the whole wave: 2 x 4 banks of u32 columns per wave in LDS (bank = lane % 4, to
//     spread lanes that hit one column), added to the two rows with one atomic per non-zero column when the wave ends.
//     A u32 cell that wraps hands its carry (2^32) to the global cell at once, so no bound on an item's size is needed.
//   * below that, a lane keeps ONE RUN per level in registers: while the subsets found by the loop that chooses node
//     number NS have the same table row, they differ only in that last node, so a counter is bumped; the run goes out
//     (S[0], S[1] to LDS, S[2..NS-1] by one global atomic each, adding the run length) when the table row changes or
//     the loop ends.  Cliques, stars, paths and the sparse neighbourhoods of molecules give long runs.
//   * the node chosen last changes with every subset: one global 64-bit atomic per subset.  The rate of scattered
//     64-bit integer atomics on this chip has not been measured (the published figures are for float adds), so the
//     cost of this part is known only from tools/bench_groundtruth_orbits.py.
// Integer adds commute: the result equals the host's bit for bit and does not change from call to call.
constexpr int GO_MAXC = 73, GO_CPAD = 80, GO_BANKS = 4, GO_WAVES = GT_THREADS / 64;

struct GoArgs {
  const int64_t* graph_ptr;
  const int64_t* rowptr;
  const int32_t* col;
  const int32_t* node_graph;
  const int64_t* bit_off;
  const unsigned long long* bits;
  const int16_t* orb;                // [1098][5]
  int kmax, C;
  int64_t num_nodes, num_entries;
  unsigned long long* out;           // [N][C]
};

struct GoCtx {
  GtCtx g;                           // (cls and cnt unused)
  const int16_t* orb;
  unsigned* tally;                   // this lane's bank of the wave's columns: [2][GO_CPAD]
  unsigned long long* out0;          // out row of S[0]
  unsigned long long* out1;          // out row of S[1]
  unsigned long long* outg;          // out row of the graph's first node
  int C;
};

struct GoRun {
  int t;                             // table row of the run
  unsigned long long n;              // subsets in it
};

// add n to the wave's column of S[j], j < 2
__device__ __forceinline__ void go_wave_add(const GoCtx& c, int j, int column, unsigned long long n) {
  unsigned long long* row = j ? c.out1 : c.out0;
  if (n >> 32) atomicAdd(row + column, n & ~0xffffffffull);
  const unsigned lo = (unsigned)n;
  if (lo == 0) return;
  const unsigned old = atomicAdd(c.tally + j * GO_CPAD + column, lo);
  if (old > ~lo) atomicAdd(row + column, 1ull << 32);                      // the cell wrapped
}

template <int NS>
__device__ __forceinline__ void go_flush(const GoCtx& c, const int (&S)[GT_KMAX], GoRun& run) {
  if (run.n == 0) return;
  const int16_t* row = c.orb + run.t * GT_KMAX;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int column = row[j];
    if (j < 2) go_wave_add(c, j, column, run.n);
    else atomicAdd(c.outg + (int64_t)S[j] * c.C + column, run.n);
  }
  run.n = 0;
}

template <int NS>
__device__ void go_extend(const GoCtx& c, const int (&S)[GT_KMAX], unsigned mask, int ci0, int cp0);

// gt_try with the orbit tally; `run` is the run of the loop that chooses node number NS
template <int NS>
__device__ __forceinline__ bool go_try(const GoCtx& c, const int (&S)[GT_KMAX], unsigned mask, int ci, int64_t r0,
                                       int64_t e, GoRun& run) {
  const int u = (int)(c.g.col[e] - c.g.base);
  if (u >= c.g.lv) return false;
  unsigned ab = 0;
  bool in_s = false;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    in_s |= u == S[j];
    ab |= gt_adj(c.g, S[j], u) << j;
  }
  if (in_s || (ab & ((1u << ci) - 1u))) return true;
  const unsigned m2 = mask | (ab << (NS * (NS - 1) / 2));
  const int t = GT_OFF_DEV[NS + 1] + (int)m2;
  const int last = c.orb[t * GT_KMAX + NS];
  if (last >= 0) {                                 // (a class is asked for with all its positions or with none)
    atomicAdd(c.outg + (int64_t)u * c.C + last, 1ull);
    if (run.n && run.t != t) go_flush<NS>(c, S, run);
    run.t = t;
    ++run.n;
  }
  if constexpr (NS + 1 < GT_KMAX) {
    if (NS + 1 < c.g.kmax) {
      int S2[GT_KMAX];
#pragma unroll
      for (int j = 0; j < GT_KMAX; ++j) S2[j] = j < NS ? S[j] : 0;
      S2[NS] = u;
      go_extend<NS + 1>(c, S2, m2, ci, (int)(e - r0) + 1);
    }
  }
  return true;
}

template <int NS>
__device__ void go_extend(const GoCtx& c, const int (&S)[GT_KMAX], unsigned mask, int ci0, int cp0) {
  GoRun run{0, 0};
#pragma unroll
  for (int ci = 0; ci < NS; ++ci) {
    if (ci < ci0) continue;
    const int64_t r0 = c.g.rowptr[c.g.base + S[ci]], r1 = c.g.rowptr[c.g.base + S[ci] + 1];
    for (int64_t e = r0 + (ci == ci0 ? cp0 : 0); e < r1; ++e)
      if (!go_try<NS>(c, S, mask, ci, r0, e, run)) break;
  }
  go_flush<NS>(c, S, run);
}

__global__ __launch_bounds__(GT_THREADS) void go_count_kernel(GoArgs a) {
  __shared__ unsigned tally[GO_WAVES * GO_BANKS * 2 * GO_CPAD];
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned* wave_tally = tally + (tid >> 6) * (GO_BANKS * 2 * GO_CPAD);     // private to this wave: no block barrier
  const int64_t e = (int64_t)blockIdx.x * GO_WAVES + (tid >> 6);            // one wave per entry
  if (e >= a.num_entries) return;
  const int64_t v = gt_row_of_entry(a.rowptr, a.num_nodes, e);
  const int g = a.node_graph[v];
  GoCtx c;
  c.g.rowptr = a.rowptr;
  c.g.col = a.col;
  c.g.cls = nullptr;
  c.g.cnt = nullptr;
  c.g.base = a.graph_ptr[g];
  c.g.words = (int)((a.graph_ptr[g + 1] - c.g.base + 63) >> 6);
  c.g.bits = a.bits + a.bit_off[g];
  c.g.lv = (int)(v - c.g.base);
  c.g.kmax = a.kmax;
  c.orb = a.orb;
  c.C = a.C;
  c.tally = wave_tally + (lane & (GO_BANKS - 1)) * (2 * GO_CPAD);
  const int u0 = (int)(a.col[e] - c.g.base);
  if (u0 >= c.g.lv) return;                        // (wave-uniform) the root is the maximum of its subsets
  c.outg = a.out + c.g.base * a.C;
  c.out0 = a.out + v * a.C;
  c.out1 = c.outg + (int64_t)u0 * a.C;
  for (int i = lane; i < GO_BANKS * 2 * GO_CPAD; i += 64) wave_tally[i] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int S[GT_KMAX] = {c.g.lv, u0, 0, 0, 0};
  if (lane == 0) {
    const int16_t* row = a.orb + (GT_OFF_DEV[2] + 1) * GT_KMAX;
    if (row[0] >= 0) {
      go_wave_add(c, 0, row[0], 1);
      go_wave_add(c, 1, row[1], 1);
    }
  }
  if (c.g.kmax > 2) {
    const int64_t v0 = a.rowptr[v], v1 = a.rowptr[v + 1];
    const int64_t w0 = a.rowptr[c.g.base + u0], w1 = a.rowptr[c.g.base + u0 + 1];
    const int64_t rest = v1 - (e + 1), total = rest + (w1 - w0);
    GoRun run{0, 0};                               // the lane's 3-node subsets: they share S[0] and S[1]
    for (int64_t p = lane; p < total; p += 64) {
      if (p < rest)
        go_try<2>(c, S, 1u, 0, v0, e + 1 + p, run);
      else
        go_try<2>(c, S, 1u, 1, w0, w0 + (p - rest), run);
    }
    go_flush<2>(c, S, run);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int column = lane; column < a.C; column += 64) {                    // contiguous cells of the two rows
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned long long n = 0;
#pragma unroll
      for (int b = 0; b < GO_BANKS; ++b) n += wave_tally[(b * 2 + j) * GO_CPAD + column];
      if (n) atomicAdd((j ? c.out1 : c.out0) + column, n);
    }
  }
}

// NON-INDUCED counts of small queries from the census of ALL connected k-node classes (the enumerator above visits
// every connected k-subset once, so the census costs what one induced column costs):
//   out[v][q] (+)= sum_c counts[v][c] * m[c][q],   m[c][q] = occurrences of query q in class c (exact, int64).
// One thread per out element; m (at most 32 x 64 int64 = 16 KB) sits in LDS, the C counts of a row are read by the Q
// threads of that row from the same addresses.  Integer arithmetic modulo 2^64, as numpy's int64 product.
constexpr int GT_TR_MAXC = 32, GT_TR_MAXQ = 64;

struct GtTransformArgs {
  const unsigned long long* counts;  // [N][ldc]
  const unsigned long long* m;       // [C][Q]
  unsigned long long* out;           // [N][ldo]
  int64_t ldc, ldo, total;           // total = N * Q
  int C, Q, accumulate;
};

__global__ __launch_bounds__(GT_THREADS) void gt_transform_kernel(GtTransformArgs a) {
  __shared__ unsigned long long m_s[GT_TR_MAXC * GT_TR_MAXQ];
  for (int i = threadIdx.x; i < a.C * a.Q; i += GT_THREADS) m_s[i] = a.m[i];
  __syncthreads();                                 // (the only barrier: every thread reaches it)
  const int64_t idx = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const int64_t row = idx / a.Q;
  const int q = (int)(idx - row * a.Q);
  const unsigned long long* cnt = a.counts + row * a.ldc;
  unsigned long long* dst = a.out + row * a.ldo + q;
  unsigned long long sum = a.accumulate ? *dst : 0ull;
  for (int c = 0; c < a.C; ++c) sum += cnt[c] * m_s[c * a.Q + q];
  *dst = sum;
}

}  // namespace desco

using namespace desco;

namespace {
inline int gt_pair_bit(int a, int b) { return b * (b - 1) / 2 + a; }   // a < b
}

// The bitset rows of both device enumerators (this one and groundtruth_label_dev.hip).
int desco::gt_build_bitsets(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col,
                            const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                            int64_t num_words, int64_t num_nodes, int64_t num_entries, void* stream,
                            const char* who) {
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(bits, 0, (size_t)num_words * 8, s) != hipSuccess)
    return launch_status((std::string(who) + ": memset").c_str());
  if (num_entries == 0) return 0;
  const int64_t blocks = (num_entries + GT_THREADS - 1) / GT_THREADS;
  if (blocks > INT32_MAX) return fail(DESCO_EINVAL, (std::string(who) + ": too many edges").c_str());
  GtArgs a{};
  a.graph_ptr = graph_ptr;
  a.rowptr = rowptr;
  a.col = col;
  a.node_graph = node_graph;
  a.bit_off = bit_off;
  a.bits = reinterpret_cast<unsigned long long*>(bits);
  a.num_nodes = num_nodes;
  a.num_entries = num_entries;
  hipLaunchKernelGGL(gt_bits_kernel, dim3((unsigned)blocks), dim3(GT_THREADS), 0, s, a);
  return launch_status(who);
}

// HOST helper: the class table the device kernel reads.
extern "C" int desco_canonical_class_table(const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                           const int32_t* q_edges, int num_queries, int16_t* table,
                                           int* kmax_out) {
  if (!q_nodes || !q_edge_ptr || !table || !kmax_out || num_queries < 0 || num_queries > GT_MAXQ)
    return fail(DESCO_EINVAL, "desco_canonical_class_table: bad argument (at most 32 queries)");
  for (int i = 0; i < GT_OFF[GT_KMAX + 1]; ++i) table[i] = -1;
  int kmax = 0;
  for (int q = 0; q < num_queries; ++q) {
    const int k = q_nodes[q];
    if (k < 2 || k > GT_KMAX)
      return fail(DESCO_EINVAL, "desco_canonical_class_table: the device path takes queries of 2..5 nodes");
    kmax = k > kmax ? k : kmax;
    uint32_t m = 0;
    for (int e = q_edge_ptr[q]; e < q_edge_ptr[q + 1]; ++e) {
      int a = q_edges[2 * e], b = q_edges[2 * e + 1];
      if (a == b || a < 0 || b < 0 || a >= k || b >= k)
        return fail(DESCO_EINVAL, "desco_canonical_class_table: bad query edge");
      if (a > b) { const int t = a; a = b; b = t; }
      m |= 1u << gt_pair_bit(a, b);
    }
    // every relabeling of the query is a mask of its class
    int perm[GT_KMAX];
    for (int i = 0; i < k; ++i) perm[i] = i;
    for (;;) {
      uint32_t r = 0;
      for (int b = 1; b < k; ++b)
        for (int a = 0; a < b; ++a)
          if (m >> gt_pair_bit(a, b) & 1) {
            const int x = perm[a] < perm[b] ? perm[a] : perm[b];
            const int y = perm[a] < perm[b] ? perm[b] : perm[a];
            r |= 1u << gt_pair_bit(x, y);
          }
      int16_t& slot = table[GT_OFF[k] + r];
      if (slot >= 0 && slot != q)
        return fail(DESCO_EINVAL, "desco_canonical_class_table: two queries are isomorphic");
      slot = (int16_t)q;
      // next permutation
      int i = k - 2;
      while (i >= 0 && perm[i] > perm[i + 1]) --i;
      if (i < 0) break;
      int j = k - 1;
      while (perm[j] < perm[i]) --j;
      { const int t = perm[i]; perm[i] = perm[j]; perm[j] = t; }
      for (int lo = i + 1, hi = k - 1; lo < hi; ++lo, --hi) {
        const int t = perm[lo]; perm[lo] = perm[hi]; perm[hi] = t;
      }
    }
  }
  *kmax_out = kmax;
  return 0;
}

extern "C" int desco_canonical_counts_dev(const int64_t* graph_ptr, int64_t num_graphs,
                                          int64_t num_nodes, const int64_t* rowptr,
                                          int64_t num_entries, const int32_t* col,
                                          const int32_t* node_graph, const int64_t* bit_off,
                                          uint64_t* bits, int64_t num_words, const int16_t* cls,
                                          int kmax, int num_queries, int64_t* out,
                                          desco_stream_t stream) {
  if (num_nodes == 0 || num_queries == 0) return 0;
  if (!graph_ptr || !rowptr || !node_graph || !bit_off || !bits || !cls || !out || num_graphs < 0 ||
      num_nodes < 0 || num_entries < 0 || num_words < 0 || kmax < 2 || kmax > GT_KMAX ||
      num_queries < 0 || num_queries > GT_MAXQ || (num_entries > 0 && !col))
    return fail(DESCO_EINVAL, "desco_canonical_counts_dev: bad argument (queries of 2..5 nodes, at most 32)");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, (size_t)num_nodes * num_queries * 8, s) != hipSuccess)
    return launch_status("desco_canonical_counts_dev: memset");
  const int64_t wblocks = (num_entries + GT_THREADS / 64 - 1) / (GT_THREADS / 64);
  if (wblocks > INT32_MAX) return fail(DESCO_EINVAL, "desco_canonical_counts_dev: too many edges");
  if (const int rc = gt_build_bitsets(graph_ptr, rowptr, col, node_graph, bit_off, bits, num_words, num_nodes,
                                      num_entries, stream, "desco_canonical_counts_dev"))
    return rc;
  if (num_entries == 0) return 0;
  GtArgs a{graph_ptr, rowptr, col, node_graph, bit_off, reinterpret_cast<unsigned long long*>(bits),
           cls, kmax, num_queries, num_nodes, num_entries, reinterpret_cast<unsigned long long*>(out)};
  hipLaunchKernelGGL(gt_count_kernel, dim3((unsigned)wblocks), dim3(GT_THREADS), 0, s, a);
  return launch_status("desco_canonical_counts_dev");
}

extern "C" int desco_orbit_counts_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                      const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                      const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                      int64_t num_words, const int16_t* orbit_table, int kmax, int num_columns,
                                      int64_t* out, desco_stream_t stream) {
  if (num_nodes == 0 || num_columns == 0) return 0;
  if (!graph_ptr || !rowptr || !node_graph || !bit_off || !bits || !orbit_table || !out || num_graphs < 0 ||
      num_nodes < 0 || num_entries < 0 || num_words < 0 || kmax < 2 || kmax > GT_KMAX || num_columns < 0 ||
      num_columns > GO_MAXC || (num_entries > 0 && !col))
    return fail(DESCO_EINVAL, "desco_orbit_counts_dev: bad argument (queries of 2..5 nodes, at most 73 columns)");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, (size_t)num_nodes * num_columns * 8, s) != hipSuccess)
    return launch_status("desco_orbit_counts_dev: memset");
  const int64_t wblocks = (num_entries + GO_WAVES - 1) / GO_WAVES;
  if (wblocks > INT32_MAX) return fail(DESCO_EINVAL, "desco_orbit_counts_dev: too many edges");
  if (const int rc = gt_build_bitsets(graph_ptr, rowptr, col, node_graph, bit_off, bits, num_words, num_nodes,
                                      num_entries, stream, "desco_orbit_counts_dev"))
    return rc;
  if (num_entries == 0) return 0;
  GoArgs a{graph_ptr, rowptr, col, node_graph, bit_off, reinterpret_cast<const unsigned long long*>(bits),
           orbit_table, kmax, num_columns, num_nodes, num_entries, reinterpret_cast<unsigned long long*>(out)};
  hipLaunchKernelGGL(go_count_kernel, dim3((unsigned)wblocks), dim3(GT_THREADS), 0, s, a);
  return launch_status("desco_orbit_counts_dev");
}

extern "C" int desco_canonical_noninduced_transform_dev(const int64_t* counts, int64_t ldc, const int64_t* m,
                                                        int64_t num_nodes, int num_classes, int num_queries,
                                                        int accumulate, int64_t* out, int64_t ldo,
                                                        desco_stream_t stream) {
  if (num_nodes == 0 || num_queries == 0) return 0;
  if (!counts || !m || !out || num_nodes < 0 || num_classes < 1 || num_classes > GT_TR_MAXC || num_queries < 0 ||
      num_queries > GT_TR_MAXQ || ldc < num_classes || ldo < num_queries || (accumulate != 0 && accumulate != 1))
    return fail(DESCO_EINVAL,
                "desco_canonical_noninduced_transform_dev: bad argument (1..32 classes, at most 64 queries)");
  const int64_t total = num_nodes * num_queries, blocks = (total + GT_THREADS - 1) / GT_THREADS;
  if (blocks > INT32_MAX) return fail(DESCO_EINVAL, "desco_canonical_noninduced_transform_dev: too many rows");
  GtTransformArgs a{reinterpret_cast<const unsigned long long*>(counts), reinterpret_cast<const unsigned long long*>(m),
                    reinterpret_cast<unsigned long long*>(out), ldc, ldo, total, num_classes, num_queries, accumulate};
  hipLaunchKernelGGL(gt_transform_kernel, dim3((unsigned)blocks), dim3(GT_THREADS), 0, (hipStream_t)stream, a);
  return launch_status("desco_canonical_noninduced_transform_dev");
}
