// Exact canonical ground-truth counts on the GPU (C ABI: desco_canonical_counts_dev), SURVEY.md 8f
// row N1.  Same definition as the host enumerator (groundtruth.cpp):
//
//   count[v][q] = #{ node subsets S : max(S) = v, G[S] connected and isomorphic to query q }
//
// i.e. what the reference gets from networkx VF2 (MatchSubgraphWorker, workload.py:327-348, keyed by
// max(vmap.keys())) divided by the query's symmetry factor (data.py:61-67).
//
// Enumeration: the shared device walk, groundtruth_esu_dev.hpp (ESU without extension lists, one wave per CSR entry
// (v, u0) with u0 < v); the kernels here are visitors over it.  Canonical counts: matches are tallied in an LDS
// column per thread (ds_add_u32, conflict-free), reduced over the wave and flushed with one 64-bit atomic per (item,
// query).  Adjacency tests read per-graph bitset rows (built by a
// first kernel from the CSR).  Integer work, bit-exact against the host enumerator.
#include "groundtruth_esu_dev.hpp"

namespace desco {

constexpr int GT_MAXQ = 32, GT_THREADS = 256, GT_KMAX = ESU_KMAX;
// class table: for k nodes the 2^(k(k-1)/2) adjacency masks start at ESU_OFF[k]
__device__ __constant__ int GT_OFF_DEV[GT_KMAX + 2] = {ESU_OFF[0], ESU_OFF[1], ESU_OFF[2], ESU_OFF[3],
                                                       ESU_OFF[4], ESU_OFF[5], ESU_OFF[6]};

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

__global__ __launch_bounds__(GT_THREADS) void gt_bits_kernel(GtArgs a) {
  const int64_t e = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x;
  if (e >= a.num_entries) return;
  const int64_t v = esu_row_of_entry(a.rowptr, a.num_nodes, e);
  const int g = a.node_graph[v];
  const int64_t base = a.graph_ptr[g];
  const int words = (int)((a.graph_ptr[g + 1] - base + 63) >> 6);
  const int u = (int)(a.col[e] - base);
  atomicOr(a.bits + a.bit_off[g] + (v - base) * words + (u >> 6), 1ull << (u & 63));
}

struct GtVisitor {
  using Path = EsuNone;
  using Level = EsuNone;
  const int16_t* cls;
  unsigned* cnt;                     // this thread's LDS column (stride GT_THREADS)
  template <int K>
  __device__ __forceinline__ void classify(unsigned mask) const {
    const int q = cls[GT_OFF_DEV[K] + mask];
    if (q >= 0) atomicAdd(cnt + q * GT_THREADS, 1u);
  }
  template <int NS>
  __device__ __forceinline__ Path push(Path p, int) const { return p; }
  template <int K>
  __device__ __forceinline__ void found(const int (&)[ESU_KMAX], int, unsigned mask, Path, Level&) const {
    classify<K>(mask);
  }
  template <int NS>
  __device__ __forceinline__ void close(const int (&)[ESU_KMAX], Level&) const {}
};

__global__ __launch_bounds__(GT_THREADS) void gt_count_kernel(GtArgs a) {
  __shared__ unsigned cnt[GT_MAXQ * GT_THREADS];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int q = 0; q < a.Q; ++q) cnt[q * GT_THREADS + tid] = 0;
  const int64_t e = (int64_t)blockIdx.x * (GT_THREADS / 64) + (tid >> 6);     // one wave per entry
  if (e >= a.num_entries) return;                  // (no barrier below: columns are private)
  const int64_t v = esu_row_of_entry(a.rowptr, a.num_nodes, e);
  const EsuGraph c = esu_graph_of(a.graph_ptr, a.rowptr, a.col, a.node_graph, a.bit_off, a.bits, v, a.kmax);
  GtVisitor vis{a.cls, cnt + tid};
  const int u0 = (int)(a.col[e] - c.base);
  if (u0 >= c.lv) return;                          // the root is the maximum of its subsets
  if (lane == 0) vis.classify<2>(1u);
  esu_wave_walk(c, vis, v, e, u0, lane, EsuNone{});
  for (int q = 0; q < a.Q; ++q) {
    unsigned long long n = cnt[q * GT_THREADS + tid];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0 && n) atomicAdd(a.out + v * a.Q + q, n);
  }
}

// ---- orbit counts (graphlet degree vectors): C ABI desco_orbit_counts_dev ---------------------------------------------
//   out[v][column] = #{connected subsets S containing v whose induced subgraph is a requested query, v in the position
//   orbit that the column stands for}; orb[(ESU_OFF[k] + mask) * 5 + i] = the column of subset position i, or -1.
// The enumeration is the one above (same items, same lanes, same order).  What differs is the tally: a subset of k
// nodes updates k rows.  Adds that share a destination are summed on chip first:
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

struct GoRun {
  int t;                             // table row of the run
  unsigned long long n;              // subsets in it
};

struct GoVisitor {
  using Path = EsuNone;
  using Level = GoRun;
  const int16_t* orb;
  unsigned* tally;                   // this lane's bank of the wave's columns: [2][GO_CPAD]
  unsigned long long* out0;          // out row of S[0]
  unsigned long long* out1;          // out row of S[1]
  unsigned long long* outg;          // out row of the graph's first node
  int C;

  // add n to the wave's column of S[j], j < 2
  __device__ __forceinline__ void wave_add(int j, int column, unsigned long long n) const {
    unsigned long long* row = j ? out1 : out0;
    if (n >> 32) atomicAdd(row + column, n & ~0xffffffffull);
    const unsigned lo = (unsigned)n;
    if (lo == 0) return;
    const unsigned old = atomicAdd(tally + j * GO_CPAD + column, lo);
    if (old > ~lo) atomicAdd(row + column, 1ull << 32);                      // the cell wrapped
  }
  template <int NS>
  __device__ __forceinline__ Path push(Path p, int) const { return p; }
  // the run of the loop that chose node number NS goes out
  template <int NS>
  __device__ __forceinline__ void close(const int (&S)[ESU_KMAX], GoRun& run) const {
    if (run.n == 0) return;
    const int16_t* row = orb + run.t * GT_KMAX;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int column = row[j];
      if (j < 2) wave_add(j, column, run.n);
      else atomicAdd(outg + (int64_t)S[j] * C + column, run.n);
    }
    run.n = 0;
  }
  template <int K>
  __device__ __forceinline__ void found(const int (&S)[ESU_KMAX], int u, unsigned mask, Path, GoRun& run) const {
    const int t = GT_OFF_DEV[K] + (int)mask;
    const int last = orb[t * GT_KMAX + K - 1];
    if (last >= 0) {                                 // (a class is asked for with all its positions or with none)
      atomicAdd(outg + (int64_t)u * C + last, 1ull);
      if (run.n && run.t != t) close<K - 1>(S, run);
      run.t = t;
      ++run.n;
    }
  }
};

__global__ __launch_bounds__(GT_THREADS) void go_count_kernel(GoArgs a) {
  __shared__ unsigned tally[GO_WAVES * GO_BANKS * 2 * GO_CPAD];
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned* wave_tally = tally + (tid >> 6) * (GO_BANKS * 2 * GO_CPAD);     // private to this wave: no block barrier
  const int64_t e = (int64_t)blockIdx.x * GO_WAVES + (tid >> 6);            // one wave per entry
  if (e >= a.num_entries) return;
  const int64_t v = esu_row_of_entry(a.rowptr, a.num_nodes, e);
  const EsuGraph c = esu_graph_of(a.graph_ptr, a.rowptr, a.col, a.node_graph, a.bit_off, a.bits, v, a.kmax);
  GoVisitor vis;
  vis.orb = a.orb;
  vis.C = a.C;
  vis.tally = wave_tally + (lane & (GO_BANKS - 1)) * (2 * GO_CPAD);
  const int u0 = (int)(a.col[e] - c.base);
  if (u0 >= c.lv) return;                          // (wave-uniform) the root is the maximum of its subsets
  vis.outg = a.out + c.base * a.C;
  vis.out0 = a.out + v * a.C;
  vis.out1 = vis.outg + (int64_t)u0 * a.C;
  for (int i = lane; i < GO_BANKS * 2 * GO_CPAD; i += 64) wave_tally[i] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane == 0) {
    const int16_t* row = a.orb + (GT_OFF_DEV[2] + 1) * GT_KMAX;
    if (row[0] >= 0) {
      vis.wave_add(0, row[0], 1);
      vis.wave_add(1, row[1], 1);
    }
  }
  esu_wave_walk(c, vis, v, e, u0, lane, EsuNone{});
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int column = lane; column < a.C; column += 64) {                    // contiguous cells of the two rows
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned long long n = 0;
#pragma unroll
      for (int b = 0; b < GO_BANKS; ++b) n += wave_tally[(b * 2 + j) * GO_CPAD + column];
      if (n) atomicAdd((j ? vis.out1 : vis.out0) + column, n);
    }
  }
}

// ---- edge orbit counts (edge graphlet degree vectors): C ABI desco_edge_orbit_counts_dev -------------------------------
//   out[row of {a,b}][column] = #{connected subsets S containing a and b whose induced subgraph is a requested query,
//   the edge {a,b} in the edge orbit that the column stands for}; eorb[(ESU_OFF[k] + mask) * 10 + p] = the column of
//   the pair with pair bit p of the subset's positions, or -1 (class not asked for, or the pair is no edge).
// The enumeration is the one above (same items, same lanes, same order).  A subset of k nodes updates up to k(k-1)/2
// rows, and a row has to be found from two node ids.  As in the node-orbit kernel, adds that share a destination are
// summed on chip first:
//   * the item's own edge {S[0], S[1]} (pair bit 0; its row is entry_row[e]) belongs to the whole wave: 4 banks of u32
//     columns per wave in LDS, flushed with one atomic per non-zero column when the wave ends.
//     NO COUNT IS LOST in a u32 cell: every update is one LDS atomic add of lo < 2^32 that returns the cell's old value,
//     so old + lo < 2^33 and the add wraps at most once, exactly when old > ~lo; the updates of a cell are serialised,
//     so every wrap is seen by the one update that caused it, and that update hands 2^32 to the global cell at once
//     (the part of n above 2^32 goes there directly).  The cell keeps the sum modulo 2^32 and the flush adds that
//     remainder: the global cell receives the exact sum.
//   * the edges among the nodes chosen before the last one are shared by the subsets of a candidate loop that have the
//     same table row: ONE RUN per level in registers, flushed (one global atomic per edge, adding the run length; the
//     own edge to LDS) when the table row changes or the loop ends.  Their rows were found when the nodes were pushed
//     and travel in the path value (GePath), indexed by pair bit.
//   * the edges at the node chosen last change with every subset: one global 64-bit atomic each.  The row of
//     {S[ci], u} is the row of the CSR entry at which the candidate was found; the rows of the other edges at u are
//     found by bisection in the (ascending) adjacency row of the earlier node, where the bitset says u is.
// Integer adds commute: the result equals the host's bit for bit and does not change from call to call.
constexpr int GE_MAXC = 69, GE_CPAD = 72, GE_BANKS = 4, GE_WAVES = GT_THREADS / 64, GE_PAIRS = 10;

struct GeArgs {
  const int64_t* graph_ptr;
  const int64_t* rowptr;
  const int32_t* col;
  const int32_t* node_graph;
  const int64_t* bit_off;
  const unsigned long long* bits;
  const int32_t* entry_row;          // [num_entries] out row of the entry's edge
  const int16_t* eorb;               // [1098][10]
  int kmax, C;
  int64_t num_nodes, num_entries;
  unsigned long long* out;           // [num_rows][C]
};

struct GePath {
  int r[GE_PAIRS];                   // out row of the pair with that pair bit, where the pair is an edge
};

struct GeVisitor {
  static constexpr bool kWithEntry = true;
  using Path = GePath;
  using Level = GoRun;
  const int16_t* eorb;
  const int32_t* entry_row;
  const int64_t* rowptr;             // of this graph's nodes (local id)
  const int32_t* col;
  int32_t base;                      // the graph's first node
  unsigned* tally;                   // this lane's bank of the wave's columns: [GE_CPAD]
  unsigned long long* out;
  unsigned long long* out_own;       // out row of the item's edge
  int C;

  // add n to the wave's column of the item's own edge (see NO COUNT IS LOST above)
  __device__ __forceinline__ void wave_add(int column, unsigned long long n) const {
    if (n >> 32) atomicAdd(out_own + column, n & ~0xffffffffull);
    const unsigned lo = (unsigned)n;
    if (lo == 0) return;
    const unsigned old = atomicAdd(tally + column, lo);
    if (old > ~lo) atomicAdd(out_own + column, 1ull << 32);                  // the cell wrapped
  }
  // the CSR entry (s, u) for an edge {s, u}: u is in the ascending row of s, which therefore is not empty
  __device__ __forceinline__ int64_t entry_of(int s, int u) const {
    int64_t lo = rowptr[s], hi = rowptr[s + 1];
    const int32_t want = base + u;
    while (hi - lo > 1) {            // last entry with col <= want
      const int64_t mid = (lo + hi) >> 1;
      if (col[mid] <= want) lo = mid; else hi = mid;
    }
    return lo;
  }
  // u becomes node number NS: the rows of its edges to S[0..NS-1]
  template <int NS>
  __device__ __forceinline__ Path push_at(Path p, const int (&S)[ESU_KMAX], int u, unsigned ab, int ci,
                                          int64_t e) const {
#pragma unroll
    for (int j = 0; j < NS; ++j)
      if (ab >> j & 1) p.r[NS * (NS - 1) / 2 + j] = entry_row[j == ci ? e : entry_of(S[j], u)];
    return p;
  }
  // the run of the loop that chose node number NS goes out: the edges among S[0..NS-1]
  template <int NS>
  __device__ __forceinline__ void close_at(const int (&)[ESU_KMAX], const Path& p, GoRun& run) const {
    if (run.n == 0) return;
    const int16_t* row = eorb + run.t * GE_PAIRS;
    wave_add(row[0], run.n);
#pragma unroll
    for (int b = 1; b < NS * (NS - 1) / 2; ++b) {
      const int column = row[b];
      if (column >= 0) atomicAdd(out + (int64_t)p.r[b] * C + column, run.n);
    }
    run.n = 0;
  }
  template <int K>
  __device__ __forceinline__ void found(const int (&S)[ESU_KMAX], int, unsigned mask, const Path& p, GoRun& run) const {
    const int t = GT_OFF_DEV[K] + (int)mask;
    const int16_t* row = eorb + t * GE_PAIRS;
    if (row[0] < 0) return;          // pair bit 0 is the item's edge: set in every mask, so this is "class not asked for"
#pragma unroll
    for (int b = (K - 1) * (K - 2) / 2; b < K * (K - 1) / 2; ++b) {
      const int column = row[b];
      if (column >= 0) atomicAdd(out + (int64_t)p.r[b] * C + column, 1ull);
    }
    if (run.n && run.t != t) close_at<K - 1>(S, p, run);
    run.t = t;
    ++run.n;
  }
};

__global__ __launch_bounds__(GT_THREADS) void ge_count_kernel(GeArgs a) {
  __shared__ unsigned tally[GE_WAVES * GE_BANKS * GE_CPAD];
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned* wave_tally = tally + (tid >> 6) * (GE_BANKS * GE_CPAD);         // private to this wave: no block barrier
  const int64_t e = (int64_t)blockIdx.x * GE_WAVES + (tid >> 6);            // one wave per entry
  if (e >= a.num_entries) return;
  const int64_t v = esu_row_of_entry(a.rowptr, a.num_nodes, e);
  const EsuGraph c = esu_graph_of(a.graph_ptr, a.rowptr, a.col, a.node_graph, a.bit_off, a.bits, v, a.kmax);
  const int u0 = (int)(a.col[e] - c.base);
  if (u0 >= c.lv) return;                          // (wave-uniform) the root is the maximum of its subsets
  GeVisitor vis;
  vis.eorb = a.eorb;
  vis.entry_row = a.entry_row;
  vis.rowptr = a.rowptr + c.base;
  vis.col = a.col;
  vis.base = (int32_t)c.base;
  vis.C = a.C;
  vis.tally = wave_tally + (lane & (GE_BANKS - 1)) * GE_CPAD;
  vis.out = a.out;
  vis.out_own = a.out + (int64_t)a.entry_row[e] * a.C;
  for (int i = lane; i < GE_BANKS * GE_CPAD; i += 64) wave_tally[i] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane == 0) {
    const int column = a.eorb[(GT_OFF_DEV[2] + 1) * GE_PAIRS];
    if (column >= 0) vis.wave_add(column, 1);
  }
  GePath path{};
  esu_wave_walk(c, vis, v, e, u0, lane, path);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int column = lane; column < a.C; column += 64) {                    // contiguous cells of the item's row
    unsigned long long n = 0;
#pragma unroll
    for (int b = 0; b < GE_BANKS; ++b) n += wave_tally[b * GE_CPAD + column];
    if (n) atomicAdd(vis.out_own + column, n);
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

extern "C" int desco_edge_orbit_counts_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                           const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                           const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                           int64_t num_words, const int32_t* entry_row, int64_t num_rows,
                                           const int16_t* edge_orbit_table, int kmax, int num_columns, int64_t* out,
                                           desco_stream_t stream) {
  if (num_nodes == 0 || num_columns == 0 || num_rows == 0 || num_entries == 0) return 0;
  if (!graph_ptr || !rowptr || !col || !node_graph || !bit_off || !bits || !entry_row || !edge_orbit_table || !out ||
      num_graphs < 0 || num_nodes < 0 || num_entries < 0 || num_words < 0 || num_rows < 0 || num_rows > num_entries ||
      kmax < 2 || kmax > GT_KMAX || num_columns < 0 || num_columns > GE_MAXC)
    return fail(DESCO_EINVAL,
                "desco_edge_orbit_counts_dev: bad argument (queries of 2..5 nodes, at most 69 columns)");
  if (num_entries > INT32_MAX) return fail(DESCO_EINVAL, "desco_edge_orbit_counts_dev: too many edges");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, (size_t)num_rows * num_columns * 8, s) != hipSuccess)
    return launch_status("desco_edge_orbit_counts_dev: memset");
  if (const int rc = gt_build_bitsets(graph_ptr, rowptr, col, node_graph, bit_off, bits, num_words, num_nodes,
                                      num_entries, stream, "desco_edge_orbit_counts_dev"))
    return rc;
  const int64_t wblocks = (num_entries + GE_WAVES - 1) / GE_WAVES;
  GeArgs a{graph_ptr, rowptr, col, node_graph, bit_off, reinterpret_cast<const unsigned long long*>(bits),
           entry_row, edge_orbit_table, kmax, num_columns, num_nodes, num_entries,
           reinterpret_cast<unsigned long long*>(out)};
  hipLaunchKernelGGL(ge_count_kernel, dim3((unsigned)wblocks), dim3(GT_THREADS), 0, s, a);
  return launch_status("desco_edge_orbit_counts_dev");
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
