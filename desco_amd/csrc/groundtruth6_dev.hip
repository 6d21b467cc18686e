// Exact canonical counts of queries of 2..6 nodes on the GPU (C ABI: desco_canonical_counts6_dev).  Same definition
// as the host enumerator (groundtruth.cpp) and as gt_count_kernel (groundtruth_dev.hip):
//
//   out[v][q] = #{ node subsets S : max(S) = v, G[S] connected and isomorphic to query q }
//
// Enumeration: the shared device walk, groundtruth_esu_dev.hpp, to SIX nodes (the visitor declares kMax = 6): one
// wave per CSR entry (v, u0) with u0 < v, the third-node candidates dealt to the 64 lanes, the levels in registers.
// A 6-node induced mask has 15 bits; the class table (desco_canonical_class_table6) has 33 866 int16 entries and is
// read from global memory (the 2..5-node blocks, 2.2 KB, stay in L1; the 64 KiB 6-node block is served by L2).  A byte
// copy of the table in LDS under persistent workgroups was measured and lost; the tally without the run below was
// level on the benchmark shapes and behind on a hub: DESIGN.md 4.6 has the figures.
//
// ONE WALK FOR ALL COLUMNS (up to 142: every connected class of 2..6 nodes).  The tally is the node-orbit kernel's:
//   * a lane keeps ONE RUN per candidate loop in registers (G6Run: class id and a 64-bit length): while the subsets a
//     loop finds have the same class only the length is bumped; the run goes out when the class changes or the loop
//     ends.  The loop that chooses the last node of a star, a clique, a path or a molecule's chain finds one class.
//   * a run goes to the wave's u32 columns in LDS (G6_BANKS banks, bank = lane % G6_BANKS, to spread lanes that hit
//     one column), which are added to out[v][.] with one 64-bit atomic per non-zero column when the wave ends.
// NO COUNT IS LOST.  Widths: the run length is 64 bits (registers); an LDS cell is 32 bits and hands on its carry:
// every update is one LDS atomic add of lo < 2^32 that returns the cell's old value, so the add wraps at most once,
// exactly when old > ~lo; the updates of a cell are serialised, so every wrap is seen by the one update that caused it,
// and that update adds 2^32 to the global cell at once (the part of a run above 2^32 goes there directly).  The cell
// keeps the sum modulo 2^32 and the flush adds that remainder; the bank sum and the global cells are 64 bits.
// Integer adds commute: the result equals the host's bit for bit and does not change from call to call or with the
// slicing of the entries.
#include "groundtruth_esu_dev.hpp"

namespace desco {

constexpr int G6_THREADS = 256, G6_WAVES = G6_THREADS / 64, G6_BANKS = 4, G6_CPAD = 144;
static_assert(G6_CPAD >= ESU6_MAXQ, "a column per query");

// first entry of the k-node block of the class table (ESU6_OFF as a compile-time value in device code)
constexpr int g6_off(int k) { return k <= 2 ? 0 : k == 3 ? 2 : k == 4 ? 10 : k == 5 ? 74 : k == 6 ? 1098 : 33866; }
static_assert(g6_off(3) == ESU6_OFF[3] && g6_off(4) == ESU6_OFF[4] && g6_off(5) == ESU6_OFF[5] &&
              g6_off(6) == ESU6_OFF[6] && g6_off(7) == ESU6_OFF[7], "the table layout of groundtruth_esu.hpp");

struct G6Args {
  const int64_t* graph_ptr;
  const int64_t* rowptr;
  const int32_t* col;
  const int32_t* node_graph;
  const int64_t* bit_off;
  const unsigned long long* bits;
  const int16_t* cls;                // [33866] query index of the mask's isomorphism class, or -1
  int kmax, Q;
  int64_t num_nodes, entry_begin, items;
  unsigned long long* out;           // [N][Q]
};

struct G6Run {
  int q;                             // class (query index) of the run
  unsigned long long n;              // subsets in it
};

struct G6Visitor {
  static constexpr int kMax = ESU6_KMAX;
  using Path = EsuNone;
  using Level = G6Run;
  const int16_t* cls;
  unsigned* tally;                   // this lane's bank of the wave's columns: [G6_CPAD]
  unsigned long long* out_row;       // out row of the root v

  // add n to the wave's column (see NO COUNT IS LOST above)
  __device__ __forceinline__ void wave_add(int column, unsigned long long n) const {
    if (n >> 32) atomicAdd(out_row + column, n & ~0xffffffffull);
    const unsigned lo = (unsigned)n;
    if (lo == 0) return;
    const unsigned old = atomicAdd(tally + column, lo);
    if (old > ~lo) atomicAdd(out_row + column, 1ull << 32);                  // the cell wrapped
  }
  template <int NS>
  __device__ __forceinline__ Path push(Path p, int) const { return p; }
  // the run of the loop that chose node number NS goes out
  template <int NS>
  __device__ __forceinline__ void close(const int (&)[kMax], G6Run& run) const {
    if (run.n == 0) return;
    wave_add(run.q, run.n);
    run.n = 0;
  }
  template <int K>
  __device__ __forceinline__ void found(const int (&S)[kMax], int, unsigned mask, Path, G6Run& run) const {
    const int q = cls[g6_off(K) + (int)mask];
    if (q < 0) return;
    if (run.n && run.q != q) close<K - 1>(S, run);
    run.q = q;
    ++run.n;
  }
};

__global__ __launch_bounds__(G6_THREADS) void g6_count_kernel(G6Args a) {
  __shared__ unsigned tally[G6_WAVES * G6_BANKS * G6_CPAD];
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned* wave_tally = tally + (tid >> 6) * (G6_BANKS * G6_CPAD);          // private to this wave: no block barrier
  const int64_t item = (int64_t)blockIdx.x * G6_WAVES + (tid >> 6);          // one wave per entry of the slice
  if (item >= a.items) return;
  const int64_t e = a.entry_begin + item;
  const int64_t v = esu_row_of_entry(a.rowptr, a.num_nodes, e);
  const EsuGraph c = esu_graph_of(a.graph_ptr, a.rowptr, a.col, a.node_graph, a.bit_off, a.bits, v, a.kmax);
  const int u0 = (int)(a.col[e] - c.base);
  if (u0 >= c.lv) return;                          // (wave-uniform) the root is the maximum of its subsets
  G6Visitor vis;
  vis.cls = a.cls;
  vis.tally = wave_tally + (lane & (G6_BANKS - 1)) * G6_CPAD;
  vis.out_row = a.out + v * a.Q;
  for (int i = lane; i < G6_BANKS * G6_CPAD; i += 64) wave_tally[i] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane == 0) {
    const int q = a.cls[g6_off(2) + 1];
    if (q >= 0) vis.wave_add(q, 1);
  }
  esu_wave_walk(c, vis, v, e, u0, lane, EsuNone{});
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int column = lane; column < a.Q; column += 64) {                    // contiguous cells of the root's row
    unsigned long long n = 0;
#pragma unroll
    for (int b = 0; b < G6_BANKS; ++b) n += wave_tally[b * G6_CPAD + column];
    if (n) atomicAdd(vis.out_row + column, n);
  }
}

}  // namespace desco

using namespace desco;

extern "C" int desco_canonical_counts6_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                           const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                           const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                           int64_t num_words, const int16_t* cls, int kmax, int num_queries,
                                           int64_t entry_begin, int64_t entry_end, int64_t* out,
                                           desco_stream_t stream) {
  const char* who = "desco_canonical_counts6_dev";
  if (num_nodes == 0 || num_queries == 0) return 0;
  if (!graph_ptr || !rowptr || !node_graph || !bit_off || !bits || !cls || !out || num_graphs < 0 || num_nodes < 0 ||
      num_entries < 0 || num_words < 0 || kmax < 2 || kmax > ESU6_KMAX || num_queries < 0 ||
      num_queries > ESU6_MAXQ || (num_entries > 0 && !col) || entry_begin < 0 || entry_end < entry_begin ||
      entry_end > num_entries)
    return fail(DESCO_EINVAL, "desco_canonical_counts6_dev: bad argument (queries of 2..6 nodes, at most 142; "
                              "0 <= entry_begin <= entry_end <= num_entries)");
  hipStream_t s = (hipStream_t)stream;
  if (entry_begin == 0) {                          // the first slice: zero the counts, build the bitset rows
    if (hipMemsetAsync(out, 0, (size_t)num_nodes * num_queries * 8, s) != hipSuccess)
      return launch_status("desco_canonical_counts6_dev: memset");
    if (const int rc = gt_build_bitsets(graph_ptr, rowptr, col, node_graph, bit_off, bits, num_words, num_nodes,
                                        num_entries, stream, who))
      return rc;
  }
  const int64_t items = entry_end - entry_begin;
  if (items == 0) return 0;
  const int64_t blocks = (items + G6_WAVES - 1) / G6_WAVES;
  if (blocks > INT32_MAX) return fail(DESCO_EINVAL, "desco_canonical_counts6_dev: slice too large (entries / 4 > 2^31 - 1)");
  G6Args a{graph_ptr, rowptr, col, node_graph, bit_off, reinterpret_cast<const unsigned long long*>(bits), cls, kmax,
           num_queries, num_nodes, entry_begin, items, reinterpret_cast<unsigned long long*>(out)};
  hipLaunchKernelGGL(g6_count_kernel, dim3((unsigned)blocks), dim3(G6_THREADS), 0, s, a);
  return launch_status(who);
}
