// Exact canonical ground-truth counts of LABELLED queries on the GPU (C ABI: desco_canonical_counts_labelled_dev).
// Same definition as the host enumerator (groundtruth_label.cpp):
//
//   count[v][c] = #{ node subsets S : max(S) = v, G[S] connected, and G[S] with its node labels
//                    isomorphic to the labelled queries of class c }
//
// Enumeration: the shared device walk, groundtruth_esu_dev.hpp (ESU without extension lists; one wave per CSR entry
// (v, u0) with u0 < v, third-node candidates dealt round-robin to the lanes, subset / mask / cursors in registers,
// adjacency from per-graph bitset rows built by the same first kernel).  This kernel's visitor adds:
//
// Classification.  The label id of a node is gathered once, when the node is chosen, and carried down the levels as
// the running sum  lab = sum_j l_j A^j ; a found k-subset reads ONE int32 of the direct table at
// off[k] + mask A^k + lab  (groundtruth_label.hpp), which holds its class or -1.  The table is read-only and a
// graph set touches only the few entries of the (mask, labels) combinations it contains, so the reads stay in L2.
//
// Tally.  The number of classes runs to hundreds of thousands and most never occur, so there is no per-thread
// counter column: every lane keeps the class of its last hit and a run length in registers (consecutive subsets of
// one lane mostly differ in their last node only and fall into few classes) and adds the run to out[v][c] with one
// 64-bit global atomic when the class changes.  Integer adds: the result does not depend on arrival order.  All
// hits of one wave go to the one row v; the entries rooted at a hub spread over that row's classes.
#include "groundtruth_esu_dev.hpp"
#include "groundtruth_label.hpp"


namespace desco {

constexpr int GTL_THREADS = 256;

struct GtlArgs {
  const int64_t* graph_ptr;
  const int64_t* rowptr;
  const int32_t* col;
  const int32_t* node_graph;
  const int64_t* bit_off;            // [G] first bitset word of graph g
  const unsigned long long* bits;
  const int32_t* labels;             // [N] label id of every node
  const int32_t* table;              // class of (mask, labels), or -1
  unsigned off[GTL_KMAX_DEV + 2];    // table blocks (entries < 2^31: checked on the host)
  unsigned apow[GTL_KMAX_DEV + 1];   // A^j
  unsigned table_entries;
  int kmax, C;
  int64_t num_nodes, num_entries;
  unsigned long long* out;           // [N][C]
};

struct GtlVisitor {
  using Path = unsigned;             // the running label sum
  using Level = EsuNone;
  const GtlArgs* a;
  const int32_t* labels;             // this graph's labels
  unsigned long long* row;           // out[v]
  int run_c;                         // class of the pending run, -1 = none
  unsigned run_n;

  __device__ __forceinline__ void flush() {
    if (run_c >= 0) atomicAdd(row + run_c, (unsigned long long)run_n);
    run_c = -1;
    run_n = 0;
  }
  template <int K>
  __device__ __forceinline__ void classify(unsigned mask, unsigned lab) {
    const unsigned idx = a->off[K] + mask * a->apow[K] + lab;
    if (idx >= a->table_entries) return;          // (a label id outside 0..A-1: never read past the table)
    const int cl = a->table[idx];
    if (cl < 0 || cl >= a->C) return;
    if (cl != run_c) {
      flush();
      run_c = cl;
    }
    ++run_n;
  }
  template <int NS>
  __device__ __forceinline__ Path push(Path lab, int u) const {
    return lab + (unsigned)labels[u] * a->apow[NS];
  }
  template <int K>
  __device__ __forceinline__ void found(const int (&)[ESU_KMAX], int, unsigned mask, Path lab, Level&) {
    classify<K>(mask, lab);
  }
  template <int NS>
  __device__ __forceinline__ void close(const int (&)[ESU_KMAX], Level&) const {}
};

__global__ __launch_bounds__(GTL_THREADS) void gtl_count_kernel(GtlArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t e = (int64_t)blockIdx.x * (GTL_THREADS / 64) + (tid >> 6);     // one wave per entry
  if (e >= a.num_entries) return;
  const int64_t v = esu_row_of_entry(a.rowptr, a.num_nodes, e);
  const EsuGraph c = esu_graph_of(a.graph_ptr, a.rowptr, a.col, a.node_graph, a.bit_off, a.bits, v, a.kmax);
  GtlVisitor vis{&a, a.labels + c.base, a.out + v * a.C, -1, 0};
  const int u0 = (int)(a.col[e] - c.base);
  if (u0 >= c.lv) return;                          // the root is the maximum of its subsets
  const unsigned lab = (unsigned)vis.labels[c.lv] + (unsigned)vis.labels[u0] * a.apow[1];
  if (lane == 0) vis.classify<2>(1u, lab);
  esu_wave_walk(c, vis, v, e, u0, lane, lab);
  vis.flush();
}

}  // namespace desco

using namespace desco;

extern "C" int desco_canonical_counts_labelled_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                                   const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                                   const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                                   int64_t num_words, const int32_t* labels, int num_labels,
                                                   const int32_t* table, int64_t table_entries, int kmax,
                                                   int num_classes, int64_t* out, desco_stream_t stream) {
  if (num_nodes == 0 || num_classes == 0) return 0;
  if (!graph_ptr || !rowptr || !node_graph || !bit_off || !bits || !labels || !table || !out || num_graphs < 0 ||
      num_nodes < 0 || num_entries < 0 || num_words < 0 || num_classes < 0 || (num_entries > 0 && !col))
    return fail(DESCO_EINVAL, "desco_canonical_counts_labelled_dev: bad argument");
  if (kmax < 2 || kmax > GTL_KMAX_DEV)
    return fail(DESCO_EINVAL, "desco_canonical_counts_labelled_dev: the device path takes queries of 2..5 nodes");
  if (num_labels < 1 || num_labels > GTL_AMAX_DEV)
    return fail(DESCO_EINVAL, "desco_canonical_counts_labelled_dev: the device path takes 1..16 label ids");
  const GtlLayout lay = gtl_layout(kmax, num_labels);
  if (table_entries != lay.off[kmax + 1] || table_entries > INT32_MAX)
    return fail(DESCO_EINVAL, "desco_canonical_counts_labelled_dev: table_entries is not "
                              "desco_canonical_label_table_size(kmax, num_labels), or is above 2^31 - 1");
  const int64_t wblocks = (num_entries + GTL_THREADS / 64 - 1) / (GTL_THREADS / 64);
  if (wblocks > INT32_MAX) return fail(DESCO_EINVAL, "desco_canonical_counts_labelled_dev: too many edges");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, (size_t)num_nodes * num_classes * 8, s) != hipSuccess)
    return launch_status("desco_canonical_counts_labelled_dev: memset");
  if (const int rc = gt_build_bitsets(graph_ptr, rowptr, col, node_graph, bit_off, bits, num_words, num_nodes,
                                      num_entries, stream, "desco_canonical_counts_labelled_dev"))
    return rc;
  if (num_entries == 0) return 0;
  GtlArgs a{};
  a.graph_ptr = graph_ptr;
  a.rowptr = rowptr;
  a.col = col;
  a.node_graph = node_graph;
  a.bit_off = bit_off;
  a.bits = reinterpret_cast<const unsigned long long*>(bits);
  a.labels = labels;
  a.table = table;
  for (int k = 0; k <= GTL_KMAX_DEV + 1; ++k) a.off[k] = (unsigned)lay.off[k < kmax + 1 ? k : kmax + 1];
  // (A^j for j <= kmax is below the table size; the higher powers are never used)
  for (int j = 0; j <= GTL_KMAX_DEV; ++j) a.apow[j] = j <= kmax ? (unsigned)lay.apow[j] : 0u;
  a.table_entries = (unsigned)table_entries;
  a.kmax = kmax;
  a.C = num_classes;
  a.num_nodes = num_nodes;
  a.num_entries = num_entries;
  a.out = reinterpret_cast<unsigned long long*>(out);
  hipLaunchKernelGGL(gtl_count_kernel, dim3((unsigned)wblocks), dim3(GTL_THREADS), 0, s, a);
  return launch_status("desco_canonical_counts_labelled_dev");
}
