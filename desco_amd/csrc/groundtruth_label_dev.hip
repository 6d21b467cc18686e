// Exact canonical ground-truth counts of LABELLED queries on the GPU (C ABI: desco_canonical_counts_labelled_dev).
// Same definition as the host enumerator (groundtruth_label.cpp):
//
//   count[v][c] = #{ node subsets S : max(S) = v, G[S] connected, and G[S] with its node labels
//                    isomorphic to the labelled queries of class c }
//
// Enumeration: the walk of groundtruth_dev.hip (ESU without extension lists; one wave per CSR entry (v, u0) with
// u0 < v, third-node candidates dealt round-robin to the lanes, subset / mask / cursors in registers, adjacency
// from per-graph bitset rows built by the same first kernel).  What differs:
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
#include "common_device.hpp"
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

struct GtlCtx {
  const int64_t* rowptr;
  const int32_t* col;
  const unsigned long long* bits;    // this graph's rows
  const int32_t* labels;             // this graph's labels
  const GtlArgs* a;
  int64_t base;
  int words, lv, kmax;
  unsigned long long* row;           // out[v]
  int run_c;                         // class of the pending run, -1 = none
  unsigned run_n;
};

__device__ __forceinline__ int64_t gtl_row_of_entry(const int64_t* __restrict__ rowptr, int64_t n, int64_t e) {
  int64_t lo = 0, hi = n;            // last row with rowptr[row] <= e
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rowptr[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ unsigned gtl_adj(const GtlCtx& c, int a, int b) {
  return (unsigned)(c.bits[(int64_t)a * c.words + (b >> 6)] >> (b & 63)) & 1u;
}

__device__ __forceinline__ void gtl_flush(GtlCtx& c) {
  if (c.run_c >= 0) atomicAdd(c.row + c.run_c, (unsigned long long)c.run_n);
  c.run_c = -1;
  c.run_n = 0;
}

template <int K>
__device__ __forceinline__ void gtl_classify(GtlCtx& c, unsigned mask, unsigned lab) {
  const unsigned idx = c.a->off[K] + mask * c.a->apow[K] + lab;
  if (idx >= c.a->table_entries) return;          // (a label id outside 0..A-1: never read past the table)
  const int cl = c.a->table[idx];
  if (cl < 0 || cl >= c.a->C) return;
  if (cl != c.run_c) {
    gtl_flush(c);
    c.run_c = cl;
  }
  ++c.run_n;
}

template <int NS>
__device__ void gtl_extend(GtlCtx& c, const int (&S)[GTL_KMAX_DEV], unsigned mask, unsigned lab, int ci0, int cp0);

// candidate at position e of the adjacency row (starting at r0) of S[ci] for node number NS of the subset: taken iff
// it is below the root, new, and adjacent to no subset node before S[ci].  Returns false when the row has passed the
// root's id (rows ascend: nothing further qualifies).
template <int NS>
__device__ __forceinline__ bool gtl_try(GtlCtx& c, const int (&S)[GTL_KMAX_DEV], unsigned mask, unsigned lab, int ci,
                                        int64_t r0, int64_t e) {
  const int u = (int)(c.col[e] - c.base);
  if (u >= c.lv) return false;
  unsigned ab = 0;
  bool in_s = false;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    in_s |= u == S[j];
    ab |= gtl_adj(c, S[j], u) << j;
  }
  if (in_s || (ab & ((1u << ci) - 1u))) return true;     // u entered the extension set earlier
  const unsigned m2 = mask | (ab << (NS * (NS - 1) / 2));
  const unsigned lab2 = lab + (unsigned)c.labels[u] * c.a->apow[NS];
  gtl_classify<NS + 1>(c, m2, lab2);
  if constexpr (NS + 1 < GTL_KMAX_DEV) {
    if (NS + 1 < c.kmax) {
      int S2[GTL_KMAX_DEV];
#pragma unroll
      for (int j = 0; j < GTL_KMAX_DEV; ++j) S2[j] = j < NS ? S[j] : 0;
      S2[NS] = u;
      gtl_extend<NS + 1>(c, S2, m2, lab2, ci, (int)(e - r0) + 1);
    }
  }
  return true;
}

// choose node number NS of the subset (S[0..NS-1] chosen, induced mask `mask`, label sum `lab`); candidates start at
// key (ci0, cp0)
template <int NS>
__device__ void gtl_extend(GtlCtx& c, const int (&S)[GTL_KMAX_DEV], unsigned mask, unsigned lab, int ci0, int cp0) {
#pragma unroll
  for (int ci = 0; ci < NS; ++ci) {
    if (ci < ci0) continue;
    const int64_t r0 = c.rowptr[c.base + S[ci]], r1 = c.rowptr[c.base + S[ci] + 1];
    for (int64_t e = r0 + (ci == ci0 ? cp0 : 0); e < r1; ++e)
      if (!gtl_try<NS>(c, S, mask, lab, ci, r0, e)) break;
  }
}

__global__ __launch_bounds__(GTL_THREADS) void gtl_count_kernel(GtlArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t e = (int64_t)blockIdx.x * (GTL_THREADS / 64) + (tid >> 6);     // one wave per entry
  if (e >= a.num_entries) return;
  const int64_t v = gtl_row_of_entry(a.rowptr, a.num_nodes, e);
  const int g = a.node_graph[v];
  GtlCtx c;
  c.rowptr = a.rowptr;
  c.col = a.col;
  c.a = &a;
  c.base = a.graph_ptr[g];
  c.words = (int)((a.graph_ptr[g + 1] - c.base + 63) >> 6);
  c.bits = a.bits + a.bit_off[g];
  c.labels = a.labels + c.base;
  c.lv = (int)(v - c.base);
  c.kmax = a.kmax;
  c.row = a.out + v * a.C;
  c.run_c = -1;
  c.run_n = 0;
  const int u0 = (int)(a.col[e] - c.base);
  if (u0 >= c.lv) return;                          // the root is the maximum of its subsets
  const int S[GTL_KMAX_DEV] = {c.lv, u0, 0, 0, 0};
  const unsigned lab = (unsigned)c.labels[c.lv] + (unsigned)c.labels[u0] * a.apow[1];
  if (lane == 0) gtl_classify<2>(c, 1u, lab);
  if (c.kmax > 2) {
    // candidates for the third node: v's row behind u0, then u0's row; position p -> lane p % 64
    const int64_t v0 = a.rowptr[v], v1 = a.rowptr[v + 1];
    const int64_t w0 = a.rowptr[c.base + u0], w1 = a.rowptr[c.base + u0 + 1];
    const int64_t rest = v1 - (e + 1), total = rest + (w1 - w0);
    for (int64_t p = lane; p < total; p += 64) {
      if (p < rest)
        gtl_try<2>(c, S, 1u, lab, 0, v0, e + 1 + p);
      else
        gtl_try<2>(c, S, 1u, lab, 1, w0, w0 + (p - rest));
    }
  }
  gtl_flush(c);
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
