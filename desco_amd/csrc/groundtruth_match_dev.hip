// Exact canonical ground-truth counts of LARGE queries on the GPU (C ABI: desco_canonical_counts_match_dev and its
// labelled form desco_canonical_counts_match_labelled_dev).
// Same definition and same plan as the host matcher (groundtruth_match.cpp, groundtruth_match.hpp):
//
//   count[v][q] = #{ node subsets S : max(S) = v, G[S] isomorphic to query q }      (induced)
//
// counted as the maps of q into G that send the record's anchor to v, every other node below v, match edges AND
// non-edges against all earlier positions and meet the record's order constraints -- one map per subset.
//
// Work item = (CSR entry (v, u0) with u0 < v, plan record), handled by ONE WAVE (the split groundtruth_dev.hip
// adopted: the items rooted at hubs grow with the cube of the degree and worse, one thread per item left whole
// launches waiting for them).  u0 is the image of position 1, whose candidates are v's row by construction; an item
// whose u0 is not below v retires at once.  The candidates of position 2 (the adjacency row of the image of its
// parent, v or u0) are dealt round-robin to the 64 lanes, and every lane walks positions 3..k-1 depth-first on its
// own: images (int32) and row cursors (int64 entry indices) live in a per-lane LDS column, 16 levels deep
// (192 B per lane, 48 KB per workgroup of 256: three workgroups per CU of the 160 KB LDS); the record's
// per-position words sit in LDS once per wave.  Adjacency tests read the per-graph bitset rows that
// gt_build_bitsets makes (the first kernel of desco_canonical_counts_dev).  A lane counts its matches in a
// register; the wave reduces them and issues one 64-bit integer atomic per item: bit-identical from run to run.
//
// The work of a large query on a dense graph is unbounded in principle (as VF2's is), so one call covers only the
// CSR entries [entry_begin, entry_end): the caller cuts the entries into slices and checks every status.
//
// LABELLED form (the second instantiation of the kernel template; the unlabelled one compiles to what it was).  The
// plan is the labelled one (groundtruth_match.hpp): records over labelled classes, sorted by (label of position 0,
// label of position 1), with a bucket table.  The reference's F^k expansion gives hundreds of records of which almost
// all die on the labels of v and u0, so the work item is (CSR entry, j) with j < the LARGEST BUCKET: the wave reads
// label[v] and label[u0], finds their bucket (lane i compares bucket i; no bucket: a label no query position carries,
// retire) and takes the bucket's j-th record, or retires when the bucket is shorter.  Dead items dominate, so the row
// of the entry is found by the whole wave too (64 probes per step).  Every surviving item has positions 0 and 1
// matched; the label of a later position's candidate (one 4-byte load; the wanted label sits in LDS with the rest
// of the record) is tested before the bitset loop.
//
// NON-INDUCED mode (desco_canonical_counts_match_mode_dev, desco_canonical_counts_match_labelled_mode_dev with
// induced = 0; two more instantiations of the kernel template, the two above compile to what they were): count[v][q] =
// the occurrences of q as a not necessarily induced subgraph whose largest node is v, i.e. the injective edge-preserving
// maps with maximum image v divided by |Aut(q)|.  Same plans, same items, same slices: a set adjacency-mask bit still
// asks for an edge, a clear bit asks nothing (groundtruth_match.cpp has the argument).
#include <type_traits>

#include "groundtruth_esu_dev.hpp"
#include "groundtruth_match.hpp"

namespace desco {

constexpr int GTM_THREADS = 256, GTM_WAVES = GTM_THREADS / 64;

struct GtmArgs {
  const int64_t* graph_ptr;
  const int64_t* rowptr;
  const int32_t* col;
  const int32_t* node_graph;
  const int64_t* bit_off;
  const unsigned long long* bits;
  const int32_t* plan;               // device copy, header included
  int num_anchors, Q;
  int64_t num_nodes, entry_begin, num_items;       // items = (entry_end - entry_begin) * num_anchors
  unsigned long long* out;           // [N][Q]
};

struct GtmLabArgs : GtmArgs {          // num_anchors = the largest bucket: items = (entry_end - entry_begin) * that
  const int32_t* labels;               // [N]
  const int32_t* buckets;              // the plan's bucket table (device)
  int num_buckets;
};

// the same arguments for the non-induced instantiations (the type selects the mode at compile time)
struct GtmMonoArgs : GtmArgs {};
struct GtmLabMonoArgs : GtmLabArgs {};

// The row of esu_row_of_entry (groundtruth_esu_dev.hpp), found by the whole wave: lane i probes the i-th of 64 evenly
// spaced rows of [lo, hi), so that a dead item of the labelled kernel costs three dependent loads here instead of
// log2(n).  All 64 lanes are active.
__device__ __forceinline__ int64_t gtm_row_of_entry_wave(const int64_t* __restrict__ rowptr, int64_t n, int64_t e,
                                                         int lane) {
  int64_t lo = 0, hi = n;            // rowptr[lo] <= e, the answer is in [lo, hi)
  while (hi - lo > 1) {
    const int64_t step = (hi - lo + 63) >> 6, p = lo + lane * step;
    const int c = __popcll(__ballot(p < hi && rowptr[p] <= e));          // a prefix of the lanes, lane 0 included
    hi = min(hi, lo + c * step);
    lo += (c - 1) * step;
  }
  return lo;
}

struct GtmCtx {
  const unsigned long long* bits;    // this graph's rows
  int words, lv;
  const int* img;                    // this lane's LDS column (stride GTM_THREADS)
  const unsigned* lvl;               // this wave's record: [2 * i] = adj | parent << 16, [2 * i + 1] = lt | gt << 16
  const int32_t* lab;                // labelled: this graph's node labels, and
  const int* qlab;                   // this wave's per-position labels (LDS)
};

// does u fit position `level`, given the images of the positions before it?  IND: a clear mask bit means NOT adjacent
template <bool LAB, bool IND>
__device__ __forceinline__ bool gtm_fits(const GtmCtx& c, int level, int u) {
  if constexpr (LAB) {
    if (c.lab[u] != c.qlab[level]) return false;
  }
  const unsigned want = c.lvl[2 * level] & 0xffffu, order = c.lvl[2 * level + 1];
  const unsigned long long* row = c.bits + (int64_t)u * c.words;
  for (int j = 0; j < level; ++j) {
    const int w = c.img[j * GTM_THREADS];
    const unsigned a = (unsigned)(row[w >> 6] >> (w & 63)) & 1u;
    if constexpr (IND) {
      if (u == w || a != ((want >> j) & 1u)) return false;
    } else {
      if (u == w || (((want >> j) & 1u) & ~a)) return false;
    }
    if (((order >> j) & 1u) && !(u < w)) return false;
    if (((order >> (16 + j)) & 1u) && !(u > w)) return false;
  }
  return true;
}

template <class Args>
__global__ __launch_bounds__(GTM_THREADS) void gtm_count_kernel(Args a) {
  constexpr bool LAB = std::is_base_of<GtmLabArgs, Args>::value;
  constexpr bool IND = !std::is_same<Args, GtmMonoArgs>::value && !std::is_same<Args, GtmLabMonoArgs>::value;
  constexpr int HEAD = LAB ? GTML_HEAD : GTM_HEAD, REC = LAB ? GTML_REC : GTM_REC;
  __shared__ int img_s[GTM_KMAX * GTM_THREADS];
  __shared__ long long cur_s[GTM_KMAX * GTM_THREADS];
  __shared__ unsigned lvl_s[GTM_WAVES * 2 * GTM_KMAX];
  __shared__ int qlab_s[LAB ? GTM_WAVES * GTM_KMAX : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t item = (int64_t)blockIdx.x * GTM_WAVES + wave;
  bool live = item < a.num_items;
  int anchor = live ? (int)(item % a.num_anchors) : 0;
  int64_t e = 0, v = 0;
  if constexpr (LAB) {                             // the record: the (item % largest bucket)-th of bucket (label v, label u0)
    if (live) {
      e = a.entry_begin + item / a.num_anchors;
      v = gtm_row_of_entry_wave(a.rowptr, a.num_nodes, e, lane);
      const int64_t u = a.col[e];
      live = u < v;                                // the root is the maximum of its subsets
      if (live) {
        const int32_t l0 = a.labels[v], l1 = a.labels[u];
        live = false;
        for (int b0 = 0; b0 < a.num_buckets; b0 += 64) {         // lane i reads bucket b0 + i: one load per 64 buckets
          const int32_t* b = a.buckets + (int64_t)min(b0 + lane, a.num_buckets - 1) * GTML_BUCKET;
          const unsigned long long hit = __ballot(b0 + lane < a.num_buckets && b[0] == l0 && b[1] == l1);
          if (hit) {
            const int32_t* mine = a.buckets + (int64_t)(b0 + __ffsll(hit) - 1) * GTML_BUCKET;
            live = mine[2] + anchor < mine[3];
            if (live) anchor += mine[2];
            break;
          }
        }
      }
    }
    if (!live) anchor = 0;
  }
  const int32_t* rec = a.plan + HEAD + (int64_t)anchor * REC;
  unsigned* lvl = lvl_s + wave * 2 * GTM_KMAX;
  if (lane < GTM_KMAX) {
    lvl[2 * lane] = ((unsigned)rec[GTM_ADJ + lane] & 0xffffu) | ((unsigned)rec[GTM_PARENT + lane] << 16);
    lvl[2 * lane + 1] = ((unsigned)rec[GTM_LT + lane] & 0xffffu) | ((unsigned)rec[GTM_GT + lane] << 16);
    if constexpr (LAB) qlab_s[wave * GTM_KMAX + lane] = rec[GTML_LABEL + lane];
  }
  __syncthreads();                                 // (the only barrier: every wave reaches it)
  if (!live) return;
  const int k = rec[GTM_K], q = rec[GTM_QUERY];
  if constexpr (!LAB) {
    e = a.entry_begin + item / a.num_anchors;
    v = esu_row_of_entry(a.rowptr, a.num_nodes, e);
  }
  const int g = a.node_graph[v];
  const int64_t base = a.graph_ptr[g];
  GtmCtx c;
  c.words = (int)((a.graph_ptr[g + 1] - base + 63) >> 6);
  c.bits = a.bits + a.bit_off[g];
  c.lv = (int)(v - base);
  c.lvl = lvl;
  if constexpr (LAB) {
    c.lab = a.labels + base;
    c.qlab = qlab_s + wave * GTM_KMAX;
  }
  int* img = img_s + tid;
  long long* cur = cur_s + tid;
  c.img = img;
  const int u0 = (int)(a.col[e] - base);
  if (u0 >= c.lv) return;                          // the root is the maximum of its subsets
  img[0] = c.lv;
  img[GTM_THREADS] = u0;                           // (position 1: adjacent to the root, nothing else to test)
  unsigned long long found = 0;
  if (k == 2) {
    found = lane == 0;
  } else {
    const int64_t p2 = base + img[(lvl[4] >> 16) * GTM_THREADS];
    const int64_t r0 = a.rowptr[p2], r1 = a.rowptr[p2 + 1];
    for (int64_t e2 = r0 + lane; e2 < r1; e2 += 64) {
      const int u2 = (int)(a.col[e2] - base);
      if (u2 >= c.lv) break;                       // rows ascend
      if (!gtm_fits<LAB, IND>(c, 2, u2)) continue;
      if (k == 3) {
        ++found;
        continue;
      }
      img[2 * GTM_THREADS] = u2;
      int level = 3;
      cur[3 * GTM_THREADS] = a.rowptr[base + img[(lvl[6] >> 16) * GTM_THREADS]];
      while (level >= 3) {
        const int64_t p = base + img[(lvl[2 * level] >> 16) * GTM_THREADS];
        const int64_t ec = cur[level * GTM_THREADS];
        int u = c.lv;
        if (ec < a.rowptr[p + 1]) u = (int)(a.col[ec] - base);
        if (u >= c.lv) {                           // row exhausted or past the root: back up
          --level;
          continue;
        }
        cur[level * GTM_THREADS] = ec + 1;
        if (!gtm_fits<LAB, IND>(c, level, u)) continue;
        if (level + 1 == k) {
          ++found;
        } else {
          img[level * GTM_THREADS] = u;
          ++level;
          cur[level * GTM_THREADS] = a.rowptr[base + img[(lvl[2 * level] >> 16) * GTM_THREADS]];
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) found += __shfl_xor(found, o, 64);
  if (lane == 0 && found) atomicAdd(a.out + v * a.Q + q, found);
}

}  // namespace desco

using namespace desco;

namespace {

template <class Args>
int gtm_launch(const std::string& name, const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
               const int64_t* rowptr, int64_t num_entries, const int32_t* col, const int32_t* node_graph,
               const int64_t* bit_off, uint64_t* bits, int64_t num_words, const int32_t* plan_host,
               const int32_t* plan_dev, int64_t plan_entries, int num_queries, int64_t entry_begin, int64_t entry_end,
               int64_t* out, desco_stream_t stream) {
  const char* who = name.c_str();
  if (num_nodes == 0 || num_queries == 0) return 0;
  if (!graph_ptr || !rowptr || !node_graph || !bit_off || !bits || !plan_dev || !out || num_graphs < 0 ||
      num_nodes < 0 || num_entries < 0 || num_words < 0 || num_queries < 0 || (num_entries > 0 && !col) ||
      entry_begin < 0 || entry_end < entry_begin || entry_end > num_entries)
    return fail(DESCO_EINVAL, (name + ": bad argument").c_str());
  if (const int rc = match_plan_check(who, plan_host, plan_entries, num_queries)) return rc;
  const int num_anchors = plan_host[1];
  hipStream_t s = (hipStream_t)stream;
  if (entry_begin == 0) {                          // the first slice: zero the counts, build the bitset rows
    if (hipMemsetAsync(out, 0, (size_t)num_nodes * num_queries * 8, s) != hipSuccess)
      return launch_status((name + ": memset").c_str());
    if (const int rc = gt_build_bitsets(graph_ptr, rowptr, col, node_graph, bit_off, bits, num_words, num_nodes,
                                        num_entries, stream, who))
      return rc;
  }
  const int64_t items = (entry_end - entry_begin) * num_anchors;
  if (items == 0) return 0;
  const int64_t blocks = (items + GTM_WAVES - 1) / GTM_WAVES;
  if (blocks > INT32_MAX)
    return fail(DESCO_EINVAL, (name + ": slice too large (entries x anchors / 4 > 2^31 - 1)").c_str());
  Args a;
  static_cast<GtmArgs&>(a) = GtmArgs{graph_ptr, rowptr, col, node_graph, bit_off,
                                     reinterpret_cast<const unsigned long long*>(bits), plan_dev, num_anchors,
                                     num_queries, num_nodes, entry_begin, items,
                                     reinterpret_cast<unsigned long long*>(out)};
  hipLaunchKernelGGL(gtm_count_kernel<Args>, dim3((unsigned)blocks), dim3(GTM_THREADS), 0, s, a);
  return launch_status(who);
}

template <class Args>
int gtm_launch_labelled(const std::string& name, const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                        const int64_t* rowptr, int64_t num_entries, const int32_t* col, const int32_t* node_graph,
                        const int64_t* bit_off, uint64_t* bits, int64_t num_words, const int32_t* labels,
                        const int32_t* plan_host, const int32_t* plan_dev, int64_t plan_entries, int num_classes,
                        int64_t entry_begin, int64_t entry_end, int64_t* out, desco_stream_t stream) {
  const char* who = name.c_str();
  if (num_nodes == 0 || num_classes == 0) return 0;
  if (!graph_ptr || !rowptr || !node_graph || !bit_off || !bits || !labels || !plan_dev || !out || num_graphs < 0 ||
      num_nodes < 0 || num_entries < 0 || num_words < 0 || num_classes < 0 || (num_entries > 0 && !col) ||
      entry_begin < 0 || entry_end < entry_begin || entry_end > num_entries)
    return fail(DESCO_EINVAL, (name + ": bad argument").c_str());
  if (const int rc = match_plan_labelled_check(who, plan_host, plan_entries, num_classes)) return rc;
  const int num_recs = plan_host[1], num_buckets = plan_host[2], largest = plan_host[3];
  hipStream_t s = (hipStream_t)stream;
  if (entry_begin == 0) {                          // the first slice: zero the counts, build the bitset rows
    if (hipMemsetAsync(out, 0, (size_t)num_nodes * num_classes * 8, s) != hipSuccess)
      return launch_status((name + ": memset").c_str());
    if (const int rc = gt_build_bitsets(graph_ptr, rowptr, col, node_graph, bit_off, bits, num_words, num_nodes,
                                        num_entries, stream, who))
      return rc;
  }
  const int64_t items = (entry_end - entry_begin) * largest;     // (entry, j-th record of the entry's bucket)
  if (items == 0) return 0;
  const int64_t blocks = (items + GTM_WAVES - 1) / GTM_WAVES;
  if (blocks > INT32_MAX)
    return fail(DESCO_EINVAL, (name + ": slice too large (entries x largest bucket / 4 > 2^31 - 1)").c_str());
  Args a;
  static_cast<GtmArgs&>(a) = GtmArgs{graph_ptr, rowptr, col, node_graph, bit_off,
                                     reinterpret_cast<const unsigned long long*>(bits), plan_dev, largest, num_classes,
                                     num_nodes, entry_begin, items, reinterpret_cast<unsigned long long*>(out)};
  a.labels = labels;
  a.buckets = plan_dev + GTML_HEAD + (int64_t)num_recs * GTML_REC;
  a.num_buckets = num_buckets;
  hipLaunchKernelGGL(gtm_count_kernel<Args>, dim3((unsigned)blocks), dim3(GTM_THREADS), 0, s, a);
  return launch_status(who);
}

}  // namespace

extern "C" int desco_canonical_counts_match_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                                const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                                const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                                int64_t num_words, const int32_t* plan_host, const int32_t* plan_dev,
                                                int64_t plan_entries, int num_queries, int64_t entry_begin,
                                                int64_t entry_end, int64_t* out, desco_stream_t stream) {
  return gtm_launch<GtmArgs>("desco_canonical_counts_match_dev", graph_ptr, num_graphs, num_nodes, rowptr, num_entries,
                             col, node_graph, bit_off, bits, num_words, plan_host, plan_dev, plan_entries, num_queries,
                             entry_begin, entry_end, out, stream);
}

extern "C" int desco_canonical_counts_match_mode_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                                     const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                                     const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                                     int64_t num_words, const int32_t* plan_host,
                                                     const int32_t* plan_dev, int64_t plan_entries, int num_queries,
                                                     int induced, int64_t entry_begin, int64_t entry_end, int64_t* out,
                                                     desco_stream_t stream) {
  const char* who = "desco_canonical_counts_match_mode_dev";
  if (induced != 0 && induced != 1)
    return fail(DESCO_EINVAL, "desco_canonical_counts_match_mode_dev: induced must be 0 or 1");
  return induced ? gtm_launch<GtmArgs>(who, graph_ptr, num_graphs, num_nodes, rowptr, num_entries, col, node_graph,
                                       bit_off, bits, num_words, plan_host, plan_dev, plan_entries, num_queries,
                                       entry_begin, entry_end, out, stream)
                 : gtm_launch<GtmMonoArgs>(who, graph_ptr, num_graphs, num_nodes, rowptr, num_entries, col, node_graph,
                                           bit_off, bits, num_words, plan_host, plan_dev, plan_entries, num_queries,
                                           entry_begin, entry_end, out, stream);
}

extern "C" int desco_canonical_counts_match_labelled_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                                         const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                                         const int32_t* node_graph, const int64_t* bit_off,
                                                         uint64_t* bits, int64_t num_words, const int32_t* labels,
                                                         const int32_t* plan_host, const int32_t* plan_dev,
                                                         int64_t plan_entries, int num_classes, int64_t entry_begin,
                                                         int64_t entry_end, int64_t* out, desco_stream_t stream) {
  return gtm_launch_labelled<GtmLabArgs>("desco_canonical_counts_match_labelled_dev", graph_ptr, num_graphs, num_nodes,
                                         rowptr, num_entries, col, node_graph, bit_off, bits, num_words, labels,
                                         plan_host, plan_dev, plan_entries, num_classes, entry_begin, entry_end, out,
                                         stream);
}

extern "C" int desco_canonical_counts_match_labelled_mode_dev(
    const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes, const int64_t* rowptr, int64_t num_entries,
    const int32_t* col, const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits, int64_t num_words,
    const int32_t* labels, const int32_t* plan_host, const int32_t* plan_dev, int64_t plan_entries, int num_classes,
    int induced, int64_t entry_begin, int64_t entry_end, int64_t* out, desco_stream_t stream) {
  const char* who = "desco_canonical_counts_match_labelled_mode_dev";
  if (induced != 0 && induced != 1)
    return fail(DESCO_EINVAL, "desco_canonical_counts_match_labelled_mode_dev: induced must be 0 or 1");
  return induced ? gtm_launch_labelled<GtmLabArgs>(who, graph_ptr, num_graphs, num_nodes, rowptr, num_entries, col,
                                                   node_graph, bit_off, bits, num_words, labels, plan_host, plan_dev,
                                                   plan_entries, num_classes, entry_begin, entry_end, out, stream)
                 : gtm_launch_labelled<GtmLabMonoArgs>(who, graph_ptr, num_graphs, num_nodes, rowptr, num_entries, col,
                                                       node_graph, bit_off, bits, num_words, labels, plan_host,
                                                       plan_dev, plan_entries, num_classes, entry_begin, entry_end, out,
                                                       stream);
}
