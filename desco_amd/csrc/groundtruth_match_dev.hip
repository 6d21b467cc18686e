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
//
// The kernel template itself is groundtruth_match_dev.hpp: occurrences_dev.hip instantiates it twice more, to LIST the
// maps instead of counting them; the four instantiations here compile to what they were.
#include "groundtruth_match_dev.hpp"

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
