// Listing the occurrences of ONE query on the GPU (C ABI: desco_list_occurrences_dev; definition in
// include/desco_hip.h, OCCURRENCE LISTING; host twin desco_list_occurrences in groundtruth_match.cpp).
//
// The kernel is the matcher's walk (gtm_count_kernel, groundtruth_match_dev.hpp) instantiated to LIST: same work item
// (one wave per (CSR entry, anchor record)), same LDS columns, same single barrier -- but where the counting
// instantiations add 1 to a register, a lane that completes a map
//   1. takes slot = atomicAdd(&cursor[v], 1) (a returning atomic on the anchor's own word),
//   2. sets *overflow and stores nothing if the slot is outside the anchor's segment [ptr[v], ptr[v + 1]) or the
//      destination row outside [0, rows_capacity),
//   3. else stores its k images, permuted from matching positions to query-node order, as row
//      ptr[v] - ptr_base + slot.
// ptr is the exclusive scan of the matcher's own count column, so with a correct ptr every slot is taken exactly once
// and nothing overflows; with ANY ptr, cursor or plan_dev no store leaves rows[0 .. rows_capacity * k) (gtm_emit checks
// slot, row and column).  The order of the rows inside a segment is the order of arrival: the caller sorts every
// segment (desco_amd/occurrences.py) to reach the defined, bit-identical order.
#include "groundtruth_match_dev.hpp"
#include "occurrences.hpp"

using namespace desco;

namespace {

template <class Args>
int list_launch(const char* who, const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes, const int64_t* rowptr,
                int64_t num_entries, const int32_t* col, const int32_t* node_graph, const int64_t* bit_off,
                uint64_t* bits, int64_t num_words, const int32_t* plan_host, const int32_t* plan_dev,
                int64_t plan_entries, int64_t entry_begin, int64_t entry_end, const int64_t* ptr, int64_t ptr_base,
                int32_t* cursor, int64_t rows_capacity, int32_t* rows, int32_t* overflow, desco_stream_t stream) {
  const std::string name(who);
  if (num_graphs < 0 || num_nodes < 0 || num_entries < 0 || num_words < 0 || rows_capacity < 0)
    return fail(DESCO_EINVAL, (name + ": negative size").c_str());
  if (!graph_ptr || !rowptr || !node_graph || !bit_off || !bits || !plan_dev || !ptr || !cursor || !overflow ||
      (num_entries > 0 && !col) || (rows_capacity > 0 && !rows))
    return fail(DESCO_EINVAL, (name + ": null pointer").c_str());
  if (entry_begin < 0 || entry_end < entry_begin || entry_end > num_entries)
    return fail(DESCO_EINVAL, (name + ": entry range outside [0, num_entries]").c_str());
  if (const int rc = list_plan_check(who, plan_host, plan_entries)) return rc;
  const int num_anchors = plan_host[1];
  hipStream_t s = (hipStream_t)stream;
  if (entry_begin == 0) {                          // the first slice: zero the cursors and the flag, build the bitset rows
    if ((num_nodes > 0 && hipMemsetAsync(cursor, 0, (size_t)num_nodes * 4, s) != hipSuccess) ||
        hipMemsetAsync(overflow, 0, 4, s) != hipSuccess)
      return launch_status((name + ": memset").c_str());
    if (num_nodes > 0)
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
                                     reinterpret_cast<const unsigned long long*>(bits), plan_dev, num_anchors, 1,
                                     num_nodes, entry_begin, items, nullptr};
  a.ptr = ptr;
  a.ptr_base = ptr_base;
  a.rows_capacity = rows_capacity;
  a.cursor = cursor;
  a.rows = rows;
  a.overflow = overflow;
  hipLaunchKernelGGL(gtm_count_kernel<Args>, dim3((unsigned)blocks), dim3(GTM_THREADS), 0, s, a);
  return launch_status(who);
}

}  // namespace

extern "C" int desco_list_occurrences_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                          const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                          const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                          int64_t num_words, const int32_t* plan_host, const int32_t* plan_dev,
                                          int64_t plan_entries, int num_queries, int induced, int64_t entry_begin,
                                          int64_t entry_end, const int64_t* ptr, int64_t ptr_base, int32_t* cursor,
                                          int64_t rows_capacity, int32_t* rows, int32_t* overflow,
                                          desco_stream_t stream) {
  const char* who = "desco_list_occurrences_dev";
  if (num_queries != 1) return fail(DESCO_EINVAL, "desco_list_occurrences_dev: one query per call (plan[0] must be 1)");
  if (induced != 0 && induced != 1) return fail(DESCO_EINVAL, "desco_list_occurrences_dev: induced must be 0 or 1");
  return induced ? list_launch<GtmListArgs>(who, graph_ptr, num_graphs, num_nodes, rowptr, num_entries, col, node_graph,
                                            bit_off, bits, num_words, plan_host, plan_dev, plan_entries, entry_begin,
                                            entry_end, ptr, ptr_base, cursor, rows_capacity, rows, overflow, stream)
                 : list_launch<GtmListMonoArgs>(who, graph_ptr, num_graphs, num_nodes, rowptr, num_entries, col,
                                                node_graph, bit_off, bits, num_words, plan_host, plan_dev, plan_entries,
                                                entry_begin, entry_end, ptr, ptr_base, cursor, rows_capacity, rows,
                                                overflow, stream);
}
