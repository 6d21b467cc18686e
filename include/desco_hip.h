/*
 * desco_hip.h -- C ABI of libdesco_hip.so, the MI355X (gfx950) native layer of the DeSCo hot path.
 *
 * The reference (fuvty/DeSCo) has no FFI: its hot path is Python calling PyG / torch ops.  This
 * header is the boundary a maintainer would bind (ctypes stub in INTEGRATION.md) to replace those
 * call sites.  Each entry point names the reference call site it replaces (paths relative to the
 * reference root, see SURVEY.md section 8a for the row ids A1..A15 / K1..K24).
 *
 * Conventions
 *   - every function returns 0 on success, otherwise a hipError_t value (device entry points) or a
 *     negative DESCO_E* code (argument errors); desco_last_error() gives a message (thread local).
 *   - device entry points take DEVICE pointers and a hipStream_t passed as void* (NULL = default
 *     stream); they only enqueue work, never allocate, never synchronise (graph-capture safe).
 *   - host entry points (desco_partition_*) take HOST pointers.
 *   - the hidden width H is fixed at 64 (reference default --neigh_hidden_dim/--gossip_hidden_dim,
 *     config.py:250,316); feature rows are fp32.
 *   - "virtual row" CSR: destination row i with relation slot s is virtual row i*S+s.
 */
#ifndef DESCO_HIP_H
#define DESCO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DESCO_ABI_VERSION 6
#define DESCO_H 64

#define DESCO_EINVAL (-1)
#define DESCO_ENOMEM (-2)

#define DESCO_ACT_NONE 0
#define DESCO_ACT_RELU 1
#define DESCO_ACT_LEAKY 2 /* slope given separately */

typedef void* desco_stream_t;

int desco_abi_version(void);
/* number of visible HIP devices, or a negative hipError_t when the runtime cannot initialise */
int desco_device_count(void);
const char* desco_last_error(void);

/* ------------------------------------------------------------------------------------------
 * HOST: canonical-partition builder.
 * Replaces NeighborhoodDataset.process (workload.py:243-294: get_neigh_hetero data.py:375-396,
 * k_neigh data.py:329-338, NetworkxToHetero transforms.py:319-412), the per-item ToTconvHetero
 * transform (transforms.py:180-255) and PyG's hetero collate, for a whole dataset at once.
 *
 * Input: G graphs stored as one CSR over global node ids (graph g owns nodes
 * graph_ptr[g]..graph_ptr[g+1]-1, ascending = the reference's nx node order); adjacency must be
 * symmetric, without self loops or duplicates, each row sorted ascending.
 *
 * Output (after desco_partition_sizes / desco_partition_export):
 *   B neighborhoods (one per node whose canonical neighborhood has >= 1 edge), N_c count rows.
 *   Row order: count rows of neighborhood 0, 1, ... (ascending original id inside each), then
 *   the B canonical rows; canonical row of neighborhood b is N_c + b.
 *   neigh_index[B][2] = (graph id, node id inside the graph)   (nx_neighs_index, workload.py:189-195)
 *   indicator[num_nodes]                                       (nx_neighs_indicator)
 *   count_ptr[B+1]: count rows of neighborhood b are count_ptr[b]..count_ptr[b+1]-1
 *   count_orig[N_c]: global node id of every count row
 *   vrowptr[4*(N_c+B)+1], vcol[E]: destination-major CSR with 4 relation slots per row,
 *      slot = 2*(source is the canonical node) + (edge is a "tride" edge, i.e. NOT in a triangle);
 *      vcol holds source ROW ids, ascending inside a slot.
 * quirk_batch > 0 emulates PyG's remove_self_loops on the bipartite edge types for reference
 * batches of quirk_batch consecutive neighborhoods (gnn_model.py:389-390); 0 = off.
 * ------------------------------------------------------------------------------------------ */
typedef struct desco_partition desco_partition;

int desco_partition_build(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                          const int32_t* col, int depth, int quirk_batch, int num_threads,
                          desco_partition** out);
int desco_partition_sizes(const desco_partition* p, int64_t* num_neigh, int64_t* num_count,
                          int64_t* num_edges, int64_t* num_nodes);
int desco_partition_export(const desco_partition* p, int64_t* neigh_index, uint8_t* indicator,
                           int32_t* count_ptr, int32_t* count_orig, int32_t* vrowptr,
                           int32_t* vcol);
void desco_partition_free(desco_partition* p);

/* The neighborhood definition (`mode` of the *_mode entry points; the entry points without it build DESCO_NEIGH_BALL):
 *   DESCO_NEIGH_BALL        BFS ball of radius depth in the full graph, ids <= v, component of v (get_neigh_hetero,
 *                           data.py:375-396)
 *   DESCO_NEIGH_RESTRICTED  depth BFS rounds from v that only step onto ids <= v (k_neigh_canonical / get_neigh_canonical,
 *                           data.py:341-372: the homogeneous ablation); a subset of the former, connected as built.
 * Edges, slots, row order and the output layout are the same in both.  quirk_batch must be 0 with
 * DESCO_NEIGH_RESTRICTED (DESCO_EINVAL otherwise). */
#define DESCO_NEIGH_BALL 0
#define DESCO_NEIGH_RESTRICTED 1
int desco_partition_build_mode(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                               const int32_t* col, int depth, int mode, int quirk_batch, int num_threads,
                               desco_partition** out);

/* Optional re-ordering of a block's count rows (host arrays, same layout in and out): inside every neighborhood the
 * count rows are sorted by their number of count -> count sources (the neighborhood's heavier relation slot first,
 * descending when neigh_key[b] is even, ascending when odd -- pass the canonical node's id inside its graph so that the
 * order is a property of the neighborhood, not of its place in a block or of the shard its graph is in; NULL = the index b), vcol is relabelled and kept ascending inside a slot, count_orig
 * follows the rows; count_ptr, the canonical rows and every per-neighborhood quantity are unchanged.  Row order inside a
 * neighborhood is this library's convention (data.py:375-396 leaves it to CPython set order), and the fused layer kernel
 * needs as many gather steps per 16-row tile as the tile's highest-degree row: -9 % on Syn_1827 shapes. */
int desco_partition_degree_sort(const int32_t* count_ptr, int64_t num_neigh, const int32_t* vrowptr,
                                const int32_t* vcol, const int32_t* count_orig, int32_t* count_orig_out,
                                int32_t* vrowptr_out, int32_t* vcol_out, const int64_t* neigh_key, int num_threads);

/* ------------------------------------------------------------------------------------------
 * DEVICE: the same canonical-partition builder on the GPU (csrc/partition_dev.hip), one wavefront
 * per target node, output streamed into the flat 4-slot CSR in device memory.
 * Inputs (device): graph_ptr[G+1] int64, node_graph[V] (graph id of every node), the CSR
 * rowptr[V+1] / col over global node ids (int32; symmetric, loop-free, rows sorted ascending);
 * n_max = nodes of the largest graph (sizes the per-wave LDS workspace: graphs above ~4400 nodes
 * return DESCO_EINVAL -> use the host builder); num_waves (multiple of 4) = wavefronts to launch.
 *   1. desco_partition_dev_count -> nsize[V] (0 = node skipped), ecnt_count[V], ecnt_canon[V]
 *   2. desco_partition_dev_scan  -> exclusive scans b_index / row_off / eoff_count / eoff_canon [V]
 *      and totals4 = (B, N_c, E_count, E_canon); the caller reads totals4 and allocates the outputs
 *   3. desco_partition_dev_fill  -> neigh_index[B,2], indicator[V], count_ptr[B+1], count_orig[N_c],
 *      vrowptr[4(N_c+B)+1], vcol[E]  -- bit-identical to desco_partition_export (quirk_batch = 0).
 * ------------------------------------------------------------------------------------------ */
int desco_partition_dev_count(const int64_t* graph_ptr, const int32_t* node_graph,
                              const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int depth,
                              int n_max, int num_waves, int32_t* nsize, int32_t* ecnt_count,
                              int32_t* ecnt_canon, desco_stream_t stream);
int desco_partition_dev_scan(const int32_t* nsize, const int32_t* ecnt_count,
                             const int32_t* ecnt_canon, int64_t num_nodes, int64_t* b_index,
                             int64_t* row_off, int64_t* eoff_count, int64_t* eoff_canon,
                             int64_t* totals4, desco_stream_t stream);
int desco_partition_dev_fill(const int64_t* graph_ptr, const int32_t* node_graph,
                             const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int depth,
                             int n_max, int num_waves, const int64_t* b_index, const int64_t* row_off,
                             const int64_t* eoff_count, const int64_t* eoff_canon, int64_t num_neigh,
                             int64_t num_count, int64_t edges_count, int64_t edges_canon,
                             int64_t* neigh_index, uint8_t* indicator, int32_t* count_ptr,
                             int32_t* count_orig, int32_t* vrowptr, int32_t* vcol,
                             desco_stream_t stream);
/* the same two passes with the neighborhood definition as an argument (DESCO_NEIGH_*); the scan is shared */
int desco_partition_dev_count_mode(const int64_t* graph_ptr, const int32_t* node_graph,
                                   const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int depth,
                                   int mode, int n_max, int num_waves, int32_t* nsize, int32_t* ecnt_count,
                                   int32_t* ecnt_canon, desco_stream_t stream);
int desco_partition_dev_fill_mode(const int64_t* graph_ptr, const int32_t* node_graph,
                                  const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int depth,
                                  int mode, int n_max, int num_waves, const int64_t* b_index,
                                  const int64_t* row_off, const int64_t* eoff_count, const int64_t* eoff_canon,
                                  int64_t num_neigh, int64_t num_count, int64_t edges_count,
                                  int64_t edges_canon, int64_t* neigh_index, uint8_t* indicator,
                                  int32_t* count_ptr, int32_t* count_orig, int32_t* vrowptr, int32_t* vcol,
                                  desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DEVICE: from the device partition to the arrays a batch's kernels read (csrc/batch_dev.hip).  Integer kernels that
 * reproduce the host routines bit for bit; all pointers are device pointers, every entry point launches on `stream`,
 * never allocates and never synchronises.  num_neigh == 0 (for the slice: b0 == b1) returns 0 and launches nothing.
 *
 * desco_partition_dev_slice: neighborhoods [b0, b1) of a partition (num_neigh neighborhoods, num_count count rows) as a
 *   block of their own (NeighborhoodPartition.slice): count_ptr_out[b1-b0+1] re-based, count_orig_out[block_count],
 *   vrowptr_out[4(block_count + b1-b0)+1] = the count rows' then the canonical rows' pointers re-based, vcol_out
 *   [block_edges] re-labelled.  block_count = count_ptr[b1] - count_ptr[b0] and block_edges = (vrowptr[4 c1] -
 *   vrowptr[4 c0]) + (vrowptr[4(N_c+b1)] - vrowptr[4(N_c+b0)]) are read back by the caller, who allocates the outputs.
 *
 * desco_partition_dev_degree_sort: the device twin of desco_partition_degree_sort (same keys, same stable order, vcol
 *   re-labelled and ascending inside every (row, slot) segment of any length).  num_count = count_ptr[num_neigh],
 *   num_edges = vrowptr[4(num_count + num_neigh)].  neigh_key: int64 read at neigh_key[b * neigh_key_stride] (column 1
 *   of neigh_index: pointer + 1, stride 2), NULL = the index b.  workspace: at least
 *   desco_partition_dev_degree_sort_workspace(num_count, num_edges) bytes, 8-byte aligned; it also holds the keys of
 *   a neighborhood too large for the workgroup's LDS (more than 4608 rows), which is sorted there, slower, with the
 *   same result.  num_blocks: workgroups per launch, 0 = chosen by the library (the result does not depend on it).
 *
 * desco_pool_index_dev: pool_bits / pool_slot [ceil(num_count / 16)] of the fused pooling (per 16-row tile: bitmap of
 *   the count rows that end a neighborhood, first partial slot) and totals4 = (num_slots, largest, smallest number of
 *   count rows of a neighborhood, 0).  A smallest number of 0 means the index is not usable.
 *
 * desco_neigh_rows_dev: scatter_index[b] = graph_ptr[neigh_index[b][0]] + neigh_index[b][1] and neigh_graph_ptr[g] =
 *   neighborhoods of the graphs before g (g = 0..num_graphs; neighborhoods are ordered by graph).
 * ------------------------------------------------------------------------------------------ */
int desco_partition_dev_slice(const int32_t* count_ptr, const int32_t* vrowptr, const int32_t* vcol,
                              const int32_t* count_orig, int64_t num_neigh, int64_t num_count, int64_t b0, int64_t b1,
                              int64_t block_count, int64_t block_edges, int32_t* count_ptr_out,
                              int32_t* count_orig_out, int32_t* vrowptr_out, int32_t* vcol_out, desco_stream_t stream);
size_t desco_partition_dev_degree_sort_workspace(int64_t num_count, int64_t num_edges);
int desco_partition_dev_degree_sort(const int32_t* count_ptr, int64_t num_neigh, int64_t num_count, int64_t num_edges,
                                    const int32_t* vrowptr, const int32_t* vcol, const int32_t* count_orig,
                                    const int64_t* neigh_key, int64_t neigh_key_stride, int32_t* count_orig_out,
                                    int32_t* vrowptr_out, int32_t* vcol_out, void* workspace, int num_blocks,
                                    desco_stream_t stream);
int desco_pool_index_dev(const int32_t* count_ptr, int64_t num_neigh, int64_t num_count, int32_t* pool_bits,
                         int32_t* pool_slot, int64_t* totals4, desco_stream_t stream);
int desco_neigh_rows_dev(const int64_t* neigh_index, int64_t num_neigh, const int64_t* graph_ptr, int64_t num_graphs,
                         int32_t* scatter_index, int32_t* neigh_graph_ptr, desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Typed CSR of WHOLE graphs: what the model without canonical partition (to_hetero_wo_canonical) reads of its target
 * graphs -- one node type, the two relation slots of the query model (csrc/graph_tconv.cpp, csrc/graph_tconv_dev.hip).
 * Input: the CSR of a graph set over global node ids, rowptr int64 / col int32 (symmetric, loop free, rows ascending),
 * and a block of whole graphs in it, the nodes [node0, node0 + num_nodes) (graph_ptr[g0] .. graph_ptr[g1]; the graph
 * boundaries inside the block play no part, an edge never leaves its graph).  Output, re-based to the block:
 *   vrowptr[2 num_nodes + 1]: entry 2 v + t starts the sources of row v in slot t; slot 0 = "union_triangle" (source
 *      and row share a neighbour), slot 1 = "union_tride" (they do not) -- ToTconvHetero, transforms.py:180-255
 *   vcol[num_edges]: source rows (node id - node0), ascending inside each (row, slot)
 * with num_edges = rowptr[node0 + num_nodes] - rowptr[node0] <= INT32_MAX.  A source outside the block counts as tride.
 *
 * desco_graph_tconv: HOST arrays, OpenMP over rows (num_threads 0 = the runtime's default).
 * desco_graph_tconv_dev: DEVICE arrays; edge0 = rowptr[node0] and num_edges are passed by the caller (who allocated
 *   vcol with them); workspace: desco_graph_tconv_dev_workspace(num_edges) bytes, 8-byte aligned (may be NULL without
 *   edges).  Three launches on `stream` (flag, scan, fill), no allocation, no synchronisation, no atomics; the work of
 *   a lane does not grow with the degree of a hub and nothing is sized by the largest graph.  Bit-identical to the
 *   host routine.
 * ------------------------------------------------------------------------------------------ */
int desco_graph_tconv(const int64_t* rowptr, const int32_t* col, int64_t node0, int64_t num_nodes, int32_t* vrowptr,
                      int32_t* vcol, int num_threads);
size_t desco_graph_tconv_dev_workspace(int64_t num_edges);
int desco_graph_tconv_dev(const int64_t* rowptr, const int32_t* col, int64_t node0, int64_t num_nodes, int64_t edge0,
                          int64_t num_edges, int32_t* vrowptr, int32_t* vcol, void* workspace, desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Data-set statistics: graph features of node sets (csrc/subgraph_stats.cpp, csrc/subgraph_stats_dev.hip).
 * Input: the CSR of a graph set over global node ids (rowptr int64 [num_nodes + 1], col int32; symmetric, loop free,
 * rows ascending) and S node sets: set s = set_nodes[set_ptr[s] .. set_ptr[s+1]), global ids of ONE graph, strictly
 * ascending.  For a set M: H = G[M]; C = the connected component of H with the most nodes, a tie going to the
 * component that holds the smallest id.  Output per set:
 *   out_i64[s][6] = { members = |M|, n = |C|, m = edges of C, diameter of C (0 for n = 1),
 *                     dist_sum = sum of d(s,t) over ORDERED pairs s != t of C, triangles of C }
 *   out_f64[s]    = clustering_sum = sum over v in C of 2 T(v) / (d(v) (d(v) - 1)), a term being 0 for d(v) < 2.
 * Each term is one fp64 division of two exact integers; the terms are summed by the balanced pairwise tree over the
 * positions of the members in M (position i meets position i + s at stride s = 1, 2, 4, ..; positions outside C and
 * beyond |M| are +0.0), the same on both sides.  An empty set gets zeros.
 *
 * desco_subgraph_stats: HOST arrays, sets of any size (queue BFS, no |M|^2 memory); OpenMP over sets, and over the
 *   sources of a set above 4096 members (num_threads 0 = the runtime's default); the result does not depend on
 *   num_threads.  DESCO_EINVAL naming the argument for: a null pointer with num_sets > 0, a set_ptr that is not
 *   monotone, an id outside the graph, a set that is not strictly ascending -- before any work.
 * desco_subgraph_stats_dev: DEVICE arrays.  One launch on `stream` for the sets set_ids[0 .. num_ids) (int64 indices
 *   into set_ptr, the caller's responsibility), each of at most 64 * words members, words in {1, 2, 4, 8, 16} (any
 *   other value: DESCO_EINVAL naming `words`); only the rows of those sets are written.  A set with more members than
 *   64 * words, with an id outside the graph or not strictly ascending gets members and n = -1 (the rest 0) and no
 *   other work: the caller passes those rows to desco_subgraph_stats.  Null pointers and misaligned 64-bit arrays are
 *   refused by name before any launch.  No allocation, no synchronisation, no atomics on global memory; equal to the
 *   host routine bit for bit, the fp64 field included, whichever bucket a set runs in.
 * ------------------------------------------------------------------------------------------ */
int desco_subgraph_stats(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int64_t* set_ptr,
                         const int32_t* set_nodes, int64_t num_sets, int num_threads, int64_t* out_i64, double* out_f64);
int desco_subgraph_stats_dev(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int64_t* set_ptr,
                             const int32_t* set_nodes, const int64_t* set_ids, int64_t num_ids, int words,
                             int64_t* out_i64, double* out_f64, desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * NULL MODEL: degree-preserving rewiring by double edge switches (csrc/null_model.hpp, csrc/null_model.cpp,
 * csrc/null_model_dev.hip).  Input: a graph set (graph_ptr int64 [G + 1], rowptr int64 [N + 1] from 0, col int32 global
 * ids; symmetric, loop free, rows strictly ascending).  Every (graph g, replica r) pair is ONE sequential Markov chain:
 *   edge slots: a graph with m undirected edges has m slots; slot i holds an ORDERED pair (a_i, b_i), at first the CSR
 *     entries (v, u) with u < v in CSR order as (a, b) = (u, v).  A slot keeps the orientation it was last written with.
 *   attempt t = 0 .. swaps_per_edge * m - 1:
 *     w = Philox4x32-10(counter = {lo32(t), hi32(t), lo32(graph_base + g), lo32(replica_base + r)},
 *                       key = {lo32(seed), hi32(seed)});
 *     i = (uint64(w0) * m) >> 32, j = (uint64(w1) * m) >> 32, flip = w2 & 1;  reject if i == j;
 *     (a, b) = slot i, (c, d) = slot j, c and d exchanged if flip;  the proposed edges are {a, d} and {c, b}: reject
 *     if a == d or c == b, or if either is an edge of the current graph;  else slot i <- (a, d), slot j <- (c, b), and
 *     the graph loses {a, b}, {c, d} and gains the two new edges.
 *   Graphs with m < 2 come back unchanged.
 * Output: col_out int32 [replicas][E] (E = rowptr[N]; replica r's col for the SAME graph_ptr / rowptr -- degrees are
 * preserved -- every row ascending) and accepted int32 [replicas][G], the accepted switches of every chain.
 * graph_base / replica_base offset the counter, so that a slice of the graphs or a chunk of the replicas reproduces
 * the bits of the whole call.
 *
 * HOST desco_null_model_rewire: OpenMP over chains (num_threads 0 = the runtime's default); the result does not depend
 *   on num_threads.  DESCO_EINVAL naming the entry point for: negative counts or bases, swaps_per_edge < 0, a null
 *   pointer with non-empty input, a graph_ptr / rowptr that is not monotone from 0, ids outside the node's graph,
 *   loops, rows that are not strictly ascending (unsorted), an asymmetric adjacency, a graph of 2^32 edges or more,
 *   swaps_per_edge * m beyond 2^63.
 * HOST desco_null_model_draw: out[3] = (i, j, flip) of attempt t of chain (graph, replica) over m slots, 1 <= m < 2^32.
 * DEVICE desco_null_model_rewire_dev (gfx950): device arrays; ONE launch on `stream` for the graphs graph_ids[0 ..
 *   num_ids) (int64, device; NULL = all num_graphs), one wavefront per chain, the chain's adjacency bitset and slots in
 *   LDS.  A graph of n nodes and m edges needs a workspace of n * (ceil(n / 32) | 1) + m 32-bit words; max_words is
 *   the caller's bound on that over the launch's graphs and sizes the launch's LDS.  A bound above
 *   DESCO_NULL_MODEL_DEV_MAX_WORDS is refused (DESCO_EINVAL naming the limit): a graph that needs more goes to the
 *   host routine.  num_edges = E, the row length of col_out.  A graph that breaks the bound, holds
 *   an id outside itself or a loop, or whose entries do not pair up gets accepted = -1 and its col_out untouched.  Only
 *   the rows of the launch's graphs are written.  No allocation, no synchronisation, no global atomics; equal to the
 *   host routine bit for bit.
 * ------------------------------------------------------------------------------------------ */
#define DESCO_NULL_MODEL_DEV_MAX_WORDS 40960 /* 160 KiB of LDS: e.g. 1104 nodes with 2320 edges */
int desco_null_model_rewire(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, int64_t num_graphs,
                            int64_t graph_base, int replicas, int64_t replica_base, int64_t swaps_per_edge,
                            uint64_t seed, int num_threads, int32_t* col_out, int32_t* accepted);
int desco_null_model_draw(uint64_t seed, int64_t graph, int64_t replica, uint64_t t, int64_t m, int64_t* out);
int desco_null_model_rewire_dev(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, int64_t num_graphs,
                                int64_t num_edges, const int64_t* graph_ids, int64_t num_ids, int64_t max_words,
                                int64_t graph_base, int replicas, int64_t replica_base, int64_t swaps_per_edge,
                                uint64_t seed, int32_t* col_out, int32_t* accepted, desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CORE / TRUSS: k-core and k-truss decomposition of every graph of a set (csrc/core_truss.hpp, csrc/core_truss.cpp,
 * csrc/core_truss_dev.hip).  Input: a graph set (graph_ptr int64 [G + 1], rowptr int64 [N + 1] from 0, col int32 global
 * ids; symmetric, loop free, rows strictly ascending).  Exact integer functions of the graph:
 *   core[v]     the largest k such that v lies in a subgraph whose every node has degree >= k inside it; an isolated
 *               node has 0 (networkx.core_number).
 *   support[e]  the triangles through edge e = the common neighbours of its ends (the non-induced triangle column of
 *               the edge orbit counts).
 *   truss[e]    >= 2: the largest k such that e lies in a subgraph whose every edge is in >= k - 2 triangles inside it
 *               (e is an edge of networkx.k_truss(G, k) iff truss[e] >= k).
 * core has one row per node; truss and support one row per undirected edge, M = E / 2 rows in the order of the CSR
 * entries (v, u) with u < v (the rows of the edge orbit counts).  Both decompositions are unique: they do not depend on
 * the order in which a level is peeled.  Any output may be NULL, and nothing is computed for it that no other needs.
 *
 * HOST desco_core_truss: OpenMP over graphs (num_threads 0 = the runtime's default); the result does not depend on
 *   num_threads.  DESCO_EINVAL naming the entry point for: a negative count, a null pointer with non-empty input, a
 *   graph_ptr / rowptr that is not monotone from 0, ids outside the node's graph, loops, rows that are not strictly
 *   ascending (unsorted), an asymmetric adjacency -- before any output is written.
 * DEVICE desco_core_truss_dev (gfx950): device arrays; ONE launch on `stream` for the graphs graph_ids[0 .. num_ids)
 *   (int64, device; NULL = all num_graphs), one workgroup per graph, the graph and its peel in LDS.  num_edges = M;
 *   entry_row int32 [E]: the row of the edge of every CSR entry, both directions of an edge naming one row.  A graph of
 *   n nodes and m edges needs a workspace of n + 4 + 3 m + max(3 m, n) 32-bit words (csrc/core_truss.hpp); max_words
 *   is the caller's bound on that over the launch's graphs and sizes the launch's LDS (one wave per graph up to
 *   DESCO_CORE_TRUSS_WAVE_WORDS, four above).  A bound above DESCO_CORE_TRUSS_DEV_MAX_WORDS is refused (DESCO_EINVAL
 *   naming the limit): a graph that needs more goes to the host routine.  status int32 [G]: 0 for a graph that was
 *   decomposed; -1, and no other word of it written, for a graph that breaks the bound, holds an id outside itself, a
 *   loop or an unsorted row, or whose entries do not pair up through entry_row.  Only the rows of the launch's graphs
 *   are written.  No allocation, no synchronisation, no global atomics; equal to the host routine bit for bit.
 * ------------------------------------------------------------------------------------------ */
#define DESCO_CORE_TRUSS_DEV_MAX_WORDS 40960 /* 160 KiB of LDS: e.g. 4000 nodes with 6100 edges */
#define DESCO_CORE_TRUSS_WAVE_WORDS 512
int desco_core_truss(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, int64_t num_graphs,
                     int num_threads, int32_t* core_out, int32_t* truss_out, int32_t* support_out);
int desco_core_truss_dev(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, int64_t num_graphs,
                         int64_t num_edges, const int32_t* entry_row, const int64_t* graph_ids, int64_t num_ids,
                         int64_t max_words, int32_t* core_out, int32_t* truss_out, int32_t* support_out,
                         int32_t* status, desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CLIQUE CENSUS: the exact number of k-cliques for every k = 1 .. kmax of every graph of a set, per graph and per node,
 * and the clique number (csrc/clique_census.hpp, csrc/clique_census.cpp, csrc/clique_census_dev.hip).  Counted by
 * pivoting (Jain and Seshadhri, "The power of pivoting for exact clique counting", WSDM 2020): no clique is listed, a
 * clique K_n is a single branch.  Input: a graph set as in CORE / TRUSS.
 *
 * Outputs (any may be NULL), kmax in 1..DESCO_CLIQUE_MAX_K.  All clique arithmetic is on uint64 with wrap-around, stored
 * as int64 bit patterns: exact wherever the true value is below 2^64 (every column of every graph whose cliques have at
 * most 66 nodes).
 *   graph_cliques int64 [G, kmax]  column k - 1 = the k-cliques of the graph (column 0 nodes, 1 edges, 2 triangles)
 *   node_cliques  int64 [N, kmax]  column k - 1 = the k-cliques that contain the node (column 0 is 1, column 1 the degree)
 *   omega         int32 [G]        the clique number, exact whatever kmax is; 0 for a graph without nodes
 *
 * PEEL ORDER: key[v] int32 = the index of the pass in which v leaves the level-synchronous core peel.  At level
 *   k = 0, 1, ... a pass removes every node whose remaining degree is at most k AT THE START of that pass; a level
 *   repeats passes until one removes nothing.  Only passes that remove a node are numbered; the numbering runs on across
 *   levels and starts again at 0 for every graph.  The key is unique, and core[v] (the level at which v left) is the
 *   core number of CORE / TRUSS.  Under a key the OUT-NEIGHBOURS of v are its neighbours u with (key[u], u) >
 *   (key[v], v); under the peel key there are at most core[v] of them, hence at most the graph's degeneracy.
 *
 * CENSUS: for every root v, on the subgraph induced by v's out-neighbours: a branch holds r "held" nodes (v first) and
 *   p "pivot" nodes and a candidate set P.  It picks a pivot u in P (the member with most neighbours in P, the first of
 *   those), recurses on P & N(u) with u added to the pivots, and then for every w in P \ N(u) \ {u} in turn recurses on
 *   P & N(w) with w held and removes w from P.  A leaf (P empty) adds, for k = r .. min(r + p, kmax), C(p, k - r) to the
 *   graph's column k and to every held node's column k, and C(p - 1, k - r - 1) to every pivot node's column k when
 *   k > r; and raises omega to r + p.  No branch is cut, so omega is exact for any kmax.
 * ORDER INDEPENDENCE: the counts depend neither on the key, nor on the pivot rule, nor on the order of branches, roots
 *   or atomics -- only the work and the device's capacity do.  Host and device agree bit for bit.
 *
 * HOST desco_peel_order (core_out may be NULL) and desco_clique_census (key int32 [N], any non-negative values, or NULL
 *   = the peel key is computed): OpenMP over graphs (num_threads 0 = the runtime's default); the result does not depend
 *   on num_threads.  No limit on the out-degree: multi-word bitsets, Pascal rows mod 2^64 up to the largest out-degree.
 *   DESCO_EINVAL naming the entry point, before any output is written, for what desco_core_truss refuses, for kmax
 *   outside 1..DESCO_CLIQUE_MAX_K and for a negative key.
 * DEVICE desco_peel_order_dev (gfx950): device arrays; ONE launch on `stream` for the graphs graph_ids[0 .. num_ids)
 *   (int64, device; NULL = all num_graphs), one workgroup per graph, the CSR and the remaining degrees in LDS.  A graph
 *   of n nodes and m edges needs 2 n + 2 m + 8 32-bit words (csrc/clique_census.hpp); max_words is the caller's bound on
 *   that over the launch's graphs and sizes the launch's LDS; above DESCO_PEEL_DEV_MAX_WORDS it is refused (DESCO_EINVAL
 *   naming the limit).  status int32 [G]: 0, or -1 -- and no other word of the graph written -- for a graph that breaks
 *   the bound or holds an id outside itself, a loop or an unsorted row.  core_out may be NULL.
 * DEVICE desco_clique_census_dev (gfx950): device arrays, key required; two launches on `stream` for the graphs
 *   graph_ids[0 .. num_ids) (NULL = all).  The first checks every graph of the launch and zeroes its output rows; the
 *   second runs one wave per root, the root's d <= max_out out-neighbours as d 64-bit adjacency rows in LDS, the lanes
 *   taking the first-level branches, each with its own stack in LDS.  max_out is the caller's bound on the out-degree
 *   over the launch's graphs and sizes the LDS per wave (csrc/clique_census.hpp); above DESCO_CLIQUE_DEV_MAX_OUT it is
 *   refused (DESCO_EINVAL naming the limit).  status int32 [G]: 0, or -1 -- and nothing else of the graph written -- for
 *   a graph with a root of more than max_out out-neighbours, a col id outside the graph, a loop or an unsorted row.
 *   Only the launch's graphs are written.  No allocation, no synchronisation; tallies by 64-bit atomics.
 * ------------------------------------------------------------------------------------------ */
#define DESCO_CLIQUE_MAX_K 64
#define DESCO_CLIQUE_DEV_MAX_OUT 64
#define DESCO_PEEL_DEV_MAX_WORDS 40960 /* 160 KiB of LDS: e.g. 5000 nodes with 15000 edges */
#define DESCO_PEEL_WAVE_WORDS 512
int desco_peel_order(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, int64_t num_graphs,
                     int num_threads, int32_t* key_out, int32_t* core_out);
int desco_clique_census(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, int64_t num_graphs,
                        const int32_t* key, int kmax, int num_threads, int64_t* graph_cliques, int64_t* node_cliques,
                        int32_t* omega);
int desco_peel_order_dev(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, int64_t num_graphs,
                         const int64_t* graph_ids, int64_t num_ids, int64_t max_words, int32_t* key_out,
                         int32_t* core_out, int32_t* status, desco_stream_t stream);
int desco_clique_census_dev(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col, int64_t num_graphs,
                            const int32_t* key, int kmax, const int64_t* graph_ids, int64_t num_ids, int max_out,
                            int64_t* graph_cliques, int64_t* node_cliques, int32_t* omega, int32_t* status,
                            desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * COLOUR REFINEMENT: 1-WL colour classes of the segments of a typed CSR block (csrc/wl_refine.hpp, csrc/wl_refine.cpp,
 * csrc/wl_refine_dev.hip).  Two segments with equal signatures after L rounds get the same prediction from every
 * L-layer model that maps a row to a function of its own state and, per GROUP of relation slots, the sum over its
 * neighbours' states, and whose head reads the anchor row and the sum over the other rows.
 *
 * All arithmetic is on uint64 with wrap-around; values are stored as int64 bit patterns.
 *   G      = 0x9E3779B97F4A7C15
 *   mix(x) = the splitmix64 finaliser: x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB;
 *            x ^= x >> 31.  mix(0) = 0, hence the "+ G" below.
 * Input: vrowptr int32 [slots * R + 1] from 0 and vcol int32 [E], row r slot s at virtual row r * slots + s (the
 *   layout of the SHMP layer kernels); slots in 1..4; group int32 [slots] (a HOST array in both entry points), every
 *   entry < slots: the slots with one group value are pooled together.  Segments: seg_ptr int32 [S + 1] over rows and
 *   anchor_base.  Segment i is the rows seg_ptr[i] .. seg_ptr[i + 1] - 1 and, when anchor_base >= 0, the one row
 *   anchor_base + i, its anchor (a neighborhood block: seg_ptr = count_ptr, anchor_base = N_c; a whole-graph block:
 *   seg_ptr = graph_ptr, anchor_base = -1).  init int64 [R] or NULL.
 * Initial colour: init[r] when given; otherwise 1 for an anchor row and 0 for any other row.
 * One round, for a row of colour c:  m_g = sum of mix(c[src] + G) over the row's entries whose slot maps to group g;
 *   h = mix(c + G);  for g = 0 .. slots - 1 in order: h = mix(h ^ (m_g + (g + 1) * G));  the new colour is h.  Every
 *   row of a segment is updated from the previous round's colours.  rounds in 0..DESCO_WL_MAX_ROUNDS.
 * Signature of a segment after the last round:  p = sum of mix(c[r] + G) over its non-anchor rows;  with an anchor a:
 *   sig = mix(mix(c[a] + G) ^ (p + G));  without: sig = mix(p + G).
 * ORDER INDEPENDENCE: every sum is commutative modulo 2^64, so any evaluation order -- the twin's sequential walk, the
 *   kernel's lanes and its wave reductions -- gives the same bits, and so does any order of the rows inside a segment.
 * COLLISIONS: the colours are 64-bit hashes; a collision would merge two classes.  The partition into equal-signature
 *   classes is exact up to such a collision (the tests hold it to an exact tuple-colour refinement).
 * GUARD: an entry of vcol may point only into its own segment, anchor included.  A segment that breaks this -- or whose
 *   rows, anchor or row pointers lie outside the block -- gets status[i] = -1 and nothing else written; otherwise
 *   status[i] = 0, sig[i] and, when colours != NULL, the final colours of its rows (int64 [R]) are written.
 *
 * HOST desco_wl_refine: OpenMP over segments (num_threads 0 = the runtime's default); the result does not depend on
 *   num_threads.  DESCO_EINVAL naming the entry point for: slots or rounds out of range, a group entry >= slots, a
 *   negative count, a null pointer where an array is required, a vrowptr that is not monotone from 0.
 * DEVICE desco_wl_refine_dev (gfx950): device arrays (group on the host); ONE launch on `stream` for the segments
 *   seg_ids[0 .. num_ids) (int64, device; NULL = all num_segs).  All rounds and the signature of a segment run in this
 *   one launch: both colour buffers of the segment sit in LDS (16 bytes per row + 64) and ping-pong.  max_rows is the
 *   caller's bound on the rows of a segment (anchor included) over the launch and sizes its LDS: one wave per segment
 *   up to DESCO_WL_WAVE_ROWS, one workgroup of four above.  A bound above DESCO_WL_DEV_MAX_ROWS is refused
 *   (DESCO_EINVAL naming the limit): a larger segment goes to the host routine.  A segment over the launch's bound
 *   gets status -1.  No allocation, no synchronisation, no atomics; equal to the host routine bit for bit.
 * ------------------------------------------------------------------------------------------ */
#define DESCO_WL_MAX_ROUNDS 64
#define DESCO_WL_DEV_MAX_ROWS 10236 /* 64 + 16 * rows bytes = 160 KiB of LDS */
#define DESCO_WL_WAVE_ROWS 128
int desco_wl_refine(const int32_t* vrowptr, const int32_t* vcol, int64_t num_rows, int slots, const int32_t* group,
                    const int32_t* seg_ptr, int64_t num_segs, int64_t anchor_base, const int64_t* init, int rounds,
                    int num_threads, int64_t* sig, int64_t* colours, int32_t* status);
int desco_wl_refine_dev(const int32_t* vrowptr, const int32_t* vcol, int64_t num_rows, int slots, const int32_t* group,
                        const int32_t* seg_ptr, int64_t num_segs, int64_t anchor_base, const int64_t* init, int rounds,
                        const int64_t* seg_ids, int64_t num_ids, int64_t max_rows, int64_t* sig, int64_t* colours,
                        int32_t* status, desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GRAPH GENERATORS: the six families of the synthetic training sets -- ER, WS, Random = G(n, m), BA, EBA = extended
 * Barabasi-Albert, Power = Holme-Kim power-law cluster -- every graph forced connected through a random tree over its
 * components and randomly relabelled (csrc/graph_gen.hpp is this definition as code, shared by csrc/graph_gen.cpp and
 * csrc/graph_gen_dev.hip).  The families are sequential restatements of the textbook algorithms, equal in distribution
 * to networkx's generators; no bit of any other generator is reproduced.
 *
 * INPUT, per graph, integers only: family int32 (0 ER, 1 WS, 2 Random, 3 BA, 4 EBA, 5 Power), n int32 >= 1, param
 *   int64 [2], threshold uint64 [2] in [0, 2^32].  A Bernoulli(p) draw is uint64(word) < threshold = floor(p 2^32); the
 *   caller does all float arithmetic (desco_amd/generators.py: family_params).
 *     ER      threshold[0] = p.            WS     param = (k, edge target of the fallback), threshold[0] = p.
 *     Random  param[0] = m.                BA     param[0] = m, 1 <= m < n.
 *     EBA     param[0] = m, 1 <= m < n, threshold = (p, p + q).        Power  param[0] = m, 1 <= m <= n, threshold[0] = p.
 *   n = 1 is the single node whatever the parameters say.
 * DRAWS: word i of the sequence (graph, stream) is word i & 3 of
 *     Philox4x32-10(counter = {lo32(i >> 2), hi32(i >> 2), lo32(graph_base + g), stream}, key = {lo32(seed), hi32(seed)})
 *   (the Philox of the null model).  stream: 0 the family's body, 1 the Random body (as a family and as WS's fallback),
 *   2 connection, 3 relabel, 16 + i the i-th WS try.  Unless said otherwise a phase takes its words in order, one per
 *   draw.  A uniform integer in [0, W) is (uint64(word) * W) >> 32.  No draw depends on another graph.
 * PREFERENTIAL CHOICE over the nodes below c with integer weights: r uniform in [0, sum of the weights); the node
 *   whose interval of the prefix sums in id order holds r.  "m distinct targets": choices are repeated until m distinct
 *   nodes were seen; they are kept in the order of their first draw.
 * FAMILIES (node ids before the relabelling):
 *   ER      the pair (u < v) has index v (v - 1) / 2 + u and is an edge iff word[index] of stream 0 < threshold.
 *   Random  complete if m >= n (n - 1) / 2.  Otherwise attempts (u, v) = two uniform nodes, skipped if u == v or the
 *           edge exists, until m edges stand.
 *   WS      h = k / 2 (integer).  A try: the ring lattice {u, (u + j) mod n}, j = 1 .. h; then for j = 1 .. h and
 *           u = 0 .. n - 1 in that order one Bernoulli word; if selected and deg(u) < n - 1: w uniform, redrawn while
 *           w == u or {u, w} is an edge; the edge {u, (u + j) mod n} is replaced by {u, w}.  Tries i = 0 .. 99, each on
 *           stream 16 + i, until one is connected.  After 100, or when h == 0: the Random family with the edge target.
 *   BA      the star of node 0 and nodes 1 .. m; every node s = m + 1 .. n - 1 joins m distinct targets among the nodes
 *           below s, weight = degree.
 *   EBA     m isolated nodes; for s = m .. n - 1 with c = s existing nodes, E edges, full = c - 1, room = c full / 2:
 *           one word a.  a < threshold[0] and E + m <= room: flag every node of degree < full; m times (stop when no
 *           node is flagged): src = the k-th flagged node in id order, k uniform; dst = preferential with weight
 *           deg + 1, zero for src and its neighbours; add {src, dst}; unflag src if saturated, unflag dst if saturated.
 *           Else threshold[0] <= a < threshold[1] and m <= E < room: flag every node with 0 < degree < full; m times:
 *           node = the k-th flagged; old = its k'-th neighbour in id order; dst = preferential as above around node;
 *           {node, old} becomes {node, dst}; unflag old if it is isolated now; dst: unflagged if it was flagged and is
 *           saturated now, flagged if it was not and has degree 1 now (a node that merely leaves saturation is not
 *           flagged again).  Always: s joins m distinct targets, weight deg + 1.  The weight deg + 1 is exactly the
 *           multiplicity of a node in the model's attachment list (shown in csrc/graph_gen.hpp); where that list or
 *           the flagged set would be empty the remaining iterations of the step are skipped.
 *   Power   m isolated nodes of weight 1; for s = m .. n - 1: m distinct targets by weight, taken in draw order.  The
 *           first is joined.  Until m targets were taken: one Bernoulli word; if selected and the last target has
 *           neighbours that are neither s nor joined to s, the k-th of them in id order, k uniform, is joined and gains
 *           one weight, and this does not count; otherwise the next target is joined (or stands already) and gains one
 *           weight either way.  Then s gains weight m.
 * CONNECTION: components numbered 0 .. c - 1 by their smallest member.  c > 1: a Pruefer sequence of c - 2 uniform
 *   draws in [0, c) is decoded (every entry is joined to the smallest node that is a leaf by then; the last leaf to
 *   c - 1); for every tree edge (i, j) as decoded, the k-th member of i and then the k'-th member of j in id order, k
 *   and k' uniform over the components as they were before the connection, are joined.
 * RELABEL: key[v] = word[v] of stream 3; the new id of v is the rank of (key[v], v).
 * flags: DESCO_GRAPH_GEN_NO_CONNECT leaves the connection out, DESCO_GRAPH_GEN_NO_RELABEL the relabelling (what the
 *   distribution tests compare with other generators); 0 is the recipe.
 * OUTPUT: graph_ptr int64 [G + 1] = the prefix sums of n and bit_ptr int64 [G + 1] = the prefix sums of
 *   n * (ceil(n / 32) | 1), both computed by the caller from n.  bits uint32 [bit_ptr[G]]: graph g's adjacency as n
 *   rows of ceil(n / 32) | 1 words over the new ids; deg int32 [N]; status int32 [G] = tries | added << 8 with tries =
 *   the WS tries used (101: fell back to Random; 0 for other families) and added = the edges of the connection; -1
 *   for a refused graph.  One call into caller-sized rows: the caller forms rowptr = the prefix sums of deg, and
 *   desco_graph_gen_expand(_dev) writes col int32 [rowptr[N]] (global ids, rows strictly ascending, symmetric, loop
 *   free).  graph_base offsets the counter, so that a slice of the graphs reproduces the bits of the whole call.
 *
 * HOST desco_graph_gen / desco_graph_gen_expand: OpenMP over graphs (num_threads 0 = the runtime's default); the
 *   result does not depend on num_threads.  DESCO_EINVAL naming the entry point for: negative counts, a null pointer
 *   with non-empty input, an unknown family, n < 1, a threshold above 2^32, m outside its family's range, pointer
 *   arrays that are not the prefix sums of n -- before anything is written.
 * HOST desco_graph_gen_draw: out[0] = word i of (graph, stream), out[1] = (out[0] * bound) >> 32.
 * DEVICE desco_graph_gen_dev (gfx950): device arrays; ONE launch on `stream` for the graphs graph_ids[0 .. num_ids)
 *   (int64, device; NULL = all num_graphs), one workgroup per graph, the graph's whole state in LDS.  A graph of n nodes needs a workspace of n * (ceil(n / 32) | 1) + 4 n + 4 32-bit words;
 *   max_words is the caller's bound on that over the launch's graphs and sizes the launch's LDS (waves: 1 or 4 waves
 *   per graph; 0: one up to DESCO_GRAPH_GEN_WAVE_WORDS, four above).  A bound above DESCO_GRAPH_GEN_DEV_MAX_WORDS is
 *   refused (DESCO_EINVAL naming the limit): a graph that needs more goes to the host routine.  A graph that breaks
 *   the launch's bound, whose parameters the host routine would refuse, or whose graph_ptr / bit_ptr entries are not
 *   those of its n gets status -1 and nothing else written.  desco_graph_gen_expand_dev: one launch; a row whose
 *   bitset population is not its rowptr span is not written.  No allocation, no synchronisation, no global atomics;
 *   equal to the host routines bit for bit.
 * ------------------------------------------------------------------------------------------ */
#define DESCO_GRAPH_GEN_DEV_MAX_WORDS 40960 /* 160 KiB of LDS: up to 1056 nodes */
#define DESCO_GRAPH_GEN_WAVE_WORDS 2048
#define DESCO_GRAPH_GEN_NO_CONNECT 1 /* flags: the family's body alone, components stay apart */
#define DESCO_GRAPH_GEN_NO_RELABEL 2 /* flags: the ids of the definition, no relabelling */
int desco_graph_gen(const int32_t* family, const int32_t* n, const int64_t* param, const uint64_t* threshold,
                    int64_t num_graphs, int64_t graph_base, uint64_t seed, int num_threads, int flags,
                    const int64_t* graph_ptr, const int64_t* bit_ptr, uint32_t* bits, int32_t* deg, int32_t* status);
int desco_graph_gen_expand(const int64_t* graph_ptr, const int64_t* bit_ptr, const uint32_t* bits,
                           const int64_t* rowptr, int64_t num_graphs, int num_threads, int32_t* col);
int desco_graph_gen_draw(uint64_t seed, int64_t graph, int64_t stream, uint64_t i, int64_t bound, int64_t* out);
int desco_graph_gen_dev(const int32_t* family, const int32_t* n, const int64_t* param, const uint64_t* threshold,
                        int64_t num_graphs, const int64_t* graph_ids, int64_t num_ids, int64_t graph_base,
                        uint64_t seed, const int64_t* graph_ptr, const int64_t* bit_ptr, int64_t num_nodes,
                        int64_t num_bit_words, int64_t max_words, int waves, int flags, uint32_t* bits,
                        int32_t* deg, int32_t* status, desco_stream_t stream);
int desco_graph_gen_expand_dev(const int64_t* graph_ptr, const int64_t* bit_ptr, const uint32_t* bits,
                               const int64_t* rowptr, int64_t num_graphs, int64_t num_nodes, int64_t num_bit_words,
                               int64_t num_entries, int32_t* col, desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SAMPLED COUNTS: RAND-ESU (Wernicke 2006) estimates of the canonical counts below (csrc/sampled_counts.hpp,
 * csrc/sampled_counts.cpp, csrc/sampled_counts_dev.hip).  The exact enumerators visit every connected node subset
 * once; here every edge of the enumeration tree is kept with a probability that depends only on its depth, and the
 * kept subsets are tallied.  Dividing a tally by the product of the probabilities along the path gives an unbiased
 * estimate of the exact count.  Unlabelled graphs, canonical (induced) counts only.
 *
 * The tree is the one the device walk enumerates (csrc/groundtruth_esu_dev.hpp), node ids local to the graph:
 *   a tree node is a sequence (s_0 = v, s_1, .., s_{j-1}), j <= kmax; the roots are the nodes v of the graph.
 *   The key of a candidate u (u < v, u not in S, u adjacent to a member of S) is the pair (index i of the first member
 *   of S adjacent to u, position of u in s_i's ascending adjacency row), ordered lexicographically.  The children of
 *   the sequence are its candidates whose key is larger than the key that s_{j-1} had when it was chosen (for j = 1:
 *   all the neighbours u < v), in key order.  Every connected subset with maximum v is exactly one tree node.
 *   (The host's exact walk, csrc/groundtruth_esu.hpp, builds ANOTHER tree over the same subsets: which subsets a
 *   sampled walk keeps depends on the tree, so the host twin restates the device walk.)
 * The decision whether u is kept as node number d (d = 2 .. kmax; s_1 is node number 2) of (s_0, .., s_{d-2}, u), with
 * G and mix of COLOUR REFINEMENT above and the Philox of NULL MODEL:
 *   w   = Philox4x32-10(counter = {s_0, lo32(graph_base + g), lo32(replica_base + r), 0x53414D50},
 *                       key = {lo32(seed), hi32(seed)});   h_1 = w0 | w1 << 32
 *   h_d = mix(h_{d-1} ^ (uint64(u + 1) * G))          (h_{d-1}: the value of the sequence's last member)
 *   keep iff (h_d >> 32) < thr[d];   thr[d] an integer in 0 .. 2^32: probability thr[d] / 2^32, 2^32 = always, 0 = never
 * -- a function of (seed, replica, graph, the sequence, u) alone.  A kept child is tallied and descended; a dropped
 * child is neither: its whole subtree goes.
 * Output: tally int64 [num_replicas][N][Q], tally[r][v][q] = the kept subsets with maximum v whose induced subgraph is
 * of query q's class, zeroed and filled by the call.  With W_j = prod_{d=2..j} 2^32 / thr[d], tally * W_size(q) is the
 * unbiased estimate.  per_graph = 1: out is int64 [num_replicas][G][Q], the rows of every graph summed (the node rows
 * are never stored); 0: the layout above.  thr int64 [kmax + 1] is a HOST array in both entry points (entries 0 and 1
 * are not read).  All thresholds 2^32: every replica is the exact count.  graph_base / replica_base offset the counter,
 * so that a slice of the graphs or a chunk of the replicas reproduces the bits of the whole call.
 *
 * HOST desco_sampled_counts: queries as for desco_canonical_counts below, 2..kmax nodes, kmax in 2..6, pairwise
 *   non-isomorphic; OpenMP over (graph, replica) (num_threads 0 = the runtime's default); the result does not depend on
 *   num_threads.
 * DEVICE desco_sampled_counts_dev (gfx950): the device arguments of desco_canonical_counts_dev below up to num_queries
 *   (kmax in 2..5, at most 32 queries), one launch on `stream`, one wavefront per (CSR entry (v, u) with u < v,
 *   replica): a dropped level-2 decision ends the wavefront at once.  Does not allocate or synchronise; equal to the
 *   host routine bit for bit (integer adds commute), and the same from call to call.
 * Both: DESCO_EINVAL naming the entry point for a null pointer, kmax or num_queries out of range, a threshold outside
 *   0 .. 2^32, a negative count or base, and (device) more than (2^31 - 1) * 4 work items (entries x replicas).
 *   num_replicas == 0, no queries or an empty set: nothing is done, 0 is returned.
 * ------------------------------------------------------------------------------------------ */
int desco_sampled_counts(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr, const int32_t* col,
                         const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges, int num_queries,
                         int kmax, const int64_t* thr, uint64_t seed, int64_t graph_base, int64_t replica_base,
                         int num_replicas, int per_graph, int num_threads, int64_t* out);
int desco_sampled_counts_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes, const int64_t* rowptr,
                             int64_t num_entries, const int32_t* col, const int32_t* node_graph,
                             const int64_t* bit_off, uint64_t* bits, int64_t num_words, const int16_t* cls, int kmax,
                             int num_queries, const int64_t* thr, uint64_t seed, int64_t graph_base,
                             int64_t replica_base, int num_replicas, int per_graph, int64_t* out,
                             desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GRAPHLET CORRELATION: graphlet correlation matrices of the segments of an orbit table and the graphlet correlation
 * distance between them (GCD; Yaveroglu et al., "Revealing the hidden language of complex networks", 2014;
 * csrc/graphlet_correlation.hpp, csrc/graphlet_correlation.cpp, csrc/graphlet_correlation_dev.hip).
 *
 * INPUT: an orbit table counts int64 [N][ld] (desco_orbit_counts below); columns int32 [C], entries in 0 .. ld - 1, C
 *   in 0 .. DESCO_GCM_MAX_COLUMNS (a HOST array in both entry points); seg_ptr int64 [S + 1], monotone: segment s is
 *   the rows seg_ptr[s] .. seg_ptr[s + 1] - 1 (seg_ptr = graph_ptr: one segment per graph).  dummy_row = 1: every
 *   segment gets one extra row whose value is 1 in every column, so that a column of zeros is not constant.  That is
 *   the convention of the published GCD scripts as far as it is known to this project; it is STATED here, not pinned
 *   against a copy of them.  n' = the rows of a segment, the extra row included.
 * CENTRED DOUBLED RANK: for column c and row i of a segment, less = the rows of the segment with a smaller value,
 *   equal = those with the same value, i itself included:  d[i][c] = 2 less + equal - n'  -- twice the average rank
 *   (ties share the mean of their positions less + 1 .. less + equal) minus n' + 1.  An integer; every column sums to 0.
 * INTEGER MATRIX: S[a][b] = sum over the segment's rows of d[i][a] d[i][b], int64, exact while n'^3 < 2^63: a segment
 *   of more than 2097151 rows is refused.  Integer sums commute: S does not depend on the order of the rows or on any
 *   tiling, and relabelling a graph does not change it.
 * CORRELATION (Spearman's rho of the columns): rho[a][b] = (double)S[a][b] / sqrt((double)S[a][a] * (double)S[b][b]);
 *   rho[a][a] = 1; rho[a][b] = 0 where S[a][a] or S[b][b] is 0 (a column that is constant even with the dummy row).
 *   One correctly rounded IEEE operation per step, none of them contractible.
 * VECTOR: the upper triangle a < b of rho in row-major order, P = C (C - 1) / 2 doubles.
 * DISTANCE: gcd(x, y) = sqrt(acc); acc starts at 0 and runs acc = fma(t, t, acc), t = x[p] - y[p], for p = 0 .. P - 1
 *   IN THAT ORDER.  x double [Gx][P], y double [Gy][P], out[i * ldo + j] = gcd(x_i, y_j), ldo >= Gy: out may be a
 *   strided view, and only those Gx * Gy elements are written.
 *
 * HOST desco_graphlet_correlation: S_out int64 [S][C][C], rho_out double [S][C][C], either may be NULL.  OpenMP over
 *   segments (num_threads 0 = the runtime's default), ranks by a sort and its tie groups; the result does not depend
 *   on num_threads.  DESCO_EINVAL naming the entry point for: a negative count, C or dummy_row out of range, a null
 *   pointer where an array is needed, a column index outside the table, a seg_ptr that is negative or not monotone, a
 *   segment above the row limit -- before anything is written.
 * HOST desco_gcd_matrix: OpenMP over the rows of x.
 * DEVICE desco_graphlet_correlation_dev (gfx950): device arrays (columns on the host); two launches on `stream` for
 *   the segments seg_ids[0 .. num_ids) (int64, device; NULL = all num_segs): the ranks, one block per (segment,
 *   column) with the column's values in LDS, into work int32 [num_rows + num_segs][C] (segment s at row seg_ptr[s] +
 *   s); then S = D^T D, rho and the vector, one block per segment.  vec_out double [S][P]; S_out, rho_out and vec_out
 *   may each be NULL.  max_rows is the caller's bound on n' over the launch and sizes its LDS (one wave per column up
 *   to DESCO_GCM_WAVE_ROWS, four above).  A bound above DESCO_GCM_DEV_MAX_ROWS is refused (DESCO_EINVAL naming the
 *   limit): a larger segment goes to the host routine.  status int32 [S]: 0 for a segment that was computed; -1, and
 *   none of its outputs written, for one over the launch's bound or with rows outside 0 .. num_rows.  Only the
 *   launch's segments are written.  No allocation, no synchronisation, no global atomics; S equals the host routine
 *   bit for bit.
 * DEVICE desco_gcd_matrix_dev (gfx950): one launch, a 32 x 32 tile of pairs per block, every pair's fma chain in
 *   ascending p on the fp64 vector pipe (no matrix instruction: its order of summation is not the defined one).
 * ------------------------------------------------------------------------------------------ */
#define DESCO_GCM_MAX_COLUMNS 128
#define DESCO_GCM_DEV_MAX_ROWS 20480 /* one int64 column = 160 KiB of LDS */
#define DESCO_GCM_WAVE_ROWS 256
int desco_graphlet_correlation(const int64_t* seg_ptr, int64_t num_segs, const int64_t* counts, int64_t ld,
                               const int32_t* columns, int C, int dummy_row, int64_t* S_out, double* rho_out,
                               int num_threads);
int desco_gcd_matrix(const double* x, int64_t Gx, const double* y, int64_t Gy, int64_t P, double* out, int64_t ldo,
                     int num_threads);
int desco_graphlet_correlation_dev(const int64_t* seg_ptr, int64_t num_segs, int64_t num_rows, const int64_t* counts,
                                   int64_t ld, const int32_t* columns, int C, int dummy_row, const int64_t* seg_ids,
                                   int64_t num_ids, int64_t max_rows, int32_t* work, int64_t* S_out, double* rho_out,
                                   double* vec_out, int32_t* status, desco_stream_t stream);
int desco_gcd_matrix_dev(const double* x, int64_t Gx, const double* y, int64_t Gy, int64_t P, double* out, int64_t ldo,
                         desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GRAPHLET DEGREE DISTRIBUTION: per segment and orbit column, how many nodes touch the orbit k times, and the
 * graphlet degree distribution agreement between segments (GDDA; Przulj, "Biological network comparison using graphlet
 * degree distribution", Bioinformatics 2007; csrc/graphlet_distribution.hpp, csrc/graphlet_distribution.cpp,
 * csrc/graphlet_distribution_dev.hip).  Unlike the graphlet correlation it sees magnitude: two complete graphs of
 * different sizes have correlation distance 0 and agreement 0 on every orbit that both touch.
 *
 * INPUT: as for GRAPHLET CORRELATION -- counts int64 [N][ld]; columns int32 [C], a HOST array, entries in 0 .. ld - 1,
 *   C in 1 .. DESCO_GCM_MAX_COLUMNS; seg_ptr int64 [S + 1], monotone; n_s = the rows of segment s.  No dummy row.
 * DISTRIBUTION of (segment s, column c): the distinct values k >= 1 of the column over the segment's rows in ascending
 *   order, k_0 < k_1 < ..., with multiplicities d_i (rows whose value is below 1 are left out: Przulj's k starts at 1).
 *   S_i = (double)d_i / (double)k_i (both conversions round to nearest);  T = 0, T = T + S_i for i ascending IN THAT
 *   ORDER;  N_i = S_i / T.  The list may be empty (no node of the segment touches the orbit): then N is 0 everywhere.
 *   Keys and multiplicities are integers that do not depend on the order of the rows, so relabelling a graph changes
 *   no bit.
 * STORAGE (both builders): len int32 [S][C], key int64 [N * C], val double [N * C]; the list of (s, c) occupies the
 *   positions seg_ptr[s] * C + c * n_s + i, i < len[s][c]; the other positions of a computed segment are written as 0
 *   (a real key is never 0).  No scan, no allocation, no atomics and no synchronisation are needed to place a list.
 * AGREEMENT of segments x and y in column c: acc = 0; over the union of the two key lists in ascending key,
 *   t = N_x(k) - N_y(k) with a missing key contributing 0 (so t is N_x(k) or -N_y(k) there), acc = fma(t, t, acc) --
 *   a fixed order, no parallel reduction inside a pair.  D_c = sqrt(0.5 * acc);  A_c = D_c > 1.0 ? 0.0 : 1.0 - D_c (the
 *   clamp only guards rounding).  Two empty lists give A_c = 1; an empty list against a non-empty one gives
 *   1 - sqrt(0.5 sum N^2): this project's convention, STATED here and not pinned against GraphCrunch.
 *   Of the pair: sum = 0, sum = sum + A_c for c = 0 .. C - 1 IN THAT ORDER; agree = sum / (double)C.
 *   agree[i * ldo + j] for x_i and y_j, ldo >= Gy: agree may be a strided view and only those Gx * Gy elements are
 *   written; per_orbit[(i * Gy + j) * C + c] = A_c, or NULL.  The chain does not see the sign of t: agree(x, y) and
 *   agree(y, x) are the same bits, and agree(x, x) is exactly 1.
 *   Every step is one correctly rounded IEEE double operation, none contracted except the written fma.
 *
 * HOST desco_gdd_build: OpenMP over (segment, column), a sort and its runs; no row limit beyond memory.
 * HOST desco_gdd_agreement: OpenMP over the segments of x, a two-pointer merge per pair and column.  Neither result
 *   depends on num_threads (0 = the runtime's default).  DESCO_EINVAL naming the entry point for: a null pointer where
 *   an array is needed, a negative count, C outside 1 .. 128, a column index outside the table, a seg_ptr that is
 *   negative or not monotone, a len outside 0 .. n_s, ldo < Gy -- before anything is written.
 * DEVICE desco_gdd_build_dev (gfx950): device arrays (columns on the host); ONE launch on `stream` for the segments
 *   seg_ids[0 .. num_ids) (int64, device; NULL = all num_segs), a block per (segment, column) with the column in LDS:
 *   one wave up to DESCO_GCM_WAVE_ROWS, four above.  The list's own key / val slots serve as the sort's scratch.
 *   max_rows is the caller's bound on n_s over the launch and sizes its LDS; a bound above DESCO_GCM_DEV_MAX_ROWS is
 *   refused (DESCO_EINVAL naming the limit): a larger segment goes to the host routine.  status int32 [S]: 0 for a
 *   computed segment; -1, and nothing of it written, for one over the launch's bound or with rows outside
 *   0 .. num_rows.  Only the launch's segments are written.  T is added up by one wave in the defined order.
 * DEVICE desco_gdd_agreement_dev (gfx950): ONE launch, a 32 x 32 tile of pairs per block; per column the tile's lists
 *   are staged in LDS where they fit and read from global memory where they do not, so lists of ANY length are
 *   accepted (host-built lists of long segments too); every pair's merge and fma chain runs in ascending key on the
 *   fp64 vector pipe.  A len outside 0 .. n_s is clamped.  Both: no allocation, no synchronisation, no global atomics;
 *   the results equal the host routines bit for bit.
 * ------------------------------------------------------------------------------------------ */
int desco_gdd_build(const int64_t* seg_ptr, int64_t num_segs, const int64_t* counts, int64_t ld,
                    const int32_t* columns, int C, int32_t* len, int64_t* key, double* val, int num_threads);
int desco_gdd_agreement(const int64_t* x_seg_ptr, const int32_t* x_len, const int64_t* x_key, const double* x_val,
                        int64_t Gx, const int64_t* y_seg_ptr, const int32_t* y_len, const int64_t* y_key,
                        const double* y_val, int64_t Gy, int C, double* agree, int64_t ldo, double* per_orbit,
                        int num_threads);
int desco_gdd_build_dev(const int64_t* seg_ptr, int64_t num_segs, int64_t num_rows, const int64_t* counts, int64_t ld,
                        const int32_t* columns, int C, const int64_t* seg_ids, int64_t num_ids, int64_t max_rows,
                        int32_t* len, int64_t* key, double* val, int32_t* status, desco_stream_t stream);
int desco_gdd_agreement_dev(const int64_t* x_seg_ptr, const int32_t* x_len, const int64_t* x_key, const double* x_val,
                            int64_t Gx, const int64_t* y_seg_ptr, const int32_t* y_len, const int64_t* y_key,
                            const double* y_val, int64_t Gy, int C, double* agree, int64_t ldo, double* per_orbit,
                            desco_stream_t stream);

/* HOST: exact canonical (induced, symmetry-normalised) counts of connected query graphs with
 * 2..6 nodes for every node of every graph: out[v][q] = #{S : max(S) = v, G[S] isomorphic to q}.
 * Replaces the VF2 ground truth (workload.py:327-348 MatchSubgraphWorker divided by
 * data.py:61-88 SymmetricFactor; driver workload.py:551-726).  Query q has q_nodes[q] nodes and the
 * undirected edges q_edges[2*e], q_edges[2*e+1] for e in [q_edge_ptr[q], q_edge_ptr[q+1]).
 * out: int64 [num_nodes][num_queries]. */
int desco_canonical_counts(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                           const int32_t* col, const int32_t* q_nodes, const int32_t* q_edge_ptr,
                           const int32_t* q_edges, int num_queries, int num_threads,
                           int64_t* out);

/* The same counts on the GPU (csrc/groundtruth_dev.hip): queries of 2..5 nodes, at most 32, pairwise
 * non-isomorphic (the host entry above takes the general case).
 * HOST helper: table[1098] = for k = 2..5 nodes and every adjacency mask on k nodes (bit
 * b(b-1)/2 + a for the pair a < b; the masks of k nodes start at offsets 0, 2, 10, 74) the index of
 * the query of that isomorphism class, or -1; *kmax = the largest query. */
int desco_canonical_class_table(const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                const int32_t* q_edges, int num_queries, int16_t* table, int* kmax);
/* DEVICE: graph_ptr [G+1], rowptr [N+1] (int64), col [num_entries] (global node ids, rows ascending),
 * node_graph [N] (graph of every node), bit_off [G] (first word of graph g's adjacency bitset: rows of
 * ceil(n_g/64) words), bits [num_words] workspace, cls = the table above; all device pointers.
 * out: int64 [N][num_queries], zeroed and filled by the call.  Enqueues on `stream`, does not
 * allocate or synchronise. */
int desco_canonical_counts_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                               const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                               const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                               int64_t num_words, const int16_t* cls, int kmax, int num_queries,
                               int64_t* out, desco_stream_t stream);

/* The same counts on the GPU for queries of 2..6 nodes (csrc/groundtruth6_dev.hip): the walk at depth six, every
 * column in one walk.  Queries as for desco_canonical_counts: 2..6 nodes, pairwise non-isomorphic, at most 142 (every
 * connected class of 2..6 nodes: 1 + 2 + 6 + 21 + 112).
 * HOST helper desco_canonical_class_table6: table[33866] = for k = 2..6 nodes and every adjacency mask on k nodes
 *   (bit b(b-1)/2 + a for the pair a < b; the masks of k nodes start at offsets 0, 2, 10, 74, 1098; entries 0..1097 are
 *   those of desco_canonical_class_table for the same queries) the index of the query of that isomorphism class, or
 *   -1; *kmax = the largest query.  DESCO_EINVAL naming the entry point for a null pointer, a size outside "2..6
 *   nodes", "isomorphic" queries, a "bad query edge" and more than 142 queries.
 * DEVICE desco_canonical_counts6_dev: the device arguments of desco_canonical_counts_dev up to num_words, cls = the
 *   table above (device pointer), kmax in 2..6, num_queries in 1..142 (0: nothing to do), then the slice
 *   [entry_begin, entry_end) of the CSR entries.  The launch contract is desco_canonical_counts_match_dev's: the call
 *   with entry_begin = 0 zeroes out and builds the bitset rows, every call ADDS the counts of its slice; the caller
 *   cuts [0, num_entries) into ascending slices.  out: int64 [N][num_queries], bit-identical to the host enumerator
 *   from call to call and for every slicing.  Enqueues on `stream`, does not allocate or synchronise; bad arguments
 *   are refused by name before anything is launched. */
int desco_canonical_class_table6(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                                 int num_queries, int16_t* table, int* kmax);
int desco_canonical_counts6_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                int64_t num_words, const int16_t* cls, int kmax, int num_queries,
                                int64_t entry_begin, int64_t entry_end, int64_t* out, desco_stream_t stream);

/* ORBIT COUNTS (graphlet degree vectors): how many occurrences of a query contain node v, with v in a given position
 * of the query -- unlike the canonical counts above they do not depend on the node numbering.
 *   Query: connected, loop-free, 2..5 nodes, given as for desco_canonical_counts; pairwise non-isomorphic.
 *   Orbits of a query: the orbits of Aut(q) on its node positions, numbered 0, 1, .. in ascending order of their
 *     smallest member position.
 *   out[v][(q,o)] = #{S containing v : G[S] isomorphic to q, and an isomorphism G[S] -> q maps v into orbit o} (well
 *     defined: two such isomorphisms differ by an automorphism).
 *   Columns: the queries in the given order and, inside a query, its orbits in order.  The 30 connected graphs of
 *     2..5 nodes have 1 + 3 + 11 + 58 = 73 orbits.  (The numbering is this library's own.)
 *   Per graph, sum_v out[v][(q,o)] = |o| * sum_v canonical count[v][q]; the column of the 2-node query is the degree.
 * HOST helper desco_orbit_table: table[1098][5] = for k = 2..5 nodes and every adjacency mask on k nodes (the
 *   convention and the offsets 0, 2, 10, 74 of desco_canonical_class_table) the column of every position i < k of the
 *   subset, or -1 when the mask's class was not asked for; *num_columns, *kmax = the largest query.  DESCO_EINVAL
 *   naming "2..5 nodes", "connected" or "isomorphic" for queries it does not take.
 * HOST desco_orbit_counts: the arguments of desco_canonical_counts; out: int64 [num_nodes][num_columns] (the caller
 *   gets num_columns from desco_orbit_table), zeroed and filled.  OpenMP over graphs; the result does not depend on
 *   num_threads.
 * DEVICE desco_orbit_counts_dev (csrc/groundtruth_dev.hip): the arguments of desco_canonical_counts_dev with the
 *   orbit table (device pointer) in place of cls and num_columns (<= 73) in place of num_queries.  out: int64
 *   [N][num_columns], zeroed and filled by the call, equal to the host's bit for bit.  Enqueues on `stream`, does not
 *   allocate or synchronise. */
int desco_orbit_table(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges, int num_queries,
                      int16_t* table, int* num_columns, int* kmax);
int desco_orbit_counts(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr, const int32_t* col,
                       const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges, int num_queries,
                       int num_threads, int64_t* out);
int desco_orbit_counts_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes, const int64_t* rowptr,
                           int64_t num_entries, const int32_t* col, const int32_t* node_graph, const int64_t* bit_off,
                           uint64_t* bits, int64_t num_words, const int16_t* orbit_table, int kmax, int num_columns,
                           int64_t* out, desco_stream_t stream);

/* EDGE ORBIT COUNTS (edge graphlet degree vectors): how many occurrences of a query run through the edge {a, b} of a
 * graph, with the edge in a given role of the query (the chord of a diamond or its rim, ..).
 *   Query: as for the orbit counts: connected, loop-free, 2..5 nodes, pairwise non-isomorphic.
 *   Edge orbits of a query: the orbits of Aut(q) on the query's EDGE set.  The edges are ordered by their pair bit
 *     b(b-1)/2 + a (a < b, the convention of the adjacency masks); the orbits are numbered 0, 1, .. in ascending order
 *     of their smallest member.
 *   Rows: one per undirected edge of the graph set, in the order of the CSR entries (v, u) with u < v (ascending v, then
 *     ascending u) -- the work items of the ESU walk.
 *   out[e][(q,o)] = #{connected node subsets S that contain both ends of e : G[S] isomorphic to q by a map that takes e
 *     into edge orbit o}.
 *   Columns: the queries in the given order and, inside a query, its edge orbits in order.  The 30 connected graphs of
 *     2..5 nodes have 1 + 2 + 10 + 56 = 69 edge orbits.  (The numbering is this library's own; ORCA's 68 edge orbits
 *     leave out the single edge.)
 *   Per graph, sum_e out[e][(q,o)] = |o| * sum_v canonical count[v][q]; the column of the 2-node query is 1; the
 *     triangle's is the number of common neighbours of a and b.
 * HOST helper desco_edge_orbit_table: table[1098][10] = for k = 2..5 nodes and every adjacency mask on k nodes (the
 *   offsets of desco_canonical_class_table) and every pair bit p of k nodes the column of that pair, when the mask's
 *   class was asked for and the pair is an edge of the mask; else -1.  *num_columns, *kmax = the largest query.
 *   DESCO_EINVAL naming "2..5 nodes", "connected", "isomorphic" or "bad query edge" for queries it does not take.
 * HOST desco_edge_orbit_counts: the arguments of desco_orbit_counts; out: int64 [num_edges][num_columns], num_edges =
 *   the number of CSR entries (v, u) with u < v, zeroed and filled.  OpenMP over graphs; the result does not depend on num_threads.
 * DEVICE desco_edge_orbit_counts_dev (csrc/groundtruth_dev.hip): the arguments of desco_orbit_counts_dev, and after
 *   num_words: entry_row, int32 [num_entries], the row of the edge of every CSR entry (both directions of an edge name
 *   one row; every value in [0, num_rows)), and num_rows.  At most 69 columns, num_entries below 2^31.  out: int64
 *   [num_rows][num_columns], zeroed and filled by the call, equal to the host's bit for bit.  Enqueues on `stream`,
 *   does not allocate or synchronise. */
int desco_edge_orbit_table(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges, int num_queries,
                           int16_t* table, int* num_columns, int* kmax);
int desco_edge_orbit_counts(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr, const int32_t* col,
                            const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges, int num_queries,
                            int num_threads, int64_t* out);
int desco_edge_orbit_counts_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes, const int64_t* rowptr,
                                int64_t num_entries, const int32_t* col, const int32_t* node_graph,
                                const int64_t* bit_off, uint64_t* bits, int64_t num_words, const int32_t* entry_row,
                                int64_t num_rows, const int16_t* edge_orbit_table, int kmax, int num_columns,
                                int64_t* out, desco_stream_t stream);

/* LABELLED queries (--use_node_feature): out[v][c] = #{S : max(S) = v, G[S] connected, and G[S] with its node
 * labels isomorphic to the labelled queries of class c} -- the reference's VF2 with node_match on the feature
 * (workload.py:327-348) divided by the labelled symmetry factor (data.py:61-68).  Node and query labels are integer
 * ids 0..num_labels-1 (the caller maps equal feature rows to equal ids).  Query q is given as in
 * desco_canonical_counts plus its labels q_labels[o_q .. o_q + q_nodes[q] - 1], o_q = q_nodes[0] + .. + q_nodes[q-1].
 * The reference's expansion (utils.py:258-272) contains labelled copies that are isomorphic to each other, so any
 * number of queries and duplicates are accepted everywhere below and counting is per labelled isomorphism CLASS:
 * the caller expands out[:, class_of_query[q]] to query columns.
 *
 * HOST helper: class_of_query[num_queries] (classes are numbered 0..*num_classes-1 in the order of their first
 * query) and *kmax = the largest query.  Queries of 2..6 nodes, num_labels <= 256. */
int desco_canonical_label_classes(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                                  const int32_t* q_labels, int num_queries, int num_labels,
                                  int32_t* class_of_query, int* num_classes, int* kmax);
/* HOST enumerator (csrc/groundtruth_label.cpp; ESU rooted at the maximum id, OpenMP over graphs): labels [N] int32,
 * class_of_query / num_classes from the helper above, queries of 2..6 nodes, num_labels <= 256.
 * out: int64 [N][num_classes], zeroed and filled by the call.  No nodes or no queries: returns 0, touches nothing. */
int desco_canonical_counts_labelled(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                    const int32_t* col, const int32_t* labels, int num_labels,
                                    const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                                    const int32_t* q_labels, int num_queries, const int32_t* class_of_query,
                                    int num_classes, int num_threads, int64_t* out);
/* The same counts on the GPU (csrc/groundtruth_label_dev.hip): queries of 2..5 nodes and num_labels <= 16 (label
 * ids of 4 bits), any number of queries.  The kernel classifies a found k-subset with ONE read of a direct table:
 * entry  off[k] + mask * A^k + sum_j label_j * A^j  (A = num_labels; mask as in desco_canonical_class_table, labels in
 * subset order; off[2] = 0, off[k+1] = off[k] + 2^(k(k-1)/2) * A^k) holds the class or -1.
 * HOST helpers: desco_canonical_label_table_size = number of int32 entries for queries up to kmax nodes (-1 with a
 * message outside 2..5 nodes / 1..16 labels; 1024 * A^5 entries dominate at kmax = 5: 67 MB at A = 7, 134 MB at
 * A = 8 -- the caller decides what it affords, at most 2^31 - 1 entries); desco_canonical_label_table fills
 * table[table_entries] with every relabeling of every class. */
int64_t desco_canonical_label_table_size(int kmax, int num_labels);
int desco_canonical_label_table(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                                const int32_t* q_labels, int num_queries, int num_labels,
                                const int32_t* class_of_query, int num_classes, int kmax, int32_t* table,
                                int64_t table_entries);
/* DEVICE: the arguments of desco_canonical_counts_dev, then labels [N] int32 (ids 0..num_labels-1; a node with an
 * id outside that range matches nothing), the table above and its size; all device pointers.
 * out: int64 [N][num_classes], zeroed and filled by the call (64-bit integer atomics: bit-identical from run to
 * run).  Enqueues on `stream`, does not allocate or synchronise.  No nodes or no classes: returns 0. */
int desco_canonical_counts_labelled_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                        const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                        const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                        int64_t num_words, const int32_t* labels, int num_labels,
                                        const int32_t* table, int64_t table_entries, int kmax, int num_classes,
                                        int64_t* out, desco_stream_t stream);

/* LARGE queries (2..16 nodes): a pattern-guided induced-subgraph matcher next to the ESU enumerators above, whose
 * class tables of 2^(k(k-1)/2) masks stop at 6 nodes.  Same definition: out[v][q] = #{S : max(S) = v, G[S] isomorphic
 * to q}.  Queries as in desco_canonical_counts: connected, loop-free, any number, isomorphic duplicates allowed (equal
 * columns); anything else is DESCO_EINVAL with a message naming the limit.
 *
 * HOST helpers (csrc/groundtruth_match.cpp): the PLAN of a query set, a flat int32 array -- plan[0] = num_queries,
 * plan[1] = number of anchors A, then A records of 84 int32, sorted by query.  A record is one anchor: the query node
 * that is mapped to the root v while every other image stays below v, one per orbit of the query's automorphism
 * group.  rec[0] = query, rec[1] = k, rec[2] = anchor, rec[3] = divisor of the map count (always 1: see below),
 * rec[4 + i] = query node at position i of a connected matching order (position 0 = the anchor), rec[20 + i] = the
 * earlier position whose image's adjacency row supplies the candidates of position i, rec[36 + i] = mask of the
 * earlier positions whose images must be adjacent to i's (the other earlier positions must NOT be), rec[52 + i] /
 * rec[68 + i] = masks of the earlier positions whose image must be above / below i's: symmetry-breaking order
 * constraints (Grochow-Kellis) inside the anchor's stabiliser, which leave exactly one map per subset.
 * desco_canonical_match_plan_size = number of int32 entries (-1 with a message), desco_canonical_match_plan fills
 * plan[plan_entries]. */
int64_t desco_canonical_match_plan_size(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                                        int num_queries);
int desco_canonical_match_plan(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                               int num_queries, int32_t* plan, int64_t plan_entries);
/* HOST matcher (OpenMP over graphs, per-graph adjacency bitset rows, depth-first over the plan).
 * out: int64 [N][num_queries], zeroed and filled by the call. */
int desco_canonical_counts_match(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                 const int32_t* col, const int32_t* plan, int64_t plan_entries, int num_queries,
                                 int num_threads, int64_t* out);
/* DEVICE matcher (csrc/groundtruth_match_dev.hip): the device arguments of desco_canonical_counts_dev, then the plan
 * twice -- plan_host (validated here: the kernel indexes with its fields) and its device copy plan_dev -- and the
 * slice [entry_begin, entry_end) of CSR entries this call covers: one wave per (entry (v, u0) with u0 < v, record).
 * The work of a large query on a dense graph is unbounded, so the caller cuts [0, num_entries) into slices, in
 * ascending order, and checks every status; the call with entry_begin = 0 zeroes out and builds the bitset rows,
 * every call adds its slice's counts into out: int64 [N][num_queries] (64-bit integer atomics: bit-identical from
 * run to run and for every slicing).  Enqueues on `stream`, does not allocate or synchronise. */
int desco_canonical_counts_match_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                     const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                     const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                     int64_t num_words, const int32_t* plan_host, const int32_t* plan_dev,
                                     int64_t plan_entries, int num_queries, int64_t entry_begin, int64_t entry_end,
                                     int64_t* out, desco_stream_t stream);

/* LABELLED LARGE queries (--use_node_feature, 2..16 nodes): the matcher above with a label id on every query node
 * and on every graph node; a map must preserve labels as well as edges and non-edges.  Label ids are any
 * non-negative int32 (the matcher compares ids: no alphabet limit); q_labels is laid out as in
 * desco_canonical_label_classes.  Two queries are one CLASS iff a bijection between them preserves edges and labels;
 * classes are numbered in the order of their first query and the plan is built over classes, so each is matched once
 * however many isomorphic copies the reference's F^k expansion holds: the caller expands out[:, class_of_query[q]].
 *
 * The labelled PLAN: plan[0] = num_classes, plan[1] = number of records A, plan[2] = number of buckets B, plan[3] = the
 * size of the largest bucket, then A records of 100 int32, then B buckets of 4 int32.  A record is the 84-entry record
 * above -- rec[0] = the class, one record per orbit of the LABEL-PRESERVING automorphism group, order constraints
 * that break only that group (divisor 1) -- followed by rec[84 + i] = the label of position i.  Records are sorted by
 * (label of position 0, label of position 1), then class; bucket = (label 0, label 1, first record, end record) of one
 * run, ascending.  desco_canonical_match_plan_labelled_size = number of int32 entries (-1 with a message);
 * desco_canonical_match_plan_labelled fills plan[plan_entries], class_of_query[num_queries] and *num_classes. */
int64_t desco_canonical_match_plan_labelled_size(const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                                 const int32_t* q_edges, const int32_t* q_labels, int num_queries);
int desco_canonical_match_plan_labelled(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                                        const int32_t* q_labels, int num_queries, int32_t* plan, int64_t plan_entries,
                                        int32_t* class_of_query, int* num_classes);
/* HOST labelled matcher (OpenMP over graphs): labels [N] int32; a candidate's label is tested before its adjacency
 * bits.  A node whose label no query position carries matches nothing.  out: int64 [N][num_classes], zeroed and
 * filled by the call. */
int desco_canonical_counts_match_labelled(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                          const int32_t* col, const int32_t* labels, const int32_t* plan,
                                          int64_t plan_entries, int num_classes, int num_threads, int64_t* out);
/* DEVICE labelled matcher (csrc/groundtruth_match_dev.hip): the arguments of desco_canonical_counts_match_dev plus the
 * device labels [N], with the labelled plan.  One wave per (CSR entry (v, u0) of the slice, j < largest bucket): the
 * wave takes the j-th record of the bucket of (labels[v], labels[u0]) or retires, so a slice launches
 * (entry_end - entry_begin) * plan[3] waves whatever the number of records.  Slices, zeroing, atomics and the
 * no-allocation / no-synchronisation rule as desco_canonical_counts_match_dev; out: int64 [N][num_classes]. */
int desco_canonical_counts_match_labelled_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                              const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                              const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                              int64_t num_words, const int32_t* labels, const int32_t* plan_host,
                                              const int32_t* plan_dev, int64_t plan_entries, int num_classes,
                                              int64_t entry_begin, int64_t entry_end, int64_t* out,
                                              desco_stream_t stream);

/* NON-INDUCED counts (occurrences as a not necessarily induced subgraph; monomorphisms):
 *   out[v][q] = #{ injective f : {f(a), f(b)} in E(G) for every {a, b} in E(q), max(im f) = v } / |Aut(q)|,
 * int64, bit-exact.  Two occurrences on the same node set with different edge sets are two occurrences: P3 in a triangle
 * counts 3, all at the triangle's largest node.  The four entries below are the four matchers above with one more
 * argument, `induced`: 1 = the induced counts of the entry without `_mode`, 0 = the definition above; anything else is
 * DESCO_EINVAL.  The PLANS are the same bytes in both modes (anchors, order and order constraints depend on Aut(q)
 * alone, and Aut(q) acts freely on monomorphisms as it does on induced embeddings: one map per occurrence, divisor 1);
 * with induced = 0 a set bit of rec[36 + i] still asks for an edge and a clear bit asks nothing.  Everything else --
 * labels, the u < v root rule, slices, zeroing, atomics -- is as documented for the entry without `_mode`. */
int desco_canonical_counts_match_mode(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                      const int32_t* col, const int32_t* plan, int64_t plan_entries, int num_queries,
                                      int induced, int num_threads, int64_t* out);
int desco_canonical_counts_match_mode_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                          const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                          const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                          int64_t num_words, const int32_t* plan_host, const int32_t* plan_dev,
                                          int64_t plan_entries, int num_queries, int induced, int64_t entry_begin,
                                          int64_t entry_end, int64_t* out, desco_stream_t stream);
int desco_canonical_counts_match_labelled_mode(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                               const int32_t* col, const int32_t* labels, const int32_t* plan,
                                               int64_t plan_entries, int num_classes, int induced, int num_threads,
                                               int64_t* out);
int desco_canonical_counts_match_labelled_mode_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes,
                                                   const int64_t* rowptr, int64_t num_entries, const int32_t* col,
                                                   const int32_t* node_graph, const int64_t* bit_off, uint64_t* bits,
                                                   int64_t num_words, const int32_t* labels, const int32_t* plan_host,
                                                   const int32_t* plan_dev, int64_t plan_entries, int num_classes,
                                                   int induced, int64_t entry_begin, int64_t entry_end, int64_t* out,
                                                   desco_stream_t stream);
/* DEVICE: non-induced counts of SMALL queries from a census.  The ESU enumerators visit every connected k-subset once,
 * so with counts[v][c] = the induced count of EVERY connected k-node class c (desco_canonical_counts_dev on the class
 * representatives) the non-induced counts are  out[v][q] = sum_c counts[v][c] * m[c][q],  m[c][q] = the occurrences of q
 * in c (0 when their sizes differ).  counts: int64 [N][ldc], m: int64 [num_classes][num_queries] (device), out: int64
 * [N][ldo]; num_classes 1..32, num_queries <= 64; accumulate = 1 adds to out (a census cut into chunks of 32 classes),
 * 0 overwrites it.  Integer arithmetic modulo 2^64.  Enqueues on `stream`, does not allocate or synchronise. */
int desco_canonical_noninduced_transform_dev(const int64_t* counts, int64_t ldc, const int64_t* m, int64_t num_nodes,
                                             int num_classes, int num_queries, int accumulate, int64_t* out,
                                             int64_t ldo, desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * OCCURRENCE LISTING: the occurrences themselves ("which ones"), where the matchers above answer "how many".
 *
 * For a graph set and ONE query q (connected, loop-free, 2..16 nodes: a plan of desco_canonical_match_plan with
 * plan[0] = 1) the listing is rows, int32 [M][k], and ptr, int64 [N + 1].
 *   Row       one row per occurrence; column a is the image of QUERY NODE a (the query's own numbering, not the plan's
 *             matching positions: rec[4 + i] is the query node of position i).  Ids are global node ids, as col holds.
 *   induced = 1   an occurrence is a node subset S with G[S] isomorphic to q; its row is the one map q -> G[S] that
 *             meets the plan's order constraints.
 *   induced = 0   an occurrence is a copy of q: an image edge set (P3 has three in a triangle).  A monomorphism onto a
 *             copy H is an isomorphism q -> H, so the maps onto H number |Aut(q)|, Aut(q) permutes them freely, and
 *             the same constraints select one: one row per copy.
 *   Segments  ptr is the exclusive scan of the query's canonical counts in the same mode (out[:, 0] of
 *             desco_canonical_counts_match_mode): rows [ptr[v], ptr[v + 1]) are the occurrences whose largest node is v,
 *             so column `anchor` of each equals v, anchor = rec[2] of the record that found the row; a query with
 *             several anchor orbits mixes records in one segment.
 *   Order     inside a segment, ascending lexicographic order of the k columns (rows of a segment are pairwise
 *             different: the order is total).  Given the plan, rows and ptr are fully defined: the two entry points
 *             below (the second with the caller's sort) return the same bits for any slicing, chunking and thread count.
 *
 * HOST (OpenMP over graphs): lists the anchors [node_begin, node_end) into rows, row ptr[v] - ptr[node_begin] first,
 * in the final order.  Refused, by name: a plan with plan[0] != 1 or whose records do not permute the query's nodes,
 * null pointers, negative sizes, a node range outside [0, N], a descending ptr, rows_capacity below
 * ptr[node_end] - ptr[node_begin] -- and, after the walk, a ptr whose segment differs from the number of maps found at
 * some node (named in the message; no row is ever stored outside its segment). */
int desco_list_occurrences(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr, const int32_t* col,
                           const int32_t* plan, int64_t plan_entries, int induced, int num_threads, int64_t node_begin,
                           int64_t node_end, const int64_t* ptr, int64_t rows_capacity, int32_t* rows);
/* DEVICE (csrc/occurrences_dev.hip): the listing instantiation of the matcher kernel.  Arguments up to entry_end as
 * desco_canonical_counts_match_mode_dev (num_queries must be 1), slices as there; then ptr [N + 1] (device), ptr_base =
 * the row index of the first row of `rows` (ptr[v0] when the call's entries are those of the anchors from v0 on, so that
 * a chunk of anchors is emitted into a buffer of its own), cursor: int32 [N], rows: int32 [rows_capacity][k] and
 * overflow: one int32 (all device).  The call with entry_begin = 0 zeroes cursor and *overflow and builds the bitset
 * rows.  A lane that completes a map takes slot = cursor[v]++ and stores its row at ptr[v] - ptr_base + slot; a slot
 * outside [0, ptr[v + 1] - ptr[v]) or a row outside [0, rows_capacity) is NOT stored and sets *overflow = 1, so no
 * store leaves rows whatever ptr, cursor and plan_dev hold.  Rows of a segment arrive in any order: the caller sorts
 * every segment after the last slice.  With the right ptr, afterwards cursor[v] = ptr[v + 1] - ptr[v] for the anchors
 * covered and *overflow = 0.  Refused, by name: what desco_canonical_counts_match_mode_dev refuses, num_queries or
 * plan[0] != 1, records that do not permute the query's nodes, null pointers, negative sizes, entry ranges outside
 * [0, num_entries].  Enqueues on `stream`, does not allocate or synchronise. */
int desco_list_occurrences_dev(const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes, const int64_t* rowptr,
                               int64_t num_entries, const int32_t* col, const int32_t* node_graph,
                               const int64_t* bit_off, uint64_t* bits, int64_t num_words, const int32_t* plan_host,
                               const int32_t* plan_dev, int64_t plan_entries, int num_queries, int induced,
                               int64_t entry_begin, int64_t entry_end, const int64_t* ptr, int64_t ptr_base,
                               int32_t* cursor, int64_t rows_capacity, int32_t* rows, int32_t* overflow,
                               desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DEVICE kernels
 * ------------------------------------------------------------------------------------------ */

/* K1/K16  pre_mp = nn.Linear(input_dim, H) (gnn_model.py:131, 231):
 * out[i, 0:n] = feat[i, 0:k] * wt[k][n] + bias   (wt = weight transposed, [k][n] row major) */
int desco_linear_smallk_f32(const float* feat, int64_t ldf, int k, const float* wt,
                            const float* bias, float* out, int64_t ldo, int64_t m, int n,
                            desco_stream_t stream);

/* K2/K3  SAGEConv message+aggregate for all relation slots at once (gnn_model.py:392-394,
 * 402-404: index_select + scatter_add):  out[v, 0:64] = sum_{e in vrow v} x[vcol[e], 0:64].
 * A 16-lane group (float4 per lane) per destination row, eight unconditional source loads in
 * flight per lane (absent sources read a zero row); S in {1,2,4}; vcol must be readable at
 * index 0 even when there is no edge.
 * out is [num_rows*S, 64] contiguous (== [num_rows, S*64]). */
int desco_csr_gather_sum_f32(const float* x, int64_t ldx, const int32_t* vrowptr,
                             const int32_t* vcol, int64_t num_rows, int slots, float* out,
                             desco_stream_t stream);

/* K4-K6, K8, K10, K12, K18, K20, K21: every dense projection of the path.
 * C[m, n] = act( [A1 | A2][m, :] * Wt + bias[(m % bias_rows), n] + sum_j S[m, j] * Ws[j, n] )
 *   A1: [M, k1] leading dim lda1;  A2: [M, k2] leading dim lda2 (k2 may be 0);  k1, k2 % 32 == 0
 *   Wt: [(k1+k2), n] row major (= torch weight transposed);  n % 64 == 0
 *   bias: [bias_rows, n] or NULL (bias_rows >= 1);  S: [M, ns] (ns <= 4) or NULL;  Ws: [ns, n]
 * fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain per output). */
int desco_gemm_f32(const float* a1, int64_t lda1, int k1, const float* a2, int64_t lda2, int k2,
                   const float* wt, int n, const float* bias, int bias_rows, const float* s,
                   int ns, const float* ws, int act, float slope, float* c, int64_t ldc,
                   int64_t m, desco_stream_t stream);

/* Counter-based dropout of the training steps (F.dropout after every layer's relu, gnn_model.py:274; nn.Dropout =
 * post_mp.1, gnn_model.py:44-53; --gossip_dropout defaults to 0.01, config.py:316).  No mask is stored: the 32 random
 * bits of element (row, col) are word (row & 3) of
 *   Philox4x32-10(counter = {row >> 2, col | site << 24, lo32(step), hi32(step)}, key = {lo32(seed), hi32(seed)})
 * with (seed, step) = key[0], key[1] read from DEVICE memory by the kernel (desco_rng_next writes them), so forward and
 * backward of one step see the same mask and a captured step draws a fresh mask on every replay.  The element is dropped
 * iff bits < threshold; kept elements are multiplied by scale.  key == NULL: no dropout.
 * Limits: row < 2^34, col < 2^24, site < 256. */
typedef struct desco_dropout {
  const uint64_t* key;  /* device, 2 words */
  uint32_t site;        /* which dropout call of the step (independent streams) */
  uint32_t threshold;   /* round(p * 2^32), p < 1 */
  float scale;          /* 1 / (1 - p)   (0 with threshold 0xffffffff stands for p >= 1) */
} desco_dropout;

/* Up to four INDEPENDENT products of desco_gemm_f32's form in one launch (the count-row and canonical-row halves of a
 * training layer, lightning_model.py:228-254 through gnn_model.py:253-277: same step, disjoint rows, different
 * weights).  Field meaning as the arguments of desco_gemm_f32; descriptors with m == 0 are skipped. */
typedef struct desco_gemm_desc {
  const float* a1; int64_t lda1; int k1;
  const float* a2; int64_t lda2; int k2;
  const float* wt; int n;
  const float* bias; int bias_rows;
  const float* s; int ns; const float* ws;
  int act; float slope;
  float* c; int64_t ldc; int64_t m;
  /* backward use: c = v * act'(gate[row, col]) for gate = the saved activation OUTPUT (gate_act / gate_slope: its
   * activation; NULL: none) -- desco_act_grad_f32 fused into the epilogue; accum != 0: c += v instead of c = v */
  const float* gate; int64_t ldg; int gate_act; float gate_slope; int accum;
  /* drop.key != NULL: the stored value is additionally multiplied by the dropout factor of (row, col) -- forward:
   * dropout(act(..)) (relu / leaky commute with a non-negative factor, so Linear -> Dropout -> LeakyReLU of post_mp is
   * this too); backward with a gate: dC * factor * act'(gate), the factor regenerated, not read */
  desco_dropout drop;
} desco_gemm_desc;
int desco_gemm_f32_multi(int num, const desco_gemm_desc* descs, desco_stream_t stream);

/* Same contract as desco_gemm_f32 but computed on the bf16 matrix pipe with fp32-level accuracy
 * ("bf16x6": each fp32 operand is split into three bf16 terms, the six products of weight >= 2^-16
 * are accumulated in fp32; error ~2^-23 per product).  The weight is passed N-MAJOR and already
 * split: w_planes[3][n][k1+k2] = (hi, mid, lo) bf16 bit patterns of torch's native [out, in] weight,
 * produced once per weight version by desco_split_bf16x3_f32 (planes[3][count] of w[count]). */
int desco_gemm_bf16x6_f32(const float* a1, int64_t lda1, int k1, const float* a2, int64_t lda2,
                          int k2, const int16_t* w_planes, int n, const float* bias, int bias_rows,
                          const float* s, int ns, const float* ws, int act, float slope, float* c,
                          int64_t ldc, int64_t m, desco_stream_t stream);
int desco_split_bf16x3_f32(const float* w, int64_t count, int16_t* planes, desco_stream_t stream);
/* One descriptor of desco_gemm_f32_multi's form on the bf16x6 pipe: d->wt is ignored, the weight is w_planes[3][n][k1+k2]
 * (n-major, as for desco_gemm_bf16x6_f32); bias / act / gate / drop as documented for desco_gemm_desc, accum must be 0.
 * ws_rows > 1: the scalar tail's matrix is per row class -- v += sum_j s[row, j] * ws[row % ws_rows][j][col] -- which is
 * desco_affine_rows_f32 (the gossip layers' per-query tables, ws_rows = the query count) fused into the epilogue.
 * For the training step's products that stream a million rows through a 64- to 256-wide weight (the gossip step's
 * forward and input-gradient products): fp32-accurate at the HBM rate instead of the fp32 matrix pipe's. */
int desco_gemm_bf16x6_desc_f32(const desco_gemm_desc* d, const int16_t* w_planes, int ws_rows, desco_stream_t stream);
/* planes[3][n][k] of the TRANSPOSE of w [k, n] (row stride ldw >= n): the n-major planes of a weight kept as [in, out], or
 * -- for an input-gradient product dA = dZ W -- of torch's [out, in] weight read as [k = out, n = in]. */
int desco_split_bf16x3_t_f32(const float* w, int k, int n, int64_t ldw, int16_t* planes, desco_stream_t stream);
/* Up to four INDEPENDENT descriptors on the bf16x6 pipe in one launch (planes[i] = the n-major planes of descriptor i;
 * 128 x 64 tiles for every problem): the count-row and canonical-row halves of a training layer's forward and
 * input-gradient products.  As desco_gemm_bf16x6_desc_f32 without the scalar tail (ns must be 0). */
int desco_gemm_bf16x6_multi_f32(int num, const desco_gemm_desc* descs, const int16_t* const* planes,
                                desco_stream_t stream);
/* The same launch with ONE plane per weight (round-to-nearest bf16) and A rounded in the kernel: desco_gemm_bf16_f32's
 * arithmetic (the bf16 training mode, BASELINE config 3), several problems per launch. */
int desco_gemm_bf16_multi_f32(int num, const desco_gemm_desc* descs, const int16_t* const* planes,
                              desco_stream_t stream);
/* planes[num][num_planes][..] of num contiguous matrices w[num][rows][cols]: as they are ([rows][cols]) or, transpose != 0,
 * of their transposes ([cols][rows]) -- a training trunk's stacked weights, all layers in one launch.  num_planes = 3: the
 * truncation split of desco_split_bf16x3_f32; 1: round-to-nearest bf16 (desco_round_bf16_f32). */
int desco_split_bf16x3_batch_f32(const float* w, int64_t num, int rows, int cols, int transpose, int num_planes,
                                 int16_t* planes, desco_stream_t stream);

/* Same contract as desco_gemm_f32 on the fp16 matrix pipe with fp32-level accuracy in THREE products ("f16x3",
 * csrc/gemm_f16x3.hip): operands are scaled by powers of two and split into two fp16 terms (hi = rne(s x),
 * lo = rne(s x - hi): 22 significand bits); hi*hi + hi*lo + lo*hi accumulate in fp32 and the scales are undone in
 * the epilogue (exact).  Measured error <= the f32 MFMA's (tools/micro/f16x3_probe.hip).
 *   w_planes[2][n][k1+k2]: (hi, lo) fp16 bit patterns of scale * W, N-MAJOR, and w_scale[2] = {scale, 1/scale} on
 *     the DEVICE, both produced once per weight version by desco_split_f16x2_f32 (one power of two per matrix:
 *     largest |w| -> [2^14, 2^15));
 *   row_scale[m]: a bound of every row's largest |a| over [A1 | A2] (the kernel derives the power of two that puts it
 *     into [2^14, 2^15)): desco_row_absmax_f32 on the same operands, or left by the kernel that wrote A
 *     (desco_degree_affine_f32 / desco_shmp_layer_f16x3_f32 with row_absmax). */
int desco_gemm_f16x3_f32(const float* a1, int64_t lda1, int k1, const float* a2, int64_t lda2, int k2,
                         const int16_t* w_planes, const float* w_scale, int n, const float* bias,
                         int bias_rows, const float* s, int ns, const float* ws, int act, float slope,
                         float* c, int64_t ldc, int64_t m, const float* row_scale, desco_stream_t stream);
int desco_row_absmax_f32(const float* a1, int64_t lda1, int k1, const float* a2, int64_t lda2, int k2,
                        int64_t m, float* row_scale, desco_stream_t stream);
int desco_split_f16x2_f32(const float* w, int64_t count, int16_t* planes, float* scale, desco_stream_t stream);

/* bf16 training mode (BASELINE config 3): the same GEMM contract with ONE bf16 product per
 * multiply-add -- A is rounded to nearest-even bf16 inside the kernel, the N-MAJOR weight arrives
 * rounded by desco_round_bf16_f32 (out[count] bf16 bit patterns); fp32 accumulation and output. */
int desco_gemm_bf16_f32(const float* a1, int64_t lda1, int k1, const float* a2, int64_t lda2, int k2,
                        const int16_t* w_bf16, int n, const float* bias, int bias_rows,
                        const float* s, int ns, const float* ws, int act, float slope, float* c,
                        int64_t ldc, int64_t m, desco_stream_t stream);
int desco_round_bf16_f32(const float* w, int64_t count, int16_t* out, desco_stream_t stream);

/* Fused SHMP layer (K2-K7 in one launch; csrc/shmp_layer.hip, 32-row wave tiles).  For destination rows i in
 * [row0, row0+num_rows), with sm = slots_mfma <= 3, st = slots_table <= 2, S = slots_stored (sm+st <= S <= 4):
 *   out[i] = relu( sum_{s<sm} (sum_{e in vrow(i*S+s)} x[vcol[e]]) * Wt_s + x[i] * Wt_sm + bias
 *                  + sum_{sm<=s<sm+st} sum_{e in vrow(i*S+s)} ytab[vcol[e]-ytab_row0][(s-sm)*64 : +64] )
 * Wt: [(sm+1)*64, 64] row major.  "Table slots" are relations whose sources were already multiplied
 * by their weight block (ytab = x_src * [Wt_sm' | ...], ld ldy): (sum_j x_j) W = sum_j (x_j W).
 * x / out are indexed by the same global row ids as vrowptr; out must not alias x.
 * out2 (optional, may be NULL): a second copy of the produced rows, row i stored at
 * out2[(i - row0)*ldo2 ...] -- the canonical launches fill their column block of the anchor-MLP
 * operand [B, 64*(layers+1)] this way instead of a separate concatenation pass.
 * Replaces SAGEConv.propagate + lin + to_hetero sum + updates + relu
 * (gnn_model.py:262-264, 273, 392-395) without materialising the aggregates. */
int desco_shmp_layer_f32(const float* x, int64_t ldx, const int32_t* vrowptr, const int32_t* vcol,
                         int64_t row0, int64_t num_rows, int slots_stored, int slots_mfma,
                         int slots_table, const float* wt, const float* bias, const float* ytab,
                         int64_t ldy, int64_t ytab_row0, float* out, int64_t ldo, float* out2,
                         int64_t ldo2, desco_stream_t stream);
/* Same layer with the matrix work on the bf16 pipe at fp32 accuracy (the 6-product split of
 * desco_gemm_bf16x6_f32; 16-row wave tiles): wt_planes[3][64 n][(slots_mfma+1)*64 k] = desco_split_bf16x3_f32
 * of the N-MAJOR folded weight (the transpose of desco_shmp_layer_f32's wt).  slots_mfma <= 2. */
int desco_shmp_layer_bf16x6_f32(const float* x, int64_t ldx, const int32_t* vrowptr,
                                const int32_t* vcol, int64_t row0, int64_t num_rows,
                                int slots_stored, int slots_mfma, int slots_table,
                                const int16_t* wt_planes, const float* bias, const float* ytab,
                                int64_t ldy, int64_t ytab_row0, float* out, int64_t ldo, float* out2,
                                int64_t ldo2, desco_stream_t stream);

/* desco_shmp_layer_bf16x6_f32 with the layer's global_add_pool (gnn_model.py:88-89, 107) fused into
 * the epilogue: besides (or instead of: out may be NULL, e.g. for the last layer, whose count rows
 * feed nothing but the pooling) storing the produced rows, every wave sums them per segment and
 * writes ONE partial row per (wave tile, segment) to pool_part[slot][0:64].  A wave tile is
 * TR = desco_shmp_pool_tile_rows() = 16 rows:
 *   pool_bits[t] bit r = 1  <=>  row TR t + r is the LAST row of its segment (segments = contiguous row
 *                                ranges covering [row0, row0+num_rows); row0 % TR == 0),
 *   pool_slot[t]            =    first slot of tile t (tiles use consecutive slots: one per segment
 *                                that has a row in the tile),
 * both [ceil((row0+num_rows)/TR)], indexed by absolute row / TR.  desco_pool_reduce_f32 (tile_rows =
 * the same TR) then adds the partials of every segment in tile order (+ extra[b], like
 * desco_segment_sum_f32) -- together they replace one desco_segment_sum_f32 pass over the rows (a
 * full read of x) by ~(1/TR + 1/segment length) of its traffic, deterministically (no float atomics). */
int desco_shmp_pool_tile_rows(void);
int desco_shmp_layer_pool_bf16x6_f32(const float* x, int64_t ldx, const int32_t* vrowptr,
                                     const int32_t* vcol, int64_t row0, int64_t num_rows,
                                     int slots_stored, int slots_mfma, int slots_table,
                                     const int16_t* wt_planes, const float* bias, const float* ytab,
                                     int64_t ldy, int64_t ytab_row0, float* out, int64_t ldo,
                                     const uint32_t* pool_bits, const int32_t* pool_slot,
                                     float* pool_part, desco_stream_t stream);
/* The same fused layer (and its pooling variant) in the THREE-product fp16 form (csrc/shmp_layer16.hip, 16-row wave
 * tiles): wt_planes[2][64 n][(slots_mfma+1)*64 k] fp16 (hi, lo) and w_scale[2] = {scale, 1/scale} on the device, both
 * from desco_split_f16x2_f32 of the transposed folded weight; slots_mfma <= 2.  The activation side is scaled inside
 * the kernel: one power of two per (row, K block) -- the largest |value| of the row's 64 gathered sums -> [2^14,
 * 2^15) --, the accumulators follow by exact multiplications and leave the scales in the epilogue. */
int desco_shmp_layer_f16x3_f32(const float* x, int64_t ldx, const int32_t* vrowptr, const int32_t* vcol,
                               int64_t row0, int64_t num_rows, int slots_stored, int slots_mfma,
                               int slots_table, const int16_t* wt_planes, const float* w_scale,
                               const float* bias, const float* ytab, int64_t ldy, int64_t ytab_row0,
                               float* out, int64_t ldo, float* out2, int64_t ldo2, float* row_absmax,
                               const float* xself, int64_t ldxs, desco_stream_t stream);
/* xself (optional): the launch's OWN rows -- the self block's operand -- are read at xself + i * ldxs (i = the global row
 * index that addresses x) instead of from x; out may then be NULL when out2 is given (the rows are stored once, in out2's
 * tensor).  The canonical launches use both: their rows live only in the anchor operand's column blocks.
 * row_absmax (optional, [num_rows]): row_absmax[i - row0] = max(row_absmax[i - row0], max_c |out[i, c]|) is ACCUMULATED
 * over the launches that fill the column blocks of one operand (out2): its per-row bound for desco_gemm_f16x3_f32. */
int desco_shmp_layer_pool_f16x3_f32(const float* x, int64_t ldx, const int32_t* vrowptr, const int32_t* vcol,
                                    int64_t row0, int64_t num_rows, int slots_stored, int slots_mfma,
                                    int slots_table, const int16_t* wt_planes, const float* w_scale,
                                    const float* bias, const float* ytab, int64_t ldy, int64_t ytab_row0,
                                    float* out, int64_t ldo, const uint32_t* pool_bits,
                                    const int32_t* pool_slot, float* pool_part, desco_stream_t stream);

/* desco_shmp_layer_pool_f16x3_f32 for a layer input that exists as a TABLE of its distinct rows only.  The closed-form first
 * layer's output is a function of a row's S slot degrees, so X_1 has a few thousand distinct rows: x = that table (L2-resident),
 * vcol = the column ids with the sources of the MFMA slots replaced by their table rows, and the launch's OWN rows (the self
 * block's operand) are RECOMPUTED from their slot degrees with the first layer's coefficients self_coef [slots_stored + 1][64]:
 *   own row i = relu(self_coef[S] + sum_s degree_s(i) * self_coef[s])          (desco_degree_affine_f32's arithmetic)
 * -- X_1 [N, 64] is never written or read (host side: NeighborhoodBatch.degree_table_index, gnn_model.FIRST_LAYER_TABLE).
 * Results are bit-identical to the launch on the materialised tensor. */
int desco_shmp_layer_pool_table_f16x3_f32(const float* x, int64_t ldx, const int32_t* vrowptr, const int32_t* vcol,
                                          int64_t row0, int64_t num_rows, int slots_stored, int slots_mfma,
                                          int slots_table, const int16_t* wt_planes, const float* w_scale,
                                          const float* bias, const float* ytab, int64_t ldy, int64_t ytab_row0,
                                          float* out, int64_t ldo, const uint32_t* pool_bits,
                                          const int32_t* pool_slot, float* pool_part, const float* self_coef,
                                          desco_stream_t stream);

/* The f16x3 layer for a block ONE OF WHOSE TWO TABLE SLOTS has no entry at all.  Molecule graphs have no triangles: the
 * canonical->count triangle relation -- CSR slot 2 (slot = 2 (source is canonical) + tride), table slot 0 -- is empty in the
 * whole block.  One entry point for the three forms above: plain (pool_part NULL; out2, row_absmax, xself as in
 * desco_shmp_layer_f16x3_f32), pooled (pool_bits / pool_slot / pool_part) and pooled with the own rows recomputed (self_coef).
 * table_slots_empty: bit t set = the caller ASSERTS that table slot t (CSR slot slots_mfma + t) is empty; slots_table must be
 * 2.  The kernel then neither tests for nor reads that slot's 64-column block of ytab, and ytab may be the NARROW table of the
 * OTHER slot alone, [n, 64] with ldy = 64, its block at column 0 (the same kernel family: shmp_layer16_kernel<.., ST = 2, ..> with a
 * compile-time 64 in instantiations of their own, NARROW; the wide table's kernels are compiled as before) -- the table product
 * then writes half the bytes.  The narrow table needs ldx = 64, ldy = 64 and, with out, ldo = 64 (other strides: DESCO_EINVAL,
 * shape not built).  Entries of a slot asserted empty, should the assertion be false, are ignored, never read out of bounds.
 * With a wide table (ldy >= 128) the mask is not needed and not used: the launch is the respective entry point's above.
 * ldy < 64 * slots_table without a slot asserted empty is refused with DESCO_EINVAL (as it is by those).  Results are
 * bit-identical to the launch on the [n, 128] table. */
int desco_shmp_layer_narrow_f16x3_f32(const float* x, int64_t ldx, const int32_t* vrowptr, const int32_t* vcol,
                                      int64_t row0, int64_t num_rows, int slots_stored, int slots_mfma,
                                      int slots_table, const int16_t* wt_planes, const float* w_scale,
                                      const float* bias, const float* ytab, int64_t ldy, int64_t ytab_row0,
                                      float* out, int64_t ldo, float* out2, int64_t ldo2, float* row_absmax,
                                      const float* xself, int64_t ldxs, const uint32_t* pool_bits,
                                      const int32_t* pool_slot, float* pool_part, const float* self_coef,
                                      int table_slots_empty, desco_stream_t stream);

/* The pooled narrow launch above for a layer input that exists as a TABLE of its distinct rows only, the launch's own rows
 * included: x = the table [U, 64], vcol = the column ids with the sources of the MFMA slots replaced by their table rows (the
 * table slots' sources stay rows of ytab), and the launch's OWN row i (the self block's operand; i = the global row index that
 * addresses vrowptr) is read at x + self_idx[i] * ldx.  The second layer's output on molecule batches is such a table
 * (NeighborhoodBatch.layer2_table_index, gnn_model.SECOND_LAYER_GATHER): X_2's count rows are then never written or read.
 * A kernel instantiation of its own (SELFIDX; the 16 ids of a tile travel with its row pointers); the arithmetic is the
 * narrow launch's: results are bit-identical to that launch on the materialised rows x[self_idx[.]] with the original ids.
 * Arguments: those of desco_shmp_layer_narrow_f16x3_f32 plus self_idx [row0 + num_rows] (device; every entry in [0, U): the
 * caller checks, desco_index_range_check_i32).  DESCO_EINVAL, nothing launched: self_idx NULL; xself or self_coef given (one
 * source of the own rows); a pooling pointer NULL (built pooled only; out may be NULL); ldx, ldy or (with out) ldo other than
 * 64; slots_table != 2 or not exactly one table slot asserted empty. */
int desco_shmp_layer_selfidx_f16x3_f32(const float* x, int64_t ldx, const int32_t* vrowptr, const int32_t* vcol,
                                       int64_t row0, int64_t num_rows, int slots_stored, int slots_mfma,
                                       int slots_table, const int16_t* wt_planes, const float* w_scale,
                                       const float* bias, const float* ytab, int64_t ldy, int64_t ytab_row0,
                                       float* out, int64_t ldo, float* out2, int64_t ldo2, float* row_absmax,
                                       const float* xself, int64_t ldxs, const uint32_t* pool_bits,
                                       const int32_t* pool_slot, float* pool_part, const float* self_coef,
                                       int table_slots_empty, const int32_t* self_idx, desco_stream_t stream);

int desco_pool_reduce_f32(const float* pool_part, const uint32_t* pool_bits, const int32_t* pool_slot,
                          const int32_t* seg_ptr, int64_t num_seg, const float* extra,
                          int64_t ld_extra, float* out, int64_t ldo, int tile_rows,
                          desco_stream_t stream);
/* The same reduce for 1..8 layers' partial arrays in one launch (they share the tile index and the segments): HOST arrays
 * of DEVICE pointers pool_parts[num], extras[num] (or NULL; entries may be NULL), outs[num]; common ld_extra / ldo.
 * Bit-identical to num calls of desco_pool_reduce_f32. */
int desco_pool_reduce_multi_f32(int num, const float* const* pool_parts, const uint32_t* pool_bits,
                                const int32_t* pool_slot, const int32_t* seg_ptr, int64_t num_seg,
                                const float* const* extras, int64_t ld_extra, float* const* outs, int64_t ldo,
                                int tile_rows, desco_stream_t stream);

/* post_mp.0 (gnn_model.py:44-53, first Linear) on the pooled embeddings WITHOUT materialising them: row b of the operand is
 *   [ anch[b, 0:64] + rows(b) * x0 | anch[b, 64 l : 64 (l + 1)] + sum of segment b's partial rows of layer l, l = 1..L ]
 * (what desco_pool_reduce_f32 would have written, same summation order), formed in the product's load phase:
 *   c[b, 0:64] = act( operand[b, :] * W^T + bias ),  W as desco_split_bf16x3_f32 planes [3][64][64 (L + 1)].
 * anch: [m, >= 64 (L + 1)]; parts: HOST array of the L layers' DEVICE partial arrays; seg_ptr / pool_bits / pool_slot: the
 * fused pooling's index for 16-row tiles.  EVERY SEGMENT MUST LIE IN AT MOST THREE TILES (<= 33 rows; the caller checks:
 * further tiles are ignored); a segment without rows adds no partial rows.  Saves the write and the read of the pooled
 * [m, 64 (L + 1)] tensor. */
int desco_pool_post_bf16x6_f32(const float* anch, int64_t lda, int num_layers, const int16_t* w_planes, int n,
                               const float* bias, int act, float slope, float* c, int64_t ldc, int64_t m,
                               const int32_t* seg_ptr, const uint32_t* pool_bits, const int32_t* pool_slot,
                               const float* const* parts, const float* x0, int tile_rows, desco_stream_t stream);

/* desco_pool_post_bf16x6_f32 with the anchor rows as a TABLE of their distinct values: row b of the operand reads
 * anch[anch_row[b], :] where the call above reads anch[b, :] (anch_row: [m] int32 DEVICE ids into anch's rows, or NULL =
 * the call above).  Everything else -- the partial-sum lookup, the order of the sums, the split, the products -- is that
 * call's, so out equals its out on the gathered rows bit for bit.  The ids are NOT checked here: the caller range-checks
 * them once where it builds them (desco_index_range_check_i32). */
int desco_pool_post_rows_bf16x6_f32(const float* anch, int64_t lda, const int32_t* anch_row, int num_layers,
                                    const int16_t* w_planes, int n, const float* bias, int act, float slope, float* c,
                                    int64_t ldc, int64_t m, const int32_t* seg_ptr, const uint32_t* pool_bits,
                                    const int32_t* pool_slot, const float* const* parts, const float* x0, int tile_rows,
                                    desco_stream_t stream);

/* The anchor MLP and desco_pool_post_bf16x6_f32 in ONE launch: anch = act(a[:, 0:k] * Wa^T + anchor_bias) on the f16x3
 * pipe (desco_gemm_f16x3_f32's arithmetic, bit for bit: anchor_planes / anchor_scale from desco_split_f16x2_f32 of the
 * [64 (L + 1), k] weight, row_scale = a bound of each row's largest |a|), then out[b, 0:64] = post_act( operand[b, :] *
 * W0^T + post_bias ) with the operand of desco_pool_post_bf16x6_f32 formed from anch (post_planes: desco_split_bf16x3_f32
 * planes [3][64][64 (L + 1)]).  anch is never written; out is bit-identical to desco_gemm_f16x3_f32 followed by
 * desco_pool_post_bf16x6_f32.  num_layers L in {2, 5, 8} (the anchor's 64 (L + 1) columns are whole 192-column tiles);
 * k = 64 L (the constant first block folded into anchor_bias) or 64 (L + 1); tile_rows 16; m < 2^24.  A segment must lie
 * in at most three 16-row tiles (<= 33 rows: further tiles are ignored); a segment without rows adds no partial rows. */
int desco_anchor_pool_post_f16x3_f32(const float* a, int64_t lda, int k, const int16_t* anchor_planes,
                                     const float* anchor_scale, const float* anchor_bias, int act, float slope,
                                     const float* row_scale, int num_layers, const int16_t* post_planes,
                                     const float* post_bias, int post_act, float post_slope, float* out, int64_t ldo,
                                     int64_t m, const int32_t* seg_ptr, const uint32_t* pool_bits,
                                     const int32_t* pool_slot, const float* const* parts, const float* x0,
                                     int tile_rows, desco_stream_t stream);

/* post_mp.3 -> ReLU -> post_mp.5 -> ReLU -> post_mp.7 (gnn_model.py:44-53: Linear(64, 64), Linear(64, 256), Linear(256, 64))
 * in one launch:  out[i, 0:64] = W3 relu(W2 relu(W1 x[i, 0:64] + b1) + b2) + b3.  A row is read once and written once;
 * the [m, 64] and [m, 256] intermediates stay in registers (f16x3 arithmetic, fp32-accurate: the products are formed
 * transposed so that a layer's accumulators ARE the next layer's operand registers; per-row power-of-two scales).
 * wK_planes / wK_scale = desco_split_f16x2_f32 of the [out, in] weights ([2][64][64], [2][256][64], [2][64][256]);
 * biases [64], [256], [64] or NULL.  x == out is allowed (a wave reads its 32 rows before it writes them). */
int desco_post_mp_tail_f16x3_f32(const float* x, int64_t ldx, int64_t m, const int16_t* w1_planes,
                                 const float* w1_scale, const float* b1, const int16_t* w2_planes,
                                 const float* w2_scale, const float* b2, const int16_t* w3_planes,
                                 const float* w3_scale, const float* b3, float* out, int64_t ldo,
                                 desco_stream_t stream);

/* Row-wise Linear with 64 inputs on the fused layer's streaming machinery (bf16x6 arithmetic,
 * fp32-accurate): out[i, 0:64*num_blocks] = act(x[i, 0:64] * W^T + bias[0:64*num_blocks]);
 * w_planes[num_blocks][3][64 n][64 k] = desco_split_bf16x3_f32 of every 64-row block of the
 * [out, in] weight.  Memory-shaped projections (canonical table, post_mp.5, count_model target
 * half): x is read once per two output blocks, rows stream at HBM rate.  x == out is not allowed. */
int desco_linear64_bf16x6_f32(const float* x, int64_t ldx, const int16_t* w_planes, int num_blocks,
                              const float* bias, int act, float slope, float* out, int64_t ldo,
                              int64_t num_rows, desco_stream_t stream);

/* First SHMP layer (and first pooling block) when every node of a type has the same input row --
 * the default pipeline's all-zero node features (workload.py:431-440, transforms.py:380-384) make
 * pre_mp's output its bias.  Then agg_s[i] = deg_s(i) * x0_src(s) and, for rows [row0, row0+num_rows):
 *   out[i, 0:64] = act( coef[slots] + sum_{s<slots} (vrowptr[i*slots+s+1] - vrowptr[i*slots+s]) * coef[s] )
 *                  + extra[i - row0]                       (coef: [slots+1, 64]; extra optional)
 * mathematically identical to desco_shmp_layer_f32 on the constant input; no gather, no GEMM. */
int desco_degree_affine_f32(const int32_t* vrowptr, int64_t row0, int64_t num_rows, int slots,
                            const float* coef, int act, float slope, const float* extra,
                            int64_t ld_extra, float* out, int64_t ldo, float* row_absmax,
                            desco_stream_t stream);
/* The same rows for a launch that starts at row 0 (the count rows), with their global_add_pool (gnn_model.py:88-89, 107)
 * fused in as in desco_shmp_layer_pool_*: besides storing the rows (out may be NULL) every 16-row tile leaves one partial
 * row per segment that has a row in it at pool_part[pool_slot[t] + k] (pool_bits / pool_slot: the index of
 * desco_shmp_layer_pool_bf16x6_f32 for 16-row tiles); desco_pool_reduce(_multi)_f32 finishes the sums.  Saves the one
 * read of the produced rows that the segment sum of this layer cost. */
int desco_degree_affine_pool_f32(const int32_t* vrowptr, int64_t num_rows, int slots, const float* coef, int act,
                                 float slope, float* out, int64_t ldo, const uint32_t* pool_bits,
                                 const int32_t* pool_slot, float* pool_part, desco_stream_t stream);
/* row_absmax (optional, [num_rows]): row_absmax[i - row0] = max_c |out[i, c]| is WRITTEN -- the start of the per-row
 * bound desco_gemm_f16x3_f32 takes when these rows are the first column block of its operand. */

/* The count rows of a layer that was computed on its DISTINCT rows only (host side: NeighborhoodBatch.layer2_table_index,
 * gnn_model.SECOND_LAYER_TABLE): rows [0, num_rows) are out[i, 0:64] = table[cls[i], 0:64] (table [num_table, >= 64], row
 * stride ldt; cls [num_rows] in [0, num_table)), with their global_add_pool fused in exactly as in
 * desco_degree_affine_pool_f32: the same 16-row tiles, pool_bits / pool_slot index and partial rows -- bit for bit what the
 * layer kernel's pooled launch leaves for the same rows.  out may be NULL (partials only).  A class outside the table reads
 * the nearest table row (never out of bounds); desco_index_range_check_i32 is the check, made once per index. */
int desco_table_rows_pool_f32(const float* table, int64_t ldt, int64_t num_table, const int32_t* cls, int64_t num_rows,
                              float* out, int64_t ldo, const uint32_t* pool_bits, const int32_t* pool_slot,
                              float* pool_part, desco_stream_t stream);
/* The partial rows of TWO table layers over the same rows in one walk (gnn_model.POOL_TABLES: X_1 = table1[ids1] and X_2 =
 * table2[ids2] on a molecule batch): pool_part1 and pool_part2 receive, bit for bit, what desco_degree_affine_pool_f32 /
 * desco_table_rows_pool_f32 leave for the same rows and the same pool_bits / pool_slot index; out2 (optional) the second
 * layer's rows as desco_table_rows_pool_f32 writes them.  One 1024-thread block per CU; a table is staged in LDS when it
 * fits in desco_table_rows_pool2_lds_bytes() -- both tables together, else the larger one that fits alone, else the smaller
 * -- and is read from global memory otherwise.  Ids outside their table read the nearest table row (never out of bounds). */
int desco_table_rows_pool2_f32(const float* table1, int64_t ldt1, int64_t num_table1, const int32_t* ids1,
                               float* pool_part1, const float* table2, int64_t ldt2, int64_t num_table2,
                               const int32_t* ids2, float* pool_part2, int64_t num_rows, float* out2, int64_t ldo2,
                               const uint32_t* pool_bits, const int32_t* pool_slot, desco_stream_t stream);
int desco_table_rows_pool2_lds_bytes(void);
/* ... and of THREE table layers (gnn_model.THIRD_LAYER_TABLE: X_3 = table3[cls3] as well): tables, ldts, num_tables, ids and
 * pool_parts are HOST arrays of three entries, one per layer, read before the call returns; pool_parts[k] receives, bit for
 * bit, what desco_table_rows_pool_f32 leaves for table k, its ids and the same pool_bits / pool_slot index.  No rows are
 * written.  It is desco_table_rows_pooln_f32 below with num_layers = 3 -- the same launch, all three layers' rows in flight --
 * under its own name, which is the one its error messages carry. */
int desco_table_rows_pool3_f32(const float* const* tables, const int64_t* ldts, const int64_t* num_tables,
                               const int32_t* const* ids, float* const* pool_parts, int64_t num_rows,
                               const uint32_t* pool_bits, const int32_t* pool_slot, desco_stream_t stream);
/* ... and of num_layers = 1 .. desco_table_rows_pooln_max_layers() (8) table layers (gnn_model.DEEP_LAYER_TABLES: the layers
 * beyond the third as tables of their distinct rows): the arrays are HOST arrays of num_layers entries, read before the call
 * returns; pool_parts[k] receives, bit for bit, what desco_table_rows_pool_f32 leaves for table k, its ids and the same
 * pool_bits / pool_slot index.  No rows are written.  The same walk (one 1024-thread block per CU, four tiles per wait): four
 * layers' ids per id load, a second load per tile beyond four layers, the rows of one to three layers in flight at a time (all
 * of them up to three layers, two up to six, one beyond); the tables
 * are staged in LDS smallest first while they fit together in desco_table_rows_pool2_lds_bytes(), the others are read from
 * global memory.  Ids outside their table read the nearest table row (never out of bounds). */
int desco_table_rows_pooln_f32(int num_layers, const float* const* tables, const int64_t* ldts, const int64_t* num_tables,
                               const int32_t* const* ids, float* const* pool_parts, int64_t num_rows,
                               const uint32_t* pool_bits, const int32_t* pool_slot, desco_stream_t stream);
int desco_table_rows_pooln_max_layers(void);
/* The pooled sums of num_layers = 1 .. 8 table layers on one REPRESENTATIVE neighborhood per pooling class (host side:
 * NeighborhoodBatch.pool_class_index, gnn_model.POOL_CLASS_TABLE) instead of the walk over every count row.  The layer arrays
 * are HOST arrays as above.  Representative u = neighborhood rep[u] of count_ptr [num_neigh + 1]; its count rows are rows
 * s .. s + n - 1 of the block's num_rows (s = count_ptr[rep[u]], 1 <= n <= desco_class_rows_pool_max_rows() = 33), read as
 * tables[k][ids[k][i]] with the ids at their original positions.  Per layer the rows are summed exactly as the walk and
 * desco_pool_post_bf16x6_f32 sum them for that neighborhood: running sums from 0.f in row order, cut after every row i with
 * (i & 15) == 15, the pieces combined as ((p0 + p1) + p2) with absent pieces 0.f.  rep_ptr [num_rep + 1] is the compact row
 * pointer of the representatives (rep_ptr[u + 1] - rep_ptr[u] = n) and pool_bits / pool_slot ITS pooling index
 * (desco_pool_index_dev on rep_ptr, num_slots slots): pool_parts[k] [num_slots, 64] receives the combined sum in the first
 * slot of segment u and zeros in its continuation slots, so that desco_pool_post_rows_bf16x6_f32 on (rep_ptr, that index,
 * pool_parts) forms for row u, bit for bit, the operand row it forms for neighborhood rep[u] from the walk's partial rows.
 * A representative that breaks the contract writes nothing; ids outside their table read the nearest table row. */
int desco_class_rows_pool_f32(int num_layers, const float* const* tables, const int64_t* ldts, const int64_t* num_tables,
                              const int32_t* const* ids, float* const* pool_parts, const int32_t* count_ptr,
                              int64_t num_neigh, int64_t num_rows, const int64_t* rep, const int32_t* rep_ptr,
                              int64_t num_rep, const uint32_t* pool_bits, const int32_t* pool_slot, int64_t num_slots,
                              desco_stream_t stream);
int desco_class_rows_pool_max_rows(void);
/* dst[b, 0:ncols] = src[rows[b], 0:ncols] for b < num_dst (rows in [0, num_src); one outside reads the nearest row): the
 * counts of the pooling classes handed out to their neighborhoods. */
int desco_gather_rows_f32(const float* src, int64_t lds, int64_t num_src, const int32_t* rows, int64_t num_dst, int ncols,
                          float* dst, int64_t ldd, desco_stream_t stream);
/* DESCO_EINVAL when one of idx[0 .. n) (device) lies outside [0, bound); scratch: one device word.  Synchronises the
 * stream: for indices built once per batch, not for the pass. */
int desco_index_range_check_i32(const int32_t* idx, int64_t n, int64_t bound, int32_t* scratch, desco_stream_t stream);

/* Indices of the backward pass, built on the device (replaces the per-batch host transposes):
 *  desco_vcsr_transpose_sym: the transposed index of a SYMMETRIC virtual-row CSR (every edge
 *    dst<-src has its mirror src<-dst; true for canonical-partition blocks, query graphs and the
 *    gossip CSR): t_rowptr[num_rows+1] (= vrowptr[slots*j]) and t_col[E] = the virtual rows
 *    (k*slots + mirror slot) that read row j, ascending.  num_count: rows >= num_count are
 *    canonical rows (only used for slots == 4; pass num_rows otherwise).
 *  desco_segment_ids: seg_id[r] = b for seg_ptr[b] <= r < seg_ptr[b+1]. */
int desco_vcsr_transpose_sym(const int32_t* vrowptr, const int32_t* vcol, int64_t num_rows, int slots,
                             int64_t num_count, int32_t* t_rowptr, int32_t* t_col,
                             desco_stream_t stream);
int desco_segment_ids(const int32_t* seg_ptr, int64_t num_seg, int32_t* seg_id, desco_stream_t stream);

/* K9  global_add_pool (gnn_model.py:107) over contiguous row segments, plus one optional extra row
 * per segment (the anchored canonical embedding, gnn_model.py:69-73, 88-89):
 * out[b, 0:ncols] = sum_{r in [seg_ptr[b], seg_ptr[b+1])} x[r, 0:ncols] + extra[b, 0:ncols]
 * Also used for the node->graph aggregation of counts (workload.py:136-148, 303-324). */
int desco_segment_sum_f32(const float* x, int64_t ldx, int ncols, const int32_t* seg_ptr,
                          int64_t num_seg, const float* extra, int64_t ld_extra, float* out,
                          int64_t ldo, desco_stream_t stream);

/* The same for num_layers feature blocks in one launch (training trunk: X_1 .. X_L live in one buffer):
 * out[b, 64 l .. 64 l + 63] = sum_{r in segment b} x[l * layer_stride + r * ldx + 0..63] + extra[b, 64 l ..] */
int desco_segment_sum_layers_f32(const float* x, int64_t ldx, int64_t layer_stride, int num_layers,
                                 const int32_t* seg_ptr, int64_t num_seg, const float* extra,
                                 int64_t ld_extra, float* out, int64_t ldo, desco_stream_t stream);

/* K12/K13  count head (lightning_model.py:176-193, 210-221) in separable form:
 * logit[b,q] = sum_c w2[c] * leaky(T[b,c] + Qh[q,c]) + b2;  out = exp2 ? 2^logit - 1 : logit
 * T: [B, hid] (target half of count_model.0), Qh: [Q, hid] (query half + bias);
 * hid % 64 == 0, hid <= 256, Q <= 32 */
int desco_count_head_f32(const float* t, int64_t ldt, const float* qh, int64_t ldq, int hid,
                         const float* w2, float b2, const float* b2_dev, float slope,
                         int exp2_minus_1, float* out, int64_t ldo, int64_t num_b, int num_q,
                         desco_stream_t stream);   /* b2_dev != NULL: the bias is read from the device */

/* K14  GossipDataset.apply_neighborhood_count (workload.py:107-112): dst[rows[b], :] = src[b, :] */
int desco_scatter_rows_f32(const float* src, int64_t lds, const int32_t* rows, int64_t num_src,
                           int ncols, float* dst, int64_t ldd, desco_stream_t stream);

/* K15-K20, layer 0 of the gossip GNN for ALL queries at once, in closed form:
 * per node i and query q:
 *   lo/hi = neighbours j<i / j>i (== edge_weight of gnn_model.py:248),
 *   a0 = g0[q]*deg_lo + (1-g0[q])*deg_hi,  b0 = g0[q]*sum_lo x[j,q] + (1-g0[q])*sum_hi x[j,q]
 *   h1[i,q,:] = relu(a0*p[q,:] + b0*r[:] + x[i,q]*t[:] + z[q,:])
 *   scal[i,q,0] = g1[q]*deg_lo + (1-g1[q])*deg_hi,  scal[i,q,1] = x[i,q]
 * rowptr/col: symmetric CSR of the batch, col ascending per row. */
int desco_gossip_layer0_f32(const float* x, int64_t ldx, const int32_t* rowptr, const int32_t* col,
                            int64_t num_nodes, int num_q, const float* g0, const float* g1,
                            const float* p, const float* r, const float* t, const float* z,
                            float* h1, float* scal, desco_stream_t stream);

/* K18/K19 for layers >= 1, aggregate-then-transform form:
 * out[i,q,:] = sum_{j~i} (j<i ? g[q] : 1-g[q]) * h[j,q,:]      (h, out: [num_nodes, num_q, 64])
 * g == NULL selects the signed form sum_{j<i} h[j] - sum_{j>i} h[j] (= d out / d g, training). */
int desco_gossip_gather_f32(const float* h, const int32_t* rowptr, const int32_t* col,
                            int64_t num_nodes, int num_q, const float* g, float* out,
                            desco_stream_t stream);

/* Fused gossip stage (csrc/gossip_fused.hip), two launches for all queries:
 *  (1) desco_gossip_scalars_f32: scal4[i*Q+q] = (a0, b0, a1, x[i,q]) with
 *      a_l = g_l[q]*deg_lo(i) + (1-g_l[q])*deg_hi(i),  b0 = g0[q]*sum_{j<i} x[j,q] + (1-g0[q])*sum_{j>i} x[j,q]
 *  (2) desco_gossip_fused_f32: per tile of 128 nodes and one query, entirely on chip,
 *      h1 = relu(a0*p_q + b0*r + x*t + z_q);  hh = sum_j (j<i ? g1 : 1-g1)*h1_j;
 *      h2 = relu([hh|h1] w1 + a1*u + d1);  y1 = leaky_0.1([h1|h2] wp + x*tp + zp_q);
 *      y2 = relu(y1 w3 + b3);  out[i,q] = x + b7 + sum_c relu(y2 w5 + b5)[c]*w7[c]
 *      The four weight matrices are passed N-MAJOR (torch's [out, in] layout of the folded
 *      matrices: w1, wp [64,128]; w3 [64,64]; w5 [256,64]) and pre-split into bf16 planes by
 *      desco_split_bf16x3_f32: w*_planes[3][out][in].  All GEMMs run as the fp32-accurate
 *      6-product bf16 split of desco_gemm_bf16x6_f32.  p, z, r, t must be 8-byte aligned.
 * Replaces BaseGNN.forward (gossip) for every query: gnn_model.py:58-103, 230-260, 303-350 and the
 * loop of lightning_model.py:613-628; equals layer0 + gather + 4 GEMMs + rowdot of the unfused path.
 * desco_gossip_fused_f32 (the six-product bf16 form; since round 4 the cross-check of desco_gossip_fused_f16x3_f32)
 * draws its work items from a process-wide ring of 64 ticket slots taken in launch order: launches must be issued
 * from ONE stream at a time and captured launches must not be replayed concurrently with other launches of it (the
 * fp16 entry point takes a caller-owned queue instead). */
int desco_gossip_scalars_f32(const float* x, int64_t ldx, const int32_t* rowptr, const int32_t* col,
                             int64_t num_nodes, int num_q, const float* g0, const float* g1,
                             float* scal4, desco_stream_t stream);
int desco_gossip_fused_f32(const float* scal4, const int32_t* rowptr, const int32_t* col,
                           int64_t num_nodes, int num_q, const float* g1, const float* p,
                           const float* z, const float* zp, const float* r, const float* t,
                           const float* u, const float* tp, const float* d1,
                           const int16_t* w1_planes, const int16_t* wp_planes,
                           const int16_t* w3_planes, const float* b3, const int16_t* w5_planes,
                           const float* b5, const float* w7, float b7, float* out,
                           const uint8_t* tile_perm, desco_stream_t stream);
/* The same fused gossip pass in the THREE-product fp16 form (csrc/gossip_f16.hip; the product path since round 4):
 * per-node power-of-two scales carry the range; a wave owns 16 nodes x all features, all nine weight blocks stay
 * resident in LDS and a wave carries its nodes through the whole network for 5 queries per work unit with no barrier
 * in the loop.  tile_perm (optional, desco_gossip_tile_order's output): the 16 nodes of a wave are the degree-sorted
 * ranks 16 i .. 16 i + 15 of their 128-node tile (speed only; p, z, r, t must be 16-byte aligned).
 *   wstream [9][2][4096] fp16 + winv[4]: desco_gossip_f16_stream of the four desco_split_f16x2_f32 plane sets
 *     (w1, wp [2][64][128]; w3 [2][64][64]; w5 [2][256][64]) and the 1/scale of each matrix, in that order;
 *   queue: two zeroed 64-bit words owned by the caller (work-item tickets of this launch; the kernel leaves them
 *     zero).  Launches that may run CONCURRENTLY (other streams, graph replays) need queues of their own; launches
 *     on one stream can share one.
 * Work per (node, query) row: 73 728 MFMA flop (x3 products); bytes the algorithm has to move per row: its 16-byte
 * record + 4-byte result + 16 bytes per NEIGHBOUR record (deg x 16: 12 of them used) + the column ids once per node --
 * rows * 20 + 4 * (edges * (1 + 4 Q) + nodes), which is what bench.py prices `achieved` bytes with (round 4's
 * "16-B record + 4-B result" left the neighbour records out; they are 2/3 of the bytes on COX2 shapes).
 * Round 5: packed fp32 selection on, weight fragments through a register ring two pair steps ahead
 * (csrc/gossip_f16.hip); the library is only linked if no packed fp32 instruction in it has OP_SEL on src1 / src2
 * (tools/check_isa.py, profiles/r5_a_gossip_f16_hazard.md). */
int desco_gossip_f16_stream(const int16_t* w1_planes, const int16_t* wp_planes, const int16_t* w3_planes,
                            const int16_t* w5_planes, int16_t* wstream, desco_stream_t stream);
int desco_gossip_fused_f16x3_f32(const float* scal4, const int32_t* rowptr, const int32_t* col,
                                 int64_t num_nodes, int num_q, const float* g1, const float* p,
                                 const float* z, const float* zp, const float* r, const float* t,
                                 const float* u, const float* tp, const float* d1, const int16_t* wstream,
                                 const float* winv, const float* b3, const float* b5, const float* w7, float b7,
                                 float* out, const uint8_t* tile_perm, uint64_t* queue, desco_stream_t stream);
/* tile_perm (optional, 4-byte aligned, [ceil(num_nodes/128)*128] bytes from desco_gossip_tile_order): the order in
 * which the 8 waves of a block walk the rows of a 128-node tile in the neighbour-sum phase -- rows sorted by degree,
 * paired, pairs dealt to the waves in snake order (a half wave per row, the two halves of a wave in lock step, a block
 * barrier at the end: with rows in node order the phase takes 1.3-1.8x its balanced time).  NULL = node order.
 * The result does not depend on it bit for bit (every row's sum keeps its own CSR order). */
int desco_gossip_tile_order(const int32_t* rowptr, int64_t num_nodes, uint8_t* tile_perm, desco_stream_t stream);
/* The PLANNED form of desco_gossip_fused_f16x3_f32: the same network, bit for bit, with everything a work unit needs to
 * know of its 16 nodes read from a per-batch plan instead of computed from rowptr / col / tile_perm, the per-query loads
 * issued as buffer loads (scalar base that moves with the query + a 32-bit lane offset), and the operands packed.
 *   desco_gossip_plan: a function of the CSR (and the tile order) alone, once per batch.  plan holds
 *     desco_gossip_plan_words(num_nodes, tile_perm != NULL) int32 words, 16-byte aligned: per group of 16 node slots
 *     (group order = the kernel's: rows 16 g .. 16 g + 15, or with a tile order the degree-sorted ranks of the 128-node
 *     tile) 16 records of 8 words -- row, degree, bit i = neighbour i < 15 has the smaller id (bit 31: empty slot), the
 *     rows of the first four neighbours (the node's own row from the degree on), the node's first edge -- so a wave reads
 *     its group's 512 bytes in one coalesced load; then one word per group, its largest degree.  An empty slot takes
 *     the last row with degree 0.  desco_gossip_plan_host is the host twin (host pointers, same words).  col may be
 *     NULL where the batch has no edge (it is read for rows of degree > 0 only), here and in the planned entry.
 *   desco_gossip_planned_f16x3_f32: pzz [num_q][192] = p_q | z_q | zp_q; cst [900] = u, d1, tp, b3 (64 each), b5, w7
 *     (256 each), r, t (64 each) -- the kernel's LDS image -- then winv[4]; both 16-byte aligned.  tiled = the plan was
 *     built with a tile order.  Needs num_nodes * num_q * 16 < 2^32 (a record's byte offset travels in 32 bits);
 *     DESCO_EINVAL above it: callers use desco_gossip_fused_f16x3_f32 there.  queue as for that entry. */
int64_t desco_gossip_plan_words(int64_t num_nodes, int tiled);
int desco_gossip_plan(const int32_t* rowptr, const int32_t* col, int64_t num_nodes, const uint8_t* tile_perm,
                      int32_t* plan, desco_stream_t stream);
int desco_gossip_plan_host(const int32_t* rowptr, const int32_t* col, int64_t num_nodes, const uint8_t* tile_perm,
                           int32_t* plan);
int desco_gossip_planned_f16x3_f32(const float* scal4, const int32_t* col, int64_t num_nodes, int num_q,
                                   const float* g1, const float* pzz, const float* cst, const int16_t* wstream,
                                   float b7, float* out, const int32_t* plan, int tiled, uint64_t* queue,
                                   desco_stream_t stream);

/* One GossipConv layer l >= 1 of a gossip model of any depth (--gossip_layer_num != 2), over all
 * R = num_nodes * num_q rows (node i, query q) = row i * num_q + q, all matrices rows of 64 floats:
 *   hh[r]   = sum_{j in N(i), CSR order} (j < i ? g[q] : 1 - g[q]) h[j * num_q + q]      (message + aggregate)
 *   out[r]  = relu([hh[r] | h[r]] W + c3[r, 0:3] . v[q, 0:3, :])                         (lin_com folded into
 *             lin_update, the per-query affine term: c3 = (deg_hi, deg_lo - deg_hi, 1), v = (u, g u, d))
 *   acc[r] += h[r] P  (+ out[r] Pn when pn_planes is given: the last layer)               (post_mp.0 blocks)
 * -- gnn_model.py:255-277, 303-350 of the reference (GossipConv.forward, the layer loop), and the h_l blocks of
 * post_mp.0 (:44, 102).  W = [(D_a C)^T; D_b^T] [128, 64], P / Pn = the post_mp.0 blocks of h_l / h_{l+1} as [64, 64]
 * K-major matrices, each passed as the fp16 planes [2][64 (n)][K] of desco_split_f16x2_f32 of its n-major form with
 * its {scale, 1/scale}; the products run in the three-product f16x3 form (fp32 accuracy).  h, acc, out and the
 * planes 16-byte aligned; out, acc and h distinct (acc is read and written in place).  Results are bit-reproducible
 * and do not depend on the launch's tiling (every row's sum keeps its CSR order).  No host sync, no state of its own:
 * capturable in a hipGraph.  Bytes per row: 256 (h) + 256 per neighbour row + 256 (out) + 512 (acc) + 12 (c3), plus
 * the CSR. */
int desco_gossip_layer_f16x3_f32(const float* h, const int32_t* rowptr, const int32_t* col, int64_t num_nodes,
                                 int num_q, const float* g, const float* c3, const float* v, const int16_t* w_planes,
                                 const float* w_scale, const int16_t* p_planes, const float* p_scale,
                                 const int16_t* pn_planes, const float* pn_scale, float* acc, float* out,
                                 desco_stream_t stream);

/* Neighborhood models of other widths than 64 (--neigh_hidden_dim = H in 1..256, csrc/shmp_wide.hip).  The host pads
 * every H-wide block of the folded operands with zeros to width = 64 ceil(H / 64) in {64, 128, 192, 256}.
 *
 * One SAGE layer of one node-type group, fused: for rows r in [row0, row0 + num_rows) of the virtual-row CSR (vslots
 * virtual rows per row, vrowptr indexed by r * vslots + s, vcol = rows of x; the first `slots` of them are used),
 *   y[r] = relu([sum slot 0 | ... | sum slot S-1 | x[r]] Wt + bias)          Wt [(slots + 1) width, width]
 * with Wt passed as w_planes [2][width][(slots + 1) width] / w_scale = desco_split_f16x2_f32 of Wt^T; the products run
 * in the three-product f16x3 form (one power-of-two scale per (row, K-block), fp32 accumulation).  y[r] goes to
 * out[r * ldo] (absolute row; may be NULL) and to out2[(r - row0) * ld2] (relative row; may be NULL), at least one of
 * them.  slots in {2, 4}, slots <= vslots <= 4; x and the planes 16-byte aligned, ldx % 4 == 0; out / out2 must not be x.  Every row's
 * neighbours are summed in CSR order: results are bit-reproducible and do not depend on the tiling.  Capturable. */
int desco_shmp_layer_wide_f16x3_f32(const float* x, int64_t ldx, const int32_t* vrowptr, const int32_t* vcol,
                                    int vslots, int64_t row0, int64_t num_rows, int slots, int width, const int16_t* w_planes,
                                    const float* w_scale, const float* bias, float* out, int64_t ldo, float* out2,
                                    int64_t ld2, desco_stream_t stream);

/* out[(v * slots + s) * ldo + 0 : width] = sum_{e in vrow v * slots + s} x[vcol[e] * ldx + 0 : width] in CSR order, for
 * num_rows rows of slots in {1, 2, 4} virtual rows each; width % 4 == 0, width <= 256; x and out 16-byte aligned,
 * ldx, ldo multiples of 4 and >= width. */
int desco_csr_gather_sum_wide_f32(const float* x, int64_t ldx, const int32_t* vrowptr, const int32_t* vcol,
                                  int64_t num_rows, int slots, int width, float* out, int64_t ldo, desco_stream_t stream);

/* One layer of a plain (homogeneous) GIN or GCN neighborhood model, fused (--neigh_conv_type GIN / GCN,
 * csrc/plain_layer.hip), on operands zero-padded to width = 64 ceil(H / 64) in {64, 128, 192, 256}: for rows r in
 * [row0, row0 + num_rows) of a PLAIN CSR (rowptr indexed by r, col = rows of x),
 *   z[r] = sum_{e in [rowptr[r], rowptr[r + 1])} x[col[e]]  (fp32, CSR order)  + s x[r]     (s = *self_scale; 0 if NULL)
 *   h    = z W1 + b1;      num_mats == 2:  h = relu(h) W2 + b2;      y[r] = relu(h)
 * W1, W2 [width, width] are passed as planes [2][width][width] / scale = desco_split_f16x2_f32 of their transposes
 * (w2_planes, w2_scale, b2 are read for num_mats == 2 only).  Both products run in the three-product f16x3 form with
 * one power-of-two scale per row and product; relu(h) stays in the workgroup.  y[r] goes to out[r * ldo] (may be NULL)
 * and, for r >= out2_row0, to out2[(r - out2_row0) * ld2] (may be NULL), at least one of them.  x and the planes
 * 16-byte aligned, ldx % 4 == 0; out / out2 must not be x.  A row whose relu(h) is all zero gives relu(b2) exactly.
 * Results are bit-reproducible and depend neither on the tiling nor on row0.  self_scale is read on the device (no
 * host synchronisation).  Capturable. */
int desco_plain_layer_f16x3_f32(const float* x, int64_t ldx, const int32_t* rowptr, const int32_t* col,
                                const float* self_scale, int64_t row0, int64_t num_rows, int width, int num_mats,
                                const int16_t* w1_planes, const float* w1_scale, const float* b1,
                                const int16_t* w2_planes, const float* w2_scale, const float* b2, float* out,
                                int64_t ldo, float* out2, int64_t ld2, int64_t out2_row0, desco_stream_t stream);

/* desco_count_head_f32 (same arguments and results, exp2_minus_1 and b2_dev included) for hid % 64 == 0, hid <= 1024;
 * num_q <= 32; t 16-byte aligned, ldt % 4 == 0, ldt and ldq >= hid, ldo >= num_q. */
int desco_count_head_wide_f32(const float* t, int64_t ldt, const float* qh, int64_t ldq, int hid, const float* w2,
                              float b2, const float* b2_dev, float slope, int exp2_minus_1, float* out, int64_t ldo,
                              int64_t num_b, int num_q, desco_stream_t stream);

/* K21 tail: out[r] = add[r] + sum_c y[r,c]*w[c] + b   (post_mp.7 with output_dim 1, then
 * pred = neigh_pred + gossip_pred, lightning_model.py:622-625) */
int desco_rowdot_add_f32(const float* y, int64_t ldy, int ncols, const float* w, float b,
                         const float* add, float* out, int64_t num_rows, desco_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward pass (training, lightning_model.py:228-254 train_forward + autograd in the reference).
 * Input gradients reuse the forward entry points (dA = dZ * W is desco_gemm_f32 with the
 * un-transposed weight; the transpose of a CSR gather is desco_csr_gather_sum_f32 over the
 * transposed index).  All reductions are deterministic (workspace partials, fixed order).
 * ------------------------------------------------------------------------------------------ */

/* Building blocks of the fused training trunk (desco_amd/autograd.py::ShmpTrunk: the whole
 * BaseGNNCore.forward SAGE loop + anchor + pooling as ONE autograd node, its backward running the chain rule
 * on preallocated buffers -- lightning_model.py:228-254 via loss.backward()):
 *  desco_csr_gather_sum_add_f32: out[j, 0:64] = extra[j, 0:64] + sum_{e in [rowptr[j], rowptr[j+1])} x[col[e], 0:64]
 *    (one slot; out rows ldo apart, extra rows ld_extra apart, extra may be out): the transposed gather of the
 *    backward pass accumulating onto the gradient a row already has from its other consumers;
 *  desco_add_rows_f32: dst[i, 0:ncols] += src[i, 0:ncols]  (ncols % 4 == 0, 16-byte aligned rows). */
int desco_csr_gather_sum_add_f32(const float* x, int64_t ldx, const int32_t* rowptr, const int32_t* col,
                                 int64_t num_rows, const float* extra, int64_t ld_extra, float* out,
                                 int64_t ldo, desco_stream_t stream);
int desco_add_rows_f32(float* dst, int64_t ldd, const float* src, int64_t lds, int64_t num_rows, int ncols,
                       desco_stream_t stream);
/* The input-row gradient of one SHMP layer of the training trunk in one launch:
 *   out[i, 0:64] = mask_i * ( seed_i + d[i, self_off .. +63] + sum_{v in [t_rowptr[i], t_rowptr[i+1])} dv[t_col[v]] )
 * d = dZ Wt^T [num_rows, ldd] (relation-slot blocks, then the self block at column self_off_count for rows
 * < num_count, self_off_canon for the others), dv = d viewed as rows of 64 floats (t_col indexes them: the
 * transposed index over (row, slot) virtual rows with ldd / 64 blocks per row); seed_i = dpool[seg_id[i]] (the
 * pooling's broadcast gradient, rows ld_pool apart) for i < num_count, dcanon[i - num_count] (NULL: 0) otherwise;
 * mask = (relu_src[i] > 0) * mask_scale elementwise, or 1 when relu_src is NULL (mask_scale: 1, or the factor
 * 1 / (1 - p) of an F.dropout behind the relu, gnn_model.py:273-274: relu_src = dropout(relu(z)) is positive exactly
 * where the element was kept).  Replaces a seed build, two adds, the transposed gather and the activation gradient
 * (five launches) of the per-op wiring. */
int desco_shmp_bwd_dx_f32(const float* d, int64_t ldd, const int32_t* t_rowptr, const int32_t* t_col,
                          int64_t num_rows, int64_t num_count, int self_off_count, int self_off_canon,
                          const float* dpool, int64_t ld_pool, const int32_t* seg_id, const float* dcanon,
                          int64_t ld_canon, const float* relu_src, float mask_scale, float* out,
                          desco_stream_t stream);

/* bytes of workspace desco_gemm_tn_f32 needs for this shape (and the number of M slabs it uses) */
size_t desco_gemm_tn_workspace(int64_t m, int k, int n, int* splits_out);

/* weight gradient: out[k, n] (+)= A[m, k]^T * B[m, n];  k % 64 == 0, n % 64 == 0 */
int desco_gemm_tn_f32(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t m, int k,
                      int n, float* out, int64_t ldo, int accumulate, float* workspace,
                      desco_stream_t stream);

/* weight AND bias gradient of one Linear c = act([a1 | a2] wt + bias) in two launches (partials over M
 * slabs + one fixed-order reduce): dwt[k1+k2, n] = [a1 | a2]^T dz, dbias[n] = sum_m dz[m, n] (dbias may be
 * NULL; a2 may be NULL with k2 = 0).  k1 % 64 == k2 % 64 == n % 64 == 0.  Replaces two desco_gemm_tn_f32
 * and one desco_colsum_f32 call (six launches) of the training step.  m == 0 gives zero gradients (a1 / dz may then be
 * NULL).  workspace:
 * desco_linear_bwd_w_workspace(m, k1 + k2, n) bytes. */
size_t desco_linear_bwd_w_workspace(int64_t m, int k, int n);
int desco_linear_bwd_w_f32(const float* a1, int64_t lda1, int k1, const float* a2, int64_t lda2, int k2,
                           const float* dz, int64_t lddz, int64_t m, int n, float* dwt, int64_t lddw,
                           float* dbias, float* workspace, desco_stream_t stream);

/* Up to 16 independent problems of desco_linear_bwd_w_f32's form (contiguous dwt: lddw = n) in one partial launch and
 * one reduce launch: the (layer, row type) weight gradients of a training step's trunk, which nothing but the optimizer
 * waits for.  m == 0 gives zero gradients (a1 / dz may then be NULL).  workspace: desco_linear_bwd_w_multi_workspace(num, descs) bytes. */
typedef struct desco_bwd_w_desc {
  const float* a1; int64_t lda1; int k1;
  const float* a2; int64_t lda2; int k2;
  const float* dz; int64_t lddz; int64_t m; int n;
  float* dwt; float* dbias;
} desco_bwd_w_desc;
size_t desco_linear_bwd_w_multi_workspace(int num, const desco_bwd_w_desc* descs);
int desco_linear_bwd_w_multi_f32(int num, const desco_bwd_w_desc* descs, float* workspace, desco_stream_t stream);

/* bias gradient: out[n] (+)= sum_m x[m, n];  workspace: 512 * n floats */
int desco_colsum_f32(const float* x, int64_t ldx, int64_t m, int n, float* out, int accumulate,
                     float* workspace, desco_stream_t stream);

/* torch.optim.Adam's step (both models' configure_optimizers, reference lightning_model.py:160-173, 570-583:
 * Adam(lr, weight_decay), default betas / eps, L2 decay, no amsgrad) for a LIST of tensors, one launch per 128 tensors:
 *   g' = g + wd p;  m += (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;
 *   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)              (bias corrections and 1 - beta in double, as torch forms them)
 * params / grads / sizes: HOST arrays of `num` device pointers / element counts; grads[i] == NULL skips tensor i (value,
 * moments and age untouched, as torch skips parameters without gradient).  m, v: device, flat, tensor i at offset
 * sum(sizes[:i]); steps [num] float (per-tensor step count t, advanced by the launch), arrivals [num] uint32 (zero
 * before the first call; scratch), lr [1] float: all device memory, so a captured launch replays without host work. */
int desco_adam_step_f32(int num, float* const* params, const float* const* grads, const int64_t* sizes, float* m,
                        float* v, float* steps, uint32_t* arrivals, const float* lr, double beta1, double beta2,
                        double eps, double weight_decay, desco_stream_t stream);

/* The SHMP trunk of a SMALL single-type batch -- the query graphs of the neighborhood model, which the reference embeds
 * again on every training batch (lightning_model.py:204-207; BaseGNNCore.forward gnn_model.py:253-277 + global_add_pool
 * :88-89, 107) -- in ONE workgroup per direction: rows in LDS, layers separated by barriers.  num_rows <=
 * desco_shmp_trunk_small_max_rows() (144), two relation slots per row (vrowptr [2 n + 1]), exact fp32 FMA chains.
 *   fwd: X_0 = x0; X_{l+1} = relu([agg_0(X_l) | agg_1(X_l) | X_l] wt[l] + bias[l]) -> xall[l] ([L][n][64]);
 *        pooled[b, 64 l : 64 (l + 1)] = sum of X_l over rows seg_ptr[b] .. seg_ptr[b + 1]
 *   bwd: from dpooled [num_seg][ldp]: dwt [L][192][64], dbias [L][64], dx0 [n][64]; wt_t = wt with its last two axes
 *        swapped ([L][64][192]); t_rowptr / t_col: the transposed index over virtual rows 3 k + s
 *        (desco_vcsr_transpose_sym's, re-based to 3 blocks per row), seg_id [n]: the row's segment. */
int desco_shmp_trunk_small_max_rows(void);
int desco_shmp_trunk_small_fwd_f32(const float* x0, const int32_t* vrowptr, const int32_t* vcol, int num_rows,
                                   int num_layers, const float* wt, const float* bias, const int32_t* seg_ptr,
                                   int num_seg, float* xall, float* pooled, int64_t ldp, desco_stream_t stream);
int desco_shmp_trunk_small_bwd_f32(const float* x0, const float* xall, const int32_t* vrowptr, const int32_t* vcol,
                                   const int32_t* t_rowptr, const int32_t* t_col, const int32_t* seg_id, int num_rows,
                                   int num_layers, const float* wt_t, const float* dpooled, int64_t ldp, float* dwt,
                                   float* dbias, float* dx0, desco_stream_t stream);

/* round 6: the same trunk with ONE WORKGROUP PER GRAPH (segment), for batches whose graphs have at most
 * desco_shmp_trunk_graphs_max_rows() (8) rows each -- the 29 query graphs (3..5 nodes; lightning_model.py:204-207): the
 * graphs are independent of each other, so 29 workgroups stream the layers' weights side by side instead of one
 * workgroup walking 135 rows behind one weight stream.  Arguments as the _small_ entry points.  PRECONDITION: every
 * segment has at most desco_shmp_trunk_graphs_max_rows() rows -- the entry points do not check it, and rows of a segment
 * beyond the limit are silently left out (autograd.ShmpTrunkSmall.per_graph is the caller's check); the backward takes wt itself ([L][192][64], no transposed
 * copy), seg_ptr instead of seg_id, and a workspace of num_layers * num_rows * 64 floats; no limit on num_rows.
 * drop (NULL: none): F.dropout behind every layer's relu (gnn_model.py:274) -- layer l's rows are multiplied by the
 * factor of (row, col) of site drop->site + 2 l; the backward then takes mask_scale = drop->scale (1 without). */
int desco_shmp_trunk_graphs_max_rows(void);
int desco_shmp_trunk_graphs_fwd_f32(const float* x0, const int32_t* vrowptr, const int32_t* vcol, int64_t num_rows,
                                    int num_layers, const float* wt, const float* bias, const int32_t* seg_ptr,
                                    int num_seg, const desco_dropout* drop, float* xall, float* pooled, int64_t ldp,
                                    desco_stream_t stream);
int desco_shmp_trunk_graphs_bwd_f32(const float* x0, const float* xall, const int32_t* vrowptr, const int32_t* vcol,
                                    const int32_t* t_rowptr, const int32_t* t_col, const int32_t* seg_ptr, int num_seg,
                                    int64_t num_rows, int num_layers, const float* wt, const float* dpooled, int64_t ldp,
                                    float mask_scale, float* dwt, float* dbias, float* dx0, float* workspace,
                                    desco_stream_t stream);

/* Backward of desco_linear_smallk_f32 with n = 64 (pre_mp, gnn_model.py:131; feat carries no gradient):
 * dwb[k][0:64] = sum_m feat[m, k] dout[m, :] for k < K, dwb[K][0:64] = sum_m dout[m, :] (the bias gradient), in one
 * pass over dout and one reduce.  workspace: 512 * (k + 1) * 64 floats. */
int desco_linear_smallk_bwd_f32(const float* feat, int64_t ldf, int k, const float* dout, int64_t ldd, int64_t m,
                                float* dwb, float* workspace, desco_stream_t stream);

/* Backward of out[r] = add[r] + y[r, :] . w + b with y = relu(z) (post_mp.7 on post_mp.6's output, gnn_model.py:40-53):
 *   dz[r, c] = dout[r] * w[c] * (y[r, c] > 0),  dwb[c] = sum_r dout[r] * y[r, c] (c < n),  dwb[n] = sum_r dout[r]
 * in one pass over y (n % 4 == 0, n <= 1024, 256 % (n / 4) == 0).  workspace: 1024 * (n + 1) floats. */
int desco_rowdot_bwd_f32(const float* y, int64_t ldy, int n, const float* w, const float* dout, int64_t num_rows,
                         float* dz, int64_t lddz, float* dwb, float* workspace, desco_stream_t stream);

/* dz = dc * act'(c) for c = act(z) (contiguous, count elements) */
int desco_act_grad_f32(const float* dc, const float* c, int act, float slope, float* dz,
                       int64_t count, desco_stream_t stream);

/* The count head straight from the target embeddings (inference): T[b, :] = Wt emb[b, 0:64] (count_model.0's target half,
 * lightning_model.py:127-131) is formed 32 features at a time on the matrix pipe (f16x3, wt_planes / wt_scale =
 * desco_split_f16x2_f32 of the [256, 64] weight) and consumed from registers, so the [m, 256] tensor T that
 * desco_linear64_bf16x6_f32 would write and desco_count_head_f32 read never exists.  Same result as that pair up to
 * rounding.  hid must be 256 and num_q 29 (the standard query set, data.py:37); other shapes use the two-launch form. */
int desco_count_head_emb_f16x3_f32(const float* emb, int64_t lde, int64_t m, const int16_t* wt_planes,
                                   const float* wt_scale, const float* qh, int64_t ldq, int hid, const float* w2,
                                   float b2, const float* b2_dev, float slope, int exp2_minus_1, float* out,
                                   int64_t ldo, int num_q, desco_stream_t stream);

/* backward of desco_count_head_f32 (logit mode): given dl[b,q] = dLoss/dlogit,
 * dt[b,c], dqh[q,c] (contiguous [num_q, hid]), dw2[c];  (db2 = sum dl is left to the caller)
 * workspace: desco_count_head_bwd_workspace(num_b, num_q, hid) bytes (ABI 1 documented a constant of
 * 256 * (num_q+1) * hid floats; the slab count grew to 1024 -- ask, do not assume) */
size_t desco_count_head_bwd_workspace(int64_t num_b, int num_q, int hid);
int desco_count_head_bwd_f32(const float* t, int64_t ldt, const float* qh, int64_t ldq, int hid,
                             const float* w2, float slope, const float* dl, int64_t lddl,
                             int64_t num_b, int num_q, float* dt, int64_t lddt, float* dqh,
                             float* dw2, float* workspace, desco_stream_t stream);

/* Training-path helpers of the gossip stage (the fused inference kernel has the same terms folded
 * into its epilogues): a rank-ks affine term with per-query coefficient vectors,
 *   out[r,:] = act( base[r,:] + sum_{k<ks} c[r,k] * v[r % qv][k][:] ),   rows of 64, ks <= 8,
 * its weight gradient dv[qv][k][:] = sum_{r = i*qv+q} c[r,k] * dz[r,:]
 * (workspace: 64 * qv * ks * 64 floats), and a row-wise dot product out[r] = a[r,:] . b[r,:]. */
int desco_affine_rows_f32(const float* base, const float* c, int ks, const float* v, int qv,
                          int act, float slope, float* out, int64_t num_rows,
                          desco_stream_t stream);
int desco_affine_rows_bwd_f32(const float* c, int ks, const float* dz, int qv, int64_t num_rows,
                              float* dv, float* workspace, desco_stream_t stream);
int desco_rowdot2_f32(const float* a, const float* b, int ncols, float* out, int64_t num_rows,
                      desco_stream_t stream);

/* ---- round 6: dropout of the training steps (desco_dropout above) -------------------------------------------------- */

/* key_out[0..1] = state[0..1] = (seed, step); state[1] += 1.  One launch per training forward pass: the step's kernels
 * (forward and backward) read key_out, the next step gets the next counter -- also when the step is a replayed hipGraph. */
int desco_rng_next(uint64_t* state, uint64_t* key_out, desco_stream_t stream);
/* out[r, c] = the factor (0 or d->scale) of element (r, c): what the fused epilogues multiply by.  For tests (the oracle
 * takes the mask as an input) and for callers that want the mask itself. */
int desco_dropout_mask_f32(const desco_dropout* d, int64_t num_rows, int num_cols, float* out, int64_t ldo,
                           desco_stream_t stream);
/* desco_affine_rows_f32 followed by dropout: out = factor(r, c) * act(base + sum_k c[r,k] v[r % qv][k][:]) */
int desco_affine_rows_dropout_f32(const float* base, const float* c, int ks, const float* v, int qv, int act,
                                  float slope, const desco_dropout* d, float* out, int64_t num_rows,
                                  desco_stream_t stream);
/* desco_act_grad_f32 through a dropout: dz[r, c] = dc[r, c] * factor(r, c) * act'(c[r, c]) for c = factor * act(z)
 * (contiguous [num_rows, num_cols]) */
int desco_act_grad_dropout_f32(const float* dc, const float* c, int act, float slope, const desco_dropout* d,
                               float* dz, int64_t num_rows, int num_cols, desco_stream_t stream);

/* ---- round 5: the glue of the training steps (lightning_model.py:228-254, 285-289, 585-608, 630-635) ----------------- */

/* Strided 2-D copies / transposes, any number per call (24 per launch): dst[r][c] = src[r][c], or with transpose != 0
 * dst[c][r] = src[r][c] (dst is then cols x rows); accumulate != 0 adds into dst.  The moves between nn.Linear's
 * [out, in] layout and the K-major operands of the GEMM entry points, the canonical rows into the anchor operand, the
 * halves of a split weight -- what torch's .t().contiguous() / cat / slice assignment launched in rounds 2-4. */
typedef struct desco_copy2d_desc {
  const float* src; int64_t lds;
  float* dst; int64_t ldd;
  int32_t rows, cols, transpose, accumulate;
} desco_copy2d_desc;
int desco_copy2d_multi_f32(int num, const desco_copy2d_desc* descs, desco_stream_t stream);

/* The weight folding of the fused SHMP layer (gnn_model.py:253-277: per edge type SAGEConv.lin, per node type the update
 * Linear over cat(aggregate, x)) for all layers of one row type, read from the parameters where torch keeps them:
 *   wt[l][s 64 + k][n] = sum_j U_l[n][j] W_{l,s}[j][k]  (s < slots),   wt[l][slots 64 + k][n] = U_l[n][64 + k],
 *   fb[l][n] = sum_j U_l[n][j] (sum_u b_{l,u}[j]) + c_l[n].
 * table: device array, per layer [U, c, W_0 .. W_{slots-1}, b_0 .. b_{num_bias-1}] as int64 device addresses (U
 * [64, 128], W [64, 64], c / b [64], contiguous fp32; slots of one relation carry the same W address).
 * bwd: from dwt / dfb the gradient of every parameter, written at grad_offsets[same index] (in floats) of `grads`
 * (tied W: the sum over its slots, written once).  Exact fp32 FMA chains in a fixed order. */
int desco_fold_shmp_fwd_f32(const int64_t* table, int num_layers, int slots, int num_bias, float* wt, float* fb,
                            desco_stream_t stream);
int desco_fold_shmp_bwd_f32(const int64_t* table, const int64_t* grad_offsets, int num_layers, int slots, int num_bias,
                            const float* dwt, const float* dfb, float* grads, desco_stream_t stream);

/* The two training losses and their gradients in one pass (+ a one-block fold of the partial sums, fixed order):
 *   mode 0  loss = mean_i smooth_l1(pred[i] - log2(y[i] + 1))     (lightning_model.py:285-289, 246-254; beta = 1)
 *   mode 1  loss = sum_i log2(|pred[i] - y[i]| + 1)                (lightning_model.py:630-635)
 * dpred[i] = d loss / d pred[i].  workspace: 1024 floats. */
int desco_loss_f32(const float* pred, const float* y, int64_t count, int mode, float* loss, float* dpred,
                   float* workspace, desco_stream_t stream);

/* out[i] = a[i] * mul[0] + add[0] + addv[i], every term but a optional (NULL): a saved gradient times the upstream
 * gradient of its scalar loss; x + correction + post_mp.7's bias.  p[i] = value. */
int desco_affine_scalar_f32(const float* a, const float* mul, const float* add, const float* addv, float* out,
                            int64_t count, desco_stream_t stream);
int desco_fill_f32(float* p, float value, int64_t count, desco_stream_t stream);

/* The operands of the gossip training trunk as functions of the raw parameters (gnn_model.py:58-103, 230-260, 303-350;
 * algebra DESIGN.md 4.2), for num_q <= 64 queries with embeddings E [num_q, 64]; E, w_pre = pre_mp.weight[:, 0] and
 * b_pre = pre_mp.bias carry no gradient (the layer-0 input is detached, gnn_model.py:236-240):
 *   V0 [Q,6,64] = [p, g0 p, r, g0 r, t, z], V1 [Q,3,64] = [u, g1 u, db1], Vp [Q,2,64] = [tp, zp], wt1 = [(D1a C1)^T; D1b^T],
 *   wtp = [P0c^T; P0d^T], w3t = P3^T, w5t = P5^T, gates g0 / g1 = lin_gate(E), g1c = 1 - g1      (formulas: train_native.hip)
 * All matrices in nn.Linear's [out, in] layout: C0 [64,128], D0 [64,192], C1 [64,64], D1 [64,128], G0 [64,64], g2 [64]
 * (lin_gate.2.weight[0]), gb2 [1], P0 [64,256], P3 [64,64], P5 [256,64].  a, h0, h1 [Q,64]: saved for the backward.
 * bwd: the gradient of every parameter from the gradients of the outputs (dg1: the trunk's own gate gradient, may be
 * NULL); scratch: 4 * num_q * 64 floats.  One workgroup each; exact fp32 FMA chains in a fixed order. */
typedef struct desco_gossip_fold_params {
  const float *E, *w_pre, *b_pre;
  const float *C0, *cb0, *D0, *db0, *C1, *cb1, *D1, *db1;
  const float *G0[2], *gb0[2], *g2[2], *gb2[2];
  const float *P0, *p0, *P3, *P5;
  int32_t num_q;
} desco_gossip_fold_params;
typedef struct desco_gossip_fold_out {
  float *V0, *V1, *Vp, *wt1, *wtp, *w3t, *w5t, *g0, *g1, *g1c, *a, *h0, *h1;
} desco_gossip_fold_out;
typedef struct desco_gossip_fold_grads {
  const float *dV0, *dV1, *dVp, *dwt1, *dwtp, *dw3t, *dw5t, *dg1;
  float *dC0, *dcb0, *dD0, *ddb0, *dC1, *dcb1, *dD1, *ddb1;
  float *dG0[2], *dgb0[2], *dg2[2], *dgb2[2];
  float *dP0, *dp0, *dP3, *dP5;
  float* scratch;
} desco_gossip_fold_grads;
int desco_gossip_fold_fwd_f32(const desco_gossip_fold_params* p, const desco_gossip_fold_out* o, desco_stream_t stream);
int desco_gossip_fold_bwd_f32(const desco_gossip_fold_params* p, const desco_gossip_fold_out* o,
                              const desco_gossip_fold_grads* d, desco_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DESCO_HIP_H */
