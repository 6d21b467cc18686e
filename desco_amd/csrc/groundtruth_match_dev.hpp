// THE device walk of the pattern-guided matcher: gtm_count_kernel, instantiated by groundtruth_match_dev.hip (counts:
// unlabelled / labelled x induced / non-induced) and by occurrences_dev.hip (the LISTING instantiations, which store
// every map they find instead of counting it).  The argument type selects the instantiation at compile time.
//
// Work item = (CSR entry (v, u0) with u0 < v, plan record), handled by ONE WAVE; groundtruth_match_dev.hip has the
// layout and the reasons.
#pragma once
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

// LISTING (occurrences_dev.hip; `out` is unused): a match takes slot = cursor[v]++ and is stored, in query-node order,
// as row ptr[v] - ptr_base + slot of `rows` -- if slot is inside the anchor's segment [ptr[v], ptr[v + 1]) and the row
// inside [0, rows_capacity); anything else sets *overflow and stores nothing.
struct GtmListArgs : GtmArgs {
  const int64_t* ptr;                  // [N + 1]
  int64_t ptr_base, rows_capacity;
  int32_t* cursor;                     // [N]
  int32_t* rows;                       // [rows_capacity][k]
  int32_t* overflow;
};
struct GtmListMonoArgs : GtmListArgs {};

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

// LISTING: the lane's map img[0..k-2] (LDS column) + `last` at position k - 1 is one occurrence anchored at v.  `seg` =
// ptr[v + 1] - ptr[v], `row0` = ptr[v] - ptr_base (read once per wave), node[i] = the query node of position i (LDS).
// Every store is inside rows[0 .. rows_capacity * k): the slot is checked against the segment, the row against the
// buffer and the column against k, whatever ptr, cursor and plan hold.
__device__ __forceinline__ void gtm_emit(const GtmListArgs& a, int64_t v, int64_t base, int64_t seg, int64_t row0,
                                         const int* img, const int* node, int k, int last) {
  const int slot = atomicAdd(a.cursor + v, 1);
  const int64_t dst = row0 + slot;
  if (slot < 0 || slot >= seg || dst < 0 || dst >= a.rows_capacity) {
    *a.overflow = 1;
    return;
  }
  int32_t* row = a.rows + dst * k;
  for (int i = 0; i < k; ++i) {
    const unsigned c = (unsigned)node[i];
    if (c < (unsigned)k) row[c] = (int32_t)(base + (i + 1 == k ? last : img[i * GTM_THREADS]));
  }
}

template <class Args>
__global__ __launch_bounds__(GTM_THREADS) void gtm_count_kernel(Args a) {
  constexpr bool LAB = std::is_base_of<GtmLabArgs, Args>::value;
  constexpr bool LIST = std::is_base_of<GtmListArgs, Args>::value;
  constexpr bool IND = !std::is_same<Args, GtmMonoArgs>::value && !std::is_same<Args, GtmLabMonoArgs>::value &&
                       !std::is_same<Args, GtmListMonoArgs>::value;
  constexpr int HEAD = LAB ? GTML_HEAD : GTM_HEAD, REC = LAB ? GTML_REC : GTM_REC;
  __shared__ int img_s[GTM_KMAX * GTM_THREADS];
  __shared__ long long cur_s[GTM_KMAX * GTM_THREADS];
  __shared__ unsigned lvl_s[GTM_WAVES * 2 * GTM_KMAX];
  __shared__ int qlab_s[LAB ? GTM_WAVES * GTM_KMAX : 1];
  __shared__ int node_s[LIST ? GTM_WAVES * GTM_KMAX : 1];
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
    if constexpr (LIST) node_s[wave * GTM_KMAX + lane] = rec[GTM_NODE + lane];
  }
  __syncthreads();                                 // (the only barrier: every wave reaches it)
  if (!live) return;
  const int k = rec[GTM_K];
  [[maybe_unused]] const int q = rec[GTM_QUERY];
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
  [[maybe_unused]] int64_t seg = 0, row0 = 0;      // LISTING: the anchor's segment
  [[maybe_unused]] const int* node = node_s + wave * GTM_KMAX;
  if constexpr (LIST) {
    const int64_t p0 = a.ptr[v];
    seg = a.ptr[v + 1] - p0;
    row0 = p0 - a.ptr_base;
  }
  [[maybe_unused]] unsigned long long found = 0;
  if (k == 2) {
    if constexpr (LIST) {
      if (lane == 0) gtm_emit(a, v, base, seg, row0, img, node, k, u0);
    } else {
      found = lane == 0;
    }
  } else {
    const int64_t p2 = base + img[(lvl[4] >> 16) * GTM_THREADS];
    const int64_t r0 = a.rowptr[p2], r1 = a.rowptr[p2 + 1];
    for (int64_t e2 = r0 + lane; e2 < r1; e2 += 64) {
      const int u2 = (int)(a.col[e2] - base);
      if (u2 >= c.lv) break;                       // rows ascend
      if (!gtm_fits<LAB, IND>(c, 2, u2)) continue;
      if (k == 3) {
        if constexpr (LIST) gtm_emit(a, v, base, seg, row0, img, node, k, u2);
        else ++found;
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
          if constexpr (LIST) gtm_emit(a, v, base, seg, row0, img, node, k, u);
          else ++found;
        } else {
          img[level * GTM_THREADS] = u;
          ++level;
          cur[level * GTM_THREADS] = a.rowptr[base + img[(lvl[2 * level] >> 16) * GTM_THREADS]];
        }
      }
    }
  }
  if constexpr (!LIST) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) found += __shfl_xor(found, o, 64);
    if (lane == 0 && found) atomicAdd(a.out + v * a.Q + q, found);
  }
}

}  // namespace desco
