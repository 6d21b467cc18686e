// Device-side typed CSR of WHOLE graphs (C ABI: desco_graph_tconv_dev*), see include/desco_hip.h.
//
// The triangle / tride split of ToTconvHetero (transforms.py:180-255: T = A*(A@A) + A, an edge is a "tride" edge iff
// T <= 1, i.e. iff its endpoints share no neighbour) for every directed edge of a GraphSet, written as the 2-slot
// destination-major CSR the query-model kernels read (QueryBatch's arrays): the model without canonical partition
// reads whole target graphs in that form.
//
// Every row keeps all of its sources, only re-ordered (triangle sources first, tride sources after, each ascending), so
// the output places are row-local: vrowptr[2v] = rowptr[v], vrowptr[2v+1] = rowptr[v] + (triangle sources of v).  What a
// row needs from the others is the number of triangle edges in front of each of its entries.  Three launches, none of
// which knows anything about graph sizes (no per-graph workspace, no LDS):
//
//   flag   one LANE per directed edge (d <- s): do rows s and d intersect?  Both rows are sorted, so the elements of
//          the shorter one are looked up in the longer one by bisection.  A lane does that alone while the shorter row
//          has at most kLaneRow elements; the longer tests of a wave are then taken one after the other by the whole
//          wave (64 elements of the shorter row per step), so no lane ever walks a hub row.  The wave's 64 flags are
//          one ballot word; the word, its population count and every entry's row go to the workspace.
//   scan   exclusive prefix sum of the population counts (one per 64 edges).
//   fill   one lane per edge: triangle edges in front of it = prefix of its word + popcount of the word's lower bits,
//          the same at its row's two ends gives the row's triangle count -> the entry's place; one lane per row writes
//          the two row pointers.  A stable partition: sources stay ascending inside each (row, slot).
//
// No atomics: two launches on the same input write the same bytes.  Bit-identical to the host twin (graph_tconv.cpp).
#include "common_device.hpp"

namespace desco {

constexpr int kLaneRow = 16;   // a lane intersects on its own while the shorter row is at most this long

struct GraphTconvArgs {
  const int64_t* rowptr;   // [>= node0 + num_nodes + 1], global
  const int32_t* col;      // global node ids
  int64_t node0, num_nodes, edge0, num_edges;
  uint64_t* mask;          // [W] triangle flags of 64 consecutive edges, W = ceil(num_edges / 64)
  int32_t* wcnt;           // [W] their population counts
  int32_t* wpre;           // [W + 1] exclusive scan of wcnt
  int32_t* erow;           // [num_edges] row (block-local) of every entry
  int32_t* vrowptr;        // [2 num_nodes + 1]
  int32_t* vcol;           // [num_edges]
};

// x in col[lo, hi) (ascending)?
__device__ __forceinline__ bool row_has(const int32_t* __restrict__ col, int64_t lo, int64_t hi, int32_t x) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int32_t y = col[mid];
    if (y == x) return true;
    if (y < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return false;
}

__global__ __launch_bounds__(256) void graph_tconv_flag_kernel(GraphTconvArgs g) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t e = wave * 64 + lane;                 // block-local entry
  if (wave * 64 >= g.num_edges) return;               // (whole waves only: the ballots below need every lane)
  const bool live = e < g.num_edges;
  int64_t a0 = 0, alen = 0, b0 = 0, blen = 0;         // shorter row, longer row (places in col)
  bool tri = false, wide = false;
  if (live) {
    // the entry's row: the last v with rowptr[v] <= edge0 + e (rows may be empty)
    const int64_t ge = g.edge0 + e;
    int64_t lo = g.node0, hi = g.node0 + g.num_nodes;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (g.rowptr[mid] <= ge)
        lo = mid;
      else
        hi = mid;
    }
    const int64_t d = lo;
    g.erow[e] = (int32_t)(d - g.node0);
    const int64_t s = g.col[ge];
    if (s >= g.node0 && s < g.node0 + g.num_nodes) {  // (a source outside the block has no row here: tride)
      const int64_t d0 = g.rowptr[d], d1 = g.rowptr[d + 1], s0 = g.rowptr[s], s1 = g.rowptr[s + 1];
      const bool s_short = s1 - s0 <= d1 - d0;
      a0 = s_short ? s0 : d0;
      alen = s_short ? s1 - s0 : d1 - d0;
      b0 = s_short ? d0 : s0;
      blen = s_short ? d1 - d0 : s1 - s0;
      wide = alen > kLaneRow;
      if (!wide)
        for (int64_t i = 0; i < alen && !tri; ++i) tri = row_has(g.col, b0, b0 + blen, g.col[a0 + i]);
    }
  }
  // the longer tests, one at a time on all 64 lanes
  unsigned long long pend = __ballot(wide);
  while (pend) {
    const int k = __ffsll((long long)pend) - 1;
    pend &= pend - 1;
    const int64_t ka0 = __shfl(a0, k, 64), kalen = __shfl(alen, k, 64);
    const int64_t kb0 = __shfl(b0, k, 64), kblen = __shfl(blen, k, 64);
    bool found = false;
    for (int64_t i = 0; i < kalen && !found; i += 64) {
      const bool f = i + lane < kalen && row_has(g.col, kb0, kb0 + kblen, g.col[ka0 + i + lane]);
      found = __ballot(f) != 0ull;
    }
    if (lane == k) tri = found;
  }
  const unsigned long long m = __ballot(tri);
  if (lane == 0) {
    g.mask[wave] = m;
    g.wcnt[wave] = __popcll(m);
  }
}

// wpre[0..W] = exclusive prefix sums of wcnt[0..W) (one block, chunks of 1024 in sequence; W = edges / 64)
__global__ __launch_bounds__(1024) void graph_tconv_scan_kernel(const int32_t* __restrict__ wcnt, int64_t W,
                                                                int32_t* __restrict__ wpre) {
  __shared__ int32_t wsum[16];
  __shared__ int32_t carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int64_t c0 = 0; c0 < W; c0 += 1024) {
    const int64_t i = c0 + tid;
    const int32_t x = i < W ? wcnt[i] : 0;
    int32_t inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int32_t woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    const int32_t base = carry;
    if (i < W) wpre[i] = base + woff + inc - x;
    __syncthreads();
    if (tid == 1023) carry = base + woff + inc;
    __syncthreads();
  }
  if (tid == 0) wpre[W] = carry;
}

// triangle edges among the block's entries [0, x)
__device__ __forceinline__ int32_t tri_before(const GraphTconvArgs& g, int64_t x) {
  if (g.num_edges == 0) return 0;                     // (no flag / scan launch, and no workspace, without edges)
  const int b = (int)(x & 63);
  int32_t p = g.wpre[x >> 6];
  if (b) p += __popcll(g.mask[x >> 6] & ((1ull << b) - 1ull));
  return p;
}

__global__ __launch_bounds__(256) void graph_tconv_fill_kernel(GraphTconvArgs g) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < g.num_edges) {
    const int64_t d = g.node0 + g.erow[i];
    const int64_t r0 = g.rowptr[d] - g.edge0, r1 = g.rowptr[d + 1] - g.edge0;
    const int32_t p0 = tri_before(g, r0);
    const int32_t tb = tri_before(g, i) - p0, nt = tri_before(g, r1) - p0;
    const bool tri = (g.mask[i >> 6] >> (i & 63)) & 1ull;
    const int64_t pos = tri ? r0 + tb : r0 + nt + (i - r0 - tb);
    g.vcol[pos] = (int32_t)(g.col[g.edge0 + i] - g.node0);
  }
  if (i < g.num_nodes) {
    const int64_t r0 = g.rowptr[g.node0 + i] - g.edge0, r1 = g.rowptr[g.node0 + i + 1] - g.edge0;
    g.vrowptr[2 * i] = (int32_t)r0;
    g.vrowptr[2 * i + 1] = (int32_t)(r0 + tri_before(g, r1) - tri_before(g, r0));
  } else if (i == g.num_nodes) {
    g.vrowptr[2 * i] = (int32_t)g.num_edges;
  }
}

static inline int64_t tconv_words(int64_t num_edges) { return (num_edges + 63) / 64; }

}  // namespace desco

using namespace desco;

extern "C" size_t desco_graph_tconv_dev_workspace(int64_t num_edges) {
  if (num_edges < 0) return 0;
  const int64_t W = tconv_words(num_edges);
  // mask [W] (8 bytes each, first: keeps it 8-byte aligned), wcnt [W], wpre [W + 1], erow [num_edges]
  return (size_t)(8 * W + 4 * W + 4 * (W + 1) + 4 * num_edges);
}

extern "C" int desco_graph_tconv_dev(const int64_t* rowptr, const int32_t* col, int64_t node0, int64_t num_nodes,
                                     int64_t edge0, int64_t num_edges, int32_t* vrowptr, int32_t* vcol,
                                     void* workspace, desco_stream_t stream) {
  if (!rowptr || !vrowptr || node0 < 0 || num_nodes < 0 || edge0 < 0 || num_edges < 0 ||
      (num_edges > 0 && (!col || !vcol || !workspace || num_nodes == 0)) || mis8(workspace) ||
      2 * num_nodes + 1 > INT32_MAX || num_edges > INT32_MAX)
    return fail(DESCO_EINVAL, "desco_graph_tconv_dev: bad argument or more than 2^31 rows / edges");
  GraphTconvArgs a{};
  a.rowptr = rowptr;
  a.col = col;
  a.node0 = node0;
  a.num_nodes = num_nodes;
  a.edge0 = edge0;
  a.num_edges = num_edges;
  const int64_t W = tconv_words(num_edges);
  a.mask = (uint64_t*)workspace;
  a.wcnt = (int32_t*)(a.mask + W);
  a.wpre = a.wcnt + W;
  a.erow = a.wpre + W + 1;
  a.vrowptr = vrowptr;
  a.vcol = vcol;
  hipStream_t st = (hipStream_t)stream;
  if (num_edges > 0) {
    hipLaunchKernelGGL(graph_tconv_flag_kernel, dim3((unsigned)((W + 3) / 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(graph_tconv_scan_kernel, dim3(1), dim3(1024), 0, st, a.wcnt, W, a.wpre);
  }
  const int64_t items = num_edges > num_nodes + 1 ? num_edges : num_nodes + 1;
  hipLaunchKernelGGL(graph_tconv_fill_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, a);
  return launch_status("desco_graph_tconv_dev");
}
