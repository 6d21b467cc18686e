// Device side of the data-set statistics (C ABI: desco_subgraph_stats_dev), see include/desco_hip.h.
//
// Per node set M (ascending global ids of one graph): the largest connected component C of G[M] (a tie goes to the
// component holding the smallest id) and its members / n / m / diameter / distance sum / triangles (int64) and
// clustering sum (fp64).  Bit-identical to the host twin (subgraph_stats.cpp).
//
// One launch serves the sets of one WORD BUCKET W in {1, 2, 4, 8, 16}: sets of at most 64 W members, named by a list
// of set ids.  One workgroup per set (W = 1, the molecule case: one wave per set, one lane per source):
//
//   build   the induced adjacency as bitset rows of W 64-bit words in LDS.  A member whose CSR row has at most 64
//           entries is one lane's: it bisects every neighbour in the sorted member list and sets the bit with a plain
//           LDS store (the row is its own).  Longer rows (hubs) are then taken one at a time by a whole wave, 64 entries
//           per step, with LDS atomicOr.
//   bfs     one lane per source: visited / frontier / next are W-word bitsets in registers, a level ORs the rows of the
//           frontier's bits.  Lanes read different rows, so the row stride is the odd word count W | 1: consecutive rows
//           start on different banks (power-of-two strides would put every row of W = 16 on 2 of the 64 banks).  Per
//           source: reach, lowest reached id (= the component's label), eccentricity, distance sum; and, from the rows
//           alone, degree and 2 T(i) = sum over neighbours j of popcount(A[i] & A[j]).
//   select  C = the largest (reach, then smallest label) by one block-wide max; the integers are block sums / a max
//           over the sources in C (order free: integers).
//   fp64    term i = 2 T(i) / (d (d - 1)) (0 outside C and below degree 2): one IEEE division of two exact integers.
//           The terms are summed by the balanced pairwise tree over local ids (leaf i meets leaf i + s at stride
//           s = 1, 2, 4, ..).  Missing leaves are +0.0 and x + 0.0 = x, so the bits depend on the set alone -- not on
//           the bucket it runs in, the block size or the grid.  The terms re-use the rows' LDS once the rows are done.
//
// The kernel guards itself: a set with more members than its bucket holds -- or with an id outside the graph, or not
// strictly ascending -- gets `members` written and n = -1 and does no other work (the caller sends those rows to the
// host twin, which names what is wrong with them).  LDS is sized by the template argument alone.  No atomics on
// global memory, no MFMA: two launches on the same input write the same bytes.
#include "common_device.hpp"

namespace desco {

struct SubgraphStatsArgs {
  const int64_t* rowptr;     // [num_nodes + 1]
  const int32_t* col;        // global node ids, rows ascending
  int64_t num_nodes;
  const int64_t* set_ptr;    // [num_sets + 1]
  const int32_t* set_nodes;  // members, ascending inside a set
  const int64_t* set_ids;    // [num_ids] the sets of this launch
  int64_t* out_i64;          // [num_sets][6]
  double* out_f64;           // [num_sets]
};

template <int W>
struct StatsShape {
  static constexpr int kMembers = 64 * W;                         // capacity of the bucket
  static constexpr int kStride = W | 1;                           // words per LDS row (odd)
  static constexpr int kThreads = W == 1 ? 64 : W == 2 ? 128 : 256;
};

// local id of x in mem[0, m) (ascending), -1 when absent
__device__ __forceinline__ int member_index(const int32_t* __restrict__ mem, int m, int32_t x) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int32_t y = mem[mid];
    if (y == x) return mid;
    if (y < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return -1;
}

__device__ __forceinline__ void stats_refuse(const SubgraphStatsArgs& a, int64_t s, int64_t members) {
  if (threadIdx.x == 0) {
    int64_t* o = a.out_i64 + 6 * s;
    o[0] = members;
    o[1] = -1;
    o[2] = o[3] = o[4] = o[5] = 0;
    a.out_f64[s] = 0.0;
  }
}

template <int W>
__global__ __launch_bounds__(StatsShape<W>::kThreads) void subgraph_stats_kernel(SubgraphStatsArgs a) {
  constexpr int N = StatsShape<W>::kMembers, S = StatsShape<W>::kStride, T = StatsShape<W>::kThreads;
  constexpr int kWaves = T / 64;
  __shared__ uint64_t rows[N * S];
  __shared__ int32_t key[N], ecc[N], dsum[N], deg[N], tri2[N];
  __shared__ int64_t red[4][kWaves];
  __shared__ int32_t redkey[kWaves];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t s = a.set_ids[blockIdx.x];
  const int64_t p0 = a.set_ptr[s], m64 = a.set_ptr[s + 1] - p0;
  if (m64 < 0 || m64 > N) {          // (block-uniform) not this bucket's: no LDS is touched
    stats_refuse(a, s, m64);
    return;
  }
  const int m = (int)m64;
  if (m == 0) {
    if (tid == 0) {
      int64_t* o = a.out_i64 + 6 * s;
      o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = 0;
      a.out_f64[s] = 0.0;
    }
    return;
  }
  const int32_t* __restrict__ mem = a.set_nodes + p0;

  // ---- guard the ids, clear the rows -----------------------------------------------------------------------------
  int bad = 0;
  for (int i = tid; i < m; i += T) {
    const int32_t v = mem[i];
    bad |= v < 0 || v >= a.num_nodes || (i > 0 && mem[i - 1] >= v);
  }
  for (int k = tid; k < m * S; k += T) rows[k] = 0ull;
  if (__syncthreads_or(bad)) {
    stats_refuse(a, s, m64);
    return;
  }

  // ---- build -----------------------------------------------------------------------------------------------------
  int wide = 0;
  for (int i = tid; i < m; i += T) {
    const int64_t v = mem[i], r0 = a.rowptr[v], r1 = a.rowptr[v + 1];
    if (r1 - r0 > 64) {
      wide = 1;
      continue;
    }
    for (int64_t e = r0; e < r1; ++e) {
      const int j = member_index(mem, m, a.col[e]);
      if (j >= 0 && j != i) rows[i * S + (j >> 6)] |= 1ull << (j & 63);
    }
  }
  if (__syncthreads_or(wide)) {
    for (int i = wave; i < m; i += kWaves) {            // (wave-uniform)
      const int64_t v = mem[i], r0 = a.rowptr[v], r1 = a.rowptr[v + 1];
      if (r1 - r0 <= 64) continue;
      for (int64_t e = r0 + lane; e < r1; e += 64) {
        const int j = member_index(mem, m, a.col[e]);
        if (j >= 0 && j != i) atomicOr((unsigned long long*)&rows[i * S + (j >> 6)], 1ull << (j & 63));
      }
    }
    __syncthreads();
  }

  // ---- one BFS per source; degree and triangles of the source ------------------------------------------------------
  for (int i = tid; i < m; i += T) {
    uint64_t vis[W], fr[W];
#pragma unroll
    for (int k = 0; k < W; ++k) vis[k] = fr[k] = k == (i >> 6) ? 1ull << (i & 63) : 0ull;
    int d = 0, reach = 1, dist = 0;
    while (true) {
      uint64_t nx[W];
#pragma unroll
      for (int q = 0; q < W; ++q) nx[q] = 0ull;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        uint64_t f = fr[k];
        while (f) {
          const int j = k * 64 + __ffsll((long long)f) - 1;
          f &= f - 1;
          const uint64_t* r = &rows[j * S];
#pragma unroll
          for (int q = 0; q < W; ++q) nx[q] |= r[q];
        }
      }
      uint64_t any = 0ull;
      int cnt = 0;
#pragma unroll
      for (int q = 0; q < W; ++q) {
        nx[q] &= ~vis[q];
        vis[q] |= nx[q];
        fr[q] = nx[q];
        any |= nx[q];
        cnt += __popcll(nx[q]);
      }
      if (!any) break;
      ++d;
      reach += cnt;
      dist += d * cnt;
    }
    int label = 0;
#pragma unroll
    for (int q = W - 1; q >= 0; --q)
      if (vis[q]) label = q * 64 + __ffsll((long long)vis[q]) - 1;
    key[i] = reach * 2048 + (1023 - label);             // largest reach first, then the smallest label
    ecc[i] = d;
    dsum[i] = dist;

    uint64_t ai[W];
    int dg = 0, t2 = 0;
#pragma unroll
    for (int q = 0; q < W; ++q) {
      ai[q] = rows[i * S + q];
      dg += __popcll(ai[q]);
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      uint64_t f = ai[k];
      while (f) {
        const int j = k * 64 + __ffsll((long long)f) - 1;
        f &= f - 1;
        const uint64_t* r = &rows[j * S];
#pragma unroll
        for (int q = 0; q < W; ++q) t2 += __popcll(ai[q] & r[q]);
      }
    }
    deg[i] = dg;
    tri2[i] = t2;
  }

  // ---- select C ----------------------------------------------------------------------------------------------------
  int best = 0;
  for (int i = tid; i < m; i += T) best = max(best, key[i]);   // (a thread's own entries: no barrier needed yet)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
  if (lane == 0) redkey[wave] = best;
  __syncthreads();                                             // also: every read of `rows` is behind us
#pragma unroll
  for (int w = 0; w < kWaves; ++w) best = max(best, redkey[w]);

  // ---- integers; clustering terms into the rows' LDS ---------------------------------------------------------------
  int leaves = 1;
  while (leaves < m) leaves <<= 1;                             // <= N
  double* term = reinterpret_cast<double*>(rows);
  int64_t v_deg = 0, v_diam = 0, v_dist = 0, v_tri = 0;
  for (int i = tid; i < leaves; i += T) {
    double t = 0.0;
    if (i < m && key[i] == best) {
      const int dg = deg[i];
      v_deg += dg;
      v_diam = max(v_diam, (int64_t)ecc[i]);
      v_dist += dsum[i];
      v_tri += tri2[i];
      if (dg >= 2) t = (double)tri2[i] / ((double)dg * (double)(dg - 1));
    }
    term[i] = t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v_deg += __shfl_xor(v_deg, o, 64);
    v_diam = max(v_diam, __shfl_xor(v_diam, o, 64));
    v_dist += __shfl_xor(v_dist, o, 64);
    v_tri += __shfl_xor(v_tri, o, 64);
  }
  if (lane == 0) {
    red[0][wave] = v_deg;
    red[1][wave] = v_diam;
    red[2][wave] = v_dist;
    red[3][wave] = v_tri;
  }
  for (int st = 1; st < leaves; st <<= 1) {
    __syncthreads();
    for (int i = tid * 2 * st; i + st < leaves; i += T * 2 * st) term[i] += term[i + st];
  }
  __syncthreads();
  if (tid == 0) {
    v_deg = v_dist = v_tri = v_diam = 0;
    for (int w = 0; w < kWaves; ++w) {
      v_deg += red[0][w];
      v_diam = max(v_diam, red[1][w]);
      v_dist += red[2][w];
      v_tri += red[3][w];
    }
    int64_t* o = a.out_i64 + 6 * s;
    o[0] = m;
    o[1] = best >> 11;
    o[2] = v_deg / 2;
    o[3] = v_diam;
    o[4] = v_dist;
    o[5] = v_tri / 6;
    a.out_f64[s] = term[0];
  }
}

template <int W>
static int launch_subgraph_stats(const SubgraphStatsArgs& a, int64_t num_ids, hipStream_t st) {
  hipLaunchKernelGGL(subgraph_stats_kernel<W>, dim3((unsigned)num_ids), dim3(StatsShape<W>::kThreads), 0, st, a);
  return launch_status("desco_subgraph_stats_dev");
}

}  // namespace desco

using namespace desco;

extern "C" int desco_subgraph_stats_dev(const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                                        const int64_t* set_ptr, const int32_t* set_nodes, const int64_t* set_ids,
                                        int64_t num_ids, int words, int64_t* out_i64, double* out_f64,
                                        desco_stream_t stream) {
  if (words != 1 && words != 2 && words != 4 && words != 8 && words != 16)
    return fail(DESCO_EINVAL, "desco_subgraph_stats_dev: words must be 1, 2, 4, 8 or 16");
  if (num_ids < 0 || num_ids > INT32_MAX || num_nodes < 0 || num_nodes > INT32_MAX)
    return fail(DESCO_EINVAL, "desco_subgraph_stats_dev: num_ids or num_nodes negative or above 2^31");
  if (num_ids == 0) return 0;
  if (!rowptr) return fail(DESCO_EINVAL, "desco_subgraph_stats_dev: rowptr is null");
  if (!col) return fail(DESCO_EINVAL, "desco_subgraph_stats_dev: col is null");
  if (!set_ptr) return fail(DESCO_EINVAL, "desco_subgraph_stats_dev: set_ptr is null");
  if (!set_nodes) return fail(DESCO_EINVAL, "desco_subgraph_stats_dev: set_nodes is null");
  if (!set_ids) return fail(DESCO_EINVAL, "desco_subgraph_stats_dev: set_ids is null");
  if (!out_i64) return fail(DESCO_EINVAL, "desco_subgraph_stats_dev: out_i64 is null");
  if (!out_f64) return fail(DESCO_EINVAL, "desco_subgraph_stats_dev: out_f64 is null");
  if (mis8(rowptr) || mis8(set_ptr) || mis8(set_ids) || mis8(out_i64) || mis8(out_f64))
    return fail(DESCO_EINVAL, "desco_subgraph_stats_dev: a 64-bit array is not 8-byte aligned");
  const SubgraphStatsArgs a{rowptr, col, num_nodes, set_ptr, set_nodes, set_ids, out_i64, out_f64};
  hipStream_t st = (hipStream_t)stream;
  switch (words) {
    case 1: return launch_subgraph_stats<1>(a, num_ids, st);
    case 2: return launch_subgraph_stats<2>(a, num_ids, st);
    case 4: return launch_subgraph_stats<4>(a, num_ids, st);
    case 8: return launch_subgraph_stats<8>(a, num_ids, st);
    default: return launch_subgraph_stats<16>(a, num_ids, st);
  }
}
