// Graphlet degree distributions and their agreement on the GPU (C ABI: desco_gdd_build_dev, desco_gdd_agreement_dev).
// Definitions: include/desco_hip.h, "GRAPHLET DEGREE DISTRIBUTION"; the shared arithmetic: graphlet_distribution.hpp.
//
// Two kernels.
//   gdd_build_kernel      one block per (segment, column), three phases around the list's own slots [n] of key / val.
//                         A: the column's int64 values sit in LDS and every thread counts, for its rows, the values
//                            >= 1 that are smaller and the equal ones in earlier rows (LDS broadcast reads, as the rank
//                            kernel of the graphlet correlation): that is the row's position in the sorted column, and
//                            its value goes there into the val slots (as int64 bits); values < 1 go behind them as 0.
//                         B: the LDS is free again.  Every thread walks a contiguous piece of the sorted slots, counts
//                            the run heads, a block scan numbers them, and head i leaves its key in key[i] and its
//                            position in LDS.
//                         C: multiplicity = next head's position - own; S_i = d_i / k_i.  T is a sequential chain by
//                            definition: the first wave loads 64 shares at a time, one per lane, and every lane adds
//                            them in order from lane broadcasts (v_readlane), so all hold the same T; then all
//                            threads divide and write val, and the unused slots are zeroed.
//   gdd_agreement_kernel  a 32 x 32 tile of pairs per block, four pairs per thread, columns in ascending order (the
//                         sum over columns is a chain too).  Per column the tile's 64 lists are staged in a pool in
//                         LDS as far as they fit (lists above GDD_STAGE_MAX entries, and what the pool cannot take,
//                         are read from global memory where they lie); every pair runs its two-pointer merge and its
//                         fma chain in ascending key on the fp64 vector pipe.  Lanes of a wave merge lists of different
//                         lengths: that divergence is the price of the defined order.
#include "common_device.hpp"
#include "graphlet_distribution.hpp"

namespace desco {

constexpr int GDD_TILE = 32, GDD_THREADS = 256;
constexpr int GDD_POOL = 4096;                       // staged entries per column and tile: 64 KiB of keys and values
constexpr int GDD_STAGE_MAX = 512;                   // a longer list is never staged
static_assert(DESCO_GCM_MAX_COLUMNS == gdd::kMaxColumns, "column bound");
static_assert(DESCO_GCM_DEV_MAX_ROWS * 8 <= 160 * 1024, "one column must fit the LDS");
static_assert(DESCO_GCM_DEV_MAX_ROWS * 4 + 128 <= 160 * 1024, "the head positions must fit the LDS");

struct GddArgs {
  const int64_t* seg_ptr;
  const int64_t* counts;
  const int64_t* seg_ids;
  int64_t num_segs, num_rows, ld, max_rows;
  int C;
  int32_t* len;
  int64_t* key;
  double* val;
  int32_t* status;
  int32_t columns[DESCO_GCM_MAX_COLUMNS];
};

// the dynamic LDS of a launch bound: the column in phase A; 16 ints of scratch and n + 1 head positions afterwards
inline size_t gdd_build_lds(int64_t max_rows) {
  const int64_t a = 8 * max_rows, b = 64 + 4 * (max_rows + 1);
  return (size_t)(((a > b ? a : b) + 15) & ~(int64_t)15);
}

__device__ __forceinline__ double gdd_lane(double v, int lane) {          // lane: wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void gdd_build_kernel(GddArgs p) {
  extern __shared__ __attribute__((aligned(16))) int64_t gdd_lds[];
  constexpr int WAVES = THREADS / 64;
  const int tid = threadIdx.x, c = blockIdx.y, lane = tid & 63, wave = tid >> 6;
  const int64_t i = p.seg_ids ? p.seg_ids[blockIdx.x] : (int64_t)blockIdx.x;
  if (i < 0 || i >= p.num_segs) return;              // a bad id: nothing to write to  (uniform)
  const int64_t r0 = p.seg_ptr[i], r1 = p.seg_ptr[i + 1], n64 = r1 - r0;
  if (r0 < 0 || n64 < 0 || r1 > p.num_rows || n64 > p.max_rows) {
    if (tid == 0 && c == 0) p.status[i] = -1;
    return;                                          // (uniform)
  }
  const int n = (int)n64;
  int64_t* __restrict__ key = p.key + r0 * p.C + (int64_t)c * n;
  double* __restrict__ val = p.val + r0 * p.C + (int64_t)c * n;
  int64_t* __restrict__ sorted = reinterpret_cast<int64_t*>(val);
  // ---- A: the sorted column into the val slots ----------------------------------------------------------------------
  const int64_t* __restrict__ src = p.counts + p.columns[c];
  for (int l = tid; l < n; l += THREADS) {
    const int64_t v = src[(r0 + l) * p.ld];
    gdd_lds[l] = v >= 1 ? v : 0;
  }
  __syncthreads();
  for (int l = tid; l < n; l += THREADS) {
    const int64_t v = gdd_lds[l];
    int less = 0, before = 0, zeros = 0, zeros_before = 0;
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
      const int64_t w = gdd_lds[j];
      less += (w != 0) & (w < v);
      before += (w == v) & (j < l);
      zeros += w == 0;
    }
    if (v == 0) zeros_before = before;
    const int pos = v != 0 ? less + before : n - zeros + zeros_before;
    sorted[pos] = v;
  }
  __threadfence_block();
  __syncthreads();                                   // the column is consumed, the sorted slots are visible
  // ---- B: run heads ---------------------------------------------------------------------------------------------------
  int32_t* scratch = reinterpret_cast<int32_t*>(gdd_lds);                   // [16]: wave totals, the list's length
  int32_t* hpos = scratch + 16;                                             // [n + 1]
  const int chunk = (n + THREADS - 1) / THREADS;
  const int l0 = tid * chunk < n ? tid * chunk : n, l1 = l0 + chunk < n ? l0 + chunk : n;
  int heads = 0;
  {
    int64_t prev = l0 > 0 && l0 < n ? sorted[l0 - 1] : 0;
    for (int l = l0; l < l1; ++l) {
      const int64_t v = sorted[l];
      heads += (v != 0) & (v != prev);
      prev = v;
    }
  }
  int incl = heads;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) scratch[wave] = incl;
  __syncthreads();
  int base = incl - heads, runs = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int t = scratch[w];
    if (w < wave) base += t;
    runs += t;
  }
  {
    int64_t prev = l0 > 0 && l0 < n ? sorted[l0 - 1] : 0;
    for (int l = l0; l < l1; ++l) {
      const int64_t v = sorted[l];
      if (v != 0 && v != prev) {
        key[base] = v;
        hpos[base] = l;
        ++base;
      }
      if (v == 0 && prev != 0) hpos[runs] = l;      // the end of the values >= 1 (at most one such l in the block)
      prev = v;
    }
    if (tid == 0 && (n == 0 || sorted[n - 1] != 0)) hpos[runs] = n;
  }
  __threadfence_block();
  __syncthreads();                                   // the sorted slots are consumed, the keys are visible
  // ---- C: shares, their chain, the divisions -------------------------------------------------------------------------
  double* Tsh = reinterpret_cast<double*>(scratch + 8);
  if (wave == 0) {
    double T = 0.0;
    for (int b = 0; b < runs; b += 64) {
      const int e = b + lane;
      const double s = e < runs ? gdd::share((int64_t)(hpos[e + 1] - hpos[e]), key[e]) : 0.0;
      const int cnt = runs - b < 64 ? runs - b : 64;
      for (int j = 0; j < cnt; ++j) T = T + gdd_lane(s, j);
    }
    if (lane == 0) *Tsh = T;
  }
  __syncthreads();
  const double T = *Tsh;
  for (int e = tid; e < n; e += THREADS) {
    if (e < runs) {
      val[e] = gdd::share((int64_t)(hpos[e + 1] - hpos[e]), key[e]) / T;
    } else {
      key[e] = 0;
      val[e] = 0.0;
    }
  }
  if (tid == 0) {
    p.len[i * p.C + c] = runs;
    if (c == 0) p.status[i] = 0;
  }
}

struct GddSide {
  const int64_t* seg_ptr;
  const int32_t* len;
  const int64_t* key;
  const double* val;
  int64_t G;
};

__global__ __launch_bounds__(GDD_THREADS) void gdd_agreement_kernel(GddSide x, GddSide y, int C,
                                                                    double* __restrict__ agree, int64_t ldo,
                                                                    double* __restrict__ per_orbit) {
  __shared__ int64_t pool_key[GDD_POOL];
  __shared__ double pool_val[GDD_POOL];
  __shared__ int64_t seg0[2 * GDD_TILE];             // first row and rows of the tile's 64 segments (x then y)
  __shared__ int32_t rows[2 * GDD_TILE];
  __shared__ const int64_t* kp[2 * GDD_TILE];        // where each list of this column is read from
  __shared__ const double* vp[2 * GDD_TILE];
  __shared__ int32_t ln[2 * GDD_TILE], stage_off[2 * GDD_TILE];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wave = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.y * GDD_TILE, j0 = (int64_t)blockIdx.x * GDD_TILE;
  if (tid < 2 * GDD_TILE) {
    const GddSide& s = tid < GDD_TILE ? x : y;
    const int64_t g = (tid < GDD_TILE ? i0 : j0) + (tid & (GDD_TILE - 1));
    int64_t a = 0, n = 0;
    if (g < s.G) {
      a = s.seg_ptr[g];
      n = s.seg_ptr[g + 1] - a;
      n = n < 0 ? 0 : n > INT32_MAX ? INT32_MAX : n;
    }
    seg0[tid] = a;
    rows[tid] = (int32_t)n;
  }
  double sum[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int c = 0; c < C; ++c) {
    __syncthreads();                                 // the previous column's lists are consumed (first pass: seg0, rows)
    if (wave == 0) {                                 // the 64 lists of this column: lengths, and their places in the pool
      const GddSide& s = lane < GDD_TILE ? x : y;
      const int64_t g = (lane < GDD_TILE ? i0 : j0) + (lane & (GDD_TILE - 1));
      int l = 0;
      if (g < s.G) {
        l = s.len[g * C + c];
        l = l < 0 ? 0 : l > rows[lane] ? rows[lane] : l;
      }
      const int want = l <= GDD_STAGE_MAX ? l : 0;
      int incl = want;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      const bool staged = want > 0 && incl <= GDD_POOL;
      const int64_t at = seg0[lane] * C + (int64_t)c * rows[lane];
      ln[lane] = l;
      stage_off[lane] = staged ? incl - want : -1;
      kp[lane] = staged ? pool_key + (incl - want) : s.key + at;
      vp[lane] = staged ? pool_val + (incl - want) : s.val + at;
    }
    __syncthreads();
    for (int q = wave; q < 2 * GDD_TILE; q += GDD_THREADS / 64) {
      const int off = stage_off[q];
      if (off < 0) continue;                         // (uniform)
      const GddSide& s = q < GDD_TILE ? x : y;
      const int64_t at = seg0[q] * C + (int64_t)c * rows[q];
      for (int e = lane; e < ln[q]; e += 64) {
        pool_key[off + e] = s.key[at + e];
        pool_val[off + e] = s.val[at + e];
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const int a = ty + 16 * u, b = GDD_TILE + tx + 16 * v;
        const int64_t i = i0 + a, j = j0 + (b - GDD_TILE);
        if (i >= x.G || j >= y.G) continue;
        const double A = gdd::agreement(gdd::merge_chain(kp[a], vp[a], ln[a], kp[b], vp[b], ln[b]));
        if (per_orbit) per_orbit[(i * y.G + j) * C + c] = A;
        sum[u][v] = sum[u][v] + A;
      }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int64_t i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i < x.G && j < y.G) agree[i * ldo + j] = sum[u][v] / (double)C;
    }
}

template <int THREADS>
int gdd_launch_build(const GddArgs& a, int64_t num_ids, hipStream_t stream) {
  const hipError_t e = size_dynamic_lds<gdd_build_kernel<THREADS>>((int)gdd_build_lds(DESCO_GCM_DEV_MAX_ROWS));
  if (e != hipSuccess) return fail((int)e, "desco_gdd_build_dev: cannot size LDS");
  hipLaunchKernelGGL(gdd_build_kernel<THREADS>, dim3((unsigned)num_ids, (unsigned)a.C), dim3(THREADS),
                     gdd_build_lds(a.max_rows), stream, a);
  return launch_status("desco_gdd_build_dev");
}

}  // namespace desco

using namespace desco;

extern "C" int desco_gdd_build_dev(const int64_t* seg_ptr, int64_t num_segs, int64_t num_rows, const int64_t* counts,
                                   int64_t ld, const int32_t* columns, int C, const int64_t* seg_ids,
                                   int64_t num_ids, int64_t max_rows, int32_t* len, int64_t* key, double* val,
                                   int32_t* status, desco_stream_t stream) {
  if (num_segs < 0 || num_rows < 0 || num_ids < 0 || ld < 0 || max_rows < 0)
    return fail(DESCO_EINVAL, "desco_gdd_build_dev: negative num_segs, num_rows, num_ids, ld or max_rows");
  if (C < 1 || C > DESCO_GCM_MAX_COLUMNS)
    return fail(DESCO_EINVAL, "desco_gdd_build_dev: C is outside 1..128 (DESCO_GCM_MAX_COLUMNS)");
  if (!seg_ids) num_ids = num_segs;
  if (num_ids == 0) return 0;
  if (max_rows > DESCO_GCM_DEV_MAX_ROWS)
    return fail(DESCO_EINVAL,
                "desco_gdd_build_dev: a segment's rows exceed DESCO_GCM_DEV_MAX_ROWS (20480); use desco_gdd_build for "
                "it");
  if (num_ids > INT32_MAX) return fail(DESCO_EINVAL, "desco_gdd_build_dev: num_ids is above 2^31 - 1");
  if (!seg_ptr) return fail(DESCO_EINVAL, "desco_gdd_build_dev: seg_ptr is null");
  if (!columns) return fail(DESCO_EINVAL, "desco_gdd_build_dev: columns is null");
  if (!len) return fail(DESCO_EINVAL, "desco_gdd_build_dev: len is null");
  if (!status) return fail(DESCO_EINVAL, "desco_gdd_build_dev: status is null");
  if (num_rows > 0 && !counts) return fail(DESCO_EINVAL, "desco_gdd_build_dev: counts is null");
  if (num_rows > 0 && (!key || !val)) return fail(DESCO_EINVAL, "desco_gdd_build_dev: key or val is null");
  if (mis8(seg_ptr) || mis8(counts) || mis8(seg_ids) || mis8(key) || mis8(val))
    return fail(DESCO_EINVAL, "desco_gdd_build_dev: a 64-bit array is not 8-byte aligned");
  GddArgs a{};
  for (int c = 0; c < C; ++c) {
    if (columns[c] < 0 || columns[c] >= ld)
      return fail(DESCO_EINVAL, "desco_gdd_build_dev: a column index is outside 0..ld-1");
    a.columns[c] = columns[c];
  }
  a.seg_ptr = seg_ptr, a.counts = counts, a.seg_ids = seg_ids;
  a.num_segs = num_segs, a.num_rows = num_rows, a.ld = ld, a.max_rows = max_rows;
  a.C = C, a.len = len, a.key = key, a.val = val, a.status = status;
  hipStream_t s = (hipStream_t)stream;
  // one wave per (segment, column) where the launch's segments are small (DESCO_GCM_WAVE_ROWS), four above
  return max_rows <= DESCO_GCM_WAVE_ROWS ? gdd_launch_build<64>(a, num_ids, s) : gdd_launch_build<256>(a, num_ids, s);
}

extern "C" int desco_gdd_agreement_dev(const int64_t* x_seg_ptr, const int32_t* x_len, const int64_t* x_key,
                                       const double* x_val, int64_t Gx, const int64_t* y_seg_ptr,
                                       const int32_t* y_len, const int64_t* y_key, const double* y_val, int64_t Gy,
                                       int C, double* agree, int64_t ldo, double* per_orbit, desco_stream_t stream) {
  if (Gx < 0 || Gy < 0) return fail(DESCO_EINVAL, "desco_gdd_agreement_dev: negative Gx or Gy");
  if (C < 1 || C > DESCO_GCM_MAX_COLUMNS)
    return fail(DESCO_EINVAL, "desco_gdd_agreement_dev: C is outside 1..128 (DESCO_GCM_MAX_COLUMNS)");
  if (Gx == 0 || Gy == 0) return 0;
  if (ldo < Gy) return fail(DESCO_EINVAL, "desco_gdd_agreement_dev: ldo is below Gy");
  if (!agree) return fail(DESCO_EINVAL, "desco_gdd_agreement_dev: agree is null");
  if (!x_seg_ptr || !y_seg_ptr) return fail(DESCO_EINVAL, "desco_gdd_agreement_dev: seg_ptr is null");
  if (!x_len || !y_len) return fail(DESCO_EINVAL, "desco_gdd_agreement_dev: len is null");
  if (mis8(x_seg_ptr) || mis8(x_key) || mis8(x_val) || mis8(y_seg_ptr) || mis8(y_key) || mis8(y_val) || mis8(agree) ||
      mis8(per_orbit))
    return fail(DESCO_EINVAL, "desco_gdd_agreement_dev: a 64-bit array is not 8-byte aligned");
  const int64_t bx = (Gy + GDD_TILE - 1) / GDD_TILE, by = (Gx + GDD_TILE - 1) / GDD_TILE;
  if (bx > INT32_MAX || by > 65535)
    return fail(DESCO_EINVAL, "desco_gdd_agreement_dev: more than 2097120 segments of x (or 2^36 of y) in one call");
  const GddSide x{x_seg_ptr, x_len, x_key, x_val, Gx}, y{y_seg_ptr, y_len, y_key, y_val, Gy};
  hipLaunchKernelGGL(gdd_agreement_kernel, dim3((unsigned)bx, (unsigned)by), dim3(GDD_THREADS), 0, (hipStream_t)stream,
                     x, y, C, agree, ldo, per_orbit);
  return launch_status("desco_gdd_agreement_dev");
}
