// Graphlet correlation matrices and distances on the GPU (C ABI: desco_graphlet_correlation_dev, desco_gcd_matrix_dev).
// Definitions: include/desco_hip.h, "GRAPHLET CORRELATION"; the shared arithmetic: graphlet_correlation.hpp.
//
// Three kernels.
//   gcm_rank_kernel   one block per (segment, column): the column's int64 values, dummy row included, sit in LDS and
//                     every thread counts, for its rows, the smaller and the equal values among all of them (LDS
//                     broadcast reads).  d = 2 less + equal - n' goes to the int32 workspace.  Counting needs no sort
//                     and is exact whatever the ties are.  One wave per block where the launch's segments are small.
//   gcm_matrix_kernel one block per segment: S = D^T D in 4 x 4 register tiles of its upper triangle, rows staged
//                     through LDS in chunks of GCM_CHUNK; |d| < 2^15, so a product is one int32 multiply and the
//                     sum one 64-bit add (v_mad_i64_i32).  Where the tiles are fewer than the threads, a tile's rows
//                     are dealt to several threads; every partial sum is added to an int64 image of S in LDS
//                     (ds_add_u64).  Integer adds commute, so S equals the twin's bits in any order.  rho and the
//                     upper-triangle vector are computed from that image in the same launch.
//   gcd_kernel        a 32 x 32 tile of pairs per block, four pairs per thread; the x and y rows go through LDS in
//                     chunks of GCD_CHUNK entries and every pair runs its fma chain in ascending p on the fp64
//                     vector pipe.  No matrix instruction: its internal order of k is not the defined one.
#include "common_device.hpp"
#include "graphlet_correlation.hpp"

namespace desco {

constexpr int GCM_CHUNK = 32;                        // rows of D per LDS stage of the matrix kernel
constexpr int GCM_THREADS = 256;
constexpr int GCD_TILE = 32, GCD_CHUNK = 32, GCD_THREADS = 256;
static_assert((int64_t)DESCO_GCM_DEV_MAX_ROWS * DESCO_GCM_DEV_MAX_ROWS < ((int64_t)1 << 31), "d * d must fit int32");
static_assert(DESCO_GCM_DEV_MAX_ROWS * 8 <= 160 * 1024, "one column must fit the LDS");
static_assert(DESCO_GCM_MAX_COLUMNS == gcm::kMaxColumns && DESCO_GCM_MAX_COLUMNS % 4 == 0, "column bound");
static_assert(DESCO_GCM_MAX_COLUMNS * DESCO_GCM_MAX_COLUMNS * 8 + GCM_CHUNK * DESCO_GCM_MAX_COLUMNS * 4 <= 160 * 1024,
              "S and one chunk of D must fit the LDS");

struct GcmArgs {
  const int64_t* seg_ptr;
  const int64_t* counts;
  const int64_t* seg_ids;
  int64_t num_segs, num_rows, ld, max_rows;
  int C, CP, dummy;                                  // CP: C rounded up to whole tiles
  int32_t* work;                                     // [num_rows + num_segs][C]; segment i starts at seg_ptr[i] + i
  int64_t* S;
  double* rho;
  double* vec;
  int32_t* status;
  int32_t columns[DESCO_GCM_MAX_COLUMNS];
};

// the rows of segment id (block index -> id); false for a segment that this launch refuses
__device__ __forceinline__ bool gcm_segment(const GcmArgs& p, int64_t& i, int64_t& r0, int& n, int& np) {
  i = p.seg_ids ? p.seg_ids[blockIdx.x] : (int64_t)blockIdx.x;
  if (i < 0 || i >= p.num_segs) return false;        // a bad id: nothing to write to
  r0 = p.seg_ptr[i];
  const int64_t r1 = p.seg_ptr[i + 1], n64 = r1 - r0;
  if (r0 < 0 || n64 < 0 || r1 > p.num_rows || n64 + p.dummy > p.max_rows) {
    if (threadIdx.x == 0 && blockIdx.y == 0) p.status[i] = -1;
    return false;
  }
  n = (int)n64;
  np = n + p.dummy;
  return true;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void gcm_rank_kernel(GcmArgs p) {
  extern __shared__ __attribute__((aligned(16))) int64_t gcm_vals[];         // [np]
  const int tid = threadIdx.x, c = blockIdx.y;
  int64_t i, r0;
  int n, np;
  if (!gcm_segment(p, i, r0, n, np)) return;         // (uniform)
  const int64_t* __restrict__ src = p.counts + p.columns[c];
  for (int l = tid; l < np; l += THREADS) gcm_vals[l] = l < n ? src[(r0 + l) * p.ld] : 1;
  __syncthreads();
  int32_t* __restrict__ dst = p.work + (r0 + i) * p.C + c;
  for (int l = tid; l < np; l += THREADS) {
    const int64_t v = gcm_vals[l];
    int less = 0, equal = 0;
#pragma unroll 4
    for (int j = 0; j < np; ++j) {
      const int64_t w = gcm_vals[j];
      less += w < v;
      equal += w == v;
    }
    dst[(int64_t)l * p.C] = 2 * less + equal - np;
  }
}

__global__ __launch_bounds__(GCM_THREADS) void gcm_matrix_kernel(GcmArgs p) {
  extern __shared__ __attribute__((aligned(16))) int64_t gcm_lds[];
  const int tid = threadIdx.x;
  int64_t i, r0;
  int n, np;
  if (!gcm_segment(p, i, r0, n, np)) return;         // (uniform)
  const int C = p.C, CP = p.CP;
  unsigned long long* S = reinterpret_cast<unsigned long long*>(gcm_lds);    // [CP][CP], the tiles ta <= tb
  int32_t* ch = reinterpret_cast<int32_t*>(gcm_lds + CP * CP);               // [GCM_CHUNK][CP]
  for (int x = tid; x < CP * CP; x += GCM_THREADS) S[x] = 0;
  const int T1 = CP / 4, T = T1 * (T1 + 1) / 2;
  int K = GCM_THREADS / T;                           // threads per tile: each takes the rows r = slice (mod K)
  K = K < 1 ? 1 : K > GCM_CHUNK ? GCM_CHUNK : K;
  const int items = T * K;
  const int32_t* __restrict__ work = p.work + (r0 + i) * C;
  for (int base = 0; base < np; base += GCM_CHUNK) {
    const int rows = np - base < GCM_CHUNK ? np - base : GCM_CHUNK;
    __syncthreads();                                 // the previous chunk is consumed (first pass: S is zero)
    for (int x = tid; x < GCM_CHUNK * CP; x += GCM_THREADS) {
      const int r = x / CP, c = x - r * CP;
      ch[x] = r < rows && c < C ? work[(int64_t)(base + r) * C + c] : 0;
    }
    __syncthreads();
    for (int item = tid; item < items; item += GCM_THREADS) {
      const int tile = item % T, slice = item / T;
      int ta = 0, rem = tile;
      while (rem >= T1 - ta) rem -= T1 - ta, ++ta;
      const int tb = ta + rem;
      int64_t acc[4][4] = {};
      for (int r = slice; r < rows; r += K) {
        const int4 a = *reinterpret_cast<const int4*>(ch + r * CP + 4 * ta);
        const int4 b = *reinterpret_cast<const int4*>(ch + r * CP + 4 * tb);
        const int av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[u][v] += (int64_t)av[u] * (int64_t)bv[v];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (acc[u][v] != 0) atomicAdd(S + (4 * ta + u) * CP + 4 * tb + v, (unsigned long long)acc[u][v]);
    }
  }
  __syncthreads();
  const int64_t P = (int64_t)C * (C - 1) / 2;
  for (int x = tid; x < C * C; x += GCM_THREADS) {
    const int a = x / C, b = x - a * C;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const int64_t s = (int64_t)S[lo * CP + hi];
    if (p.S) p.S[i * C * C + x] = s;
    if (p.rho || (p.vec && a < b)) {
      const double r = a == b ? 1.0 : gcm::rho(s, (int64_t)S[a * CP + a], (int64_t)S[b * CP + b]);
      if (p.rho) p.rho[i * C * C + x] = r;
      if (p.vec && a < b) p.vec[i * P + gcm::pair_index(a, b, C)] = r;
    }
  }
  if (tid == 0) p.status[i] = 0;
}

__global__ __launch_bounds__(GCD_THREADS) void gcd_kernel(const double* __restrict__ x, int64_t Gx,
                                                          const double* __restrict__ y, int64_t Gy, int64_t P,
                                                          double* __restrict__ out, int64_t ldo) {
  __shared__ double xs[GCD_TILE][GCD_CHUNK + 1], ys[GCD_TILE][GCD_CHUNK + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t i0 = (int64_t)blockIdx.y * GCD_TILE, j0 = (int64_t)blockIdx.x * GCD_TILE;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int64_t p0 = 0; p0 < P; p0 += GCD_CHUNK) {
    const int pc = P - p0 < GCD_CHUNK ? (int)(P - p0) : GCD_CHUNK;
    __syncthreads();
    for (int e = tid; e < GCD_TILE * GCD_CHUNK; e += GCD_THREADS) {
      const int r = e / GCD_CHUNK, q = e % GCD_CHUNK;
      xs[r][q] = i0 + r < Gx && q < pc ? x[(i0 + r) * P + p0 + q] : 0.0;
      ys[r][q] = j0 + r < Gy && q < pc ? y[(j0 + r) * P + p0 + q] : 0.0;
    }
    __syncthreads();
    for (int q = 0; q < pc; ++q) {                   // ascending p: the order of the definition
      const double a0 = xs[ty][q], a1 = xs[ty + 16][q], b0 = ys[tx][q], b1 = ys[tx + 16][q];
      const double t00 = a0 - b0, t01 = a0 - b1, t10 = a1 - b0, t11 = a1 - b1;
      acc[0][0] = fma(t00, t00, acc[0][0]);
      acc[0][1] = fma(t01, t01, acc[0][1]);
      acc[1][0] = fma(t10, t10, acc[1][0]);
      acc[1][1] = fma(t11, t11, acc[1][1]);
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int64_t i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i < Gx && j < Gy) out[i * ldo + j] = sqrt(acc[u][v]);
    }
}

template <int THREADS>
int gcm_launch_ranks(const GcmArgs& a, int64_t num_ids, hipStream_t stream) {
  const hipError_t e = size_dynamic_lds<gcm_rank_kernel<THREADS>>(8 * DESCO_GCM_DEV_MAX_ROWS);
  if (e != hipSuccess) return fail((int)e, "desco_graphlet_correlation_dev: cannot size LDS");
  hipLaunchKernelGGL(gcm_rank_kernel<THREADS>, dim3((unsigned)num_ids, (unsigned)a.C), dim3(THREADS),
                     (size_t)(8 * ((a.max_rows + 1) & ~(int64_t)1)), stream, a);
  return launch_status("desco_graphlet_correlation_dev: ranks");
}

}  // namespace desco

using namespace desco;

extern "C" int desco_graphlet_correlation_dev(const int64_t* seg_ptr, int64_t num_segs, int64_t num_rows,
                                              const int64_t* counts, int64_t ld, const int32_t* columns, int C,
                                              int dummy_row, const int64_t* seg_ids, int64_t num_ids,
                                              int64_t max_rows, int32_t* work, int64_t* S_out, double* rho_out,
                                              double* vec_out, int32_t* status, desco_stream_t stream) {
  if (num_segs < 0 || num_rows < 0 || num_ids < 0 || ld < 0 || max_rows < 0)
    return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: negative num_segs, num_rows, num_ids, ld or max_rows");
  if (C < 0 || C > DESCO_GCM_MAX_COLUMNS)
    return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: C is outside 0..128 (DESCO_GCM_MAX_COLUMNS)");
  if (dummy_row != 0 && dummy_row != 1)
    return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: dummy_row must be 0 or 1");
  if (!seg_ids) num_ids = num_segs;
  if (num_ids == 0 || C == 0) return 0;
  if (max_rows > DESCO_GCM_DEV_MAX_ROWS)
    return fail(DESCO_EINVAL,
                "desco_graphlet_correlation_dev: a segment's rows, dummy row included, exceed "
                "DESCO_GCM_DEV_MAX_ROWS (20480); use desco_graphlet_correlation for it");
  if (num_ids > INT32_MAX) return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: num_ids is above 2^31 - 1");
  if (!seg_ptr) return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: seg_ptr is null");
  if (!columns) return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: columns is null");
  if (!work) return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: work is null");
  if (!status) return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: status is null");
  if (num_rows > 0 && !counts) return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: counts is null");
  if (mis8(seg_ptr) || mis8(counts) || mis8(seg_ids) || mis8(S_out) || mis8(rho_out) || mis8(vec_out))
    return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: a 64-bit array is not 8-byte aligned");
  GcmArgs a{};
  for (int c = 0; c < C; ++c) {
    if (columns[c] < 0 || columns[c] >= ld)
      return fail(DESCO_EINVAL, "desco_graphlet_correlation_dev: a column index is outside 0..ld-1");
    a.columns[c] = columns[c];
  }
  a.seg_ptr = seg_ptr, a.counts = counts, a.seg_ids = seg_ids;
  a.num_segs = num_segs, a.num_rows = num_rows, a.ld = ld, a.max_rows = max_rows;
  a.C = C, a.CP = (C + 3) & ~3, a.dummy = dummy_row;
  a.work = work, a.S = S_out, a.rho = rho_out, a.vec = vec_out, a.status = status;
  hipStream_t s = (hipStream_t)stream;
  // one wave per (segment, column) where the launch's segments are small (DESCO_GCM_WAVE_ROWS), four above
  if (const int rc = max_rows <= DESCO_GCM_WAVE_ROWS ? gcm_launch_ranks<64>(a, num_ids, s)
                                                     : gcm_launch_ranks<256>(a, num_ids, s))
    return rc;
  const int lds_max = DESCO_GCM_MAX_COLUMNS * DESCO_GCM_MAX_COLUMNS * 8 + GCM_CHUNK * DESCO_GCM_MAX_COLUMNS * 4;
  const hipError_t e = size_dynamic_lds<gcm_matrix_kernel>(lds_max);
  if (e != hipSuccess) return fail((int)e, "desco_graphlet_correlation_dev: cannot size LDS");
  hipLaunchKernelGGL(gcm_matrix_kernel, dim3((unsigned)num_ids), dim3(GCM_THREADS),
                     (size_t)(a.CP * a.CP * 8 + GCM_CHUNK * a.CP * 4), s, a);
  return launch_status("desco_graphlet_correlation_dev");
}

extern "C" int desco_gcd_matrix_dev(const double* x, int64_t Gx, const double* y, int64_t Gy, int64_t P, double* out,
                                    int64_t ldo, desco_stream_t stream) {
  if (Gx < 0 || Gy < 0 || P < 0) return fail(DESCO_EINVAL, "desco_gcd_matrix_dev: negative Gx, Gy or P");
  if (Gx == 0 || Gy == 0) return 0;
  if (ldo < Gy) return fail(DESCO_EINVAL, "desco_gcd_matrix_dev: ldo is below Gy");
  if (!out) return fail(DESCO_EINVAL, "desco_gcd_matrix_dev: out is null");
  if (P > 0 && (!x || !y)) return fail(DESCO_EINVAL, "desco_gcd_matrix_dev: x or y is null");
  if (mis8(x) || mis8(y) || mis8(out))
    return fail(DESCO_EINVAL, "desco_gcd_matrix_dev: an array is not 8-byte aligned");
  const int64_t bx = (Gy + GCD_TILE - 1) / GCD_TILE, by = (Gx + GCD_TILE - 1) / GCD_TILE;
  if (bx > INT32_MAX || by > 65535)
    return fail(DESCO_EINVAL, "desco_gcd_matrix_dev: more than 2097120 rows of x (or 2^36 of y) in one call");
  hipLaunchKernelGGL(gcd_kernel, dim3((unsigned)bx, (unsigned)by), dim3(GCD_THREADS), 0, (hipStream_t)stream, x, Gx, y,
                     Gy, P, out, ldo);
  return launch_status("desco_gcd_matrix_dev");
}
