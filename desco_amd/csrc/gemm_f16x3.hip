// fp32-accurate GEMM on the fp16 matrix pipe in THREE products ("f16x3"): every fp32 operand is scaled by a
// power of two and split into two fp16 terms, x s = hi + lo (hi = rne(x s), lo = rne(x s - hi): 22 significand
// bits), and
//     a*b ~= (hi*hi + hi*lo + lo*hi) / (s_a s_b)                      (dropped: lo*lo, 2^-22 |a||b| at worst)
// accumulates in fp32 on v_mfma_f32_32x32x16_f16.  Against the six-product bf16 form of gemm_split.hip: half the
// MFMAs, two operand planes instead of three (LDS image and fragment reads -33 %), 3 VALU per pair for the split
// instead of 9.  Measured error (tools/micro/f16x3_probe.hip, K = 576): rms 1.5e-8 of sum|a||b| against 2.4e-8 for
// v_mfma_f32_16x16x4_f32 and 2.0e-8 for bf16x6.
//
// fp16 has a 5-bit exponent, so the scales carry the range:
//   * weights: ONE power of two per matrix (largest |w| -> [2^14, 2^15)), applied when the planes are made
//     (desco_split_f16x2_f32), its inverse kept on the device next to the planes;
//   * activations: one power of two PER ROW over the whole K extent (largest |a| of the row -> [2^14, 2^15)), so a
//     row's products share one accumulator; derived from a per-row bound that either a pre-pass over A provides
//     (row_scale_kernel: HBM-bound, A once) or the kernel that wrote A, and undone in the epilogue together with the
//     weight scale (exact: powers of two).
// An element 2^-17 below its row maximum keeps 22 bits; smaller ones degrade gradually (lo subnormal) down to an
// absolute error of 2^-40 of the row maximum -- below the fp32 rounding error of the row's dot products.
//
// Same contract and tile structure as desco_gemm_bf16x6_f32 (gemm_split.hip: 128 x 64 WN block tile, 2x2 waves,
// K chunks of 32, A two chunks ahead, XCD-aware tile order, swizzled 64-byte plane rows, LDS-staged epilogue).
#include "gemm_f16x3.hpp"

namespace desco {

// per-row bound of the A operand: max_k |A[i, k]| (the kernel turns it into the power of two s with s * bound in
// [2^14, 2^15)).  16 lanes per row, float4 loads.  A kernel that WRITES A can leave the same array instead (the SHMP
// layer's canonical launches do, for the anchor operand): any value >= the row's largest magnitude will do.
__global__ __launch_bounds__(256) void row_scale_kernel(const float* __restrict__ a1, int64_t lda1, int k1,
                                                        const float* __restrict__ a2, int64_t lda2, int k2,
                                                        int64_t m, float* __restrict__ out) {
  const int lane16 = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int64_t r = row < m ? row : m - 1;
  float mx = 0.f;
  const float* p1 = a1 + r * lda1;
  for (int k = 4 * lane16; k < k1; k += 64) {
    const float4 v = *reinterpret_cast<const float4*>(p1 + k);
    mx = fmaxf(fmaxf(mx, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
  }
  if (k2 > 0) {
    const float* p2 = a2 + r * lda2;
    for (int k = 4 * lane16; k < k2; k += 64) {
      const float4 v = *reinterpret_cast<const float4*>(p2 + k);
      mx = fmaxf(fmaxf(mx, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane16 == 0 && row < m) out[row] = mx;
}

// BM = 128 rows per block tile (4 waves, two blocks per CU), WN = 3, 2, 1 column tiles of 64
template <int WN, int BM>
__global__ __launch_bounds__(2 * BM) __attribute__((amdgpu_waves_per_eu(2))) void gemm_f16x3_kernel(GemmF16Args g, int64_t gm,
                                                                                                   int ny) {
  constexpr int BN = 64 * WN, BPLANE = BN * FST, APLANE = BM * FST;
  constexpr int EW = 32 * WN;
  constexpr int STAGE = 2 * APLANE + 2 * BPLANE;                  // shorts (main loop: A and W chunk planes)
  constexpr int EPI = (BM / 32) * 32 * EW * 2;                    // shorts (fp32 image)
  constexpr int BODY = STAGE > EPI ? STAGE : EPI;
  extern __shared__ __attribute__((aligned(16))) short lds[];
  float* rinv = reinterpret_cast<float*>(lds + BODY);   // [BM] 1 / (row scale * weight scale)

  const int64_t id = blockIdx.x;
  const int64_t local = id >> 3;
  const int64_t mt = (local / ny) * 8 + (id & 7);
  if (mt >= gm) return;
  const int n0 = (int)(local % ny) * BN;
  const int64_t m0 = mt * BM;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  if (tid < BM) {
    const int64_t rr = m0 + tid < g.m ? m0 + tid : g.m - 1;
    rinv[tid] = pow2_inverse(f16_scale_for(g.row_scale[rr])) * g.w_scale[1];
  }
  f32x16 acc[2][WN];
  gemm_f16x3_main_loop<WN, BM>(g, lds, m0, n0, acc);

  // Epilogue (as gemm_split.hip): each 32-row half of the wave tile through a wave-private [32][32 WN] fp32 LDS
  // image -> 16-byte row-contiguous nontemporal stores.  The scales are undone here: row = (reg & 3) + 8 (reg >> 2)
  // + 4 (lane >> 5), so the four rows of a register quad are one 16-byte read of rinv.
  __syncthreads();                       // every wave is done with the last chunk's fragments
  float* st = reinterpret_cast<float*>(lds) + wave * (32 * EW);
  const int col = lane & 31;
  const bool wide = ((reinterpret_cast<uintptr_t>(g.c) & 15) == 0) && ((g.ldc & 3) == 0);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t grow0 = m0 + wr * 64 + 32 * i;
    const float* ri = rinv + wr * 64 + 32 * i + 4 * (lane >> 5);
    const float4 q0 = *reinterpret_cast<const float4*>(ri), q1 = *reinterpret_cast<const float4*>(ri + 8);
    const float4 q2 = *reinterpret_cast<const float4*>(ri + 16), q3 = *reinterpret_cast<const float4*>(ri + 24);
    const float rv[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int gcol = n0 + wc * EW + 32 * j + col;
      float wsv[4] = {0.f, 0.f, 0.f, 0.f};
      for (int q = 0; q < g.ns; ++q) wsv[q] = g.ws[(int64_t)q * g.n + gcol];
      const float b_single = (g.bias && g.bias_rows == 1) ? g.bias[gcol] : 0.f;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        const int64_t grow = grow0 + row < g.m ? grow0 + row : g.m - 1;
        float v = acc[i][j][reg] * rv[reg];
        if (g.bias) {
          if (g.bias_rows == 1)
            v += b_single;
          else
            v += g.bias[(grow % g.bias_rows) * g.n + gcol];
        }
        for (int q = 0; q < g.ns; ++q) v += g.s[grow * g.ns + q] * wsv[q];
        st[row * EW + 32 * j + col] = apply_act(v, g.act, g.slope);
      }
    }
    __syncthreads();
    float* crow = g.c + n0 + wc * EW;
#pragma unroll
    for (int p = 0; p < 4 * WN; ++p) {
      const int idx = lane + 64 * p;               // float4 index in the image: row idx / (8 WN)
      const int row = idx / (8 * WN), c4 = idx % (8 * WN);
      const float4 v = *reinterpret_cast<const float4*>(st + 4 * idx);
      const int64_t grow = grow0 + row;
      if (grow < g.m) {
        float* o = crow + grow * g.ldc + 4 * c4;
        if (wide) {
          __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4*>(o));
        } else {
          o[0] = v.x;
          o[1] = v.y;
          o[2] = v.z;
          o[3] = v.w;
        }
      }
    }
    if (i == 0) __syncthreads();
  }
}

// ---- weight planes -------------------------------------------------------------------------------------------------
// one block: scale[0] = the power of two s with s * max|w| in [2^14, 2^15), scale[1] = 1 / s
__global__ __launch_bounds__(1024) void f16_weight_scale_kernel(const float* __restrict__ w, int64_t count,
                                                                float* __restrict__ scale) {
  __shared__ float part[16];
  float mx = 0.f;
  for (int64_t i = threadIdx.x; i < count; i += 1024) mx = fmaxf(mx, fabsf(w[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, part[i]);
    const float s = f16_scale_for(mx);
    scale[0] = s;
    scale[1] = pow2_inverse(s);
  }
}

// w[count] -> planes[2][count] (hi, lo fp16 bit patterns of scale * w)
__global__ __launch_bounds__(256) void split_f16x2_kernel(const float* __restrict__ w, int64_t count,
                                                          const float* __restrict__ scale,
                                                          short* __restrict__ planes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  uint32_t hi, lo;
  split2_f16x2(w[i] * scale[0], 0.f, hi, lo);
  planes[i] = (short)(hi & 0xffffu);
  planes[count + i] = (short)(lo & 0xffffu);
}

template <int WN>
static int launch_gemm_f16x3(const GemmF16Args& g, hipStream_t stream) {
  constexpr int BM = 128, BN = 64 * WN;
  constexpr size_t stage_bytes = (size_t)(2 * BM * FST + 2 * BN * FST) * sizeof(short);
  constexpr size_t epi_bytes = (size_t)(BM / 32) * 32 * 32 * WN * sizeof(float);
  constexpr size_t lds_bytes = (stage_bytes > epi_bytes ? stage_bytes : epi_bytes) + BM * sizeof(float);
  if (hipError_t e = size_dynamic_lds<gemm_f16x3_kernel<WN, BM>>((int)lds_bytes); e != hipSuccess)
    return fail((int)e, "desco_gemm_f16x3_f32: cannot size LDS");
  const int64_t gm = (g.m + BM - 1) / BM;
  const int ny = g.n / BN;
  const int64_t blocks = ((gm + 7) / 8) * 8 * ny;
  if (blocks > INT32_MAX) return fail(DESCO_EINVAL, "desco_gemm_f16x3_f32: m too large");
  hipLaunchKernelGGL((gemm_f16x3_kernel<WN, BM>), dim3((unsigned)blocks), dim3(2 * BM), lds_bytes, stream, g, gm, ny);
  return launch_status("desco_gemm_f16x3_f32");
}

}  // namespace desco

using namespace desco;

extern "C" int desco_row_absmax_f32(const float* a1, int64_t lda1, int k1, const float* a2, int64_t lda2, int k2,
                                   int64_t m, float* row_scale, desco_stream_t stream) {
  if (m == 0) return 0;
  if (m < 0 || !a1 || !row_scale || k1 <= 0 || k1 % 4 || k2 < 0 || k2 % 4 || (k2 > 0 && !a2) || lda1 % 4 ||
      (k2 > 0 && lda2 % 4) || mis16(a1) || (k2 > 0 && mis16(a2)))
    return fail(DESCO_EINVAL, "desco_row_absmax_f32: bad argument (k % 4, 16-byte alignment)");
  const int64_t blocks = (m + 15) / 16;
  if (blocks > INT32_MAX) return fail(DESCO_EINVAL, "desco_row_absmax_f32: m too large");
  hipLaunchKernelGGL(row_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a1, lda1, k1, a2,
                     lda2, k2, m, row_scale);
  return launch_status("desco_row_absmax_f32");
}

extern "C" int desco_gemm_f16x3_f32(const float* a1, int64_t lda1, int k1, const float* a2, int64_t lda2, int k2,
                                    const int16_t* w_planes, const float* w_scale, int n, const float* bias,
                                    int bias_rows, const float* s, int ns, const float* ws, int act, float slope,
                                    float* c, int64_t ldc, int64_t m, const float* row_scale,
                                    desco_stream_t stream) {
  if (m == 0) return 0;
  if (m < 0 || !a1 || !w_planes || !w_scale || !row_scale || !c || k1 <= 0 || k1 % FBK || k2 < 0 || k2 % FBK ||
      n <= 0 || n % 64 || (k2 > 0 && !a2) || ns < 0 || ns > 4 || (ns > 0 && (!s || !ws)) ||
      (bias && bias_rows < 1) || lda1 % 4 || (k2 > 0 && lda2 % 4) || mis16(a1) || (k2 > 0 && mis16(a2)) ||
      mis16(w_planes))
    return fail(DESCO_EINVAL, "desco_gemm_f16x3_f32: bad argument (k%32, n%64, 16-byte alignment)");
  GemmF16Args g{a1, lda1, k1, a2, lda2, k2, reinterpret_cast<const short*>(w_planes), w_scale, n, bias,
                bias ? bias_rows : 1, s, ns, ws, act, slope, c, ldc, m, row_scale};
  hipStream_t st = (hipStream_t)stream;
  if (n % 192 == 0) return launch_gemm_f16x3<3>(g, st);
  if (n % 128 == 0) return launch_gemm_f16x3<2>(g, st);
  return launch_gemm_f16x3<1>(g, st);
}

extern "C" int desco_split_f16x2_f32(const float* w, int64_t count, int16_t* planes, float* scale,
                                     desco_stream_t stream) {
  if (count == 0) return 0;
  if (count < 0 || !w || !planes || !scale) return fail(DESCO_EINVAL, "desco_split_f16x2_f32: bad argument");
  const int64_t blocks = (count + 255) / 256;
  if (blocks > INT32_MAX) return fail(DESCO_EINVAL, "desco_split_f16x2_f32: count too large");
  hipLaunchKernelGGL(f16_weight_scale_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, w, count, scale);
  hipLaunchKernelGGL(split_f16x2_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, count, scale,
                     reinterpret_cast<short*>(planes));
  return launch_status("desco_split_f16x2_f32");
}
