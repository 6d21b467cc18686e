// One layer of a PLAIN (homogeneous) GIN or GCN neighborhood model, fused (--neigh_conv_type GIN / GCN).
// The host pads every operand with zeros to the padded width Wp = 64 ceil(H / 64) in {64, 128, 192, 256}; the kernel
// sees Wp only.
//
//  * plain_layer_kernel<WP, NM>: for rows r in [row0, row0 + num_rows) of a plain CSR (one entry per row),
//      z[r] = sum_{e in [rowptr[r], rowptr[r + 1])} x[col[e]]  (fp32, CSR order)  + s x[r]       (s = *self_scale, or 0)
//      h    = z W1 + b1
//      h    = relu(h) W2 + b2                                                     (NM == 2: GIN's two-Linear MLP)
//      y    = relu(h)
//    One 256-thread workgroup per 64 consecutive rows.  Sixteen lane groups of sixteen lanes gather the tile's rows
//    (float4 per lane per 64 columns, four neighbours in flight), scale each row by its own power of two and split it
//    into fp16 hi / lo planes in LDS [64][Wp + 8]; the four waves run the three-product f16x3 form
//    (v_mfma_f32_16x16x32_f16: lo*hi, hi*lo, hi*hi, fp32 accumulation) against the pre-split weight planes read from
//    L2; wave w owns output columns [w Wp / 4, (w + 1) Wp / 4) of all 64 rows.  For the second product relu(h) never
//    leaves the workgroup: the waves exchange their row maxima through LDS, every row gets a fresh power-of-two scale,
//    is split again and written back into the same LDS operand image, and the W2 product runs on it.  A row whose
//    relu(h) is all zero has scale 1 and gives relu(b2) exactly.  A row's scales are its own: a result depends neither
//    on the tiling nor on row0.
#include "tu_no_packed_f32_begin.hpp"
#include "common_device.hpp"

namespace desco {

namespace {

constexpr int PL_ROWS = 64;

struct PlainLayerArgs {
  const float* x;
  int64_t ldx;
  const int32_t* rowptr;   // plain CSR: rowptr[r] .. rowptr[r + 1]
  const int32_t* col;
  const float* self_scale; // device scalar s, or nullptr (0)
  int64_t row0, num_rows;
  const short* w1;         // planes [2][Wp][Wp] of W1^T (n-major)
  const float* w1_scale;   // {scale, 1 / scale}
  const float* b1;         // [Wp]
  const short* w2;         // NM == 2 only
  const float* w2_scale;
  const float* b2;
  float* out;              // rows row0 .. (absolute), or nullptr
  int64_t ldo;
  float* out2;             // row r at out2[(r - out2_row0) * ld2] for r >= out2_row0, or nullptr
  int64_t ld2;
  int64_t out2_row0;
};

__device__ __forceinline__ float pl_absmax4(const float4 v) {
  return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}

__device__ __forceinline__ void pl_add(float4& a, const float4 b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// a + s x with the product rounded on its own (the un-fused composition's eps x term is a tensor of its own)
__device__ __forceinline__ float pl_mul_then_add(const float a, const float s, const float x) {
#pragma clang fp contract(off)
  const float p = s * x;
  return a + p;
}

// tmp = A (LDS image, hi / lo planes) times the weight planes w [2][WP][WP] in the three-product form
template <int WP>
__device__ __forceinline__ void pl_product(const short* A, const short* __restrict__ w, const int wave, const int ar,
                                           const int kq, f32x4 (&tmp)[4][WP / 64]) {
  constexpr int AST = WP + 8, APLANE = PL_ROWS * AST, NC = WP / 64;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) tmp[t][j][e] = 0.f;
#pragma unroll 2
  for (int s = 0; s < WP / 32; ++s) {
    f16x8 ah[4], al[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const short* ap = A + (16 * t + ar) * AST + 32 * s + 8 * kq;
      ah[t] = *reinterpret_cast<const f16x8*>(ap);
      al[t] = *reinterpret_cast<const f16x8*>(ap + APLANE);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int n = wave * (WP / 4) + 16 * j + ar;
      const short* bp = w + (int64_t)n * WP + 32 * s + 8 * kq;
      const f16x8 bh = *reinterpret_cast<const f16x8*>(bp);
      const f16x8 bl = *reinterpret_cast<const f16x8*>(bp + WP * WP);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        tmp[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[t], bh, tmp[t][j], 0, 0, 0);   // smallest terms first
        tmp[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bl, tmp[t][j], 0, 0, 0);
        tmp[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bh, tmp[t][j], 0, 0, 0);
      }
    }
  }
}

template <int WP, int NM>
__global__ __launch_bounds__(256) void plain_layer_kernel(const PlainLayerArgs a) {
  constexpr int AST = WP + 8;               // A image row stride in halves (rows 4 banks apart)
  constexpr int APLANE = PL_ROWS * AST;     // halves per plane
  constexpr int NC = WP / 64;               // float4 pieces per lane per row; also 16-column tiles per wave
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* A = lds;                                                  // planes hi, lo [64][AST]
  float* rinv = reinterpret_cast<float*>(lds + 2 * APLANE);        // [64] 1 / row scale of the current operand
  float* rmax = rinv + PL_ROWS;                                    // [4 waves][64] row maxima of relu(h)

  const int tid = (int)__builtin_amdgcn_workitem_id_x(), lane = tid & 63, wave = tid >> 6;
  const int l16 = tid & 15, grp = tid >> 4;
  const int ar = lane & 15, kq = lane >> 4;
  const int64_t m0 = a.row0 + (int64_t)__builtin_amdgcn_workgroup_id_x() * PL_ROWS;
  const int64_t rend = a.row0 + a.num_rows;
  const float s = a.self_scale ? *a.self_scale : 0.f;

  // ---- gather, self term, scaled split into the A image -------------------------------------------------------------
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int r = grp + 16 * k;
    int64_t row = m0 + r;
    row = row < rend ? row : rend - 1;
    float4 v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int e0 = a.rowptr[row], e1 = a.rowptr[row + 1];
    for (int e = e0; e < e1; e += 4) {
      const int cnt = e1 - e;
      const int64_t j0 = a.col[e];
      const int64_t j1 = cnt > 1 ? a.col[e + 1] : j0, j2 = cnt > 2 ? a.col[e + 2] : j0, j3 = cnt > 3 ? a.col[e + 3] : j0;
      float4 u[4][NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int64_t off = 64 * c + 4 * l16;
        u[0][c] = *reinterpret_cast<const float4*>(a.x + j0 * a.ldx + off);
        u[1][c] = *reinterpret_cast<const float4*>(a.x + j1 * a.ldx + off);
        u[2][c] = *reinterpret_cast<const float4*>(a.x + j2 * a.ldx + off);
        u[3][c] = *reinterpret_cast<const float4*>(a.x + j3 * a.ldx + off);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {        // CSR order, one neighbour after the other
        pl_add(v[c], u[0][c]);
        if (cnt > 1) pl_add(v[c], u[1][c]);
        if (cnt > 2) pl_add(v[c], u[2][c]);
        if (cnt > 3) pl_add(v[c], u[3][c]);
      }
    }
    if (s != 0.f) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float4 u = *reinterpret_cast<const float4*>(a.x + row * a.ldx + 64 * c + 4 * l16);
        v[c].x = pl_mul_then_add(v[c].x, s, u.x);
        v[c].y = pl_mul_then_add(v[c].y, s, u.y);
        v[c].z = pl_mul_then_add(v[c].z, s, u.z);
        v[c].w = pl_mul_then_add(v[c].w, s, u.w);
      }
    }
    float mx = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) mx = fmaxf(mx, pl_absmax4(v[c]));
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float sc = f16_scale_for(mx);
    if (l16 == 0) rinv[r] = pow2_inverse(sc);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      uint32_t h0, lo0, h1, lo1;
      split2_f16x2(v[c].x * sc, v[c].y * sc, h0, lo0);
      split2_f16x2(v[c].z * sc, v[c].w * sc, h1, lo1);
      const int kk = 64 * c + 4 * l16;
      *reinterpret_cast<uint2*>(A + r * AST + kk) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(A + APLANE + r * AST + kk) = make_uint2(lo0, lo1);
    }
  }
  __syncthreads();

  // ---- h = z W1 + b1 ------------------------------------------------------------------------------------------------
  f32x4 acc[4][NC];
  pl_product<WP>(A, a.w1, wave, ar, kq, acc);
  {
    const float winv = a.w1_scale[1];
    float bn[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) bn[j] = a.b1[wave * (WP / 4) + 16 * j + ar];
    // undo the scales (C/D layout: column = lane & 15, row = 4 (lane >> 4) + e)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float f = rinv[16 * t + 4 * kq + e] * winv;
#pragma unroll
        for (int j = 0; j < NC; ++j) acc[t][j][e] = acc[t][j][e] * f + bn[j];
      }
  }

  if constexpr (NM == 2) {
    // ---- relu(h) back into the operand image: row maxima across the four waves, fresh scales, new split -------------
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float mx = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          acc[t][j][e] = fmaxf(acc[t][j][e], 0.f);
          mx = fmaxf(mx, acc[t][j][e]);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));     // the 16 lanes of one kq
        if (ar == 0) rmax[wave * PL_ROWS + 16 * t + 4 * kq + e] = mx;
      }
    __syncthreads();        // the maxima are written; every wave is done with A and rinv of the first product
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 16 * t + 4 * kq + e;
        const float mx = fmaxf(fmaxf(rmax[r], rmax[PL_ROWS + r]), fmaxf(rmax[2 * PL_ROWS + r], rmax[3 * PL_ROWS + r]));
        const float sc = f16_scale_for(mx);
        if (wave == 0 && ar == 0) rinv[r] = pow2_inverse(sc);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const int n = wave * (WP / 4) + 16 * j + ar;
          uint32_t hi, lo;
          split2_f16x2(acc[t][j][e] * sc, 0.f, hi, lo);
          A[r * AST + n] = (short)(hi & 0xffffu);
          A[APLANE + r * AST + n] = (short)(lo & 0xffffu);
        }
      }
    __syncthreads();

    // ---- h = relu(h) W2 + b2 ----------------------------------------------------------------------------------------
    pl_product<WP>(A, a.w2, wave, ar, kq, acc);
    const float winv = a.w2_scale[1];
    float bn[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) bn[j] = a.b2[wave * (WP / 4) + 16 * j + ar];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float f = rinv[16 * t + 4 * kq + e] * winv;
#pragma unroll
        for (int j = 0; j < NC; ++j) acc[t][j][e] = acc[t][j][e] * f + bn[j];
      }
  }

  // ---- epilogue: relu, stores ---------------------------------------------------------------------------------------
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int n = wave * (WP / 4) + 16 * j + ar;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t row = m0 + 16 * t + 4 * kq + e;
        if (row < rend) {
          const float y = fmaxf(acc[t][j][e], 0.f);
          if (a.out) a.out[row * a.ldo + n] = y;
          if (a.out2 && row >= a.out2_row0) a.out2[(row - a.out2_row0) * a.ld2 + n] = y;
        }
      }
    }
  }
}

template <int WP, int NM>
int launch_plain_layer(const PlainLayerArgs& g, hipStream_t stream) {
  const size_t lds = (size_t)2 * PL_ROWS * (WP + 8) * sizeof(short) + 5 * PL_ROWS * sizeof(float);
  if (lds > 65536)
    if (hipError_t e = size_dynamic_lds<plain_layer_kernel<WP, NM>>((int)lds); e != hipSuccess)
      return fail((int)e, "desco_plain_layer_f16x3_f32: cannot size LDS");
  const int64_t blocks = (g.num_rows + PL_ROWS - 1) / PL_ROWS;
  hipLaunchKernelGGL((plain_layer_kernel<WP, NM>), dim3((unsigned)blocks), dim3(256), lds, stream, g);
  return launch_status("desco_plain_layer_f16x3_f32");
}

template <int WP>
int launch_plain_layer_m(const PlainLayerArgs& g, int num_mats, hipStream_t stream) {
  return num_mats == 2 ? launch_plain_layer<WP, 2>(g, stream) : launch_plain_layer<WP, 1>(g, stream);
}

}  // namespace

}  // namespace desco

using namespace desco;

extern "C" int desco_plain_layer_f16x3_f32(const float* x, int64_t ldx, const int32_t* rowptr, const int32_t* col,
                                           const float* self_scale, int64_t row0, int64_t num_rows, int width,
                                           int num_mats, const int16_t* w1_planes, const float* w1_scale,
                                           const float* b1, const int16_t* w2_planes, const float* w2_scale,
                                           const float* b2, float* out, int64_t ldo, float* out2, int64_t ld2,
                                           int64_t out2_row0, desco_stream_t stream) {
  if (row0 < 0 || num_rows < 0 || out2_row0 < 0 || !(num_mats == 1 || num_mats == 2) ||
      !(width == 64 || width == 128 || width == 192 || width == 256))
    return fail(DESCO_EINVAL, "desco_plain_layer_f16x3_f32: bad argument (row0, num_rows, out2_row0 >= 0, num_mats in "
                              "{1, 2}, width in {64, 128, 192, 256})");
  if (!x || !rowptr || !col || !w1_planes || !w1_scale || !b1 || (!out && !out2) ||
      (num_mats == 2 && (!w2_planes || !w2_scale || !b2)))
    return fail(DESCO_EINVAL, "desco_plain_layer_f16x3_f32: bad argument (a required pointer is NULL, or neither out "
                              "nor out2 is given)");
  if (mis16(x) || mis16(w1_planes) || (num_mats == 2 && mis16(w2_planes)) || ldx % 4 || ldx < width ||
      (out && ldo < width) || (out2 && ld2 < width))
    return fail(DESCO_EINVAL, "desco_plain_layer_f16x3_f32: bad argument (x and the planes 16-byte aligned, "
                              "ldx % 4 == 0, leading dimensions >= width)");
  if (out == x || out2 == x)
    return fail(DESCO_EINVAL, "desco_plain_layer_f16x3_f32: bad argument (out and out2 must not be x)");
  if ((num_rows + PL_ROWS - 1) / PL_ROWS > INT32_MAX)
    return fail(DESCO_EINVAL, "desco_plain_layer_f16x3_f32: too many rows");
  if (num_rows == 0) return 0;
  PlainLayerArgs a{x, ldx, rowptr, col, self_scale, row0, num_rows, reinterpret_cast<const short*>(w1_planes), w1_scale,
                   b1, reinterpret_cast<const short*>(w2_planes), w2_scale, b2, out, ldo, out2, ld2, out2_row0};
  hipStream_t st = (hipStream_t)stream;
  switch (width) {
    case 64: return launch_plain_layer_m<64>(a, num_mats, st);
    case 128: return launch_plain_layer_m<128>(a, num_mats, st);
    case 192: return launch_plain_layer_m<192>(a, num_mats, st);
    default: return launch_plain_layer_m<256>(a, num_mats, st);
  }
}

#include "tu_no_packed_f32_end.hpp"
