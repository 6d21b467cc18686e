// Kernels of the neighborhood models of other widths than 64 (--neigh_hidden_dim != 64).  The host pads
// every H-wide block of the folded operands with zeros to the padded width Wp = 64 ceil(H / 64) in {64, 128, 192, 256},
// so the padded channels stay exactly 0; these kernels see Wp only.
//
//  * shmp_layer_wide_kernel<WP, S>: one SAGE layer of one node-type group, fused:
//      out = relu([sum slot 0 | ... | sum slot S-1 | x_self] Wt + b)       Wt [(S+1) Wp, Wp], fp16 planes of Wt^T
//    One 256-thread workgroup per 64 consecutive rows (not persistent).  The K dimension (up to 5 * 256) is worked one
//    Wp-wide block at a time (slot 0, ..., slot S-1, then the self row): sixteen lane groups of sixteen lanes gather the
//    block's 64 rows (float4 per lane per 64 columns; every row's neighbours summed in CSR order, four rows in flight),
//    scale each (row, block) by its own power of two and split it into fp16 hi / lo planes in LDS [64][Wp + 8]; the
//    waves then run the three-product f16x3 form (v_mfma_f32_16x16x32_f16: lo*hi, hi*lo, hi*hi, fp32 accumulation)
//    against the pre-split weight planes read from L2, and undo the block's scales into their fp32 accumulators.  Wave
//    w owns output columns [w Wp / 4, (w + 1) Wp / 4) of all 64 rows.  A result does not depend on the tiling.
//  * csr_gather_sum_wide_kernel: out[v] = sum over virtual row v of x[vcol[e], 0:width] (CSR order), one wave per
//    virtual row, one float4 column piece per lane.
//  * count_head_wide_kernel: desco_count_head_f32's separable count head for hidden widths up to 1024.
#include "tu_no_packed_f32_begin.hpp"
#include "common_device.hpp"

namespace desco {

namespace {

constexpr int SW_ROWS = 64;

struct WideLayerArgs {
  const float* x;
  int64_t ldx;
  const int32_t* vrowptr;
  const int32_t* vcol;
  int vslots;              // virtual rows per row in the CSR (>= S: the first S are used)
  int64_t row0, num_rows;
  const short* w;          // planes [2][Wp][(S+1) Wp]
  const float* w_scale;    // {scale, 1 / scale}
  const float* bias;       // [Wp]
  float* out;              // rows row0 .. (absolute), or nullptr
  int64_t ldo;
  float* out2;             // rows 0 .. num_rows - 1 (relative), or nullptr
  int64_t ld2;
};

__device__ __forceinline__ float sw_absmax4(const float4 v) {
  return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}

__device__ __forceinline__ void sw_add(float4& a, const float4 b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

template <int WP, int S>
__global__ __launch_bounds__(256) void shmp_layer_wide_kernel(const WideLayerArgs a) {
  constexpr int AST = WP + 8;               // A image row stride in halves (rows 4 banks apart)
  constexpr int APLANE = SW_ROWS * AST;     // halves per plane
  constexpr int NC = WP / 64;               // float4 pieces per lane per row; also 16-column tiles per wave
  constexpr int K = (S + 1) * WP;
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* A = lds;                                                  // planes hi, lo [64][AST]
  float* rinv = reinterpret_cast<float*>(lds + 2 * APLANE);        // [64] 1 / row scale of the current block

  const int tid = (int)__builtin_amdgcn_workitem_id_x(), lane = tid & 63, wave = tid >> 6;
  const int l16 = tid & 15, grp = tid >> 4;
  const int ar = lane & 15, kq = lane >> 4;
  const int64_t m0 = a.row0 + (int64_t)__builtin_amdgcn_workgroup_id_x() * SW_ROWS;
  const int64_t rend = a.row0 + a.num_rows;
  const float winv = a.w_scale[1];

  f32x4 acc[4][NC];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][j][e] = 0.f;

#pragma unroll 1
  for (int b = 0; b <= S; ++b) {
    // ---- gather (or self row) of block b, scaled split into the A image --------------------------------------------
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const int r = grp + 16 * k;
      int64_t row = m0 + r;
      row = row < rend ? row : rend - 1;
      float4 v[NC];
      if (b < S) {
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int e0 = a.vrowptr[row * a.vslots + b], e1 = a.vrowptr[row * a.vslots + b + 1];
        for (int e = e0; e < e1; e += 4) {
          const int cnt = e1 - e;
          const int64_t j0 = a.vcol[e];
          const int64_t j1 = cnt > 1 ? a.vcol[e + 1] : j0, j2 = cnt > 2 ? a.vcol[e + 2] : j0,
                        j3 = cnt > 3 ? a.vcol[e + 3] : j0;
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
            sw_add(v[c], u[0][c]);
            if (cnt > 1) sw_add(v[c], u[1][c]);
            if (cnt > 2) sw_add(v[c], u[2][c]);
            if (cnt > 3) sw_add(v[c], u[3][c]);
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = *reinterpret_cast<const float4*>(a.x + row * a.ldx + 64 * c + 4 * l16);
      }
      float mx = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) mx = fmaxf(mx, sw_absmax4(v[c]));
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

    // ---- block product in the three-product fp16 form ---------------------------------------------------------------
    f32x4 tmp[4][NC];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) tmp[t][j][e] = 0.f;
    const short* wb = a.w + (int64_t)b * WP + 8 * kq;
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
        const short* bp = wb + (int64_t)n * K + 32 * s;
        const f16x8 bh = *reinterpret_cast<const f16x8*>(bp);
        const f16x8 bl = *reinterpret_cast<const f16x8*>(bp + (int64_t)WP * K);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          tmp[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[t], bh, tmp[t][j], 0, 0, 0);   // smallest terms first
          tmp[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bl, tmp[t][j], 0, 0, 0);
          tmp[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bh, tmp[t][j], 0, 0, 0);
        }
      }
    }
    // undo this block's scales into the fp32 accumulators (C/D layout: column = lane & 15, row = 4 (lane >> 4) + e)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float f = rinv[16 * t + 4 * kq + e] * winv;
#pragma unroll
        for (int j = 0; j < NC; ++j) acc[t][j][e] += tmp[t][j][e] * f;
      }
    }
    __syncthreads();        // every wave is done with A and rinv before the next block overwrites them
  }

  // ---- epilogue: bias, relu, stores -------------------------------------------------------------------------------
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int n = wave * (WP / 4) + 16 * j + ar;
    const float bn = a.bias[n];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 16 * t + 4 * kq + e;
        const int64_t row = m0 + r;
        if (row < rend) {
          float y = acc[t][j][e] + bn;
          y = y > 0.f ? y : 0.f;
          if (a.out) a.out[row * a.ldo + n] = y;
          if (a.out2) a.out2[(row - a.row0) * a.ld2 + n] = y;
        }
      }
    }
  }
}

template <int WP, int S>
int launch_layer_wide(const WideLayerArgs& g, hipStream_t stream) {
  const size_t lds = (size_t)2 * SW_ROWS * (WP + 8) * sizeof(short) + SW_ROWS * sizeof(float);
  if (lds > 65536)
    if (hipError_t e = size_dynamic_lds<shmp_layer_wide_kernel<WP, S>>((int)lds); e != hipSuccess)
      return fail((int)e, "desco_shmp_layer_wide_f16x3_f32: cannot size LDS");
  const int64_t blocks = (g.num_rows + SW_ROWS - 1) / SW_ROWS;
  hipLaunchKernelGGL((shmp_layer_wide_kernel<WP, S>), dim3((unsigned)blocks), dim3(256), lds, stream, g);
  return launch_status("desco_shmp_layer_wide_f16x3_f32");
}

template <int WP>
int launch_layer_wide_s(const WideLayerArgs& g, int slots, hipStream_t stream) {
  return slots == 4 ? launch_layer_wide<WP, 4>(g, stream) : launch_layer_wide<WP, 2>(g, stream);
}

// one wave per virtual row, lane c holds columns 4c .. 4c + 3 (c < width / 4)
__global__ __launch_bounds__(256) void csr_gather_sum_wide_kernel(const float* __restrict__ x, int64_t ldx,
                                                                  const int32_t* __restrict__ vrowptr,
                                                                  const int32_t* __restrict__ vcol, int64_t num_vrows,
                                                                  int width, float* __restrict__ out, int64_t ldo) {
  const int lane = (int)__builtin_amdgcn_workitem_id_x() & 63;
  const int64_t v = (int64_t)__builtin_amdgcn_workgroup_id_x() * 4 + ((int)__builtin_amdgcn_workitem_id_x() >> 6);
  if (v >= num_vrows || 4 * lane >= width) return;
  const int e0 = vrowptr[v], e1 = vrowptr[v + 1];
  const float* xc = x + 4 * lane;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int e = e0; e < e1; e += 4) {
    const int cnt = e1 - e;
    const int64_t j0 = vcol[e];
    const int64_t j1 = cnt > 1 ? vcol[e + 1] : j0, j2 = cnt > 2 ? vcol[e + 2] : j0, j3 = cnt > 3 ? vcol[e + 3] : j0;
    const float4 u0 = *reinterpret_cast<const float4*>(xc + j0 * ldx);
    const float4 u1 = *reinterpret_cast<const float4*>(xc + j1 * ldx);
    const float4 u2 = *reinterpret_cast<const float4*>(xc + j2 * ldx);
    const float4 u3 = *reinterpret_cast<const float4*>(xc + j3 * ldx);
    sw_add(acc, u0);
    if (cnt > 1) sw_add(acc, u1);
    if (cnt > 2) sw_add(acc, u2);
    if (cnt > 3) sw_add(acc, u3);
  }
  *reinterpret_cast<float4*>(out + v * ldo + 4 * lane) = acc;
}

// out[b, q] = b2 + sum_c w2[c] leaky(T[b, c] + Qh[q, c]) as in count_head_kernel (graph_ops.hip): one thread per target
// row keeps NQ query accumulators; the block's 256 T rows stream through LDS in 16-column chunks; the whole Qh group
// (NQ x hid) and w2 sit in LDS.  blockIdx.y selects a group of NQ queries.
constexpr int HW_NQ = 8, HW_MAXHID = 1024, HW_TS = 20;
__global__ __launch_bounds__(256) void count_head_wide_kernel(const float* __restrict__ t, int64_t ldt,
                                                              const float* __restrict__ qh, int64_t ldq, int hid,
                                                              const float* __restrict__ w2, float b2,
                                                              const float* __restrict__ b2_dev, float slope, int exp2m1,
                                                              float* __restrict__ out, int64_t ldo, int64_t num_b,
                                                              int num_q, int64_t num_blocks) {
  __shared__ __attribute__((aligned(16))) float qt[HW_NQ * HW_MAXHID];   // [q - q0][hid], rows >= num_q zero
  __shared__ __attribute__((aligned(16))) float ws[HW_MAXHID];           // w2
  __shared__ __attribute__((aligned(16))) float wr[HW_MAXHID];           // (1 - slope) w2
  __shared__ __attribute__((aligned(16))) float tch[256 * HW_TS];        // T chunk [256 rows][16 (+4 pad)]
  __shared__ float sq[HW_NQ];                                            // b2 + slope (w2.Qh[q])
  const int tid = (int)__builtin_amdgcn_workitem_id_x();
  const int q0 = (int)__builtin_amdgcn_workgroup_id_y() * HW_NQ;
  if (b2_dev) b2 = *b2_dev;
  for (int i = tid; i < HW_NQ * hid; i += 256) {
    const int q = i / hid, c = i - q * hid;
    qt[i] = q0 + q < num_q ? qh[(int64_t)(q0 + q) * ldq + c] : 0.f;
  }
  for (int i = tid; i < hid; i += 256) {
    ws[i] = w2[i];
    wr[i] = (1.f - slope) * w2[i];
  }
  __syncthreads();
  if (tid < HW_NQ) {
    float s = 0.f;
    for (int c = 0; c < hid; ++c) s = fmaf(ws[c], qt[tid * hid + c], s);
    sq[tid] = slope * s + b2;
  }
  const int nch = hid / 16;
  const int lrow = tid >> 2, lpart = 4 * (tid & 3);
  for (int64_t b0 = (int64_t)__builtin_amdgcn_workgroup_id_x() * 256; b0 < num_b; b0 += num_blocks * 256) {
    float acc[HW_NQ];
#pragma unroll
    for (int j = 0; j < HW_NQ; ++j) acc[j] = 0.f;
    float st = 0.f;
    for (int ch = 0; ch < nch; ++ch) {
      __syncthreads();                                    // the previous chunk has been consumed (and sq is written)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        int64_t rr = b0 + lrow + 64 * p;
        rr = rr < num_b ? rr : num_b - 1;
        *reinterpret_cast<float4*>(tch + (lrow + 64 * p) * HW_TS + lpart) =
            *reinterpret_cast<const float4*>(t + rr * ldt + ch * 16 + lpart);
      }
      __syncthreads();
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) {
        const int c = ch * 16 + cc;
        const float tv = tch[tid * HW_TS + cc];
        st = fmaf(tv, ws[c], st);
        const float rc = wr[c];
#pragma unroll
        for (int j = 0; j < HW_NQ; ++j) acc[j] = fmaf(fmaxf(tv + qt[j * hid + c], 0.f), rc, acc[j]);
      }
    }
    const int64_t b = b0 + tid;
    if (b < num_b) {
#pragma unroll
      for (int j = 0; j < HW_NQ; ++j) {
        if (q0 + j < num_q) {
          const float v = acc[j] + (slope * st + sq[j]);
          out[b * ldo + q0 + j] = exp2m1 ? exp2f(v) - 1.f : v;
        }
      }
    }
  }
}

}  // namespace

}  // namespace desco

using namespace desco;

extern "C" int desco_shmp_layer_wide_f16x3_f32(const float* x, int64_t ldx, const int32_t* vrowptr,
                                               const int32_t* vcol, int vslots, int64_t row0, int64_t num_rows,
                                               int slots, int width, const int16_t* w_planes, const float* w_scale,
                                               const float* bias, float* out, int64_t ldo, float* out2, int64_t ld2,
                                               desco_stream_t stream) {
  if (row0 < 0 || num_rows < 0 || !(slots == 2 || slots == 4) || vslots < slots || vslots > 4 ||
      !(width == 64 || width == 128 || width == 192 || width == 256))
    return fail(DESCO_EINVAL, "desco_shmp_layer_wide_f16x3_f32: bad argument (row0, num_rows >= 0, slots in {2, 4}, "
                              "slots <= vslots <= 4, width in {64, 128, 192, 256})");
  if (num_rows == 0) return 0;
  if (!x || !vrowptr || !vcol || !w_planes || !w_scale || !bias || (!out && !out2))
    return fail(DESCO_EINVAL, "desco_shmp_layer_wide_f16x3_f32: bad argument (a required pointer is NULL, or neither "
                              "out nor out2 is given)");
  if (mis16(x) || mis16(w_planes) || ldx % 4 || ldx < width || (out && ldo < width) || (out2 && ld2 < width))
    return fail(DESCO_EINVAL, "desco_shmp_layer_wide_f16x3_f32: bad argument (x and the planes 16-byte aligned, "
                              "ldx % 4 == 0, leading dimensions >= width)");
  if (out == x || out2 == x)
    return fail(DESCO_EINVAL, "desco_shmp_layer_wide_f16x3_f32: bad argument (out and out2 must not be x)");
  if ((num_rows + SW_ROWS - 1) / SW_ROWS > INT32_MAX)
    return fail(DESCO_EINVAL, "desco_shmp_layer_wide_f16x3_f32: too many rows");
  WideLayerArgs a{x, ldx, vrowptr, vcol, vslots, row0, num_rows, reinterpret_cast<const short*>(w_planes), w_scale, bias,
                  out, ldo, out2, ld2};
  hipStream_t st = (hipStream_t)stream;
  switch (width) {
    case 64: return launch_layer_wide_s<64>(a, slots, st);
    case 128: return launch_layer_wide_s<128>(a, slots, st);
    case 192: return launch_layer_wide_s<192>(a, slots, st);
    default: return launch_layer_wide_s<256>(a, slots, st);
  }
}

extern "C" int desco_csr_gather_sum_wide_f32(const float* x, int64_t ldx, const int32_t* vrowptr, const int32_t* vcol,
                                             int64_t num_rows, int slots, int width, float* out, int64_t ldo,
                                             desco_stream_t stream) {
  if (num_rows < 0 || !(slots == 1 || slots == 2 || slots == 4) || width <= 0 || width > 256 || width % 4)
    return fail(DESCO_EINVAL, "desco_csr_gather_sum_wide_f32: bad argument (num_rows >= 0, slots in {1, 2, 4}, "
                              "width % 4 == 0, width <= 256)");
  if (num_rows == 0) return 0;
  if (!x || !vrowptr || !vcol || !out || mis16(x) || mis16(out) || ldx % 4 || ldo % 4 || ldx < width || ldo < width)
    return fail(DESCO_EINVAL, "desco_csr_gather_sum_wide_f32: bad argument (NULL pointer, x / out not 16-byte aligned, "
                              "leading dimensions not multiples of 4 or below width)");
  const int64_t nv = num_rows * slots;
  const int64_t blocks = (nv + 3) / 4;
  if (blocks > INT32_MAX) return fail(DESCO_EINVAL, "desco_csr_gather_sum_wide_f32: too many rows");
  hipLaunchKernelGGL(csr_gather_sum_wide_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx,
                     vrowptr, vcol, nv, width, out, ldo);
  return launch_status("desco_csr_gather_sum_wide_f32");
}

extern "C" int desco_count_head_wide_f32(const float* t, int64_t ldt, const float* qh, int64_t ldq, int hid,
                                         const float* w2, float b2, const float* b2_dev, float slope, int exp2_minus_1,
                                         float* out, int64_t ldo, int64_t num_b, int num_q, desco_stream_t stream) {
  if (num_b == 0 || num_q == 0) return 0;
  if (!t || !qh || !w2 || !out || num_b < 0 || num_q < 0 || num_q > 32 || hid <= 0 || hid % 64 || hid > HW_MAXHID ||
      ldt % 4 || ldt < hid || ldq < hid || ldo < num_q || mis16(t))
    return fail(DESCO_EINVAL, "desco_count_head_wide_f32: bad argument (NULL pointer, num_q > 32, hid not a multiple of "
                              "64 up to 1024, t not 16-byte aligned, ldt % 4 != 0, ldt / ldq < hid or ldo < num_q)");
  int64_t blocks = (num_b + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(count_head_wide_kernel, dim3((unsigned)blocks, (unsigned)((num_q + HW_NQ - 1) / HW_NQ)),
                     dim3(256), 0, (hipStream_t)stream, t, ldt, qh, ldq, hid, w2, b2, b2_dev, slope, exp2_minus_1, out,
                     ldo, num_b, num_q, blocks);
  return launch_status("desco_count_head_wide_f32");
}

#include "tu_no_packed_f32_end.hpp"
