// The anchor MLP, the pooled sums and post_mp.0 in one launch (desco_anchor_pool_post_f16x3_f32).  Before, the anchor GEMM
// (gemm_f16x3_kernel) wrote anch [B, 64 (L + 1)] and desco_pool_post_bf16x6_f32 read it straight back: 2 x 2.76 GB per
// COX2 x64 pass for a tensor with one consumer.  Here a workgroup owns a 128-row panel and sweeps the anchor's 192-column
// n-tiles in order, each with the UNCHANGED f16x3 main loop (gemm_f16x3.hpp: same tile, waves, K chunks, row scales, so
// every anchor value has the bits gemm_f16x3_kernel<3, 128> writes).  The epilogue of n-tile t takes its six 32-column
// pieces (K steps 192 t + 32 p of post_mp.0) in increasing order:
//   A  the two waves that hold piece p write its anchor values (scales undone, bias, activation) as an fp32 image [128][32];
//   B  every thread forms 4 rows x 4 columns of the pooled operand from the image and the segment's partial rows (layer
//      block l = 3 t + p / 2: desco_pool_post_bf16x6_f32's POOLA arithmetic, same order), splits them into bf16
//      hi / mid / lo planes and stages them with the matching 32-column slice of post_mp.0's weight planes;
//   C  the bf16x6 products of gemm_split_body<1, 3, 128> for those 32 K values (same six MFMAs, same order).
// post_mp.0's accumulators [128 x 64] stay in registers across the n-tiles; after the last one its bias and activation
// are applied and h0 [B, 64] is stored.  The output is bit-identical to the two launches it replaces.
#include "gemm_f16x3.hpp"

namespace desco {

struct AnchorPostArgs {
  GemmF16Args a;            // the anchor product (n = 64 (L + 1), a multiple of 192; bias_rows 1, no scalar tail)
  const short* w0;          // post_mp.0 bf16x3 planes [3][64][64 (L + 1)]
  const float* b0;          // [64] or NULL
  int act0;
  float slope0;
  float* out;               // h0 [m][ldo]
  int64_t ldo;
  const int32_t* seg_ptr;
  const uint32_t* pool_bits;
  const int32_t* pool_slot;
  const float* part[9];     // [1..L]: the layers' partial arrays [slots][64]
  const float* x0;          // [64]: the constant first block's row
};

using ap_bf16x8 = __attribute__((ext_vector_type(8))) short;

constexpr int kApBM = 128, kApWN = 3, kApBN = 64 * kApWN;
constexpr int kApStage = 2 * kApBM * FST + 2 * kApBN * FST;          // shorts: the main loop's chunk planes
constexpr int kApImg = 0;                                            // fp32 image of one piece [128][32] (floats from 0)
constexpr int kApA = 2 * kApBM * 32;                                 // shorts: bf16 planes of the pooled piece [3][128][32]
constexpr int kApB = kApA + 3 * kApBM * 32;                          // shorts: post_mp.0 weight slice [3][64][32]
constexpr int kApEnd = kApB + 3 * 64 * 32;
constexpr int kApBody = kApStage > kApEnd ? kApStage : kApEnd;
constexpr size_t kApLdsBytes = (size_t)kApBody * sizeof(short) + kApBM * (sizeof(float) + sizeof(int4));

__global__ __launch_bounds__(2 * kApBM) __attribute__((amdgpu_waves_per_eu(2))) void anchor_pool_post_kernel(AnchorPostArgs q) {
  // no contraction: the anchor values are gemm_f16x3_kernel's separately rounded product and bias add
#pragma clang fp contract(off)
  constexpr int BM = kApBM, WN = kApWN, BN = kApBN;
  constexpr int PA = BM * 32, PB = 64 * 32;                          // plane sizes (shorts) of the post_mp.0 operands
  extern __shared__ __attribute__((aligned(16))) short lds[];
  float* img = reinterpret_cast<float*>(lds) + kApImg;
  short* Ap = lds + kApA;
  short* Bp = lds + kApB;
  float* rinv = reinterpret_cast<float*>(lds + kApBody);             // [BM] 1 / (row scale * weight scale)
  int4* slots = reinterpret_cast<int4*>(rinv + BM);                  // [BM] step B's segment slots (-1: none), row count
  const GemmF16Args& g = q.a;

  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int ntiles = g.n / BN;
  const int Kp = g.n;                                                // post_mp.0's K = the anchor's n
  if (tid < BM) {
    const int64_t rr = m0 + tid < g.m ? m0 + tid : g.m - 1;
    rinv[tid] = pow2_inverse(f16_scale_for(g.row_scale[rr])) * g.w_scale[1];
    // the row's segment: offsets of its (at most three) partial slots, -1 = none (a segment without count rows has
    // none), and its row count
    const int a_ = q.seg_ptr[rr], e_ = q.seg_ptr[rr + 1];
    int4 so_ = make_int4(-1, -1, -1, __float_as_int((float)(e_ - a_)));
    if (e_ > a_) {
      const int t0_ = a_ >> 4, t1_ = (e_ - 1) >> 4, f_ = a_ - (t0_ << 4);
      so_.x = (q.pool_slot[t0_] + __popc(q.pool_bits[t0_] & ((1u << f_) - 1u))) * 64;
      so_.y = t1_ > t0_ ? q.pool_slot[t0_ + 1] * 64 : -1;
      so_.z = t1_ > t0_ + 1 ? q.pool_slot[t0_ + 2] * 64 : -1;
    }
    slots[tid] = so_;
  }

  // step B's map: rows arow + 32 u (u = 0..3), columns 4 ac4 .. 4 ac4 + 3 of the piece
  const int arow = tid >> 3, ac4 = tid & 7;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // the partial rows of one piece (layer l >= 1, columns c0 + 4 ac4 ..): absent slots are zeros
#define DESCO_LOAD_Q1(j_, P_)                                                                 \
  {                                                                                           \
    const int4 so_ = slots[arow + 32 * (j_)];                                                 \
    q##j_##0 = so_.x >= 0 ? *reinterpret_cast<const float4*>((P_) + so_.x) : z4;              \
    q##j_##1 = so_.y >= 0 ? *reinterpret_cast<const float4*>((P_) + so_.y) : z4;              \
    q##j_##2 = so_.z >= 0 ? *reinterpret_cast<const float4*>((P_) + so_.z) : z4;              \
  }
#define DESCO_LOAD_Q(l_, c0_)                                                                 \
  {                                                                                           \
    const float* pq_ = q.part[(l_)] + (c0_) + 4 * ac4;                                        \
    DESCO_LOAD_Q1(0, pq_) DESCO_LOAD_Q1(1, pq_) DESCO_LOAD_Q1(2, pq_) DESCO_LOAD_Q1(3, pq_)   \
  }
// pooled = (((p0 + p1) + p2) + rows * x0) + anchor (desco_pool_post_bf16x6_f32's order: layer 0 has zero partials and
// the x0 term, a layer l >= 1 zero times x0) -> the three bf16 planes of the staged piece
#define DESCO_POOL_PUT(j_, xq_)                                                               \
  {                                                                                           \
    const int row_ = arow + 32 * (j_);                                                        \
    const float nb_ = __int_as_float(slots[row_].w);                                          \
    float4 v_ = *reinterpret_cast<const float4*>(img + row_ * 32 + 4 * ac4);                  \
    float4 t_;                                                                                \
    t_.x = (((q##j_##0).x + (q##j_##1).x) + (q##j_##2).x) + __fmul_rn(nb_, (xq_).x);       \
    t_.y = (((q##j_##0).y + (q##j_##1).y) + (q##j_##2).y) + __fmul_rn(nb_, (xq_).y);       \
    t_.z = (((q##j_##0).z + (q##j_##1).z) + (q##j_##2).z) + __fmul_rn(nb_, (xq_).z);       \
    t_.w = (((q##j_##0).w + (q##j_##1).w) + (q##j_##2).w) + __fmul_rn(nb_, (xq_).w);       \
    v_.x = t_.x + v_.x;                                                                       \
    v_.y = t_.y + v_.y;                                                                       \
    v_.z = t_.z + v_.z;                                                                       \
    v_.w = t_.w + v_.w;                                                                       \
    short* d_ = Ap + row_ * 32 + gf16_chunk(row_, ac4 >> 1) + 4 * (ac4 & 1);                  \
    uint32_t h0_, m0_, l0_, h1_, m1_, l1_;                                                    \
    split2_bf16x3(v_.x, v_.y, h0_, m0_, l0_);                                                 \
    split2_bf16x3(v_.z, v_.w, h1_, m1_, l1_);                                                 \
    *reinterpret_cast<uint2*>(d_) = make_uint2(h0_, h1_);                                     \
    *reinterpret_cast<uint2*>(d_ + PA) = make_uint2(m0_, m1_);                                \
    *reinterpret_cast<uint2*>(d_ + 2 * PA) = make_uint2(l0_, l1_);                            \
  }

  // post_mp.0's weight slice of a piece: row brow (0..63) of each plane, 16 bytes per thread
  const int brow = tid >> 2, bpart = tid & 3;
  const short* pw0 = q.w0 + (int64_t)brow * Kp + 8 * bpart;
  const int64_t w0plane = (int64_t)64 * Kp;
  short* bst = Bp + brow * 32 + gf16_chunk(brow, bpart);

  f32x16 pacc0, pacc1;                 // post_mp.0: rows 64 wr + 32 i, columns 32 wc of the block's [128][64] output
#pragma unroll
  for (int e = 0; e < 16; ++e) pacc0[e] = pacc1[e] = 0.f;
  const int col = lane & 31;
  const int fsw = (lane >> 3) & 3, fh = lane >> 5;

  for (int t = 0; t < ntiles; ++t) {
    const int n0 = t * BN;
    if (t > 0) __syncthreads();        // the last piece's fragments have been read (the main loop reuses that LDS)
    f32x16 acc[2][WN];
    gemm_f16x3_main_loop<WN, BM, false>(g, lds, m0, n0, acc);
    __syncthreads();                   // every wave is done with the last chunk's fragments
    float4 q00, q01, q02, q10, q11, q12, q20, q21, q22, q30, q31, q32;
    q00 = q01 = q02 = q10 = q11 = q12 = q20 = q21 = q22 = q30 = q31 = q32 = z4;
    if (t > 0) DESCO_LOAD_Q(3 * t, 0)
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const int l = 3 * t + (p >> 1), c0 = 32 * (p & 1), kp = n0 + 32 * p;
      // A: the piece's anchor values as gemm_f16x3_kernel's epilogue forms them
      if (wc == p / 3) {
        const float b_single = g.bias ? g.bias[kp + col] : 0.f;
        // this lane's rows 64 wr + 32 i + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), column col
        const int lrow = wr * 64 + 4 * (lane >> 5);
        const float* ri = rinv + lrow;
        float* im = img + lrow * 32 + col;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const float4 r0 = *reinterpret_cast<const float4*>(ri + 32 * i);
          const float4 r1 = *reinterpret_cast<const float4*>(ri + 32 * i + 8);
          const float4 r2 = *reinterpret_cast<const float4*>(ri + 32 * i + 16);
          const float4 r3 = *reinterpret_cast<const float4*>(ri + 32 * i + 24);
          const float rv[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            float v = acc[i][p % 3][reg] * rv[reg];
            if (g.bias) v += b_single;
            im[(32 * i + (reg & 3) + 8 * (reg >> 2)) * 32] = apply_act(v, g.act, g.slope);
          }
        }
      }
      __syncthreads();
      // B: pooled operand and weight slice -> LDS planes
      {
        const float4 xq = l == 0 ? *reinterpret_cast<const float4*>(q.x0 + c0 + 4 * ac4) : z4;
        DESCO_POOL_PUT(0, xq) DESCO_POOL_PUT(1, xq) DESCO_POOL_PUT(2, xq) DESCO_POOL_PUT(3, xq)
        const uint4 w0h = *reinterpret_cast<const uint4*>(pw0 + kp);
        const uint4 w0m = *reinterpret_cast<const uint4*>(pw0 + kp + w0plane);
        const uint4 w0l = *reinterpret_cast<const uint4*>(pw0 + kp + 2 * w0plane);
        *reinterpret_cast<uint4*>(bst) = w0h;
        *reinterpret_cast<uint4*>(bst + PB) = w0m;
        *reinterpret_cast<uint4*>(bst + 2 * PB) = w0l;
      }
      // the next piece's partial rows, in flight under this piece's products
      if (p < 5) {
        const int ln = 3 * t + ((p + 1) >> 1);
        if (ln >= 1) DESCO_LOAD_Q(ln, 32 * ((p + 1) & 1))
      }
      __syncthreads();
      // C: post_mp.0 on the piece (gemm_split_body<1, 3, 128>'s fragments and product order)
      {
        const short* ap = Ap + (wr * 64 + (lane & 31)) * 32;
        const short* bp = Bp + (wc * 32 + (lane & 31)) * 32;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int co = (((2 * s + fh) ^ fsw) & 3) << 3;
          const ap_bf16x8 ah0 = *reinterpret_cast<const ap_bf16x8*>(ap + co);
          const ap_bf16x8 am0 = *reinterpret_cast<const ap_bf16x8*>(ap + PA + co);
          const ap_bf16x8 al0 = *reinterpret_cast<const ap_bf16x8*>(ap + 2 * PA + co);
          const ap_bf16x8 ah1 = *reinterpret_cast<const ap_bf16x8*>(ap + 32 * 32 + co);
          const ap_bf16x8 am1 = *reinterpret_cast<const ap_bf16x8*>(ap + 32 * 32 + PA + co);
          const ap_bf16x8 al1 = *reinterpret_cast<const ap_bf16x8*>(ap + 32 * 32 + 2 * PA + co);
          const ap_bf16x8 bh = *reinterpret_cast<const ap_bf16x8*>(bp + co);
          const ap_bf16x8 bm = *reinterpret_cast<const ap_bf16x8*>(bp + PB + co);
          const ap_bf16x8 bl = *reinterpret_cast<const ap_bf16x8*>(bp + 2 * PB + co);
          pacc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al0, bh, pacc0, 0, 0, 0);
          pacc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al1, bh, pacc1, 0, 0, 0);
          pacc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah0, bl, pacc0, 0, 0, 0);
          pacc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah1, bl, pacc1, 0, 0, 0);
          pacc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am0, bm, pacc0, 0, 0, 0);
          pacc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am1, bm, pacc1, 0, 0, 0);
          pacc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am0, bh, pacc0, 0, 0, 0);
          pacc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am1, bh, pacc1, 0, 0, 0);
          pacc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah0, bm, pacc0, 0, 0, 0);
          pacc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah1, bm, pacc1, 0, 0, 0);
          pacc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah0, bh, pacc0, 0, 0, 0);
          pacc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah1, bh, pacc1, 0, 0, 0);
        }
      }
    }
  }
#undef DESCO_LOAD_Q1
#undef DESCO_LOAD_Q
#undef DESCO_POOL_PUT

  // post_mp.0's epilogue (gemm_split_body's with WN = 1): each 32-row half through a wave-private [32][32] fp32 image ->
  // 16-byte row-contiguous stores
  __syncthreads();
  float* st = reinterpret_cast<float*>(lds) + wave * (32 * 32);
  const bool wide = ((reinterpret_cast<uintptr_t>(q.out) & 15) == 0) && ((q.ldo & 3) == 0);
  const int gcol = wc * 32 + col;
  const float b0 = q.b0 ? q.b0[gcol] : 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t grow0 = m0 + wr * 64 + 32 * i;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      float v = i == 0 ? pacc0[reg] : pacc1[reg];
      if (q.b0) v += b0;
      st[row * 32 + col] = apply_act(v, q.act0, q.slope0);
    }
    __syncthreads();
    float* crow = q.out + wc * 32;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int idx = lane + 64 * p;               // float4 index in the image: row idx / 8
      const int row = idx / 8, c4 = idx % 8;
      const float4 v = *reinterpret_cast<const float4*>(st + 4 * idx);
      const int64_t grow = grow0 + row;
      if (grow < g.m) {
        float* o = crow + grow * q.ldo + 4 * c4;
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

}  // namespace desco

using namespace desco;

extern "C" int desco_anchor_pool_post_f16x3_f32(const float* a, int64_t lda, int k, const int16_t* anchor_planes,
                                                const float* anchor_scale, const float* anchor_bias, int act,
                                                float slope, const float* row_scale, int num_layers,
                                                const int16_t* post_planes, const float* post_bias, int post_act,
                                                float post_slope, float* out, int64_t ldo, int64_t m,
                                                const int32_t* seg_ptr, const uint32_t* pool_bits,
                                                const int32_t* pool_slot, const float* const* parts, const float* x0,
                                                int tile_rows, desco_stream_t stream) {
  if (m == 0) return 0;
  if (m > (int64_t)(1 << 24))
    return fail(DESCO_EINVAL, "desco_anchor_pool_post_f16x3_f32: more than 2^24 segments (slot offsets are 31 bits)");
  const int n = 64 * (num_layers + 1);
  if (m < 0 || !a || !anchor_planes || !anchor_scale || !row_scale || !post_planes || !out || !seg_ptr || !pool_bits ||
      !pool_slot || !parts || !x0 || num_layers < 1 || num_layers > 8 || n % kApBN || (k != n && k != n - 64) ||
      tile_rows != 16 || lda % 4 || lda < k || ldo < 64 || mis16(a) || mis16(anchor_planes) || mis16(post_planes) ||
      mis16(x0))
    return fail(DESCO_EINVAL, "desco_anchor_pool_post_f16x3_f32: bad argument (L in {2, 5, 8}, k == 64 L or 64 (L + 1), "
                              "16-row tiles, 16-byte alignment)");
  AnchorPostArgs q{};
  q.a = GemmF16Args{a, lda, k, nullptr, 0, 0, reinterpret_cast<const short*>(anchor_planes), anchor_scale, n, anchor_bias,
                    1, nullptr, 0, nullptr, act, slope, nullptr, 0, m, row_scale};
  q.w0 = reinterpret_cast<const short*>(post_planes);
  q.b0 = post_bias;
  q.act0 = post_act;
  q.slope0 = post_slope;
  q.out = out;
  q.ldo = ldo;
  q.seg_ptr = seg_ptr;
  q.pool_bits = pool_bits;
  q.pool_slot = pool_slot;
  q.x0 = x0;
  for (int l = 1; l <= num_layers; ++l) {
    if (!parts[l - 1] || mis16(parts[l - 1]))
      return fail(DESCO_EINVAL, "desco_anchor_pool_post_f16x3_f32: NULL / misaligned partial array");
    q.part[l] = parts[l - 1];
  }
  if (hipError_t e = size_dynamic_lds<anchor_pool_post_kernel>((int)kApLdsBytes); e != hipSuccess)
    return fail((int)e, "desco_anchor_pool_post_f16x3_f32: cannot size LDS");
  const int64_t blocks = (m + kApBM - 1) / kApBM;
  hipLaunchKernelGGL(anchor_pool_post_kernel, dim3((unsigned)blocks), dim3(2 * kApBM), kApLdsBytes, (hipStream_t)stream, q);
  return launch_status("desco_anchor_pool_post_f16x3_f32");
}
