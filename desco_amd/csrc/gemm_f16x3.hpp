// The f16x3 GEMM's block-tile main loop (gemm_f16x3.hip has the arithmetic and the contract), shared by the plain GEMM
// and by the anchor MLP with its pooling + post_mp.0 epilogue (anchor_post.hip): both produce the same accumulator bits.
#pragma once
#include "common_device.hpp"

namespace desco {

struct GemmF16Args {
  const float* a1;
  int64_t lda1;
  int k1;
  const float* a2;
  int64_t lda2;
  int k2;
  const short* w;         // planes [2][n][k1+k2] (hi, lo) of the scaled weight
  const float* w_scale;   // device [2]: {scale, 1 / scale}
  int n;
  const float* bias;
  int bias_rows;
  const float* s;
  int ns;
  const float* ws;
  int act;
  float slope;
  float* c;
  int64_t ldc;
  int64_t m;
  const float* row_scale;  // [m] bound of each row's largest |a| (desco_row_absmax_f32 or the producer of A)
};

constexpr int FBK = 32, FST = 32;              // K chunk; plane row stride in halves (64 B, no padding)
// same swizzle as gemm_split.hip: 16-byte chunk c of plane row r sits at chunk c ^ ((r >> 3) & 3)
__device__ __forceinline__ int gf16_chunk(const int row, const int c) { return ((c ^ (row >> 3)) & 3) << 3; }

// acc[i][j] = the 2 x WN 32x32 accumulators of this wave for rows m0 + 64 wr + 32 i, columns n0 + 32 WN wc + 32 j of
// the block tile, scaled (row scale times weight scale; the caller undoes both).  Uses the first
// 2 (BM + 64 WN) FST shorts of `lds`; returns with other waves possibly still reading the last chunk's fragments.
// A2 = false: the caller guarantees k2 == 0 (no second operand: its row pointers are not kept in registers).
template <int WN, int BM, bool A2 = true>
__device__ __forceinline__ void gemm_f16x3_main_loop(const GemmF16Args& g, short* lds, const int64_t m0, const int n0,
                                                     f32x16 (&acc)[2][WN]) {
  constexpr int NT = 2 * BM;
  constexpr int BN = 64 * WN, BPLANE = BN * FST, APLANE = BM * FST;
  constexpr int AR = BM / 4;
  constexpr int BR = NT / 4;
  constexpr int BJ = (BN + BR - 1) / BR;
  short* Ap = lds;                  // planes hi, lo of the A chunk [BM][32]
  short* Bp = lds + 2 * APLANE;     // planes hi, lo of the W chunk [BN][32]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int K = g.k1 + g.k2;
  const int nchunks = K / FBK;

  const int arow = tid >> 3, ac4 = tid & 7;
  const int64_t mlast = g.m - 1;
  int64_t r0 = m0 + arow, r1 = r0 + AR, r2 = r0 + 2 * AR, r3 = r0 + 3 * AR;
  r0 = r0 < g.m ? r0 : mlast;
  r1 = r1 < g.m ? r1 : mlast;
  r2 = r2 < g.m ? r2 : mlast;
  r3 = r3 < g.m ? r3 : mlast;
  const float sc0 = f16_scale_for(g.row_scale[r0]), sc1 = f16_scale_for(g.row_scale[r1]);
  const float sc2 = f16_scale_for(g.row_scale[r2]), sc3 = f16_scale_for(g.row_scale[r3]);
  const float* p10 = g.a1 + r0 * g.lda1 + 4 * ac4;
  const float* p11 = g.a1 + r1 * g.lda1 + 4 * ac4;
  const float* p12 = g.a1 + r2 * g.lda1 + 4 * ac4;
  const float* p13 = g.a1 + r3 * g.lda1 + 4 * ac4;
  const float* p20 = A2 && g.k2 ? g.a2 + r0 * g.lda2 + 4 * ac4 - g.k1 : p10;
  const float* p21 = A2 && g.k2 ? g.a2 + r1 * g.lda2 + 4 * ac4 - g.k1 : p11;
  const float* p22 = A2 && g.k2 ? g.a2 + r2 * g.lda2 + 4 * ac4 - g.k1 : p12;
  const float* p23 = A2 && g.k2 ? g.a2 + r3 * g.lda2 + 4 * ac4 - g.k1 : p13;
  const int brow = tid >> 2, bpart = tid & 3;
  const short* pw = g.w + (int64_t)(n0 + brow) * K + 8 * bpart;
  const int64_t wplane = (int64_t)g.n * K;
  const int64_t wj = (int64_t)BR * K;
  const bool v0 = BR <= BN || brow < BN;
  const bool v1 = BJ > 1 && brow + BR < BN;
  const bool v2 = BJ > 2 && brow + 2 * BR < BN;

  float4 ra0, ra1, ra2, ra3;                   // A chunk about to be stored
  float4 rn0, rn1, rn2, rn3;                   // A chunk after it
  uint4 rb00, rb01, rb10, rb11, rb20, rb21;    // W planes of the next chunk
  rb00 = rb01 = rb10 = rb11 = rb20 = rb21 = make_uint4(0, 0, 0, 0);
#define DESCO_LOAD_A(d_, kk_)                                                                 \
  {                                                                                           \
    const int k_ = (kk_);                                                                     \
    const bool s1_ = !A2 || k_ < g.k1;                                                        \
    d_##0 = *reinterpret_cast<const float4*>((s1_ ? p10 : p20) + k_);                         \
    d_##1 = *reinterpret_cast<const float4*>((s1_ ? p11 : p21) + k_);                         \
    d_##2 = *reinterpret_cast<const float4*>((s1_ ? p12 : p22) + k_);                         \
    d_##3 = *reinterpret_cast<const float4*>((s1_ ? p13 : p23) + k_);                         \
  }
#define DESCO_LOAD_WJ(j_, v_)                                                                 \
  if (BJ > (j_) && (v_)) {                                                                    \
    rb##j_##0 = *reinterpret_cast<const uint4*>(w_ + (j_) * wj);                              \
    rb##j_##1 = *reinterpret_cast<const uint4*>(w_ + (j_) * wj + wplane);                     \
  }
#define DESCO_LOAD_W(kk_)                                                                     \
  {                                                                                           \
    const short* w_ = pw + (kk_);                                                             \
    DESCO_LOAD_WJ(0, v0) DESCO_LOAD_WJ(1, v1) DESCO_LOAD_WJ(2, v2)                            \
  }
#define DESCO_PUT(row_, v_, sc_)                                                              \
  {                                                                                           \
    short* d_ = Ap + (row_)*FST + gf16_chunk((row_), ac4 >> 1) + 4 * (ac4 & 1);               \
    uint32_t h0_, l0_, h1_, l1_;                                                              \
    split2_f16x2(v_.x * (sc_), v_.y * (sc_), h0_, l0_);                                       \
    split2_f16x2(v_.z * (sc_), v_.w * (sc_), h1_, l1_);                                       \
    *reinterpret_cast<uint2*>(d_) = make_uint2(h0_, h1_);                                     \
    *reinterpret_cast<uint2*>(d_ + APLANE) = make_uint2(l0_, l1_);                            \
  }
#define DESCO_STORE_WJ(j_, v_)                                                                \
  if (BJ > (j_) && (v_)) {                                                                    \
    short* bj_ = Bp + (brow + (j_) * BR) * FST + gf16_chunk(brow + (j_) * BR, bpart);         \
    *reinterpret_cast<uint4*>(bj_) = rb##j_##0;                                               \
    *reinterpret_cast<uint4*>(bj_ + BPLANE) = rb##j_##1;                                      \
  }
#define DESCO_STORE_CHUNK()                                                                   \
  {                                                                                           \
    DESCO_PUT(arow, ra0, sc0)                                                                 \
    DESCO_PUT(arow + AR, ra1, sc1)                                                            \
    DESCO_PUT(arow + 2 * AR, ra2, sc2)                                                        \
    DESCO_PUT(arow + 3 * AR, ra3, sc3)                                                        \
    DESCO_STORE_WJ(0, v0) DESCO_STORE_WJ(1, v1) DESCO_STORE_WJ(2, v2)                         \
  }

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  DESCO_LOAD_A(ra, 0)
  DESCO_LOAD_W(0)
  DESCO_LOAD_A(rn, (nchunks > 1 ? 1 : 0) * FBK)
  for (int ch = 0; ch < nchunks; ++ch) {
    if (ch > 0) __syncthreads();          // previous chunk's fragments have been read
    DESCO_STORE_CHUNK()
    __syncthreads();
    const int chn = ch + 1 < nchunks ? ch + 1 : ch;
    const int chnn = ch + 2 < nchunks ? ch + 2 : chn;
    ra0 = rn0; ra1 = rn1; ra2 = rn2; ra3 = rn3;
    DESCO_LOAD_W(chn * FBK)                // in flight under the MFMAs
    DESCO_LOAD_A(rn, chnn * FBK)           // two chunks ahead (HBM latency)
    // lane (r = lane&31, h = lane>>5): A[row r][k = 16 s + 8 h + j], B[k = 16 s + 8 h + j][col r]
    const int fsw = (lane >> 3) & 3, fh = lane >> 5;
    const short* ap = Ap + (wr * 64 + (lane & 31)) * FST;
    const short* bp = Bp + (wc * 32 * WN + (lane & 31)) * FST;
#pragma unroll
    for (int s = 0; s < FBK / 16; ++s) {
      f16x8 ah[2], al[2];
      const int co = (((2 * s + fh) ^ fsw) & 3) << 3;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ah[i] = *reinterpret_cast<const f16x8*>(ap + i * 32 * FST + co);
        al[i] = *reinterpret_cast<const f16x8*>(ap + i * 32 * FST + APLANE + co);
      }
      f16x8 bh[WN], bl[WN];
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        const short* bt = bp + j * 32 * FST + co;
        bh[j] = *reinterpret_cast<const f16x8*>(bt);
        bl[j] = *reinterpret_cast<const f16x8*>(bt + BPLANE);
      }
      // smallest terms first; one product of ALL 2 WN accumulators at a time: an accumulator comes round again after
      // 2 WN MFMAs, not after two (a dependent 32x32x16 MFMA issued within its predecessor's 64 cycles waits for it)
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[0], bh[j], acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[1], bh[j], acc[1][j], 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[0], bl[j], acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[1], bl[j], acc[1][j], 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[0], bh[j], acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[1], bh[j], acc[1][j], 0, 0, 0);
      }
    }
  }
#undef DESCO_LOAD_A
#undef DESCO_LOAD_W
#undef DESCO_LOAD_WJ
#undef DESCO_PUT
#undef DESCO_STORE_CHUNK
#undef DESCO_STORE_WJ
}

}  // namespace desco
