// One GossipConv layer l >= 1 of a gossip model of any depth, over all R = N Q (node, query) rows:
//
//   hh      = sum_j (j < i ? g[q] : 1 - g[q]) h[j Q + q, :]                  (CSR order of node i)
//   out     = relu([hh | h] W + C3[r] . V[q])                                W = [(D_a C)^T; D_b^T]  [128, 64]
//   acc    += h P     (+ out Pn on the last layer)                           P, Pn: post_mp.0 blocks of h_l, h_{l+1}
//
// One 256-thread workgroup per 64 consecutive rows (not persistent).
//  * Gather: sixteen lane groups of sixteen lanes (float4 per lane: one 256-byte row per group); group G gathers rows
//    G, G + 16, G + 32, G + 48 of the tile, four neighbour rows in flight, summed in the row's own CSR order (split by
//    direction and gated as gossip_gather_kernel does), so a result does not depend on the tiling.  The Q rows of one
//    node have one degree and sit next to each other: they are dealt to different groups, so a hub node's rows spread
//    over the whole workgroup rather than serialising one group (with Q >= 16 every group of such a tile gets the same
//    neighbour count).
//  * The gathered hh and the row's own h are scaled by one power of two per row and split into fp16 hi / lo planes
//    ("f16x3", gemm_f16x3.hip) in an LDS image [64 rows][128 k]; the weights come pre-split (desco_split_f16x2_f32)
//    and each wave holds the B fragments of its 16 output columns in registers for the whole tile.
//  * Product: v_mfma_f32_16x16x32_f16, three products (lo*hi, hi*lo, hi*hi) per step, fp32 accumulation; wave w owns
//    output columns 16 w .. 16 w + 15 of all 64 rows (four 16-row tiles): [hh | h] W (K = 128) and h P (K = 64, the
//    second half of the same image).
//  * Last layer (Pn given): out goes through an fp32 LDS image, is scaled and split like the input rows, and one more
//    K = 64 product adds out Pn to the accumulator.
// Every load into LDS goes through registers (no LDS-DMA form).  Bytes per row: 256 (h) + 256 per neighbour + 256 (out)
// + 512 (acc read and written) + 12 (C3), plus the CSR.
#include "common_device.hpp"

namespace desco {

namespace {

constexpr int GL_ROWS = 64;                     // rows per workgroup tile
constexpr int GL_AST = 136;                     // A image row stride in halves (128 + 8: rows 4 banks apart)
constexpr int GL_APLANE = GL_ROWS * GL_AST;     // halves per plane
constexpr int GL_FST = 68;                      // fp32 image row stride (floats)

struct GossipLayerArgs {
  const float* h;
  const int32_t* rowptr;
  const int32_t* col;
  int64_t num_nodes;
  int num_q;
  const float* g;
  const float* c3;
  const float* v;
  const short* w;          // planes [2][64][128]
  const float* w_scale;    // {scale, 1 / scale}
  const short* p;          // planes [2][64][64]
  const float* p_scale;
  const short* pn;         // planes [2][64][64] or nullptr
  const float* pn_scale;
  float* acc;
  float* out;
};

// one lane's float4 piece of row r, already scaled -> hi / lo planes at columns k .. k + 3
__device__ __forceinline__ void gl_put(short* A, const int r, const int k, const float4 v, const float sc) {
  uint32_t h0, l0, h1, l1;
  split2_f16x2(v.x * sc, v.y * sc, h0, l0);
  split2_f16x2(v.z * sc, v.w * sc, h1, l1);
  *reinterpret_cast<uint2*>(A + r * GL_AST + k) = make_uint2(h0, h1);
  *reinterpret_cast<uint2*>(A + GL_APLANE + r * GL_AST + k) = make_uint2(l0, l1);
}

__device__ __forceinline__ float gl_absmax4(const float4 v) {
  return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}

__device__ __forceinline__ float gl_groupmax(float m) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}

// B fragments of one wave: weight planes [2][64][K], output columns n0 .. n0 + 15, K/32 steps
template <int K>
__device__ __forceinline__ void gl_load_b(const short* __restrict__ w, const int n, const int kq, f16x8* bh,
                                          f16x8* bl) {
  const short* p = w + (int64_t)n * K + 8 * kq;
#pragma unroll
  for (int s = 0; s < K / 32; ++s) {
    bh[s] = *reinterpret_cast<const f16x8*>(p + 32 * s);
    bl[s] = *reinterpret_cast<const f16x8*>(p + 64 * K + 32 * s);
  }
}

// acc[t] += A[16 t + (lane & 15)][k0 + ...] x B over NS steps of 32
template <int NS>
__device__ __forceinline__ void gl_product(const short* A, const int k0, const int lane, const f16x8* bh,
                                           const f16x8* bl, f32x4* acc) {
  const int ar = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const short* ap = A + (16 * t + ar) * GL_AST + k0 + 8 * kq;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const f16x8 ah = *reinterpret_cast<const f16x8*>(ap + 32 * s);
      const f16x8 al = *reinterpret_cast<const f16x8*>(ap + GL_APLANE + 32 * s);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[s], acc[t], 0, 0, 0);   // smallest terms first
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[s], acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[s], acc[t], 0, 0, 0);
    }
  }
}

template <bool LAST>
__global__ __launch_bounds__(256) void gossip_layer_kernel(const GossipLayerArgs a) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* A = lds;                                                        // planes hi, lo [64][GL_AST]
  float* rinv = reinterpret_cast<float*>(lds + 2 * GL_APLANE);           // [64] 1 / row scale of the input rows
  float* rinv2 = rinv + GL_ROWS;                                         // [64] ... of the output rows (LAST)
  float* F = rinv2 + GL_ROWS;                                            // [64][GL_FST] fp32 output image (LAST)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = tid & 15, grp = tid >> 4;
  const int Q = a.num_q;
  const int64_t R = a.num_nodes * Q;
  const int64_t m0 = (int64_t)blockIdx.x * GL_ROWS;
  const int64_t i0 = m0 / Q;
  const int q0 = (int)(m0 - i0 * Q);

  // this wave's weight fragments: in flight under the gather
  const int n = 16 * wave + (lane & 15), kq = lane >> 4;
  f16x8 wh[4], wl[4], ph[2], pl[2];
  gl_load_b<128>(a.w, n, kq, wh, wl);
  gl_load_b<64>(a.p, n, kq, ph, pl);

  // ---- gather + stage -------------------------------------------------------------------------------------------
  const int64_t ld = (int64_t)Q * 64;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int r = grp + 16 * k;
    int64_t row = m0 + r;
    row = row < R ? row : R - 1;
    const uint32_t qr = (uint32_t)(q0 + (int)(row - m0));
    const int64_t i = i0 + qr / (uint32_t)Q;
    const int q = (int)(qr % (uint32_t)Q);
    const float gq = a.g[q];
    const int e0 = a.rowptr[i], e1 = a.rowptr[i + 1];
    const int64_t qoff = (int64_t)q * 64 + 4 * l16;
    const float4 hv = *reinterpret_cast<const float4*>(a.h + row * 64 + 4 * l16);
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
#define GL_ADD(v_, j_)                                                        \
  if ((j_) < i) { lo.x += v_.x; lo.y += v_.y; lo.z += v_.z; lo.w += v_.w; }   \
  else { hi.x += v_.x; hi.y += v_.y; hi.z += v_.z; hi.w += v_.w; }
    for (int e = e0; e < e1; e += 4) {
      const int c = e1 - e;
      const int64_t j0 = a.col[e];
      const int64_t j1 = c > 1 ? a.col[e + 1] : j0, j2 = c > 2 ? a.col[e + 2] : j0, j3 = c > 3 ? a.col[e + 3] : j0;
      const float4 v0 = *reinterpret_cast<const float4*>(a.h + j0 * ld + qoff);
      const float4 v1 = *reinterpret_cast<const float4*>(a.h + j1 * ld + qoff);
      const float4 v2 = *reinterpret_cast<const float4*>(a.h + j2 * ld + qoff);
      const float4 v3 = *reinterpret_cast<const float4*>(a.h + j3 * ld + qoff);
      GL_ADD(v0, j0)
      if (c > 1) { GL_ADD(v1, j1) }
      if (c > 2) { GL_ADD(v2, j2) }
      if (c > 3) { GL_ADD(v3, j3) }
    }
#undef GL_ADD
    const float gh = 1.f - gq;
    const float4 hh = make_float4(gq * lo.x + gh * hi.x, gq * lo.y + gh * hi.y, gq * lo.z + gh * hi.z,
                                  gq * lo.w + gh * hi.w);
    const float mx = gl_groupmax(fmaxf(gl_absmax4(hh), gl_absmax4(hv)));
    const float sc = f16_scale_for(mx);
    if (l16 == 0) rinv[r] = pow2_inverse(sc);
    gl_put(A, r, 4 * l16, hh, sc);
    gl_put(A, r, 64 + 4 * l16, hv, sc);
  }
  __syncthreads();

  // ---- products ----------------------------------------------------------------------------------------------------
  f32x4 accH[4], accP[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) accH[t][e] = accP[t][e] = 0.f;
  gl_product<4>(A, 0, lane, wh, wl, accH);
  gl_product<2>(A, 64, lane, ph, pl, accP);

  // ---- epilogue: out = relu(. + C3 V), then the accumulator ----------------------------------------------------------
  // C/D layout of the 16x16 MFMA: column = lane & 15, row = 4 (lane >> 4) + reg of each 16-row tile
  const float winv = a.w_scale[1], pinv = a.p_scale[1];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * t + 4 * kq + e;
      int64_t row = m0 + r;
      row = row < R ? row : R - 1;
      const int q = (int)((uint32_t)(q0 + (int)(row - m0)) % (uint32_t)Q);
      const float* c = a.c3 + row * 3;
      const float* vq = a.v + (int64_t)q * 192 + n;
      float y = accH[t][e] * (rinv[r] * winv);
      y += c[0] * vq[0] + c[1] * vq[64] + c[2] * vq[128];
      y = y > 0.f ? y : 0.f;
      if (m0 + r < R) a.out[row * 64 + n] = y;
      if (LAST) F[r * GL_FST + n] = y;
    }
  }
  f32x4 accN[4];
  if (LAST) {
    // out Pn: the output rows through the same scaled split (the A image's first half; every wave is done with it)
    f16x8 nh[2], nl[2];
    gl_load_b<64>(a.pn, n, kq, nh, nl);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const int r = grp + 16 * k;
      const float4 yv = *reinterpret_cast<const float4*>(F + r * GL_FST + 4 * l16);
      const float sc = f16_scale_for(gl_groupmax(gl_absmax4(yv)));
      if (l16 == 0) rinv2[r] = pow2_inverse(sc);
      gl_put(A, r, 4 * l16, yv, sc);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) accN[t][e] = 0.f;
    gl_product<2>(A, 0, lane, nh, nl, accN);
  }
  const float pninv = LAST ? a.pn_scale[1] : 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * t + 4 * kq + e;
      const int64_t row = m0 + r;
      if (row < R) {
        float s = a.acc[row * 64 + n] + accP[t][e] * (rinv[r] * pinv);
        if (LAST) s += accN[t][e] * (rinv2[r] * pninv);
        a.acc[row * 64 + n] = s;
      }
    }
  }
}

template <bool LAST>
int launch_gossip_layer(const GossipLayerArgs& g, int64_t blocks, hipStream_t stream) {
  const size_t lds = (size_t)2 * GL_APLANE * sizeof(short) + 2 * GL_ROWS * sizeof(float) +
                     (LAST ? (size_t)GL_ROWS * GL_FST * sizeof(float) : 0);
  hipLaunchKernelGGL((gossip_layer_kernel<LAST>), dim3((unsigned)blocks), dim3(256), lds, stream, g);
  return launch_status("desco_gossip_layer_f16x3_f32");
}

}  // namespace

}  // namespace desco

using namespace desco;

extern "C" int desco_gossip_layer_f16x3_f32(const float* h, const int32_t* rowptr, const int32_t* col,
                                            int64_t num_nodes, int num_q, const float* g, const float* c3,
                                            const float* v, const int16_t* w_planes, const float* w_scale,
                                            const int16_t* p_planes, const float* p_scale,
                                            const int16_t* pn_planes, const float* pn_scale, float* acc, float* out,
                                            desco_stream_t stream) {
  if (num_nodes < 0 || num_q < 1)
    return fail(DESCO_EINVAL, "desco_gossip_layer_f16x3_f32: bad argument (num_nodes >= 0, num_q >= 1)");
  if (num_nodes == 0) return 0;
  if (!h || !rowptr || !col || !g || !c3 || !v || !w_planes || !w_scale || !p_planes || !p_scale || !acc || !out ||
      (pn_planes != nullptr) != (pn_scale != nullptr))
    return fail(DESCO_EINVAL, "desco_gossip_layer_f16x3_f32: bad argument (a required pointer is NULL, or only one of "
                              "pn_planes / pn_scale is given)");
  if (mis16(h) || mis16(acc) || mis16(out) || mis16(w_planes) || mis16(p_planes) || (pn_planes && mis16(pn_planes)))
    return fail(DESCO_EINVAL, "desco_gossip_layer_f16x3_f32: bad argument (h, acc, out and the planes must be 16-byte "
                              "aligned)");
  if (out == h || acc == h || acc == out)
    return fail(DESCO_EINVAL, "desco_gossip_layer_f16x3_f32: bad argument (out, acc and h must be distinct buffers)");
  if (num_nodes > INT64_MAX / num_q / 64)
    return fail(DESCO_EINVAL, "desco_gossip_layer_f16x3_f32: too many rows");
  const int64_t rows = num_nodes * num_q;
  const int64_t blocks = (rows + GL_ROWS - 1) / GL_ROWS;
  if (blocks > INT32_MAX) return fail(DESCO_EINVAL, "desco_gossip_layer_f16x3_f32: too many rows");
  GossipLayerArgs a{h, rowptr, col, num_nodes, num_q, g, c3, v, reinterpret_cast<const short*>(w_planes), w_scale,
                    reinterpret_cast<const short*>(p_planes), p_scale, reinterpret_cast<const short*>(pn_planes),
                    pn_scale, acc, out};
  hipStream_t st = (hipStream_t)stream;
  return pn_planes ? launch_gossip_layer<true>(a, blocks, st) : launch_gossip_layer<false>(a, blocks, st);
}
