// Fused SHMP layer for gfx950: SAGEConv gather-aggregate for every relation slot, the per-relation
// Linear, the to_hetero sum, the update Linear and the ReLU (gnn_model.py:262-264, 273, 389-395) in
// ONE launch; the aggregates never touch HBM.
//
//   out[i] = relu( sum_{s<sm} (sum_{e in vrow(i,s)} x[vcol[e]]) * Wt[s] + x[i] * Wt[sm] + bias
//                  + sum_{sm<=s<sm+st} sum_{e in vrow(i,s)} ytab[vcol[e]-ytab_row0][(s-sm)*64 : +64] )
//
// "MFMA slots" (s < sm) are gathered into LDS and multiplied on the matrix cores; "table slots"
// are the same linear map re-associated, (sum_j x_j) W = sum_j (x_j W): their sources were already
// multiplied by W (ytab), so they are a row add in the epilogue.  The host uses the table form for
// the canonical->count relations (at most one source per row), cutting K from 320 to 192.
//
// Structure (wave-autonomous, persistent, software-pipelined):
//   * block = 8 waves = one CU (2 waves per SIMD, <= 256 VGPRs each); all (sm+1) 64x64 weight blocks
//     are loaded into LDS ONCE per block and stay resident while the block strides over 256-row tiles;
//   * every wave owns 32 destination rows of a tile end to end and never meets a block barrier in
//     the tile loop;
//   * the CSR slice of the wave's NEXT tile is prefetched under the current tile's work: its row
//     pointers into a second private LDS buffer, its first 256 source ids into registers that are
//     written over the (then dead) id buffer at the tile switch; ids 256..WCAP of a dense tile are
//     fetched at the switch;
//   * gathers are batched and branch-free: lane group g8 (8 lanes x float4) serves rows it*8+g8,
//     it = 0..3, and one step fetches two sources x both 128-B halves for all four rows = 16 loads
//     in flight together; absent sources read a row of zeros instead of being predicated away (a
//     load under a divergent branch is fenced by its own s_waitcnt and serialises the round trips);
//   * the first gather step of the next LIVE K block is issued BEFORE the MFMAs of block b, and the
//     first live block of the next tile before the epilogue stores of the current one, so
//     feature-row latency hides under the matrix work of the same wave; a relation slot without a
//     source in the wave's 32 rows is dead: no gather, no MFMAs (exact zeros);
//   * rows with more than 2 sources in a slot take up to EXTRA_STEPS more batched steps; beyond that
//     (hub rows, canonical rows of dense neighborhoods, ids past WCAP) they are finished
//     cooperatively by the whole wave (8 lane groups stride over one row's sources);
//   * table slots run as one extra pseudo K block: their pre-transformed source rows are gathered
//     the same way, staged in the A image and ADDED to the accumulators in the C/D layout;
//   * HBM traffic per row and layer: one 256-B read of x, one 256-B write, ~20 B of indices
//     (neighbour re-reads hit L2 / MALL: a neighborhood's rows are contiguous).
//
// Arithmetic: exact fp32, v_mfma_f32_32x32x2_f32 on an fp32 A image [32][33] and fp32 weights [K][64]
// (sm <= 3).  The split forms of the same layer (bf16x6, f16x3; fused pooling) run in 16-row wave tiles,
// shmp_layer16.hip.  This file also holds linear64_kernel, the layer's self block on its own in the bf16x6
// form (desco_linear64_bf16x6_f32).
#include "common_device.hpp"
#include "shmp_args.hpp"

namespace desco {

constexpr int WR = 32;        // rows per wave
constexpr int NW = 8;         // waves per block (2 per SIMD)
constexpr int AH = 33;        // half-K fp32 A image row stride (floats): conflict-free ds_read_b32
constexpr int APS = 40;       // half-K bf16 plane row stride (shorts, 80 B): conflict-free ds_read_b128
constexpr int RPN = WR * MAXS + 1;
constexpr int EXTRA_STEPS = 9; // batched 2-source steps after the prefetched one (<= 20 sources per row)
constexpr int WCAP = 512;     // source ids staged per wave (longer slices fall back to global);
                              // one buffer: the next tile's first 256 ids wait in registers until
                              // the switch, a denser tile fetches the rest then
constexpr int A_FLOATS = 3 * WR * APS / 2;               // A region per wave: max(32*33, 3*32*40/2) floats (the layer
                                                         // kernel's fp32 image, linear64_kernel's bf16 planes)
constexpr int WAVE_LDS = A_FLOATS + 2 * RPN + WCAP;      // floats per wave
static_assert(A_FLOATS >= WR * AH, "the fp32 image must fit in the plane region");

// absent sources of a batched gather step read this row instead of being predicated away
__device__ __attribute__((aligned(16))) float shmp_zero_row[64] = {};

__device__ __forceinline__ void f4add(float4& a, const float4 b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// ---- gather machinery: shmp_gather.hpp, over the rows it = 0..3 of a lane group; what differs from the 16-row
//      kernel follows here ----------------------------------------------------------------------------------
#define DESCO_ROWS(M, ...) M(0, ##__VA_ARGS__) M(1, ##__VA_ARGS__) M(2, ##__VA_ARGS__) M(3, ##__VA_ARGS__)
#include "shmp_gather.hpp"
// the row itself: rows beyond nr re-read the wave's last valid row (never stored)
#define DESCO_ISSUE_SELF(it_)                                                                  \
  {                                                                                            \
    const int r_ = (it_) * 8 + g8;                                                             \
    const float* p_ = xb + (grow0 + (r_ < nr ? r_ : nr - 1)) * LDX;                          \
    u##it_##0 = *reinterpret_cast<const float4*>(p_);                                          \
    u##it_##1 = *reinterpret_cast<const float4*>(p_ + 32);                                     \
  }
// first step of the table pseudo block (cursors: DESCO_TAB_CUR)
#define DESCO_ISSUE_TAB(it_)                                                                \
  {                                                                                         \
    DESCO_TAB_CUR(it_)                                                                      \
    const int i0_ = ec[k0_ ? ca_ : 0], i1_ = ec[k1_ ? na_ : 0];                             \
    const float* p0_ = k0_ ? yb + (int64_t)i0_ * LDY : zrow;                              \
    u##it_##0 = *reinterpret_cast<const float4*>(p0_);                                      \
    u##it_##1 = *reinterpret_cast<const float4*>(p0_ + 32);                                 \
    if (ST > 1) {                                                                           \
      const float* p1_ = k1_ ? yb + 64 + (int64_t)i1_ * LDY : zrow;                       \
      w##it_##0 = *reinterpret_cast<const float4*>(p1_);                                    \
      w##it_##1 = *reinterpret_cast<const float4*>(p1_ + 32);                               \
    }                                                                                       \
  }
// consume the step; leave the cursor of table slot 0 in (c, n) and of slot 1 in (d, m)
#define DESCO_CONSUME_TAB(it_)                                                              \
  {                                                                                         \
    DESCO_TAB_CUR(it_)                                                                      \
    f4add(lo##it_, u##it_##0);                                                              \
    f4add(hi##it_, u##it_##1);                                                              \
    if (ST > 1) {                                                                           \
      f4add(lo##it_, w##it_##0);                                                            \
      f4add(hi##it_, w##it_##1);                                                            \
    }                                                                                       \
    c##it_ = ca_ + (k0_ ? 1 : 0);                                                           \
    n##it_ = na_;                                                                           \
    d##it_ = na_ + (k1_ ? 1 : 0);                                                           \
    m##it_ = nb_;                                                                           \
  }
// first step of the first LIVE block after block a_ (a_ = -1: of the tile); dead slots are left
// out of the software pipeline altogether, so the block behind one is not issued late.  The slot
// index is a wave-uniform runtime value here (one copy of the gather issue code per site).
#define DESCO_ISSUE_AFTER(a_)                                                              \
  {                                                                                        \
    if ((a_) < KB - 1) {                                                                   \
      int nb_ = KB - 1;                                                                    \
      if ((a_) + 3 < KB - 1 && ((live >> ((a_) + 3)) & 1)) nb_ = (a_) + 3;                  \
      if ((a_) + 2 < KB - 1 && ((live >> ((a_) + 2)) & 1)) nb_ = (a_) + 2;                  \
      if ((a_) + 1 < KB - 1 && ((live >> ((a_) + 1)) & 1)) nb_ = (a_) + 1;                  \
      if (nb_ < KB - 1) {                                                                  \
        DESCO_CURS(nb_)                                                                    \
        DESCO_ROWS(DESCO_ISSUE2, xb, LDX)                                                  \
      } else {                                                                             \
        DESCO_ROWS(DESCO_ISSUE_SELF)                                                       \
      }                                                                                    \
    } else if ((a_) + 1 < NB) {                                                            \
      DESCO_ISSUE_BLOCK((a_) + 1)                                                          \
    }                                                                                      \
  }
// write one fp32 half image (every lane writes: row = it*8 + g8, 4 floats at 4*l8)
#define DESCO_PUT_F32(av_, it_)                         \
  {                                                     \
    float* d_ = Aw + ((it_) * 8 + g8) * AH + 4 * l8;    \
    d_[0] = av_.x;                                      \
    d_[1] = av_.y;                                      \
    d_[2] = av_.z;                                      \
    d_[3] = av_.w;                                      \
  }
// write one half image as three bf16 planes (row = it*8 + g8, 4 bf16 at 4*l8 of every plane)
#define DESCO_PUT_X6(av_, it_)                                                  \
  {                                                                             \
    uint32_t h0_, m0_, l0_, h1_, m1_, l1_;                                      \
    split2_bf16x3(av_.x, av_.y, h0_, m0_, l0_);                                   \
    split2_bf16x3(av_.z, av_.w, h1_, m1_, l1_);                                   \
    short* d_ = Ap + ((it_) * 8 + g8) * APS + 4 * l8;                           \
    *reinterpret_cast<uint2*>(d_) = make_uint2(h0_, h1_);                       \
    *reinterpret_cast<uint2*>(d_ + WR * APS) = make_uint2(m0_, m1_);            \
    *reinterpret_cast<uint2*>(d_ + 2 * WR * APS) = make_uint2(l0_, l1_);        \
  }
// 32 f32 MFMAs on the staged half h_ of K block b_: A[i = lane&31][k = lane>>5], B[k][j = lane&31]
#define DESCO_MFMA_HALF_F32(b_, h_)                                                        \
  {                                                                                        \
    const float* as_ = Aw + (lane & 31) * AH + (lane >> 5);                                \
    const float* bs_ = Bimg + ((b_) * 64 + (h_) * 32 + (lane >> 5)) * 64 + (lane & 31);    \
    _Pragma("unroll") for (int kk = 0; kk < 16; ++kk) {                                    \
      const float a_ = as_[2 * kk];                                                        \
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_, bs_[2 * kk * 64], acc0, 0, 0, 0);    \
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_, bs_[2 * kk * 64 + 32], acc1, 0, 0, 0); \
    }                                                                                      \
  }
// 24 bf16 MFMAs (6-product split) on the staged half: lane (r = lane&31, q = lane>>5) holds
// A[row r][k = 16 s + 8 q + 0..7] and B[k = 16 s + 8 q + 0..7][col r] of every plane
#define DESCO_MFMA_HALF_X6(b_, h_)                                                                \
  {                                                                                               \
    const short* ap_ = Ap + (lane & 31) * APS + 8 * (lane >> 5);                                  \
    const short* bp_ = Wp + (lane & 31) * WST + (b_) * 64 + (h_) * 32 + 8 * (lane >> 5);          \
    _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_) {                                            \
      const bf16x8 ah_ = *reinterpret_cast<const bf16x8*>(ap_ + 16 * s_);                         \
      const bf16x8 am_ = *reinterpret_cast<const bf16x8*>(ap_ + WR * APS + 16 * s_);              \
      const bf16x8 al_ = *reinterpret_cast<const bf16x8*>(ap_ + 2 * WR * APS + 16 * s_);          \
      const bf16x8 b0h_ = *reinterpret_cast<const bf16x8*>(bp_ + 16 * s_);                        \
      const bf16x8 b0m_ = *reinterpret_cast<const bf16x8*>(bp_ + WPL + 16 * s_);                  \
      const bf16x8 b0l_ = *reinterpret_cast<const bf16x8*>(bp_ + 2 * WPL + 16 * s_);              \
      const bf16x8 b1h_ = *reinterpret_cast<const bf16x8*>(bp_ + 32 * WST + 16 * s_);             \
      const bf16x8 b1m_ = *reinterpret_cast<const bf16x8*>(bp_ + 32 * WST + WPL + 16 * s_);       \
      const bf16x8 b1l_ = *reinterpret_cast<const bf16x8*>(bp_ + 32 * WST + 2 * WPL + 16 * s_);   \
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_, b0h_, acc0, 0, 0, 0);                   \
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_, b1h_, acc1, 0, 0, 0);                   \
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_, b0l_, acc0, 0, 0, 0);                   \
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_, b1l_, acc1, 0, 0, 0);                   \
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am_, b0m_, acc0, 0, 0, 0);                   \
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am_, b1m_, acc1, 0, 0, 0);                   \
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am_, b0h_, acc0, 0, 0, 0);                   \
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am_, b1h_, acc1, 0, 0, 0);                   \
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_, b0m_, acc0, 0, 0, 0);                   \
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_, b1m_, acc1, 0, 0, 0);                   \
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_, b0h_, acc0, 0, 0, 0);                   \
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_, b1h_, acc1, 0, 0, 0);                   \
    }                                                                                             \
  }
// add the staged (fp32) table half rows in the C/D layout: acc[reg] += stage[row(reg)][lane&31]
#define DESCO_TAB_HALF(acc_)                                                               \
  {                                                                                        \
    _Pragma("unroll") for (int reg = 0; reg < 16; ++reg)                                   \
        acc_[reg] += Aw[((reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)) * AH + cl];         \
  }

// KB = sm + 1 resident weight blocks (1..4), ST table slots (0..2), LD64: x rows are 64 floats and ytab
// rows 64*ST floats apart (the product path's layouts): source-row addresses then need a shift instead of a
// 64-bit multiply per gathered row
template <int KB, int ST, bool LD64>
__global__ __launch_bounds__(NW * 64) void shmp_layer_f32_kernel(ShmpArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int W_FLOATS = KB * 64 * 64;
  float* Bimg = lds;                                       // [KB*64][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* Aw = lds + W_FLOATS + wave * WAVE_LDS;            // fp32 half image [32][33]
  int* rpb = reinterpret_cast<int*>(Aw + A_FLOATS);        // 2 x [32*S+1] row pointers (absolute)
  int* ec = rpb + 2 * RPN;                                 // [WCAP] source ids of the current tile

  // ---- resident weights -------------------------------------------------------------------
  for (int i = tid; i < KB * 1024; i += NW * 64)
    *reinterpret_cast<float4*>(Bimg + 4 * i) = *reinterpret_cast<const float4*>(g.wt + 4 * i);
  __syncthreads();

  const int g8 = lane >> 3, l8 = lane & 7;                 // 8 groups of 8 lanes: one half row each
  const int cl = lane & 31;
  const int S = g.S;
  const int nslot = WR * S + 1;                            // <= 129: at most 3 per lane
  const int64_t ntiles = (g.num_rows + NW * WR - 1) / (NW * WR);
  constexpr int NB = KB + (ST > 0 ? 1 : 0);                // K blocks incl. the table pseudo block
  const int64_t LDX = LD64 ? 64 : g.ldx, LDY = LD64 ? 64 * (ST > 0 ? ST : 1) : g.ldy;
  const float* xb = g.x + 4 * l8;
  const float* yb = ST > 0 ? g.ytab + 4 * l8 - g.ytab_row0 * LDY : nullptr;
  const float* zrow = shmp_zero_row + 4 * l8;
  (void)yb;

  // ---- this wave's first tile (XCD-aware order: shmp_gather.hpp) --------------------------------
  int64_t tile = xcd_first_tile(), tend = ntiles;
  int tstride = gridDim.x;
  int64_t w0 = tile * (NW * WR) + wave * WR;               // first row of this wave (relative)
  if (tile >= tend || w0 >= g.num_rows) return;            // no barrier below: idle waves may leave
  int nr = (int)((g.num_rows - w0) < WR ? (g.num_rows - w0) : WR);
  int64_t grow0 = g.row0 + w0;
  int cur = 0;
  int* rp = rpb;
  if (S > 0) {                                             // S == 0: no CSR at all (plain row-wise Linear)
    const int nptr = nr * S + 1;
    for (int i = lane; i < nslot; i += 64)
      rp[i] = g.vrowptr[grow0 * S + (i < nptr ? i : nptr - 1)];
    const int eb = rp[0], ecnt = rp[WR * S] - eb;
    for (int i = lane; i < ecnt && i < WCAP; i += 64) ec[i] = g.vcol[eb + i];
  } else if (lane == 0) {
    rp[0] = 0;
    rpb[RPN] = 0;
  }
  int ebase = rp[0];

  float4 lo0, lo1, lo2, lo3, hi0, hi1, hi2, hi3;           // gathered sums of the current block
  float4 u00, u01, u10, u11, u20, u21, u30, u31;           // in flight: first source (lo, hi) of row it
  float4 w00, w01, w10, w11, w20, w21, w30, w31;           // in flight: second source
  w00 = w01 = w10 = w11 = w20 = w21 = w30 = w31 = make_float4(0.f, 0.f, 0.f, 0.f);
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0, n0 = 0, n1 = 0, n2 = 0, n3 = 0;   // cursors [c, n) rel. to ebase
  // bit b: relation slot b has at least one source among this wave's 32 rows.  A slot that is empty
  // for the whole wave tile (triangle edges in molecule graphs, tride edges in clique unions) is an
  // all-zero K block: it is left out of the tile's block sequence (wave-uniform; it would add exact
  // zeros), and the first gather step of the block behind it is issued in its place
  int live = 0;
  DESCO_TILE_LIVE()
  DESCO_ISSUE_AFTER(-1)

  for (;;) {
    int* rpn = rpb + (cur ^ 1) * RPN;
    // ---- prefetch the row pointers of the next tile (registers now, LDS later) --------------
    const int64_t tn = tile + tstride;
    const int64_t w0n = tn * (NW * WR) + wave * WR;
    const bool has_next = tn < tend && w0n < g.num_rows;
    const int nrn = has_next ? (int)((g.num_rows - w0n) < WR ? (g.num_rows - w0n) : WR) : 0;
    int p0 = 0, p1 = 0, p2 = 0;
    if (has_next && S > 0) {
      const int nptr = nrn * S + 1;
      const int32_t* src = g.vrowptr + (g.row0 + w0n) * S;
      p0 = src[lane < nptr ? lane : nptr - 1];
      if (lane + 64 < nslot) p1 = src[lane + 64 < nptr ? lane + 64 : nptr - 1];
      if (lane + 128 < nslot) p2 = src[lane + 128 < nptr ? lane + 128 : nptr - 1];
    }
    int qn0 = 0, qn1 = 0, qn2 = 0, qn3 = 0;   // source ids of the next tile (registers until the tile ends)
    int ebn = 0, ecntn = 0;

    // ---- accumulator init: bias ----------------------------------------------------------------
    f32x16 acc0, acc1;
    {
      const float bv0 = g.bias ? g.bias[cl] : 0.f, bv1 = g.bias ? g.bias[32 + cl] : 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        acc0[i] = bv0;
        acc1[i] = bv1;
      }
    }
    // K blocks: b < KB-1 = relation slot b (gathered x rows), b == KB-1 = the row itself,
    // b == KB (ST > 0) = table pseudo block (gathered ytab rows, added in the C/D layout)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < KB - 1 && !((live >> b) & 1)) continue;      // empty relation slot (wave-uniform)
      // ---- complete the gather of block b ------------------------------------------------------
      DESCO_ZERO_SUMS()
      if (b < KB - 1) {
        DESCO_FINISH(xb, LDX)
      } else if (b == KB - 1) {
        lo0 = u00; hi0 = u01; lo1 = u10; hi1 = u11;
        lo2 = u20; hi2 = u21; lo3 = u30; hi3 = u31;
      } else {
        // canonical->count relations have at most one source per row: one step covers both table
        // slots; anything beyond that (general inputs) takes the cooperative path
        int d0, d1, d2, d3, m0, m1, m2, m3;
        DESCO_CONSUME_TAB(0) DESCO_CONSUME_TAB(1) DESCO_CONSUME_TAB(2) DESCO_CONSUME_TAB(3)
        if (__any((c0 < n0) | (c1 < n1) | (c2 < n2) | (c3 < n3))) {
          DESCO_COOP(0, yb, LDY) DESCO_COOP(1, yb, LDY) DESCO_COOP(2, yb, LDY)
          DESCO_COOP(3, yb, LDY)
        }
        if (ST > 1 && __any((d0 < m0) | (d1 < m1) | (d2 < m2) | (d3 < m3))) {
          c0 = d0; c1 = d1; c2 = d2; c3 = d3;
          n0 = m0; n1 = m1; n2 = m2; n3 = m3;
          DESCO_COOP(0, yb + 64, LDY) DESCO_COOP(1, yb + 64, LDY) DESCO_COOP(2, yb + 64, LDY)
          DESCO_COOP(3, yb + 64, LDY)
        }
      }
      if (b == KB - 1 && has_next) {
        // next tile's row pointers have landed: publish them, then fetch its source ids
        rpn[lane] = p0;
        if (lane + 64 < nslot) rpn[lane + 64] = p1;
        if (lane + 128 < nslot) rpn[lane + 128] = p2;
        ebn = rpn[0];
        ecntn = rpn[WR * S] - ebn;
        if (lane < ecntn) qn0 = g.vcol[ebn + lane];
        if (lane + 64 < ecntn) qn1 = g.vcol[ebn + lane + 64];
        if (lane + 128 < ecntn) qn2 = g.vcol[ebn + lane + 128];
        if (lane + 192 < ecntn) qn3 = g.vcol[ebn + lane + 192];
      }
      // ---- the two 32-column halves of block b; the first gather step of block b+1 goes out
      //      under this block's MFMAs (after the low halves have left their registers)
      DESCO_PUT_F32(lo0, 0) DESCO_PUT_F32(lo1, 1) DESCO_PUT_F32(lo2, 2) DESCO_PUT_F32(lo3, 3)
      DESCO_ISSUE_AFTER(b)
      if (b >= KB) {
        DESCO_TAB_HALF(acc0)
      } else {
        DESCO_MFMA_HALF_F32(b, 0)
      }
      DESCO_PUT_F32(hi0, 0) DESCO_PUT_F32(hi1, 1) DESCO_PUT_F32(hi2, 2) DESCO_PUT_F32(hi3, 3)
      if (b >= KB) {
        DESCO_TAB_HALF(acc1)
      } else {
        DESCO_MFMA_HALF_F32(b, 1)
      }
    }

    // ---- switch to the next tile: publish its source ids and launch its first gather step ------
    const int64_t grow_out = grow0;
    const int nr_out = nr;
    if (has_next) {
      if (lane < ecntn) ec[lane] = qn0;            // (the current tile's ids are dead by now)
      if (lane + 64 < ecntn) ec[lane + 64] = qn1;
      if (lane + 128 < ecntn) ec[lane + 128] = qn2;
      if (lane + 192 < ecntn) ec[lane + 192] = qn3;
      if (ecntn > 256) {                           // dense tile (wave-uniform): ids 256..511 now
        for (int i = 256 + lane; i < ecntn && i < WCAP; i += 64) ec[i] = g.vcol[ebn + i];
      }
      cur ^= 1;
      rp = rpn;
      ebase = ebn;
      tile = tn;
      w0 = w0n;
      nr = nrn;
      grow0 = g.row0 + w0n;
      DESCO_TILE_LIVE()
      DESCO_ISSUE_AFTER(-1)
    }

    // ---- epilogue: relu + store; C/D map col = lane&31, row = (reg&3)+8*(reg>>2)+4*(lane>>5) ----
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      acc0[reg] = apply_act(acc0[reg], g.act, g.slope);
      acc1[reg] = apply_act(acc1[reg], g.act, g.slope);
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int r = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      if (r < nr_out) {
        float* o = g.out + (grow_out + r) * g.ldo + cl;
        o[0] = acc0[reg];
        o[32] = acc1[reg];
        if (g.out2) {          // e.g. the canonical rows' column block of the anchor-MLP operand
          float* o2 = g.out2 + (grow_out - g.row0 + r) * g.ldo2 + cl;
          o2[0] = acc0[reg];
          o2[32] = acc1[reg];
        }
      }
    }
    if (!has_next) break;
  }
}

// ---- streaming row-wise Linear, K = 64 (desco_linear64_bf16x6_f32) ---------------------------------
// The layer kernel's self block on its own: no CSR, NJ resident 64x64 weight blocks (NJ output
// column blocks per pass over x, so x is read once per NJ*64 outputs), rows of the next tile in
// flight under the current tile's MFMAs and stores.
struct Lin64Args {
  const float* x;
  int64_t ldx;
  const short* wplanes;     // [NJ][3][64 n][64 k]
  const float* bias;        // [NJ*64] or null
  float* out;               // first of the NJ column blocks
  int64_t ldo;
  int64_t num_rows;
  int act;
  float slope;
};

template <int NJ>
__global__ __launch_bounds__(NW * 64) void linear64_kernel(Lin64Args g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int WST = 72, WPL = 64 * WST;                  // one weight block: [3][64][72] shorts
  constexpr int W_FLOATS = NJ * 3 * WPL / 2;
  short* wbase = reinterpret_cast<short*>(lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* Aw = lds + W_FLOATS + wave * A_FLOATS;
  short* Ap = reinterpret_cast<short*>(Aw);
  for (int i = tid; i < NJ * 3 * 64 * 8; i += NW * 64) {   // [NJ*3*64 rows][8 chunks of 8 shorts]
    const int row = i >> 3, ch = i & 7;
    *reinterpret_cast<uint4*>(wbase + row * WST + 8 * ch) =
        *reinterpret_cast<const uint4*>(g.wplanes + (int64_t)row * 64 + 8 * ch);
  }
  __syncthreads();
  const int g8 = lane >> 3, l8 = lane & 7, cl = lane & 31;
  const int64_t ntiles = (g.num_rows + NW * WR - 1) / (NW * WR);
  int64_t tile = blockIdx.x;
  int64_t w0 = tile * (NW * WR) + wave * WR;
  if (tile >= ntiles || w0 >= g.num_rows) return;
  const float* xb = g.x + 4 * l8;
  float4 u00, u01, u10, u11, u20, u21, u30, u31;
#define DESCO_LIN_LOAD(it_)                                                        \
  {                                                                                \
    const int64_t r_ = w0 + (it_) * 8 + g8;                                        \
    const float* p_ = xb + (r_ < g.num_rows ? r_ : g.num_rows - 1) * g.ldx;        \
    u##it_##0 = *reinterpret_cast<const float4*>(p_);                              \
    u##it_##1 = *reinterpret_cast<const float4*>(p_ + 32);                         \
  }
  // bias of the lane's two columns per output block, once: a load inside the tile loop is waited for at
  // the accumulator init, and vector memory returns in order -- the wait would also drain the prefetch of
  // the next tile's rows issued just before it
  float bv[NJ][2];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    bv[j][0] = g.bias ? g.bias[64 * j + cl] : 0.f;
    bv[j][1] = g.bias ? g.bias[64 * j + 32 + cl] : 0.f;
  }
  DESCO_LIN_LOAD(0) DESCO_LIN_LOAD(1) DESCO_LIN_LOAD(2) DESCO_LIN_LOAD(3)
  for (;;) {
    const float4 lo0 = u00, hi0 = u01, lo1 = u10, hi1 = u11, lo2 = u20, hi2 = u21, lo3 = u30, hi3 = u31;
    const int64_t row_out = w0;
    const int nr = (int)((g.num_rows - w0) < WR ? (g.num_rows - w0) : WR);
    const int64_t tn = tile + gridDim.x;
    const int64_t w0n = tn * (NW * WR) + wave * WR;
    const bool has_next = tn < ntiles && w0n < g.num_rows;
    if (has_next) {
      tile = tn;
      w0 = w0n;
      DESCO_LIN_LOAD(0) DESCO_LIN_LOAD(1) DESCO_LIN_LOAD(2) DESCO_LIN_LOAD(3)
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const short* Wp = wbase + j * 3 * WPL;
      f32x16 acc0, acc1;
      {
        const float bv0 = bv[j][0], bv1 = bv[j][1];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          acc0[i] = bv0;
          acc1[i] = bv1;
        }
      }
      DESCO_PUT_X6(lo0, 0) DESCO_PUT_X6(lo1, 1) DESCO_PUT_X6(lo2, 2) DESCO_PUT_X6(lo3, 3)
      DESCO_MFMA_HALF_X6(0, 0)
      DESCO_PUT_X6(hi0, 0) DESCO_PUT_X6(hi1, 1) DESCO_PUT_X6(hi2, 2) DESCO_PUT_X6(hi3, 3)
      DESCO_MFMA_HALF_X6(0, 1)
      if (nr == WR) {                       // whole tile: one base address, no per-row tests
        float* o = g.out + (row_out + 4 * (lane >> 5)) * g.ldo + 64 * j + cl;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int r = (reg & 3) + 8 * (reg >> 2);
          __builtin_nontemporal_store(apply_act(acc0[reg], g.act, g.slope), o + r * g.ldo);
          __builtin_nontemporal_store(apply_act(acc1[reg], g.act, g.slope), o + r * g.ldo + 32);
        }
      } else {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int r = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
          if (r < nr) {
            float* o = g.out + (row_out + r) * g.ldo + 64 * j + cl;
            o[0] = apply_act(acc0[reg], g.act, g.slope);
            o[32] = apply_act(acc1[reg], g.act, g.slope);
          }
        }
      }
    }
    if (!has_next) break;
  }
#undef DESCO_LIN_LOAD
}

template <int KB, int ST, bool LD64>
static hipError_t shmp_launch_one(const ShmpArgs& g, unsigned grid, hipStream_t st) {
  constexpr size_t shmem = sizeof(float) * ((size_t)KB * 64 * 64 + (size_t)NW * WAVE_LDS);
  static_assert(shmem <= 160 * 1024, "SHMP layer: LDS budget exceeded");
  const hipError_t e = size_dynamic_lds<shmp_layer_f32_kernel<KB, ST, LD64>>(160 * 1024);
  if (e == hipSuccess)
    hipLaunchKernelGGL((shmp_layer_f32_kernel<KB, ST, LD64>), dim3(grid), dim3(NW * 64), shmem, st, g);
  return e;
}

template <int KB>
static hipError_t shmp_launch_st(const ShmpArgs& g, unsigned grid, hipStream_t st) {
  const bool ld64 = g.ldx == 64 && (g.st == 0 || g.ldy == 64 * g.st);
#define DESCO_ONE(ST_) \
  return ld64 ? shmp_launch_one<KB, ST_, true>(g, grid, st) : shmp_launch_one<KB, ST_, false>(g, grid, st);
  switch (g.st) {
    case 0: DESCO_ONE(0)
    case 1: DESCO_ONE(1)
    default:
      if constexpr (KB <= 3) {           // sm + st <= 4 slots: four weight blocks leave room for one table slot
        DESCO_ONE(2)
      }
      return hipSuccess;
  }
#undef DESCO_ONE
}

}  // namespace desco

extern "C" int desco_shmp_layer_f32(const float* x, int64_t ldx, const int32_t* vrowptr,
                                    const int32_t* vcol, int64_t row0, int64_t num_rows,
                                    int slots_stored, int slots_mfma, int slots_table,
                                    const float* wt, const float* bias, const float* ytab,
                                    int64_t ldy, int64_t ytab_row0, float* out, int64_t ldo,
                                    float* out2, int64_t ldo2, desco_stream_t stream) {
  using namespace desco;
  if (num_rows == 0) return 0;
  ShmpArgs g{};
  g.x = x;
  g.ldx = ldx;
  g.vrowptr = vrowptr;
  g.vcol = vcol;
  g.row0 = row0;
  g.num_rows = num_rows;
  g.S = slots_stored;
  g.sm = slots_mfma;
  g.st = slots_table;
  g.wt = wt;
  g.bias = bias;
  g.ytab = ytab;
  g.ldy = ldy;
  g.ytab_row0 = ytab_row0;
  g.out = out;
  g.ldo = ldo;
  g.out2 = out2;
  g.ldo2 = ldo2;
  g.act = DESCO_ACT_RELU;
  if (!shmp_args_ok(g, wt) || slots_mfma > 3 || !out)
    return fail(DESCO_EINVAL, "desco_shmp_layer_f32: bad argument (slots_mfma <= 3, slots_table <= 2)");
  const unsigned grid = persistent_grid((num_rows + NW * WR - 1) / (NW * WR));
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  switch (slots_mfma) {
    case 0: e = shmp_launch_st<1>(g, grid, st); break;
    case 1: e = shmp_launch_st<2>(g, grid, st); break;
    case 2: e = shmp_launch_st<3>(g, grid, st); break;
    default: e = shmp_launch_st<4>(g, grid, st); break;
  }
  if (e != hipSuccess) return fail((int)e, "desco_shmp_layer_f32: cannot size LDS");
  return launch_status("desco_shmp_layer_f32");
}

// Row-wise Linear with K = 64 inputs (see linear64_kernel): out[i, 0:64*nb] = act(x[i, 0:64] * W^T + bias),
// w_planes = nb blocks [3][64 n][64 k].  Two column blocks per pass over x where possible.
extern "C" int desco_linear64_bf16x6_f32(const float* x, int64_t ldx, const int16_t* w_planes,
                                         int num_blocks, const float* bias, int act, float slope,
                                         float* out, int64_t ldo, int64_t num_rows,
                                         desco_stream_t stream) {
  using namespace desco;
  if (num_rows == 0 || num_blocks == 0) return 0;
  if (!x || !w_planes || !out || num_rows < 0 || num_blocks < 0 || ldx % 4 || mis16(x) ||
      mis16(w_planes) || x == out || mis16(out) || ldo % 4)
    return fail(DESCO_EINVAL, "desco_linear64_bf16x6_f32: bad argument");
  const unsigned grid = persistent_grid((num_rows + NW * WR - 1) / (NW * WR));
  hipError_t e = size_dynamic_lds<linear64_kernel<1>>(160 * 1024);
  if (e == hipSuccess) e = size_dynamic_lds<linear64_kernel<2>>(160 * 1024);
  if (e != hipSuccess) return fail((int)e, "desco_linear64_bf16x6_f32: cannot size LDS");
  constexpr size_t wave_bytes = sizeof(float) * (size_t)NW * A_FLOATS;
  for (int j = 0; j < num_blocks;) {
    const int nj = num_blocks - j >= 2 ? 2 : 1;
    Lin64Args a{x, ldx, reinterpret_cast<const short*>(w_planes) + (int64_t)j * 3 * 64 * 64,
                bias ? bias + 64 * j : nullptr, out + 64 * j, ldo, num_rows, act, slope};
    const size_t shmem = (size_t)nj * 3 * 64 * 72 * sizeof(short) + wave_bytes;
    if (nj == 2)
      hipLaunchKernelGGL(linear64_kernel<2>, dim3(grid), dim3(NW * 64), shmem, (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL(linear64_kernel<1>, dim3(grid), dim3(NW * 64), shmem, (hipStream_t)stream, a);
    j += nj;
  }
  return launch_status("desco_linear64_bf16x6_f32");
}
