// Gather machinery of the fused SHMP layer kernels, shared by shmp_layer.hip (32-row wave tiles: lane group g8 serves
// rows it * 8 + g8, it = 0..3) and shmp_layer16.hip (16-row wave tiles: it = 0, 1).  Macros: every temporary is a named
// register.  They use the enclosing scope's rp, ec, ebase, grow0, nr, xb, yb, zrow, g, S, g8, l8, KB and the
// registers lo*/hi* (sums), u*/w* (loads in flight), c*/n* (cursors).
//
// The including file supplies, before the first use:
//   DESCO_ROWS(M, ...)   M(it, ...) for every row `it` of a lane group: M(0, ...) M(1, ...) [M(2, ...) M(3, ...)]
//   WCAP, EXTRA_STEPS    ids staged per wave; batched two-source steps after the prefetched one
//   f4add(float4&, float4)
//   DESCO_ISSUE_SELF(it), DESCO_ISSUE_TAB(it)   first step of the self block / the table pseudo block (DESCO_ISSUE_BLOCK)
// What differs between the two tilings stays in their files: the self rows' registers, the live bits of the table slots,
// DESCO_ISSUE_AFTER, operand staging, the MFMA macros and the prefetch of the next tile.  The macros stay defined to
// the end of the including file (one translation unit per tiling).
// Included inside namespace desco, once per file.
#pragma once

// XCD-aware tile order: blocks b, b+8, b+16, ... share an XCD (round-robin dispatch) and its 4 MB L2,
// so a neighborhood's rows -- the sources of all its tiles -- should be gathered by ONE XCD.  Measured
// (profiles/r2_f_ab_xcd_order.log): +0.5 % on Syn_1827 / MSRC+IMDB shapes, 0 on COX2 shapes (the
// gathers are not what bounds the kernel); contiguous eighths per XCD were 8 % SLOWER on Syn shapes
// (the dataset is ordered by graph size: the XCD with the dense end finishes last).  Speed only: any
// block -> XCD placement gives the same result.
__device__ __forceinline__ int64_t xcd_first_tile() {
  // chunks of (grid / 8) consecutive tiles go round robin over the XCDs: XCD x works on the 32
  // neighbouring tiles of chunk 8 j + x in sweep j (locality), heavy and light regions of the dataset
  // are spread over all XCDs (balance)
  if ((gridDim.x & 7) == 0) return (int64_t)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  return blockIdx.x;
}

#define DESCO_CUR(it_, slot_)                              \
  {                                                        \
    const int v_ = ((it_) * 8 + g8) * S + (slot_);         \
    c##it_ = rp[v_] - ebase;                               \
    n##it_ = rp[v_ + 1] - ebase;                           \
  }
#define DESCO_CURS(slot_) DESCO_ROWS(DESCO_CUR, slot_)
// two sources of row it_ (staged ids only: e < WCAP), unconditional loads
#define DESCO_ISSUE2(it_, base_, ld_)                                                 \
  {                                                                                   \
    const int m_ = n##it_ < WCAP ? n##it_ : WCAP;                                     \
    const bool k0_ = c##it_ < m_, k1_ = c##it_ + 1 < m_;                              \
    const int i0_ = ec[k0_ ? c##it_ : 0], i1_ = ec[k1_ ? c##it_ + 1 : 0];             \
    const float* p0_ = k0_ ? (base_) + (int64_t)i0_ * (ld_) : zrow;                   \
    const float* p1_ = k1_ ? (base_) + (int64_t)i1_ * (ld_) : zrow;                   \
    u##it_##0 = *reinterpret_cast<const float4*>(p0_);                                \
    u##it_##1 = *reinterpret_cast<const float4*>(p0_ + 32);                           \
    w##it_##0 = *reinterpret_cast<const float4*>(p1_);                                \
    w##it_##1 = *reinterpret_cast<const float4*>(p1_ + 32);                           \
    c##it_ += (k0_ ? 1 : 0) + (k1_ ? 1 : 0);                                          \
  }
#define DESCO_CONSUME2(it_)                                                           \
  {                                                                                   \
    f4add(lo##it_, u##it_##0);                                                        \
    f4add(hi##it_, u##it_##1);                                                        \
    f4add(lo##it_, w##it_##0);                                                        \
    f4add(hi##it_, w##it_##1);                                                        \
  }
#define DESCO_ZERO_SUM(it_) lo##it_ = hi##it_ = make_float4(0.f, 0.f, 0.f, 0.f);
#define DESCO_ZERO_SUMS() { DESCO_ROWS(DESCO_ZERO_SUM) }
// "| row it_ has a staged id left" / "| row it_ has a source left" / "| row it_ has a source in slot s_"
#define DESCO_OR_STAGED(it_) | (c##it_ < (n##it_ < WCAP ? n##it_ : WCAP))
#define DESCO_OR_OPEN(it_) | (c##it_ < n##it_)
#define DESCO_OR_SOURCE(it_, s_) | (rp[((it_) * 8 + g8) * S + (s_) + 1] > rp[((it_) * 8 + g8) * S + (s_)])
#define DESCO_ANY_STAGED() __any(0 DESCO_ROWS(DESCO_OR_STAGED))
// table pseudo block: the first source of table slot 0 (-> u) and of table slot 1 (-> w) of row it_
#define DESCO_TAB_CUR(it_)                                                                  \
  const int v_ = ((it_) * 8 + g8) * S + g.sm;                                               \
  const int ca_ = rp[v_] - ebase, na_ = rp[v_ + 1] - ebase;                                 \
  const int nb_ = ST > 1 ? rp[v_ + 2] - ebase : na_;                                        \
  const bool k0_ = ca_ < (na_ < WCAP ? na_ : WCAP);                                         \
  const bool k1_ = ST > 1 && na_ < (nb_ < WCAP ? nb_ : WCAP);
// heavy rows (hub / canonical rows of dense neighborhoods, or ids beyond the staged WCAP): the
// whole wave cooperates on one row at a time -- lane group k takes sources c+k, c+k+8, ... and
// the 8 partial sums are folded with three xor-shuffles (lanes with equal l8 hold the same columns)
#define DESCO_COOP(it_, base_, ld_)                                                       \
  {                                                                                       \
    unsigned long long m_ = __ballot(c##it_ < n##it_);                                    \
    while (m_) {                                                                          \
      const int sl_ = __builtin_ctzll(m_);                                                \
      const int og_ = sl_ >> 3;                                                           \
      const int cc_ = __shfl(c##it_, sl_, 64), nn_ = __shfl(n##it_, sl_, 64);             \
      float4 p_ = make_float4(0.f, 0.f, 0.f, 0.f), q_ = p_;                               \
      for (int e_ = cc_ + g8; e_ < nn_; e_ += 8) {                                        \
        const int64_t j_ = e_ < WCAP ? ec[e_] : g.vcol[ebase + e_];                       \
        const float* s_ = (base_) + j_ * (ld_);                                           \
        const float4 v0_ = *reinterpret_cast<const float4*>(s_);                          \
        const float4 v1_ = *reinterpret_cast<const float4*>(s_ + 32);                     \
        f4add(p_, v0_);                                                                   \
        f4add(q_, v1_);                                                                   \
      }                                                                                   \
      _Pragma("unroll") for (int o_ = 8; o_ < 64; o_ <<= 1) {                             \
        p_.x += __shfl_xor(p_.x, o_, 64);                                                 \
        p_.y += __shfl_xor(p_.y, o_, 64);                                                 \
        p_.z += __shfl_xor(p_.z, o_, 64);                                                 \
        p_.w += __shfl_xor(p_.w, o_, 64);                                                 \
        q_.x += __shfl_xor(q_.x, o_, 64);                                                 \
        q_.y += __shfl_xor(q_.y, o_, 64);                                                 \
        q_.z += __shfl_xor(q_.z, o_, 64);                                                 \
        q_.w += __shfl_xor(q_.w, o_, 64);                                                 \
      }                                                                                   \
      if (g8 == og_) {                                                                    \
        f4add(lo##it_, p_);                                                               \
        f4add(hi##it_, q_);                                                               \
        c##it_ = n##it_;                                                                  \
      }                                                                                   \
      m_ &= ~(0xffULL << (og_ * 8));                                                      \
    }                                                                                     \
  }
// finish a gathered block whose first step is already in flight: consume it, up to EXTRA_STEPS more
// batched steps (two sources per row each: all rows of a lane group advance together), then
// the cooperative path for rows that are heavier still (one row at a time, the whole wave on it)
#define DESCO_FINISH(base_, ld_)                                                           \
  {                                                                                        \
    DESCO_ROWS(DESCO_CONSUME2)                                                             \
    for (int st_ = 0; st_ < EXTRA_STEPS && DESCO_ANY_STAGED(); ++st_) {                    \
      DESCO_ROWS(DESCO_ISSUE2, base_, ld_)                                                 \
      DESCO_ROWS(DESCO_CONSUME2)                                                           \
    }                                                                                      \
    if (__any(0 DESCO_ROWS(DESCO_OR_OPEN))) {                                              \
      DESCO_ROWS(DESCO_COOP, base_, ld_)                                                   \
    }                                                                                      \
  }
// first step of block b_ (cursors + loads); nothing waits on the loads here
#define DESCO_ISSUE_BLOCK(b_)                                                              \
  {                                                                                        \
    if ((b_) < KB - 1) {                                                                   \
      DESCO_CURS(b_)                                                                       \
      DESCO_ROWS(DESCO_ISSUE2, xb, LDX)                                                    \
    } else if ((b_) == KB - 1) {                                                           \
      DESCO_ROWS(DESCO_ISSUE_SELF)                                                         \
    } else {                                                                               \
      DESCO_ROWS(DESCO_ISSUE_TAB)                                                          \
    }                                                                                      \
  }
// bit s of `live`: relation slot s (an MFMA slot) has at least one source among the wave's rows
#define DESCO_SLOT_ANY(s_) (__any(0 DESCO_ROWS(DESCO_OR_SOURCE, s_)) != 0)
#define DESCO_SLOT_LIVE(s_) (DESCO_SLOT_ANY(s_) ? 1 << (s_) : 0)
#define DESCO_TILE_LIVE()                                        \
  {                                                              \
    live = 0;                                                    \
    if (KB - 1 > 0) live |= DESCO_SLOT_LIVE(0);                  \
    if (KB - 1 > 1) live |= DESCO_SLOT_LIVE(1);                  \
    if (KB - 1 > 2) live |= DESCO_SLOT_LIVE(2);                  \
  }
