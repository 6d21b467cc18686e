// Arguments of the fused SHMP layer kernels (shmp_layer.hip: the f32 form, 32-row wave tiles; shmp_layer16.hip: the
// bf16x6 and f16x3 split forms, 16-row wave tiles).
#pragma once
#include <stdint.h>
#include "common_host.hpp"

namespace desco {

constexpr int MAXS = 4;       // relation slots stored per row

struct ShmpArgs {
  const float* x;
  int64_t ldx;
  const int32_t* vrowptr;
  const int32_t* vcol;
  int64_t row0, num_rows;
  int S, sm, st;
  // (16-row form, NARROW instantiations only: st = 2, ytab = the [n, 64] block of ONE table slot at column 0, ldy = 64)  bit t:
  // the caller asserts that table slot t (CSR slot sm + t) has no entry in the whole block -- molecule graphs have no
  // triangles, so the canonical->count triangle relation (table slot 0) is empty; that slot is neither tested for nor read
  // (desco_shmp_layer_narrow_f16x3_f32).  Sits in what was padding: the other members keep their offsets.
  int tab_empty;
  const float* wt;          // f32 mode: [(sm+1)*64][64]
  const short* wplanes;     // x6 mode: [3][64 n][(sm+1)*64 k] bf16 planes (hi, mid, lo); f16x3 mode: [2][64 n][..] fp16 (hi, lo)
  const float* wscale;      // f16x3 mode: device {scale, 1/scale} of the weight planes (desco_split_f16x2_f32); else null
  const float* bias;
  const float* ytab;
  int64_t ldy, ytab_row0;
  float* out;
  int64_t ldo;
  float* out2;              // optional second copy of the output rows (row i - row0 of a [num_rows, *] view)
  int64_t ldo2;
  float* row_absmax;        // optional (with out2): row_absmax[i - row0] = max(row_absmax[i - row0], max_c |out[i, c]|) -- the
                            // per-row bound desco_gemm_f16x3_f32 wants for the operand these rows are a column block of
  int act;                  // DESCO_ACT_* of the epilogue (relu for the SHMP layer)
  float slope;
  // fused pooling (global_add_pool of the produced rows, gnn_model.py:107; 16-row form only), optional: see
  // desco_shmp_layer_pool_bf16x6_f32 in desco_hip.h.  out may then be null (rows not stored).
  const uint32_t* pool_bits;   // [ceil(rows / 16)] bit r of word t: row 16 t + r is the last row of its segment
  const int32_t* pool_slot;    // [ceil(rows / 16)] first partial slot of 16-row tile t
  float* pool_part;            // [num slots][64] partial segment sums
  // round 6 (16-row form only): the launch's OWN rows (the self block's operand) read from another tensor than the gather
  // sources: row i of the launch at xself + i * ldxs (i = the same global row index that addresses x).  The canonical
  // launches use it to read their rows from the anchor operand's column block (row stride 576) -- the only place the
  // canonical rows are stored since -- and pass out = NULL (rows go to out2 alone).  NULL: the rows come from x.
  const float* xself;
  int64_t ldxs;
  // ... or not read at all: with self_coef [S + 1][64] the launch's own row i is RECOMPUTED from its S slot degrees d_s (the
  // tile's row pointers are in LDS anyway) as relu(coef[S] + sum_s d_s coef[s]) -- the closed-form first layer
  // (desco_degree_affine_f32's arithmetic, bit for bit).  With x = a table of the distinct rows of that layer's output and
  // column ids that address the table, X_1 [N, 64] need not exist (gnn_model.FIRST_LAYER_TABLE).
  const float* self_coef;
  // ... or read from the SAME table as the sources: with self_idx the launch's own row i is x + self_idx[i] * ldx (i = the
  // global row index that addresses vrowptr) -- x is a table of the distinct rows of the layer's input, vcol holds table
  // ids, and the input rows [N, 64] need not exist (desco_shmp_layer_selfidx_f16x3_f32; the pooled narrow fp16 form, with
  // neither xself nor self_coef).  Last member: the others keep their offsets.
  const int32_t* self_idx;
};

// The argument checks both forms share: operands present and 16-byte aligned (float4 loads and stores), slot counts
// within S <= MAXS, out / out2 not aliasing x.  Each form adds its own (slots_mfma bound, out, pooling, ...).
inline bool shmp_args_ok(const ShmpArgs& g, const void* weights) {
  return g.x && (g.vrowptr || g.S == 0) && weights && g.row0 >= 0 && g.num_rows >= 0 && g.sm >= 0 && g.st >= 0 &&
         g.st <= 2 && g.sm + g.st <= g.S && g.S <= MAXS && !(g.S == 0 && (g.sm || g.st)) && (g.st == 0 || g.ytab) &&
         g.ldx % 4 == 0 && (g.st == 0 || g.ldy % 4 == 0) && !mis16(g.x) && !mis16(weights) &&
         (g.st == 0 || !mis16(g.ytab)) && g.x != g.out && g.x != g.out2 && (!g.out || (!mis16(g.out) && g.ldo % 4 == 0)) &&
         (!g.out2 || (!mis16(g.out2) && g.ldo2 % 4 == 0));
}

}  // namespace desco
