// Graphlet correlation matrices and distances, the host twin (C ABI: desco_graphlet_correlation, desco_gcd_matrix).
// Definitions: include/desco_hip.h, "GRAPHLET CORRELATION"; the shared arithmetic: graphlet_correlation.hpp.
//
// Per segment and column the rows are sorted by value and walked in tie groups: a group that starts at sorted position
// s and holds e rows has less = s and equal = e, so d = 2 s + e - n' for each of its rows.  D is kept column-major, and
// S[a][b] is the int64 dot product of two of its columns.  OpenMP over segments; nothing depends on the thread count.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/desco_hip.h"
#include "common_host.hpp"
#include "graphlet_correlation.hpp"

#ifdef _OPENMP
#include <omp.h>
#endif

namespace gcm = desco::gcm;

extern "C" int desco_graphlet_correlation(const int64_t* seg_ptr, int64_t num_segs, const int64_t* counts, int64_t ld,
                                          const int32_t* columns, int C, int dummy_row, int64_t* S_out,
                                          double* rho_out, int num_threads) {
  if (num_segs < 0 || ld < 0) return desco::fail(DESCO_EINVAL, "desco_graphlet_correlation: negative num_segs or ld");
  if (C < 0 || C > gcm::kMaxColumns)
    return desco::fail(DESCO_EINVAL, "desco_graphlet_correlation: C is outside 0..128 (DESCO_GCM_MAX_COLUMNS)");
  if (dummy_row != 0 && dummy_row != 1)
    return desco::fail(DESCO_EINVAL, "desco_graphlet_correlation: dummy_row must be 0 or 1");
  if (num_segs == 0 || C == 0 || (!S_out && !rho_out)) return 0;
  if (!seg_ptr) return desco::fail(DESCO_EINVAL, "desco_graphlet_correlation: seg_ptr is null");
  if (!columns) return desco::fail(DESCO_EINVAL, "desco_graphlet_correlation: columns is null");
  for (int c = 0; c < C; ++c)
    if (columns[c] < 0 || columns[c] >= ld)
      return desco::fail(DESCO_EINVAL, "desco_graphlet_correlation: a column index is outside 0..ld-1");
  if (seg_ptr[0] < 0) return desco::fail(DESCO_EINVAL, "desco_graphlet_correlation: seg_ptr is negative");
  for (int64_t s = 0; s < num_segs; ++s) {
    if (seg_ptr[s + 1] < seg_ptr[s])
      return desco::fail(DESCO_EINVAL, "desco_graphlet_correlation: seg_ptr is not monotone");
    if (seg_ptr[s + 1] - seg_ptr[s] + dummy_row > gcm::kMaxRows)
      return desco::fail(DESCO_EINVAL,
                         "desco_graphlet_correlation: a segment has more than 2097151 rows (the int64 sums are exact "
                         "only below)");
  }
  if (seg_ptr[num_segs] > seg_ptr[0] && !counts)
    return desco::fail(DESCO_EINVAL, "desco_graphlet_correlation: counts is null");
#ifdef _OPENMP
  const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
  (void)num_threads;
#endif
  bool oom = false;
#pragma omp parallel num_threads(nt)
  {
    std::vector<int32_t> D;                          // [C][n'] column-major
    std::vector<int64_t> val, S;
    std::vector<int32_t> order;
#pragma omp for schedule(dynamic, 1)
    for (int64_t s = 0; s < num_segs; ++s) try {
      const int64_t r0 = seg_ptr[s], n = seg_ptr[s + 1] - r0, np = n + dummy_row;
      D.resize((size_t)C * (size_t)np);
      val.resize((size_t)np);
      order.resize((size_t)np);
      S.assign((size_t)C * C, 0);
      for (int c = 0; c < C; ++c) {
        const int64_t* src = counts + columns[c];
        for (int64_t i = 0; i < n; ++i) val[(size_t)i] = src[(r0 + i) * ld];
        if (dummy_row) val[(size_t)n] = 1;
        for (int64_t i = 0; i < np; ++i) order[(size_t)i] = (int32_t)i;
        std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return val[x] < val[y]; });
        int32_t* d = D.data() + (size_t)c * (size_t)np;
        for (int64_t g0 = 0; g0 < np;) {
          int64_t g1 = g0 + 1;
          while (g1 < np && val[order[(size_t)g1]] == val[order[(size_t)g0]]) ++g1;
          const int32_t rank = (int32_t)(2 * g0 + (g1 - g0) - np);
          for (int64_t j = g0; j < g1; ++j) d[order[(size_t)j]] = rank;
          g0 = g1;
        }
      }
      for (int a = 0; a < C; ++a)
        for (int b = a; b < C; ++b) {
          const int32_t* x = D.data() + (size_t)a * (size_t)np;
          const int32_t* y = D.data() + (size_t)b * (size_t)np;
          int64_t acc = 0;
          for (int64_t i = 0; i < np; ++i) acc += (int64_t)x[i] * (int64_t)y[i];
          S[(size_t)a * C + b] = S[(size_t)b * C + a] = acc;
        }
      if (S_out) std::memcpy(S_out + (size_t)s * C * C, S.data(), sizeof(int64_t) * (size_t)C * C);
      if (rho_out) {
        double* r = rho_out + (size_t)s * C * C;
        for (int a = 0; a < C; ++a)
          for (int b = 0; b < C; ++b)
            r[(size_t)a * C + b] =
                a == b ? 1.0 : gcm::rho(S[(size_t)a * C + b], S[(size_t)a * C + a], S[(size_t)b * C + b]);
      }
    } catch (const std::bad_alloc&) {
#pragma omp atomic write
      oom = true;
    }
  }
  if (oom) return desco::fail(DESCO_ENOMEM, "desco_graphlet_correlation: out of memory");
  return 0;
}

extern "C" int desco_gcd_matrix(const double* x, int64_t Gx, const double* y, int64_t Gy, int64_t P, double* out,
                                int64_t ldo, int num_threads) {
  if (Gx < 0 || Gy < 0 || P < 0) return desco::fail(DESCO_EINVAL, "desco_gcd_matrix: negative Gx, Gy or P");
  if (Gx == 0 || Gy == 0) return 0;
  if (ldo < Gy) return desco::fail(DESCO_EINVAL, "desco_gcd_matrix: ldo is below Gy");
  if (!out) return desco::fail(DESCO_EINVAL, "desco_gcd_matrix: out is null");
  if (P > 0 && (!x || !y)) return desco::fail(DESCO_EINVAL, "desco_gcd_matrix: x or y is null");
#ifdef _OPENMP
  const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
  (void)num_threads;
#endif
#pragma omp parallel for schedule(static) num_threads(nt)
  for (int64_t i = 0; i < Gx; ++i) {
    const double* xi = x + i * P;
    for (int64_t j = 0; j < Gy; ++j) {
      const double* yj = y + j * P;
      double acc = 0.0;
      for (int64_t p = 0; p < P; ++p) {
        const double t = xi[p] - yj[p];
        acc = std::fma(t, t, acc);
      }
      out[i * ldo + j] = std::sqrt(acc);
    }
  }
  return 0;
}
