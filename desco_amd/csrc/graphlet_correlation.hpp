// The arithmetic of the graphlet correlation matrices and distances, for both sides of the compiler: the gfx950 kernels
// (graphlet_correlation_dev.hip) and the host twin (graphlet_correlation.cpp).  Definitions: include/desco_hip.h,
// "GRAPHLET CORRELATION".
//
//   d[i][c]  = 2 less + equal - n'          (int32; |d| < n')
//   S[a][b]  = sum_i d[i][a] d[i][b]        (int64; exact while n'^3 < 2^63)
//   rho[a][b] = (double)S[a][b] / sqrt((double)S[a][a] * (double)S[b][b]),  1 on the diagonal, 0 beside a constant column
//   gcd(x, y) = sqrt(acc),  acc = fma(t, t, acc) with t = x[p] - y[p], p ascending from acc = 0
// Every floating-point step is one correctly rounded IEEE operation on both sides and none can be contracted with
// another (the product feeds a square root, the difference feeds both operands of the fma), so the two sides are
// expected to agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DESCO_GCM_HD __host__ __device__ inline
#else
#define DESCO_GCM_HD inline
#endif

namespace desco {
namespace gcm {

constexpr int64_t kMaxRows = 2097151;                // n'^3 < 2^63
constexpr int kMaxColumns = 128;                     // DESCO_GCM_MAX_COLUMNS

DESCO_GCM_HD double rho(int64_t sab, int64_t saa, int64_t sbb) {
  if (saa == 0 || sbb == 0) return 0.0;
  const double den = sqrt((double)saa * (double)sbb);
  return (double)sab / den;
}

// position of (a, b), a < b, in the row-major upper triangle of a C x C matrix
DESCO_GCM_HD int64_t pair_index(int a, int b, int C) { return (int64_t)a * (2 * C - a - 1) / 2 + (b - a - 1); }

}  // namespace gcm
}  // namespace desco
