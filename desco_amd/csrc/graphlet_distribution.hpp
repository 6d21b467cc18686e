// The arithmetic of the graphlet degree distributions and their agreement, for both sides of the compiler: the gfx950
// kernels (graphlet_distribution_dev.hip) and the host twin (graphlet_distribution.cpp).  Definitions:
// include/desco_hip.h, "GRAPHLET DEGREE DISTRIBUTION".
//
//   S_i  = (double)d_i / (double)k_i                 (k_i the i-th distinct value >= 1 of the column, d_i its rows)
//   T    = T + S_i, i ascending from T = 0;  N_i = S_i / T
//   acc  = fma(t, t, acc) over the union of two key lists in ascending key, t = N_x(k) - N_y(k) (a missing key: 0)
//   A_c  = D > 1 ? 0 : 1 - D,  D = sqrt(0.5 * acc);  agree = (A_0 + A_1 + ... in that order) / (double)C
// Every floating-point step is one correctly rounded IEEE operation on both sides and none can be contracted with
// another (no product feeds a sum except inside the written fma), so the two sides are expected to agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DESCO_GDD_HD __host__ __device__ inline
#else
#define DESCO_GDD_HD inline
#endif

namespace desco {
namespace gdd {

constexpr int kMaxColumns = 128;                     // DESCO_GCM_MAX_COLUMNS

DESCO_GDD_HD double share(int64_t d, int64_t k) { return (double)d / (double)k; }

// the squared-difference chain of two lists over the union of their keys, ascending
DESCO_GDD_HD double merge_chain(const int64_t* kx, const double* vx, int64_t lx, const int64_t* ky, const double* vy,
                                int64_t ly) {
  double acc = 0.0;
  int64_t a = 0, b = 0;
  while (a < lx && b < ly) {
    const int64_t ka = kx[a], kb = ky[b];
    double t;
    if (ka == kb) {
      t = vx[a] - vy[b];
      ++a, ++b;
    } else if (ka < kb) {
      t = vx[a];
      ++a;
    } else {
      t = -vy[b];
      ++b;
    }
    acc = fma(t, t, acc);
  }
  for (; a < lx; ++a) acc = fma(vx[a], vx[a], acc);
  for (; b < ly; ++b) {
    const double t = -vy[b];
    acc = fma(t, t, acc);
  }
  return acc;
}

DESCO_GDD_HD double agreement(double acc) {
  const double D = sqrt(0.5 * acc);
  return D > 1.0 ? 0.0 : 1.0 - D;
}

}  // namespace gdd
}  // namespace desco
