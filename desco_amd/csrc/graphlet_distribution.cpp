// Graphlet degree distributions and their agreement, the host twin (C ABI: desco_gdd_build, desco_gdd_agreement).
// Definitions: include/desco_hip.h, "GRAPHLET DEGREE DISTRIBUTION"; the shared arithmetic: graphlet_distribution.hpp.
//
// Builder: per (segment, column) the values >= 1 are sorted and walked in runs; a run of d rows of value k is the entry
// (k, d / k), and the entries are divided by their sum taken in ascending key.  OpenMP over (segment, column).
// Agreement: per pair and column a two-pointer merge of the two lists, OpenMP over the rows of x.  Nothing depends on
// the thread count.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/desco_hip.h"
#include "common_host.hpp"
#include "graphlet_distribution.hpp"

#ifdef _OPENMP
#include <omp.h>
#endif

namespace gdd = desco::gdd;

extern "C" int desco_gdd_build(const int64_t* seg_ptr, int64_t num_segs, const int64_t* counts, int64_t ld,
                               const int32_t* columns, int C, int32_t* len, int64_t* key, double* val,
                               int num_threads) {
  if (num_segs < 0 || ld < 0) return desco::fail(DESCO_EINVAL, "desco_gdd_build: negative num_segs or ld");
  if (C < 1 || C > gdd::kMaxColumns)
    return desco::fail(DESCO_EINVAL, "desco_gdd_build: C is outside 1..128 (DESCO_GCM_MAX_COLUMNS)");
  if (num_segs == 0) return 0;
  if (!seg_ptr) return desco::fail(DESCO_EINVAL, "desco_gdd_build: seg_ptr is null");
  if (!columns) return desco::fail(DESCO_EINVAL, "desco_gdd_build: columns is null");
  if (!len) return desco::fail(DESCO_EINVAL, "desco_gdd_build: len is null");
  for (int c = 0; c < C; ++c)
    if (columns[c] < 0 || columns[c] >= ld)
      return desco::fail(DESCO_EINVAL, "desco_gdd_build: a column index is outside 0..ld-1");
  if (seg_ptr[0] < 0) return desco::fail(DESCO_EINVAL, "desco_gdd_build: seg_ptr is negative");
  for (int64_t s = 0; s < num_segs; ++s)
    if (seg_ptr[s + 1] < seg_ptr[s]) return desco::fail(DESCO_EINVAL, "desco_gdd_build: seg_ptr is not monotone");
  if (seg_ptr[num_segs] > seg_ptr[0]) {
    if (!counts) return desco::fail(DESCO_EINVAL, "desco_gdd_build: counts is null");
    if (!key || !val) return desco::fail(DESCO_EINVAL, "desco_gdd_build: key or val is null");
  }
#ifdef _OPENMP
  const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
  (void)num_threads;
#endif
  bool oom = false;
  const int64_t items = num_segs * C;
#pragma omp parallel num_threads(nt)
  {
    std::vector<int64_t> v;
#pragma omp for schedule(dynamic, 16)
    for (int64_t item = 0; item < items; ++item) try {
      const int64_t s = item / C;
      const int c = (int)(item - s * C);
      const int64_t r0 = seg_ptr[s], n = seg_ptr[s + 1] - r0;
      v.clear();
      const int64_t* src = counts + columns[c];
      for (int64_t i = 0; i < n; ++i) {
        const int64_t x = src[(r0 + i) * ld];
        if (x >= 1) v.push_back(x);
      }
      std::sort(v.begin(), v.end());
      int64_t* k = key + r0 * C + (int64_t)c * n;
      double* w = val + r0 * C + (int64_t)c * n;
      int64_t runs = 0;
      double T = 0.0;
      for (size_t g0 = 0; g0 < v.size();) {
        size_t g1 = g0 + 1;
        while (g1 < v.size() && v[g1] == v[g0]) ++g1;
        k[runs] = v[g0];
        w[runs] = gdd::share((int64_t)(g1 - g0), v[g0]);
        T = T + w[runs];
        ++runs;
        g0 = g1;
      }
      for (int64_t i = 0; i < runs; ++i) w[i] = w[i] / T;
      for (int64_t i = runs; i < n; ++i) k[i] = 0, w[i] = 0.0;
      len[s * C + c] = (int32_t)runs;
    } catch (const std::bad_alloc&) {
#pragma omp atomic write
      oom = true;
    }
  }
  if (oom) return desco::fail(DESCO_ENOMEM, "desco_gdd_build: out of memory");
  return 0;
}

namespace {

// the checks of one side of desco_gdd_agreement; nullptr when it is sound
const char* bad_side(const int64_t* seg_ptr, const int32_t* len, const int64_t* key, const double* val, int64_t G,
                     int C) {
  if (!seg_ptr) return "desco_gdd_agreement: seg_ptr is null";
  if (!len) return "desco_gdd_agreement: len is null";
  if (seg_ptr[0] < 0) return "desco_gdd_agreement: seg_ptr is negative";
  for (int64_t s = 0; s < G; ++s) {
    const int64_t n = seg_ptr[s + 1] - seg_ptr[s];
    if (n < 0) return "desco_gdd_agreement: seg_ptr is not monotone";
    for (int c = 0; c < C; ++c)
      if (len[s * C + c] < 0 || len[s * C + c] > n) return "desco_gdd_agreement: a len is outside 0..the segment's rows";
  }
  if (seg_ptr[G] > seg_ptr[0] && (!key || !val)) return "desco_gdd_agreement: key or val is null";
  return nullptr;
}

}  // namespace

extern "C" int desco_gdd_agreement(const int64_t* x_seg_ptr, const int32_t* x_len, const int64_t* x_key,
                                   const double* x_val, int64_t Gx, const int64_t* y_seg_ptr, const int32_t* y_len,
                                   const int64_t* y_key, const double* y_val, int64_t Gy, int C, double* agree,
                                   int64_t ldo, double* per_orbit, int num_threads) {
  if (Gx < 0 || Gy < 0) return desco::fail(DESCO_EINVAL, "desco_gdd_agreement: negative Gx or Gy");
  if (C < 1 || C > gdd::kMaxColumns)
    return desco::fail(DESCO_EINVAL, "desco_gdd_agreement: C is outside 1..128 (DESCO_GCM_MAX_COLUMNS)");
  if (Gx == 0 || Gy == 0) return 0;
  if (ldo < Gy) return desco::fail(DESCO_EINVAL, "desco_gdd_agreement: ldo is below Gy");
  if (!agree) return desco::fail(DESCO_EINVAL, "desco_gdd_agreement: agree is null");
  if (const char* m = bad_side(x_seg_ptr, x_len, x_key, x_val, Gx, C)) return desco::fail(DESCO_EINVAL, m);
  if (const char* m = bad_side(y_seg_ptr, y_len, y_key, y_val, Gy, C)) return desco::fail(DESCO_EINVAL, m);
#ifdef _OPENMP
  const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
  (void)num_threads;
#endif
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
  for (int64_t i = 0; i < Gx; ++i) {
    const int64_t x0 = x_seg_ptr[i], nx = x_seg_ptr[i + 1] - x0;
    for (int64_t j = 0; j < Gy; ++j) {
      const int64_t y0 = y_seg_ptr[j], ny = y_seg_ptr[j + 1] - y0;
      double sum = 0.0;
      for (int c = 0; c < C; ++c) {
        const int64_t px = x0 * C + (int64_t)c * nx, py = y0 * C + (int64_t)c * ny;
        const double acc = gdd::merge_chain(x_key + px, x_val + px, x_len[i * C + c], y_key + py, y_val + py,
                                            y_len[j * C + c]);
        const double A = gdd::agreement(acc);
        if (per_orbit) per_orbit[(i * Gy + j) * C + c] = A;
        sum = sum + A;
      }
      agree[i * ldo + j] = sum / (double)C;
    }
  }
  return 0;
}
