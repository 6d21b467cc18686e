// Host twin of graph_tconv_dev.hip (C ABI: desco_graph_tconv), see include/desco_hip.h.
//
// The 2-slot typed CSR of whole graphs -- slot 0 = sources the row shares a neighbour with ("union_triangle"), slot 1
// = the others ("union_tride"); ToTconvHetero, transforms.py:180-255 -- from the definition: per row, per source, do
// the two sorted adjacency rows intersect?  The elements of the shorter row are looked up in the longer one.  Rows are
// independent (a row keeps all of its sources, re-ordered), so the loop over rows is the OpenMP loop.
#include <algorithm>
#include <cstdint>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/desco_hip.h"
#include "common_host.hpp"

namespace {

inline bool rows_intersect(const int32_t* col, int64_t a0, int64_t a1, int64_t b0, int64_t b1) {
  if (a1 - a0 > b1 - b0) {
    std::swap(a0, b0);
    std::swap(a1, b1);
  }
  for (int64_t i = a0; i < a1; ++i)
    if (std::binary_search(col + b0, col + b1, col[i])) return true;
  return false;
}

}  // namespace

extern "C" int desco_graph_tconv(const int64_t* rowptr, const int32_t* col, int64_t node0, int64_t num_nodes,
                                 int32_t* vrowptr, int32_t* vcol, int num_threads) {
  if (!rowptr || !vrowptr || node0 < 0 || num_nodes < 0 || 2 * num_nodes + 1 > INT32_MAX)
    return desco::fail(DESCO_EINVAL, "desco_graph_tconv: bad argument or more than 2^31 rows");
  const int64_t edge0 = rowptr[node0], num_edges = rowptr[node0 + num_nodes] - edge0;
  if (num_edges < 0 || num_edges > INT32_MAX || (num_edges > 0 && (!col || !vcol)))
    return desco::fail(DESCO_EINVAL, "desco_graph_tconv: bad argument or more than 2^31 edges");
#ifdef _OPENMP
  const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 256) num_threads(nt)
#endif
  for (int64_t i = 0; i < num_nodes; ++i) {
    const int64_t d = node0 + i, r0 = rowptr[d], r1 = rowptr[d + 1];
    std::vector<int32_t> tride;
    int64_t out = r0 - edge0;
    vrowptr[2 * i] = (int32_t)out;
    for (int64_t e = r0; e < r1; ++e) {
      const int64_t s = col[e];
      const bool tri = s >= node0 && s < node0 + num_nodes && rows_intersect(col, rowptr[s], rowptr[s + 1], r0, r1);
      if (tri)
        vcol[out++] = (int32_t)(s - node0);
      else
        tride.push_back((int32_t)(s - node0));
    }
    vrowptr[2 * i + 1] = (int32_t)out;
    std::copy(tride.begin(), tride.end(), vcol + out);
  }
  vrowptr[2 * num_nodes] = (int32_t)num_edges;
  return 0;
}
