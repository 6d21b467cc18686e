// Device-side batch set-up (C ABI: desco_partition_dev_slice, desco_partition_dev_degree_sort, desco_pool_index_dev,
// desco_neigh_rows_dev), see include/desco_hip.h.
//
// What lies between the device partition builder (partition_dev.hip) and the arrays the layer kernels read, as integer
// kernels that reproduce the host routines bit for bit (NeighborhoodPartition.slice, desco_partition_degree_sort,
// NeighborhoodBatch.pool_index, the scatter / segment indices of InferencePipeline):
//
//   slice        one element-wise launch: the four arrays of neighborhoods [b0, b1) re-based to a block of their own
//   degree sort  1. one workgroup per neighborhood: slot totals -> primary slot, 64-bit keys, the stable order, then
//                   count_orig_out and the rows' new vrowptr by a workgroup scan.  Up to kRankRows rows (one wavefront
//                   per neighborhood): rank by counting, keys in LDS.  Above: (key, old index) pairs sorted in LDS by
//                   a bitonic network.  Above kSortLdsRows rows (more than the device builder can emit): keys in the
//                   caller's workspace, rank by counting there -- slower, same result.  A neighborhood's rows are
//                   only permuted among themselves, so its first edge offset is the old one and no scan crosses a
//                   neighborhood.
//                2. one wavefront per row: sources copied to their new place, renamed through new_of_old
//                3. one wavefront per row: every (row, slot) segment sorted ascending by rank counting, any length
//   pool index   one thread per 16-row tile (binary search of the tile's first neighborhood, walk over the ends inside
//                the tile), then one workgroup scans the tiles' slot counts and reduces the neighborhood sizes
//   neigh rows   one thread per neighborhood / per graph (binary search: neighborhoods are ordered by graph)
//
// Rank counting is quadratic in the rows: with the keys in LDS every lane of a wavefront reads the same key (a
// broadcast), 256 rows are 1024 steps per lane.  The pair sort of a 4400-row neighborhood (the largest the device
// builder accepts) is 91 exchange steps of 16 pairs per thread.  No result depends on the order in which workgroups or
// wavefronts arrive: every output element has exactly one writer and there is no atomic.
#include "common_device.hpp"

namespace desco {

constexpr int kRankRows = 256;          // up to here a wavefront ranks a neighborhood's rows by counting
constexpr int kSortLdsRows = 4608;      // (key, index) pairs held in LDS (54 KB): above the device builder's largest graph

// ---------------------------------------------------------------------------------------------- slice
__global__ __launch_bounds__(256) void part_slice_kernel(const int32_t* __restrict__ cp, const int32_t* __restrict__ vr,
                                                         const int32_t* __restrict__ vcol,
                                                         const int32_t* __restrict__ corig, int64_t Nc, int64_t b0,
                                                         int64_t b1, int32_t* __restrict__ cp_out,
                                                         int32_t* __restrict__ corig_out, int32_t* __restrict__ vr_out,
                                                         int32_t* __restrict__ vcol_out) {
  const int64_t c0 = cp[b0], c1 = cp[b1], nc = c1 - c0, nb = b1 - b0;
  const int64_t ec0 = vr[4 * c0], ec1 = vr[4 * c1], eb0 = vr[4 * (Nc + b0)], eb1 = vr[4 * (Nc + b1)];
  const int64_t ecn = ec1 - ec0, ne = ecn + (eb1 - eb0);
  const int64_t n_cp = nb + 1, n_vr = 4 * (nc + nb) + 1;
  const int64_t total = n_cp + nc + n_vr + ne;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t k = i;
    if (k < n_cp) {
      cp_out[k] = (int32_t)(cp[b0 + k] - c0);
      continue;
    }
    k -= n_cp;
    if (k < nc) {
      corig_out[k] = corig[c0 + k];
      continue;
    }
    k -= nc;
    if (k < n_vr) {
      vr_out[k] = (int32_t)(k < 4 * nc ? vr[4 * c0 + k] - ec0 : vr[4 * (Nc + b0) + (k - 4 * nc)] - eb0 + ecn);
      continue;
    }
    k -= n_vr;
    const int64_t col = vcol[k < ecn ? ec0 + k : eb0 + (k - ecn)];
    vcol_out[k] = (int32_t)(col < Nc ? col - c0 : col - Nc - b0 + nc);
  }
}

// ---------------------------------------------------------------------------------------------- degree sort
template <int WAVES>
__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t* red) {      // result to every thread
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t t = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) t += red[w];
  return t;
}

// compare-exchange of the (key, old index) pairs at i < j: the smaller pair to i.  Positions >= n hold a virtual
// +infinity that never moves (every exchange of the network below sends the larger element to the higher index), so
// the arrays need no padding to a power of two.
__device__ __forceinline__ void pair_cmpx(int64_t* key, int32_t* idx, int i, int j, int n) {
  if (j < n) {
    const int64_t ki = key[i], kj = key[j];
    const int32_t xi = idx[i], xj = idx[j];
    if (ki > kj || (ki == kj && xi > xj)) {
      key[i] = kj;
      key[j] = ki;
      idx[i] = xj;
      idx[j] = xi;
    }
  }
}

// LARGE = false: 64 threads, neighborhoods of at most kRankRows rows, stable rank by counting.
// LARGE = true: 256 threads, the larger ones: (key, old index) pairs sorted in LDS by a bitonic network whose exchanges
// all point the same way (the index breaks ties: a strict order, so the result is the stable order); a neighborhood
// above kSortLdsRows rows keeps its keys in the workspace and is ranked by counting there.
template <int THREADS, bool LARGE>
__global__ __launch_bounds__(THREADS) void degree_rank_kernel(const int32_t* __restrict__ cp,
                                                              const int32_t* __restrict__ vr,
                                                              const int32_t* __restrict__ corig,
                                                              const int64_t* __restrict__ nkey, int64_t nkey_stride,
                                                              int64_t B, int64_t Nc, int64_t* keys_ws, int32_t* order,
                                                              int32_t* new_of_old, int32_t* __restrict__ corig_out,
                                                              int32_t* __restrict__ vr_out) {
  constexpr int WAVES = THREADS / 64;
  constexpr int CAP = LARGE ? kSortLdsRows : kRankRows;
  __shared__ int64_t skey[CAP];
  __shared__ int32_t sidx[LARGE ? kSortLdsRows : 1];
  __shared__ int64_t red[WAVES];
  __shared__ int32_t wsum[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    if (!LARGE) {
      // canonical rows keep their place and their sources: the edges before them are the same edges, permuted
      if (tid < 4) vr_out[4 * (Nc + b) + tid] = vr[4 * (Nc + b) + tid];
      if (b == B - 1 && tid == 4) vr_out[4 * (Nc + B)] = vr[4 * (Nc + B)];
    }
    const int64_t c0 = cp[b];
    const int n = (int)(cp[b + 1] - c0);
    if (n <= 0 || LARGE != (n > kRankRows)) continue;                 // the same for the whole workgroup
    int64_t t0 = 0, t1 = 0;
    for (int i = tid; i < n; i += THREADS) {
      const int32_t* v = vr + 4 * (c0 + i);
      t0 += v[1] - v[0];
      t1 += v[2] - v[1];
    }
    const int64_t tot0 = block_sum_i64<WAVES>(t0, red);
    const int64_t tot1 = block_sum_i64<WAVES>(t1, red);
    const int ps = tot1 >= tot0 ? 1 : 0;
    const int64_t sign = ((nkey ? nkey[b * nkey_stride] : b) & 1) ? 1 : -1;
    const bool in_lds = n <= CAP;
    int64_t* key = in_lds ? skey : keys_ws + c0;
    for (int i = tid; i < n; i += THREADS) {
      const int32_t* v = vr + 4 * (c0 + i);
      const int64_t dp = v[ps + 1] - v[ps], dq = v[2 - ps] - v[1 - ps];
      key[i] = sign * ((dp << 32) + dq);
      if (LARGE && in_lds) sidx[i] = i;
    }
    __syncthreads();
    if (LARGE && in_lds) {
      int P = 1;
      while (P < n) P <<= 1;
      for (int k = 2; k <= P; k <<= 1) {
        const int h = k >> 1;
        for (int t = tid; t < (P >> 1); t += THREADS) {               // first step of a merge: i <-> its mirror
          const int base = (t & ~(h - 1)) << 1, off = t & (h - 1);
          pair_cmpx(skey, sidx, base + off, base + k - 1 - off, n);
        }
        __syncthreads();
        for (int s = h >> 1; s > 0; s >>= 1) {
          for (int t = tid; t < (P >> 1); t += THREADS) {
            const int i = ((t & ~(s - 1)) << 1) | (t & (s - 1));
            pair_cmpx(skey, sidx, i, i + s, n);
          }
          __syncthreads();
        }
      }
      for (int r = tid; r < n; r += THREADS) {
        const int i = sidx[r];
        new_of_old[c0 + i] = (int32_t)(c0 + r);
        order[c0 + r] = (int32_t)(c0 + i);
        corig_out[c0 + r] = corig[c0 + i];
      }
    } else {
      // stable rank: rows with a smaller key + rows with an equal key and a smaller old index
      for (int i = tid; i < n; i += THREADS) {
        const int64_t ki = key[i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
          const int64_t kj = key[j];
          r += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
        }
        new_of_old[c0 + i] = (int32_t)(c0 + r);
        order[c0 + r] = (int32_t)(c0 + i);
        corig_out[c0 + r] = corig[c0 + i];
      }
    }
    __syncthreads();                                                  // order[] of this neighborhood is complete
    // new row pointers: exclusive scan of the permuted rows' edge totals, from the neighborhood's old first offset
    int32_t carry = vr[4 * c0];
    for (int p0 = 0; p0 < n; p0 += THREADS) {
      const int p = p0 + tid;
      int32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
      if (p < n) {
        const int32_t* v = vr + 4 * (int64_t)order[c0 + p];
        d0 = v[1] - v[0];
        d1 = v[2] - v[1];
        d2 = v[3] - v[2];
        d3 = v[4] - v[3];
      }
      const int32_t t = d0 + d1 + d2 + d3;
      int32_t inc = t;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int32_t u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
      }
      if (lane == 63) wsum[wave] = inc;
      __syncthreads();
      int32_t woff = 0, chunk = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        if (w < wave) woff += wsum[w];
        chunk += wsum[w];
      }
      if (p < n) {
        const int32_t s0 = carry + woff + inc - t;
        int32_t* o = vr_out + 4 * (c0 + p);
        o[0] = s0;
        o[1] = s0 + d0;
        o[2] = s0 + d0 + d1;
        o[3] = s0 + d0 + d1 + d2;
      }
      carry += chunk;
      __syncthreads();
    }
  }
}

// one wavefront per output row: its sources move with it (slot by slot the same lengths), renamed
__global__ __launch_bounds__(256) void degree_rename_kernel(const int32_t* __restrict__ vr,
                                                            const int32_t* __restrict__ vcol,
                                                            const int32_t* __restrict__ order,
                                                            const int32_t* __restrict__ new_of_old,
                                                            const int32_t* __restrict__ vr_out, int64_t Nc,
                                                            int64_t rows, int32_t* __restrict__ tmp) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < rows; p += waves) {
    const int64_t old = p < Nc ? (int64_t)order[p] : p;
    const int64_t a = vr[4 * old], len = vr[4 * old + 4] - a, o = vr_out[4 * p];
    for (int64_t k = lane; k < len; k += 64) {
      const int32_t c = vcol[a + k];
      tmp[o + k] = c < Nc ? new_of_old[c] : c;
    }
  }
}

// one wavefront per output row: each of its 4 slot segments sorted ascending (rank counting; equal values keep their
// order, which for equal integers is not observable)
__global__ __launch_bounds__(256) void segment_sort_kernel(const int32_t* __restrict__ vr_out,
                                                           const int32_t* __restrict__ tmp, int64_t rows,
                                                           int32_t* __restrict__ vcol_out) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < rows; p += waves) {
    for (int s = 0; s < 4; ++s) {
      const int64_t o = vr_out[4 * p + s];
      const int len = (int)(vr_out[4 * p + s + 1] - o);
      const int32_t* seg = tmp + o;
      for (int e = lane; e < len; e += 64) {
        const int32_t x = seg[e];
        int r = 0;
        for (int j = 0; j < len; ++j) {
          const int32_t y = seg[j];
          r += (y < x || (y == x && j < e)) ? 1 : 0;
        }
        vcol_out[o + r] = x;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- pool index
constexpr int kPoolTile = 16;       // rows per wave tile of the layer kernel (desco_shmp_pool_tile_rows)

__global__ __launch_bounds__(256) void pool_tiles_kernel(const int32_t* __restrict__ cp, int64_t B, int64_t nc,
                                                         int64_t tiles, int32_t* __restrict__ bits_out,
                                                         int32_t* __restrict__ nseg_out) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < tiles; t += (int64_t)gridDim.x * 256) {
    const int64_t lo = kPoolTile * t;
    const int64_t hi = lo + kPoolTile - 1 < nc - 1 ? lo + kPoolTile - 1 : nc - 1;
    // first neighborhood with a row at or after `lo`: smallest b with cp[b + 1] > lo (cp[B] = nc > lo)
    int64_t l = 0, r = B - 1;
    while (l < r) {
      const int64_t m = (l + r) >> 1;
      if (cp[m + 1] > lo) r = m; else l = m + 1;
    }
    uint32_t bits = 0;
    int32_t pop = 0;
    for (int64_t b = l; b < B; ++b) {
      const int64_t end = (int64_t)cp[b + 1] - 1;
      if (end > hi) break;
      bits |= 1u << (uint32_t)(end & (kPoolTile - 1));
      ++pop;
    }
    const int32_t runs_on = ((bits >> (uint32_t)(hi & (kPoolTile - 1))) & 1u) ? 0 : 1;
    bits_out[t] = (int32_t)bits;
    nseg_out[t] = pop + runs_on;
  }
}

// One workgroup: exclusive scan of the tiles' slot counts in place (chunks of 1024 x 8 in sequence, as
// partition_scan_kernel does), and the largest / smallest neighborhood.  totals = (num_slots, max rows, min rows, 0).
__global__ __launch_bounds__(1024) void pool_scan_kernel(const int32_t* __restrict__ cp, int64_t B, int64_t tiles,
                                                         int32_t* slot, int64_t* totals) {
  __shared__ int64_t wsum[16];
  __shared__ int32_t wmax[16], wmin[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < tiles; c0 += 8192) {
    const int64_t i0 = c0 + (int64_t)tid * 8;
    int32_t x[8];
    int64_t sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      x[k] = i0 + k < tiles ? slot[i0 + k] : 0;
      sum += x[k];
    }
    int64_t inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int64_t woff = 0, chunk = 0;
    for (int w = 0; w < 16; ++w) {
      if (w < wave) woff += wsum[w];
      chunk += wsum[w];
    }
    int64_t run = carry + woff + inc - sum;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (i0 + k < tiles) slot[i0 + k] = (int32_t)run;       // the caller refuses a total of 2^31 or more
      run += x[k];
    }
    carry += chunk;
    __syncthreads();
  }
  int32_t mx = INT32_MIN, mn = INT32_MAX;
  for (int64_t b = tid; b < B; b += 1024) {
    const int32_t d = cp[b + 1] - cp[b];
    mx = d > mx ? d : mx;
    mn = d < mn ? d : mn;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int32_t a = __shfl_xor(mx, o, 64), c = __shfl_xor(mn, o, 64);
    mx = a > mx ? a : mx;
    mn = c < mn ? c : mn;
  }
  if (lane == 0) {
    wmax[wave] = mx;
    wmin[wave] = mn;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) {
      mx = wmax[w] > mx ? wmax[w] : mx;
      mn = wmin[w] < mn ? wmin[w] : mn;
    }
    totals[0] = carry;
    totals[1] = mx;
    totals[2] = mn;
    totals[3] = 0;
  }
}

// ---------------------------------------------------------------------------------------------- neighborhood rows
__global__ __launch_bounds__(256) void neigh_rows_kernel(const int64_t* __restrict__ ni, const int64_t* __restrict__ gp,
                                                         int64_t B, int64_t G, int32_t* __restrict__ scatter,
                                                         int32_t* __restrict__ ngp) {
  const int64_t total = B + G + 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (i < B) {
      scatter[i] = (int32_t)(gp[ni[2 * i]] + ni[2 * i + 1]);
    } else {
      // neighborhoods of the graphs before g: first b whose graph id is >= g
      const int64_t g = i - B;
      int64_t l = 0, r = B;
      while (l < r) {
        const int64_t m = (l + r) >> 1;
        if (ni[2 * m] >= g) r = m; else l = m + 1;
      }
      ngp[g] = (int32_t)l;
    }
  }
}

static unsigned grid_for(int64_t items, int per_block, int64_t cap = 1 << 20) {
  int64_t g = (items + per_block - 1) / per_block;
  g = g < 1 ? 1 : g;
  return (unsigned)(g > cap ? cap : g);
}

}  // namespace desco

using namespace desco;

extern "C" int desco_partition_dev_slice(const int32_t* count_ptr, const int32_t* vrowptr, const int32_t* vcol,
                                         const int32_t* count_orig, int64_t num_neigh, int64_t num_count, int64_t b0,
                                         int64_t b1, int64_t block_count, int64_t block_edges, int32_t* count_ptr_out,
                                         int32_t* count_orig_out, int32_t* vrowptr_out, int32_t* vcol_out,
                                         desco_stream_t stream) {
  if (!count_ptr || !vrowptr || !count_ptr_out || !vrowptr_out || num_neigh < 0 || num_count < 0 || b0 < 0 ||
      b0 > b1 || b1 > num_neigh || block_count < 0 || block_count > num_count || block_edges < 0 ||
      block_edges > INT32_MAX || (block_count > 0 && (!count_orig || !count_orig_out)) ||
      (block_edges > 0 && (!vcol || !vcol_out)))
    return fail(DESCO_EINVAL, "desco_partition_dev_slice: bad argument (0 <= b0 <= b1 <= num_neigh)");
  if (b0 == b1) return 0;
  const int64_t total = (b1 - b0 + 1) + block_count + 4 * (block_count + (b1 - b0)) + 1 + block_edges;
  hipLaunchKernelGGL(part_slice_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, count_ptr,
                     vrowptr, vcol, count_orig, num_count, b0, b1, count_ptr_out, count_orig_out, vrowptr_out,
                     vcol_out);
  return launch_status("desco_partition_dev_slice");
}

extern "C" size_t desco_partition_dev_degree_sort_workspace(int64_t num_count, int64_t num_edges) {
  if (num_count < 0 || num_edges < 0) return 0;
  // keys (int64, used by neighborhoods above the LDS limit) + order + new_of_old + renamed sources
  return (size_t)(16 * num_count + 4 * num_edges);
}

extern "C" int desco_partition_dev_degree_sort(const int32_t* count_ptr, int64_t num_neigh, int64_t num_count,
                                               int64_t num_edges, const int32_t* vrowptr, const int32_t* vcol,
                                               const int32_t* count_orig, const int64_t* neigh_key,
                                               int64_t neigh_key_stride, int32_t* count_orig_out, int32_t* vrowptr_out,
                                               int32_t* vcol_out, void* workspace, int num_blocks,
                                               desco_stream_t stream) {
  if (!count_ptr || !vrowptr || !vrowptr_out || num_neigh < 0 || num_count < 0 || num_edges < 0 ||
      num_edges > INT32_MAX || 4 * (num_count + num_neigh) + 1 > INT32_MAX || num_blocks < 0 ||
      (neigh_key && neigh_key_stride < 1) || (num_count > 0 && (!count_orig || !count_orig_out || !workspace)) ||
      (num_edges > 0 && (!vcol || !vcol_out || !workspace)))
    return fail(DESCO_EINVAL, "desco_partition_dev_degree_sort: bad argument");
  if (num_neigh == 0) return 0;
  const int64_t B = num_neigh, Nc = num_count;
  int64_t* keys = (int64_t*)workspace;
  int32_t* order = (int32_t*)(keys + Nc);
  int32_t* new_of_old = order + Nc;
  int32_t* tmp = new_of_old + Nc;
  hipStream_t st = (hipStream_t)stream;
  const unsigned g1 = num_blocks > 0 ? (unsigned)num_blocks : grid_for(B, 1, 1 << 16);
  hipLaunchKernelGGL((degree_rank_kernel<64, false>), dim3(g1), dim3(64), 0, st, count_ptr, vrowptr, count_orig,
                     neigh_key, neigh_key_stride, B, Nc, keys, order, new_of_old, count_orig_out, vrowptr_out);
  hipLaunchKernelGGL((degree_rank_kernel<256, true>), dim3(g1), dim3(256), 0, st, count_ptr, vrowptr, count_orig,
                     neigh_key, neigh_key_stride, B, Nc, keys, order, new_of_old, count_orig_out, vrowptr_out);
  if (num_edges > 0) {
    const unsigned g2 = num_blocks > 0 ? (unsigned)num_blocks : grid_for(Nc + B, 4, 1 << 18);
    hipLaunchKernelGGL(degree_rename_kernel, dim3(g2), dim3(256), 0, st, vrowptr, vcol, order, new_of_old, vrowptr_out,
                       Nc, Nc + B, tmp);
    hipLaunchKernelGGL(segment_sort_kernel, dim3(g2), dim3(256), 0, st, vrowptr_out, tmp, Nc + B, vcol_out);
  }
  return launch_status("desco_partition_dev_degree_sort");
}

extern "C" int desco_pool_index_dev(const int32_t* count_ptr, int64_t num_neigh, int64_t num_count, int32_t* pool_bits,
                                    int32_t* pool_slot, int64_t* totals4, desco_stream_t stream) {
  const int64_t tiles = num_count < 0 ? 0 : (num_count + kPoolTile - 1) / kPoolTile;
  if (!count_ptr || !totals4 || num_neigh < 0 || num_count < 0 || (tiles > 0 && (!pool_bits || !pool_slot)))
    return fail(DESCO_EINVAL, "desco_pool_index_dev: bad argument");
  if (num_neigh == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (tiles > 0)
    hipLaunchKernelGGL(pool_tiles_kernel, dim3(grid_for(tiles, 256)), dim3(256), 0, st, count_ptr, num_neigh, num_count,
                       tiles, pool_bits, pool_slot);
  hipLaunchKernelGGL(pool_scan_kernel, dim3(1), dim3(1024), 0, st, count_ptr, num_neigh, tiles, pool_slot, totals4);
  return launch_status("desco_pool_index_dev");
}

extern "C" int desco_neigh_rows_dev(const int64_t* neigh_index, int64_t num_neigh, const int64_t* graph_ptr,
                                    int64_t num_graphs, int32_t* scatter_index, int32_t* neigh_graph_ptr,
                                    desco_stream_t stream) {
  if (!graph_ptr || !neigh_graph_ptr || num_neigh < 0 || num_graphs < 0 || num_neigh > INT32_MAX ||
      (num_neigh > 0 && (!neigh_index || !scatter_index)))
    return fail(DESCO_EINVAL, "desco_neigh_rows_dev: bad argument");
  if (num_neigh == 0) return 0;                     // neigh_graph_ptr is all zero: the caller's zero fill
  hipLaunchKernelGGL(neigh_rows_kernel, dim3(grid_for(num_neigh + num_graphs + 1, 256)), dim3(256), 0,
                     (hipStream_t)stream, neigh_index, graph_ptr, num_neigh, num_graphs, scatter_index,
                     neigh_graph_ptr);
  return launch_status("desco_neigh_rows_dev");
}
