// Device side of the clique census (C ABI: desco_peel_order_dev, desco_clique_census_dev), see include/desco_hip.h,
// "CLIQUE CENSUS".  Equal to the host twins (clique_census.cpp) bit for bit: the peel key is unique, and the counts are
// sums of integers modulo 2^64 that depend neither on the key, nor on the pivots, nor on the order of the atomics.
//
// peel_order_kernel   one workgroup per graph (64 threads up to DESCO_PEEL_WAVE_WORDS, 256 above), the graph's CSR and
//   the remaining degrees in LDS (clique_census.hpp).  A pass has two halves with a barrier between them: (mark) every
//   live node of degree <= k -- on the degrees of the START of the pass -- gets key = pass and core = k and its degree
//   word becomes -1 - pass; (take) every node marked in this pass takes one from each LIVE neighbour (LDS atomic; a live
//   degree counts the live neighbours, so it stays >= 0 and the sign test cannot race).  A pass that marks nobody raises k
//   to the smallest live degree, or ends the peel; it is not numbered.
// census_check_kernel one workgroup per graph: every entry's id inside the graph, no loop, rows ascending, every
//   out-degree <= max_out.  A graph that fails gets status -1 and nothing else; one that passes gets status 0 and its
//   rows of the outputs zeroed.
// census_kernel       kSlices workgroups per graph; their waves share the roots of the graph, one wave per root at a time.
//   (gather) the out-neighbours of the root, ascending, by ballot; (rows) lane i merges the sorted CSR row of
//   out-neighbour i with the sorted out-neighbour list into the 64-bit row i; (split) the first-level branches -- the
//   pivot's and one per non-neighbour of the pivot -- go to one lane each; (walk) every lane walks its branch with a
//   stack of (candidate set, set still to branch on) in LDS, the held and pivot sets in two registers; a leaf adds its
//   binomials to the wave's tallies in LDS (64-bit LDS atomics); (flush) the tallies go to the outputs with one global
//   atomic per non-zero word, and omega with one atomicMax per root.
//   Every index is below its array by construction: ids are checked by census_check_kernel before this kernel reads
//   key[] with them, d <= max_out is checked there too, and a stack is never deeper than the lane's start set has
//   members (each push removes at least the pivot from the set it pushes), which is below d.
#include "common_device.hpp"

#include "clique_census.hpp"

namespace desco {

using u64 = unsigned long long;

struct BinomTable {
  uint64_t c[65][65];
  constexpr BinomTable() : c{} {
    for (int n = 0; n <= 64; ++n) {
      c[n][0] = 1;
      for (int j = 1; j <= 64; ++j) c[n][j] = n == 0 ? 0 : c[n - 1][j] + c[n - 1][j - 1];
    }
  }
};
__device__ const BinomTable kBinom{};

struct PeelArgs {
  const int64_t* graph_ptr;
  const int64_t* rowptr;
  const int32_t* col;
  const int64_t* graph_ids;
  int64_t num_graphs, ws_words;
  int32_t* key;
  int32_t* core;
  int32_t* status;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void peel_order_kernel(PeelArgs p) {
  extern __shared__ uint32_t pk_lds[];
  const int tid = threadIdx.x;
  const int64_t g = p.graph_ids ? p.graph_ids[blockIdx.x] : (int64_t)blockIdx.x;
  if (g < 0 || g >= p.num_graphs) return;                        // (uniform) a bad id: nothing to write to
  const int64_t n0 = p.graph_ptr[g], n = p.graph_ptr[g + 1] - n0;
  int32_t* __restrict__ status = p.status + g;
  if (n <= 0) {
    if (tid == 0) *status = n == 0 ? 0 : -1;
    return;
  }
  const int64_t e0 = p.rowptr[n0], e1 = p.rowptr[n0 + n];
  const int64_t m2 = e1 - e0;
  if (m2 < 0 || (m2 & 1) || n > INT32_MAX / 4 || m2 > INT32_MAX / 4 || clique_census::peel_words(n, m2 >> 1) > p.ws_words) {
    if (tid == 0) *status = -1;                                  // (uniform) not this launch's: no LDS is touched
    return;
  }
  const int nn = (int)n, ee = (int)m2;
  int& sh_flag = reinterpret_cast<int*>(pk_lds)[0];
  int& sh_min = reinterpret_cast<int*>(pk_lds)[1];
  uint32_t* rp = pk_lds + 3;                                     // [nn + 1]
  uint32_t* entry = rp + nn + 1;                                 // [ee]
  int* deg = reinterpret_cast<int*>(entry + ee);                 // [nn]

  // ---- load and check ----------------------------------------------------------------------------------------------
  if (tid == 0) sh_flag = 0;
  int bad = 0;
  for (int v = tid; v <= nn; v += THREADS) {
    const int64_t o = p.rowptr[n0 + v] - e0;
    bad |= o < 0 || o > m2 || (v < nn && p.rowptr[n0 + v + 1] - e0 < o);
    rp[v] = (uint32_t)(o < 0 ? 0 : o > m2 ? m2 : o);
  }
  __syncthreads();
  for (int v = tid; v < nn; v += THREADS) {
    int64_t prev = -1;
    const uint32_t q0 = rp[v], q1 = rp[v + 1];
    for (uint32_t q = q0; q < q1; ++q) {                         // (offsets clamped to [0, ee]; q1 < q0 runs nothing)
      const int64_t u = (int64_t)p.col[e0 + q] - n0;
      const bool ok = u >= 0 && u < n && u != v && u > prev;
      bad |= !ok;
      entry[q] = ok ? (uint32_t)u : (uint32_t)v;                 // (a word that is always a valid index)
      prev = ok ? u : prev;
    }
    deg[v] = q1 >= q0 ? (int)(q1 - q0) : 0;
  }
  if (bad) sh_flag = 1;
  __syncthreads();
  if (sh_flag) {                                                 // (uniform: an LDS word read behind a barrier)
    if (tid == 0) *status = -1;
    return;
  }

  // ---- peel --------------------------------------------------------------------------------------------------------
  int32_t* __restrict__ key = p.key + n0;
  int32_t* __restrict__ core = p.core ? p.core + n0 : nullptr;
  int k = 0, pass = 0;
  for (;;) {
    __syncthreads();
    if (tid == 0) sh_flag = 0, sh_min = INT_MAX;
    __syncthreads();
    for (int v = tid; v < nn; v += THREADS) {                    // mark
      const int d = deg[v];
      if (d < 0) continue;
      if (d <= k) {
        key[v] = pass;
        if (core) core[v] = k;
        deg[v] = -1 - pass;
        sh_flag = 1;
      } else {
        atomicMin(&sh_min, d);
      }
    }
    __syncthreads();
    if (!sh_flag) {
      if (sh_min == INT_MAX) break;
      k = sh_min;
      continue;
    }
    for (int v = tid; v < nn; v += THREADS) {                    // take
      if (deg[v] != -1 - pass) continue;
      for (uint32_t q = rp[v]; q < rp[v + 1]; ++q) {
        const uint32_t u = entry[q];
        if (deg[u] >= 0) atomicSub(&deg[u], 1);
      }
    }
    ++pass;
  }
  if (tid == 0) *status = 0;
}

template <int THREADS>
int launch_peel(const PeelArgs& a, int64_t num_ids, hipStream_t stream) {
  const hipError_t e = size_dynamic_lds<peel_order_kernel<THREADS>>(4 * DESCO_PEEL_DEV_MAX_WORDS);
  if (e != hipSuccess) return fail((int)e, "desco_peel_order_dev: cannot size LDS");
  hipLaunchKernelGGL(peel_order_kernel<THREADS>, dim3((unsigned)num_ids), dim3(THREADS), (size_t)(4 * a.ws_words), stream,
                     a);
  return launch_status("desco_peel_order_dev");
}

// ---- census ------------------------------------------------------------------------------------------------------------
struct CensusArgs {
  const int64_t* graph_ptr;
  const int64_t* rowptr;
  const int32_t* col;
  const int32_t* key;
  const int64_t* graph_ids;
  int64_t num_graphs;
  int kmax, max_out;
  u64* graph_cliques;   // [G, kmax] or null
  u64* node_cliques;    // [N, kmax] or null
  int32_t* omega;       // [G] or null
  int32_t* status;      // [G]
};

__device__ __forceinline__ bool comes_after(int ku, int64_t u, int kv, int64_t v) { return ku > kv || (ku == kv && u > v); }

__global__ __launch_bounds__(256) void census_check_kernel(CensusArgs p) {
  __shared__ int sh_bad;
  const int tid = threadIdx.x;
  const int64_t g = p.graph_ids ? p.graph_ids[blockIdx.x] : (int64_t)blockIdx.x;
  if (g < 0 || g >= p.num_graphs) return;                        // (uniform) a bad id: nothing to write to
  const int64_t n0 = p.graph_ptr[g], n1 = p.graph_ptr[g + 1];
  if (n1 < n0 || n1 - n0 > INT32_MAX) {
    if (tid == 0) p.status[g] = -1;
    return;
  }
  if (tid == 0) sh_bad = 0;
  __syncthreads();
  const int64_t e0 = p.rowptr[n0], e1 = p.rowptr[n1];
  int bad = 0;
  for (int64_t v = n0 + tid; v < n1; v += 256) {
    const int64_t q0 = p.rowptr[v], q1 = p.rowptr[v + 1];
    bad |= q1 < q0 || q0 < e0 || q1 > e1;
    for (int64_t q = q0; q < q1 && !bad; ++q) {                  // first every id of the row, then key[] with them
      const int64_t u = p.col[q];
      bad |= u < n0 || u >= n1 || u == v || (q > q0 && p.col[q - 1] >= u);
    }
    if (bad) break;
    const int kv = p.key[v];
    int out = 0;
    for (int64_t q = q0; q < q1; ++q) out += comes_after(p.key[p.col[q]], p.col[q], kv, v);
    bad |= out > p.max_out;
  }
  if (bad) sh_bad = 1;
  __syncthreads();
  if (sh_bad) {                                                  // (uniform)
    if (tid == 0) p.status[g] = -1;
    return;
  }
  if (p.graph_cliques)
    for (int k = tid; k < p.kmax; k += 256) p.graph_cliques[g * p.kmax + k] = 0;
  if (p.node_cliques)
    for (int64_t i = n0 * p.kmax + tid; i < n1 * p.kmax; i += 256) p.node_cliques[i] = 0;
  if (tid == 0) {
    if (p.omega) p.omega[g] = 0;
    p.status[g] = 0;
  }
}

// the member of P with most neighbours in P, the first of those (P != 0)
__device__ __forceinline__ int pick_pivot(const u64* __restrict__ rows, u64 P) {
  int u = 0, best = -1;
  for (u64 bits = P; bits; bits &= bits - 1) {
    const int i = __builtin_ctzll(bits);
    const int c = __popcll(rows[i] & P);
    if (c > best) best = c, u = i;
  }
  return u;
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void census_kernel(CensusArgs p) {
  extern __shared__ u64 cc_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = p.graph_ids ? p.graph_ids[blockIdx.x] : (int64_t)blockIdx.x;
  if (g < 0 || g >= p.num_graphs) return;                        // (uniform)
  if (p.status[g] != 0) return;                                  // (uniform) refused by census_check_kernel
  const int64_t n0 = p.graph_ptr[g], n = p.graph_ptr[g + 1] - n0;
  const int mo = p.max_out > 0 ? p.max_out : 1, kmax = p.kmax;    // (the entry point sizes the LDS the same way)
  // the wave's words (clique_census.hpp, wave_bytes)
  u64* base = cc_lds + (size_t)wave * (clique_census::wave_bytes(mo, kmax) / 8);
  u64* rows = base;                                              // [mo]
  int32_t* nodes = reinterpret_cast<int32_t*>(rows + mo);        // [mo], global ids
  u64* stackP = rows + mo + (mo + 1) / 2;                        // [mo][64]
  u64* stackT = stackP + (size_t)mo * 64;                        // [mo][64]
  u64* tally = stackT + (size_t)mo * 64;                         // [mo + 1][kmax]: row 0 the root, row 1 + i out-neighbour i
  const int tally_words = (mo + 1) * kmax;
  for (int i = lane; i < tally_words; i += 64) tally[i] = 0;

  const int64_t stride = (int64_t)WAVES * gridDim.y;
  const int64_t first = (int64_t)blockIdx.y * WAVES + wave;
  const int64_t rounds = (n + stride - 1) / stride;              // the same for every wave of the grid row: the barriers
  int best = 0;                                                  //  below are reached by all of the workgroup
  for (int64_t round = 0; round < rounds; ++round) {
    const int64_t vl = first + round * stride;
    const bool active = vl < n;
    const int64_t v = n0 + (active ? vl : 0);
    int d = 0;
    if (active) {                                                // ---- gather (wave uniform)
      const int kv = p.key[v];
      const int64_t q0 = p.rowptr[v], q1 = p.rowptr[v + 1];
      for (int64_t q = q0; q < q1; q += 64) {
        const bool in = q + lane < q1;
        const int32_t u = in ? p.col[q + lane] : 0;
        const bool take = in && comes_after(p.key[u], u, kv, v);
        const u64 mask = __ballot(take);
        const int at = d + __popcll(mask & ((u64(1) << lane) - 1));
        if (take && at < mo) nodes[at] = u;                      // (d <= mo was checked; the test keeps the index honest)
        d += __popcll(mask);
      }
      d = d < mo ? d : mo;
    }
    __syncthreads();
    if (active && lane < d) {                                    // ---- rows: merge two ascending lists
      const int32_t w = nodes[lane];
      int64_t q = p.rowptr[w];
      const int64_t q1 = p.rowptr[w + 1];
      int j = 0;
      u64 row = 0;
      while (q < q1 && j < d) {
        const int32_t x = p.col[q], y = nodes[j];
        if (x == y) row |= u64(1) << j;
        q += x <= y;
        j += y <= x;
      }
      rows[lane] = row & ~(u64(1) << lane);
    }
    __syncthreads();
    if (active) {                                                // ---- split and walk
      const u64 all = d == 64 ? ~u64(0) : (u64(1) << d) - 1;
      u64 H = 0, V = 0, cur = 0;
      bool walking = false;
      if (d == 0) {
        walking = lane == 0;                                     // the root alone: one leaf
      } else {
        const int u0 = pick_pivot(rows, all);
        const u64 T0 = all & ~rows[u0];                          // the pivot and its non-neighbours: one branch each
        if (lane < __popcll(T0)) {
          u64 t = T0;
          for (int i = 0; i < lane; ++i) t &= t - 1;
          const int x = __builtin_ctzll(t);
          const u64 earlier = T0 & ((u64(1) << x) - 1);
          walking = true;
          if (x == u0) V = u64(1) << x, cur = all & rows[x];
          else H = u64(1) << x, cur = all & ~earlier & rows[x];
        }
      }
      int depth = 0;
      while (walking) {
        while (cur) {                                            // descend along the pivots
          const int u = pick_pivot(rows, cur);
          const u64 bit = u64(1) << u;
          stackP[depth * 64 + lane] = cur;
          stackT[depth * 64 + lane] = cur & ~rows[u] & ~bit;
          ++depth;
          V |= bit;
          cur &= rows[u];
        }
        {                                                        // a leaf
          const int r = 1 + __popcll(H), q = __popcll(V);
          best = r + q > best ? r + q : best;
          const int top = r + q < kmax ? r + q : kmax;
          for (int k = r; k <= top; ++k) {
            const u64 c = kBinom.c[q][k - r];
            atomicAdd(&tally[k - 1], c);
            if (p.node_cliques) {
              for (u64 bits = H; bits; bits &= bits - 1) atomicAdd(&tally[(1 + __builtin_ctzll(bits)) * kmax + k - 1], c);
              if (k > r) {
                const u64 c2 = kBinom.c[q - 1][k - r - 1];
                for (u64 bits = V; bits; bits &= bits - 1)
                  atomicAdd(&tally[(1 + __builtin_ctzll(bits)) * kmax + k - 1], c2);
              }
            }
          }
        }
        for (;;) {                                               // back up to the next branch
          if (depth == 0) {
            walking = false;
            break;
          }
          u64 P = stackP[(depth - 1) * 64 + lane], T = stackT[(depth - 1) * 64 + lane];
          const u64 done = P & (H | V);                          // the one member of P on the path: the child just left
          H &= ~done, V &= ~done, P &= ~done;
          if (T == 0) {
            --depth;
            continue;
          }
          const u64 w = T & (~T + 1);
          stackP[(depth - 1) * 64 + lane] = P;
          stackT[(depth - 1) * 64 + lane] = T & ~w;
          H |= w;
          cur = P & rows[__builtin_ctzll(w)];                    // (empty: a leaf at once)
          break;
        }
      }
    }
    __syncthreads();
    if (active) {                                                // ---- flush
      for (int i = lane; i < tally_words; i += 64) {
        const u64 c = tally[i];
        if (c == 0) continue;
        tally[i] = 0;
        const int row = i / kmax, k = i - row * kmax;
        if (row == 0 && p.graph_cliques) atomicAdd(&p.graph_cliques[g * kmax + k], c);
        if (p.node_cliques) atomicAdd(&p.node_cliques[(row == 0 ? v : (int64_t)nodes[row - 1]) * kmax + k], c);
      }
    }
    __syncthreads();
  }
  if (p.omega) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int other = __shfl_xor(best, o, 64);
      best = other > best ? other : best;
    }
    if (lane == 0 && best > 0) atomicMax(&p.omega[g], best);
  }
}

template <int WAVES>
int launch_census(const CensusArgs& a, int64_t num_ids, hipStream_t stream) {
  const hipError_t e = size_dynamic_lds<census_kernel<WAVES>>(clique_census::kLdsBytes);
  if (e != hipSuccess) return fail((int)e, "desco_clique_census_dev: cannot size LDS");
  const size_t lds = (size_t)WAVES * (size_t)clique_census::wave_bytes(a.max_out > 0 ? a.max_out : 1, a.kmax);
  hipLaunchKernelGGL(census_kernel<WAVES>, dim3((unsigned)num_ids, clique_census::kSlices), dim3(WAVES * 64), lds, stream,
                     a);
  return launch_status("desco_clique_census_dev");
}

}  // namespace desco

using namespace desco;

extern "C" int desco_peel_order_dev(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col,
                                    int64_t num_graphs, const int64_t* graph_ids, int64_t num_ids, int64_t max_words,
                                    int32_t* key_out, int32_t* core_out, int32_t* status, desco_stream_t stream) {
  if (num_graphs < 0 || num_ids < 0) return fail(DESCO_EINVAL, "desco_peel_order_dev: negative num_graphs or num_ids");
  if (max_words < 0) return fail(DESCO_EINVAL, "desco_peel_order_dev: negative max_words");
  if (!graph_ids) num_ids = num_graphs;
  if (num_ids == 0) return 0;
  if (max_words > DESCO_PEEL_DEV_MAX_WORDS)
    return fail(DESCO_EINVAL,
                "desco_peel_order_dev: a graph's workspace, 2 n + 2 m + 8 words, exceeds DESCO_PEEL_DEV_MAX_WORDS "
                "(40960); use desco_peel_order for it");
  if (num_ids > INT32_MAX) return fail(DESCO_EINVAL, "desco_peel_order_dev: num_ids is above 2^31 - 1");
  if (!graph_ptr) return fail(DESCO_EINVAL, "desco_peel_order_dev: graph_ptr is null");
  if (!rowptr) return fail(DESCO_EINVAL, "desco_peel_order_dev: rowptr is null");
  if (!col) return fail(DESCO_EINVAL, "desco_peel_order_dev: col is null");
  if (!key_out) return fail(DESCO_EINVAL, "desco_peel_order_dev: key_out is null");
  if (!status) return fail(DESCO_EINVAL, "desco_peel_order_dev: status is null");
  if (mis8(graph_ptr) || mis8(rowptr) || mis8(graph_ids))
    return fail(DESCO_EINVAL, "desco_peel_order_dev: a 64-bit array is not 8-byte aligned");
  PeelArgs a;
  a.graph_ptr = graph_ptr, a.rowptr = rowptr, a.col = col, a.graph_ids = graph_ids;
  a.num_graphs = num_graphs, a.ws_words = (max_words + 3) & ~(int64_t)3;
  a.key = key_out, a.core = core_out, a.status = status;
  return a.ws_words <= DESCO_PEEL_WAVE_WORDS ? launch_peel<64>(a, num_ids, (hipStream_t)stream)
                                             : launch_peel<256>(a, num_ids, (hipStream_t)stream);
}

extern "C" int desco_clique_census_dev(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col,
                                       int64_t num_graphs, const int32_t* key, int kmax, const int64_t* graph_ids,
                                       int64_t num_ids, int max_out, int64_t* graph_cliques, int64_t* node_cliques,
                                       int32_t* omega, int32_t* status, desco_stream_t stream) {
  if (num_graphs < 0 || num_ids < 0) return fail(DESCO_EINVAL, "desco_clique_census_dev: negative num_graphs or num_ids");
  if (max_out < 0) return fail(DESCO_EINVAL, "desco_clique_census_dev: negative max_out");
  if (kmax < 1 || kmax > DESCO_CLIQUE_MAX_K)
    return fail(DESCO_EINVAL, "desco_clique_census_dev: kmax is outside 1..DESCO_CLIQUE_MAX_K (64)");
  if (!graph_ids) num_ids = num_graphs;
  if (num_ids == 0) return 0;
  if (max_out > DESCO_CLIQUE_DEV_MAX_OUT)
    return fail(DESCO_EINVAL,
                "desco_clique_census_dev: an out-degree exceeds DESCO_CLIQUE_DEV_MAX_OUT (64); use desco_clique_census "
                "for that graph");
  if (num_ids > INT32_MAX) return fail(DESCO_EINVAL, "desco_clique_census_dev: num_ids is above 2^31 - 1");
  if (!graph_ptr) return fail(DESCO_EINVAL, "desco_clique_census_dev: graph_ptr is null");
  if (!rowptr) return fail(DESCO_EINVAL, "desco_clique_census_dev: rowptr is null");
  if (!col) return fail(DESCO_EINVAL, "desco_clique_census_dev: col is null");
  if (!key) return fail(DESCO_EINVAL, "desco_clique_census_dev: key is null");
  if (!status) return fail(DESCO_EINVAL, "desco_clique_census_dev: status is null");
  if (mis8(graph_ptr) || mis8(rowptr) || mis8(graph_ids) || mis8(graph_cliques) || mis8(node_cliques))
    return fail(DESCO_EINVAL, "desco_clique_census_dev: a 64-bit array is not 8-byte aligned");
  CensusArgs a;
  a.graph_ptr = graph_ptr, a.rowptr = rowptr, a.col = col, a.key = key, a.graph_ids = graph_ids;
  a.num_graphs = num_graphs, a.kmax = kmax, a.max_out = max_out;
  a.graph_cliques = reinterpret_cast<u64*>(graph_cliques), a.node_cliques = reinterpret_cast<u64*>(node_cliques);
  a.omega = omega, a.status = status;
  hipLaunchKernelGGL(census_check_kernel, dim3((unsigned)num_ids), dim3(256), 0, (hipStream_t)stream, a);
  if (const int rc = launch_status("desco_clique_census_dev")) return rc;
  if (!graph_cliques && !node_cliques && !omega) return 0;
  switch (clique_census::waves_per_group(max_out > 0 ? max_out : 1, kmax)) {
    case 4: return launch_census<4>(a, num_ids, (hipStream_t)stream);
    case 2: return launch_census<2>(a, num_ids, (hipStream_t)stream);
    default: return launch_census<1>(a, num_ids, (hipStream_t)stream);
  }
}
