// Device side of the k-core / k-truss decomposition (C ABI: desco_core_truss_dev), see include/desco_hip.h,
// "CORE / TRUSS".  Equal to the host twin (core_truss.cpp) bit for bit: both decompositions are unique, whatever the
// order in which the nodes or edges of a level leave, so the parallel peel returns the sequential peel's integers.
//
// One workgroup per graph (THREADS = 64 for the smallest workspace bucket, 256 above it); the whole graph sits in the
// workgroup's LDS workspace (core_truss.hpp: three control words, rowptr, one word per CSR entry = neighbour | edge
// row << 16, one word per edge = its two ends, and the peel's words), sized by the launch's largest graph.
//
//   load     rowptr and entries from global memory, local ids; a lower entry (v, u), u < v, writes the ends of its edge
//            row, and after a barrier EVERY entry checks that the ends of the row it names are its own two nodes: with
//            m lower entries, m upper ones and every row below m, that makes the rows a pairing of the entries.
//   core     peel[v] = remaining degree.  Level k: every live node of degree <= k gets core number k, is marked dead and
//            takes one from each neighbour (LDS atomic); repeated until a pass removes nothing; then k = the smallest
//            live degree (exact: the pass that found it removed nothing).  A decrement that lands on a dead node, or
//            between a neighbour's test and its removal, changes nothing: a node only ever leaves at the level it
//            would have left at anyway.
//   support  lane per edge: merge of the two sorted rows.
//   truss    Level k, sub-round: (collect) every live edge of support <= k - 2 becomes FRONT, gets truss number k and
//            joins the frontier list; (walk) lane per frontier edge e = (u, v): for every common neighbour w whose two
//            edges e1 = (u, w), e2 = (v, w) are not GONE -- the triangle is destroyed in THIS sub-round -- the ONE
//            DECREMENT RULE: neither e1 nor e2 FRONT: e takes one from both; exactly one of them FRONT, say e1: the
//            edge with the smaller row of e and e1 takes one from e2; both FRONT: nobody.  So an edge that stays loses
//            exactly one per destroyed triangle.  (retire) the frontier becomes GONE.  An empty frontier raises k to
//            the smallest live support + 2 (exact: nothing was walked), and no live edge ends the peel.
//
// The kernel guards itself: a graph whose workspace exceeds the launch's, whose rowptr is not monotone, which holds an
// id outside itself, a loop, an unsorted row or an edge row outside its own, or whose entries do not pair up gets
// status = -1 and no other word written.  Every LDS index is below the workspace by construction: node ids are checked
// against n, edge rows against m and entry offsets against 2 m before anything is indexed with them.  No global
// atomics: a graph has one owner.
#include "common_device.hpp"
#include "core_truss.hpp"

namespace desco {

struct CoreTrussArgs {
  const int64_t* graph_ptr;   // [num_graphs + 1]
  const int64_t* rowptr;      // [num_nodes + 1]
  const int32_t* col;         // global ids
  const int32_t* entry_row;   // [E] edge row of every CSR entry
  const int64_t* graph_ids;   // [num_ids] the graphs of this launch, or null: all of them
  int64_t num_graphs, num_edges;
  int64_t ws_words;           // LDS words of the launch
  int32_t* core;              // [N] or null
  int32_t* truss;             // [M] or null
  int32_t* support;           // [M] or null
  int32_t* status;            // [num_graphs]
};

constexpr int kDead = -(1 << 30);                      // a removed node's degree: stays negative under any decrements
constexpr uint32_t kLive = 0u, kFront = 1u, kGone = 2u;

template <int THREADS>
__global__ __launch_bounds__(THREADS) void core_truss_kernel(CoreTrussArgs p) {
  extern __shared__ uint32_t ct_lds[];
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
  const int64_t m = (e1 - e0) >> 1, r0 = e0 >> 1;
  if (e1 < e0 || ((e1 - e0) & 1) || (e0 & 1) || n > 65535 || m > 65535 || r0 + m > p.num_edges ||
      core_truss::workspace_words(n, m) > p.ws_words) {
    if (tid == 0) *status = -1;                                  // (uniform) not this launch's: no LDS is touched
    return;
  }
  const int nn = (int)n, mm = (int)m;
  int& sh_flag = reinterpret_cast<int*>(ct_lds)[0];              // the workgroup's three control words
  int& sh_min = reinterpret_cast<int*>(ct_lds)[1];
  int& sh_count = reinterpret_cast<int*>(ct_lds)[2];
  uint32_t* rp = ct_lds + 3;                                     // [nn + 1]
  uint32_t* entry = rp + nn + 1;                                 // [2 mm]
  uint32_t* ends = entry + 2 * mm;                               // [mm]
  uint32_t* peel = ends + mm;                                    // [max(3 mm, nn)]
  int* deg = reinterpret_cast<int*>(peel);
  uint32_t* sup = peel;
  uint32_t* state = peel + mm;
  uint32_t* front = peel + 2 * mm;

  // ---- load and check ----------------------------------------------------------------------------------------------
  if (tid == 0) sh_flag = 0, sh_count = 0;
  int bad = 0;
  for (int v = tid; v <= nn; v += THREADS) {
    const int64_t o = p.rowptr[n0 + v] - e0;
    bad |= o < 0 || o > 2 * m || (v < nn && p.rowptr[n0 + v + 1] - e0 < o);
    rp[v] = (uint32_t)(o < 0 ? 0 : o > 2 * m ? 2 * m : o);
  }
  __syncthreads();
  int lower = 0;
  for (int v = tid; v < nn; v += THREADS) {
    int prev = -1;
    for (uint32_t q = rp[v]; q < rp[v + 1]; ++q) {               // (monotone offsets within [0, 2 m], or bad is set and
      const int64_t u = (int64_t)p.col[e0 + q] - n0;             //  the clamped offsets still are)
      const int64_t r = (int64_t)p.entry_row[e0 + q] - r0;
      const bool ok = u >= 0 && u < n && u != v && u > prev && r >= 0 && r < m;
      bad |= !ok;
      entry[q] = ok ? (uint32_t)u | ((uint32_t)r << 16) : 0xffffffffu;
      if (ok) {
        prev = (int)u;
        if (u < v) ends[r] = (uint32_t)u | ((uint32_t)v << 16), ++lower;
      }
    }
  }
  if (lower) atomicAdd(&sh_count, lower);
  __syncthreads();
  for (int v = tid; v < nn; v += THREADS)
    for (uint32_t q = rp[v]; q < rp[v + 1]; ++q) {
      const uint32_t w = entry[q];
      if (w == 0xffffffffu) continue;
      const uint32_t u = w & 0xffffu, r = w >> 16;
      bad |= ends[r] != ((uint32_t)v < u ? (uint32_t)v | (u << 16) : u | ((uint32_t)v << 16));
    }
  if (bad) sh_flag = 1;
  __syncthreads();
  if (sh_flag || sh_count != mm) {                               // (uniform: LDS words read behind a barrier)
    if (tid == 0) *status = -1;
    return;
  }

  // ---- core peel ---------------------------------------------------------------------------------------------------
  if (p.core) {
    int32_t* __restrict__ core = p.core + n0;
    for (int v = tid; v < nn; v += THREADS) deg[v] = (int)(rp[v + 1] - rp[v]);
    int k = 0;
    for (;;) {
      __syncthreads();
      if (tid == 0) sh_flag = 0, sh_min = INT_MAX;
      __syncthreads();
      for (int v = tid; v < nn; v += THREADS) {
        const int d = deg[v];
        if (d < 0) continue;
        if (d <= k) {
          core[v] = k;
          deg[v] = kDead;
          for (uint32_t q = rp[v]; q < rp[v + 1]; ++q) atomicSub(&deg[entry[q] & 0xffffu], 1);
          sh_flag = 1;
        } else {
          atomicMin(&sh_min, d);
        }
      }
      __syncthreads();
      if (sh_flag) continue;
      if (sh_min == INT_MAX) break;
      k = sh_min;
    }
    __syncthreads();                                             // the peel's words change hands
  }

  // ---- support -----------------------------------------------------------------------------------------------------
  if ((p.truss || p.support) && mm > 0) {
    for (int e = tid; e < mm; e += THREADS) {
      const uint32_t u = ends[e] & 0xffffu, v = ends[e] >> 16;
      uint32_t i = rp[u], i1 = rp[u + 1], j = rp[v], j1 = rp[v + 1];
      uint32_t s = 0;
      while (i < i1 && j < j1) {
        const uint32_t x = entry[i] & 0xffffu, y = entry[j] & 0xffffu;
        s += x == y;
        i += x <= y;
        j += y <= x;
      }
      sup[e] = s;
      state[e] = kLive;
      if (p.support) p.support[r0 + e] = (int32_t)s;
    }
  }

  // ---- truss peel --------------------------------------------------------------------------------------------------
  if (p.truss && mm > 0) {
    int32_t* __restrict__ truss = p.truss + r0;
    int k = 2;
    for (;;) {
      __syncthreads();
      if (tid == 0) sh_count = 0, sh_min = INT_MAX;
      __syncthreads();
      for (int e = tid; e < mm; e += THREADS) {                  // collect
        if (state[e] != kLive) continue;
        const int s = (int)sup[e];
        if (s <= k - 2) {
          state[e] = kFront;
          truss[e] = k;
          front[atomicAdd(&sh_count, 1)] = (uint32_t)e;          // (at most one slot per edge: below mm)
        } else {
          atomicMin(&sh_min, s);
        }
      }
      __syncthreads();
      const int count = sh_count;
      if (count == 0) {
        if (sh_min == INT_MAX) break;
        k = sh_min + 2;
        continue;
      }
      for (int f = tid; f < count; f += THREADS) {               // walk
        const uint32_t e = front[f];
        const uint32_t u = ends[e] & 0xffffu, v = ends[e] >> 16;
        uint32_t i = rp[u], i1 = rp[u + 1], j = rp[v], j1 = rp[v + 1];
        while (i < i1 && j < j1) {
          const uint32_t a = entry[i], b = entry[j];
          const uint32_t x = a & 0xffffu, y = b & 0xffffu;
          if (x == y) {
            const uint32_t ea = a >> 16, eb = b >> 16;
            const uint32_t sa = state[ea], sb = state[eb];
            if (sa != kGone && sb != kGone) {
              if (sa == kLive && sb == kLive) {
                atomicSub(&sup[ea], 1u);
                atomicSub(&sup[eb], 1u);
              } else if (sa == kFront && sb == kLive) {
                if (e < ea) atomicSub(&sup[eb], 1u);
              } else if (sa == kLive && sb == kFront) {
                if (e < eb) atomicSub(&sup[ea], 1u);
              }
            }
          }
          i += x <= y;
          j += y <= x;
        }
      }
      __syncthreads();
      for (int f = tid; f < count; f += THREADS) state[front[f]] = kGone;        // retire
    }
  }
  if (tid == 0) *status = 0;
}

template <int THREADS>
int launch(const CoreTrussArgs& a, int64_t num_ids, hipStream_t stream) {
  const hipError_t e = size_dynamic_lds<core_truss_kernel<THREADS>>(4 * DESCO_CORE_TRUSS_DEV_MAX_WORDS);
  if (e != hipSuccess) return fail((int)e, "desco_core_truss_dev: cannot size LDS");
  hipLaunchKernelGGL(core_truss_kernel<THREADS>, dim3((unsigned)num_ids), dim3(THREADS), (size_t)(4 * a.ws_words),
                     stream, a);
  return launch_status("desco_core_truss_dev");
}

}  // namespace desco

using namespace desco;

extern "C" int desco_core_truss_dev(const int64_t* graph_ptr, const int64_t* rowptr, const int32_t* col,
                                    int64_t num_graphs, int64_t num_edges, const int32_t* entry_row,
                                    const int64_t* graph_ids, int64_t num_ids, int64_t max_words, int32_t* core_out,
                                    int32_t* truss_out, int32_t* support_out, int32_t* status, desco_stream_t stream) {
  if (num_graphs < 0 || num_ids < 0 || num_edges < 0)
    return fail(DESCO_EINVAL, "desco_core_truss_dev: negative num_graphs, num_ids or num_edges");
  if (max_words < 0) return fail(DESCO_EINVAL, "desco_core_truss_dev: negative max_words");
  if (!graph_ids) num_ids = num_graphs;
  if (num_ids == 0) return 0;
  if (max_words > DESCO_CORE_TRUSS_DEV_MAX_WORDS)
    return fail(DESCO_EINVAL,
                "desco_core_truss_dev: a graph's workspace, n + 4 + 3 m + max(3 m, n) words, exceeds "
                "DESCO_CORE_TRUSS_DEV_MAX_WORDS (40960); use desco_core_truss for it");
  if (num_ids > INT32_MAX) return fail(DESCO_EINVAL, "desco_core_truss_dev: num_ids is above 2^31 - 1");
  if (!graph_ptr) return fail(DESCO_EINVAL, "desco_core_truss_dev: graph_ptr is null");
  if (!rowptr) return fail(DESCO_EINVAL, "desco_core_truss_dev: rowptr is null");
  if (!status) return fail(DESCO_EINVAL, "desco_core_truss_dev: status is null");
  if (num_edges > 0 && !col) return fail(DESCO_EINVAL, "desco_core_truss_dev: col is null");
  if (num_edges > 0 && !entry_row) return fail(DESCO_EINVAL, "desco_core_truss_dev: entry_row is null");
  if (mis8(graph_ptr) || mis8(rowptr) || mis8(graph_ids))
    return fail(DESCO_EINVAL, "desco_core_truss_dev: a 64-bit array is not 8-byte aligned");
  CoreTrussArgs a;
  a.graph_ptr = graph_ptr, a.rowptr = rowptr, a.col = col, a.entry_row = entry_row, a.graph_ids = graph_ids;
  a.num_graphs = num_graphs, a.num_edges = num_edges;
  a.ws_words = (max_words + 3) & ~(int64_t)3;
  a.core = core_out, a.truss = truss_out, a.support = support_out, a.status = status;
  // one wave per graph where the launch's graphs are small (DESCO_CORE_TRUSS_WAVE_WORDS), four above
  return a.ws_words <= DESCO_CORE_TRUSS_WAVE_WORDS ? launch<64>(a, num_ids, (hipStream_t)stream)
                                                   : launch<256>(a, num_ids, (hipStream_t)stream);
}
