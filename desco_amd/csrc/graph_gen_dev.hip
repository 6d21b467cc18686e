// Device side of the synthetic graph generators (C ABI: desco_graph_gen_dev, desco_graph_gen_expand_dev), see
// include/desco_hip.h, "GRAPH GENERATORS".  Equal to the host twin (graph_gen.cpp) bit for bit: the sequential parts of
// the definition are the very functions of graph_gen.hpp the twin runs, and the parallel parts compute order-free
// results (a bit per pair, the smallest member of a component, a rank, a gather).
//
// One workgroup per graph (THREADS = 64 or 256); the graph's whole state sits in the workgroup's LDS workspace
// (graph_gen.hpp: adjacency bitset, the arrays A B C D, four control words), sized by the launch's largest graph.
//
//   clear        all lanes.
//   ER           a lane per Philox call: four pairs per call, a pair's bit set in both rows by an LDS atomic; the
//                degrees are the rows' popcounts.
//   WS, Random, BA, EBA, Power
//                the growth and rewiring bodies are chains in which every draw depends on the graph so far.  Wave 0 runs
//                the shared definition with all 64 lanes in step (graph_gen.hpp, "THE WAVE FORMS"): the chain itself is
//                executed by every lane alike, and its searches over the nodes -- the preferential choice as a wave
//                prefix sum over the weights and a ballot, the sum of the weights, the k-th flagged node -- are split
//                over the lanes.  WS's connectivity test between tries is the parallel one below.
//   components   label propagation on the bitset rows, all lanes: B[v] = min over v's row of B, with pointer jumping,
//                until a sweep changes nothing -- the fixed point is the smallest member, which the twin's walk gives.
//   connection   wave 0, the shared definition (a chain of draws over c components; member counts and the k-th member by
//                ballot).
//   relabel      a lane per node: key, then rank by counting the (key, id) pairs below its own.
//   output       a lane per new row: the row is gathered through the inverse ranks into the packed bitset in global
//                memory, with the degree beside it.
//
// The kernel guards itself: a graph whose parameters check_params refuses, whose workspace exceeds the launch's, or
// whose graph_ptr / bit_ptr entries are not those of its n or end beyond the arrays gets status = -1 and no other word
// written.  Every LDS index is below the workspace: node ids are below n by construction of every draw
// ((word * n) >> 32 < n) and the arrays have n words.  No global atomics: a graph has one owner.
#include "common_device.hpp"
#include "common_host.hpp"
#include "graph_gen.hpp"
#include "../../include/desco_hip.h"

namespace desco {

namespace gg = graph_gen;

struct GraphGenArgs {
  const int32_t* family;      // [G]
  const int32_t* n;           // [G]
  const int64_t* param;       // [G][2]
  const uint64_t* threshold;  // [G][2]
  const int64_t* graph_ptr;   // [G + 1]
  const int64_t* bit_ptr;     // [G + 1]
  const int64_t* graph_ids;   // [num_ids] the graphs of this launch, or null: all of them
  int64_t num_graphs, num_nodes, num_bit_words, ws_words;
  uint64_t seed;
  int64_t graph_base;
  int flags;
  uint32_t* bits;
  int32_t* deg;
  int32_t* status;
};

// B[v] = the smallest member of v's component; returns the number of components (uniform).  ctl: two LDS words.
template <int THREADS>
__device__ int components_parallel(gg::Graph& g, int* ctl) {
  const int tid = threadIdx.x, n = g.n, rw = g.rw;
  for (int v = tid; v < n; v += THREADS) g.B[v] = (uint32_t)v;
  for (;;) {
    __syncthreads();
    if (tid == 0) ctl[0] = 0;
    __syncthreads();
    int changed = 0;
    for (int v = tid; v < n; v += THREADS) {
      uint32_t m = g.B[v];
      for (int j = 0; j < rw; ++j)
        for (uint32_t w = g.adj[v * rw + j]; w; w &= w - 1) {
          const uint32_t b = g.B[32 * j + __builtin_ctz(w)];
          m = b < m ? b : m;
        }
      const uint32_t mm = g.B[m];                  // (labels only ever fall, and B[x] <= x names a member of x's
      m = mm < m ? mm : m;                         //  component: a stale read is still a valid, larger label)
      if (m < g.B[v]) g.B[v] = m, changed = 1;
    }
    if (changed) ctl[0] = 1;
    __syncthreads();
    if (!ctl[0]) break;
  }
  if (tid == 0) ctl[1] = 0;
  __syncthreads();
  int roots = 0;
  for (int v = tid; v < n; v += THREADS) roots += (int)g.B[v] == v;
  if (roots) atomicAdd(&ctl[1], roots);
  __syncthreads();
  const int count = ctl[1];
  __syncthreads();                                 // (the caller may clear the control words next)
  return count;
}

template <int THREADS>
__device__ void clear_parallel(uint32_t* ws, int64_t words) {
  for (int64_t i = threadIdx.x; i < words; i += THREADS) ws[i] = 0;
  __syncthreads();
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void graph_gen_kernel(GraphGenArgs p) {
  extern __shared__ uint32_t gg_lds[];
  const int tid = threadIdx.x;
  const int64_t gi = p.graph_ids ? p.graph_ids[blockIdx.x] : (int64_t)blockIdx.x;
  if (gi < 0 || gi >= p.num_graphs) return;                      // (uniform) a bad id: nothing to write to
  const int32_t family = p.family[gi], n32 = p.n[gi];
  const int64_t pa = p.param[2 * gi], pb = p.param[2 * gi + 1];
  const uint64_t t0 = p.threshold[2 * gi], t1 = p.threshold[2 * gi + 1];
  const int64_t n0 = p.graph_ptr[gi], b0 = p.bit_ptr[gi];
  if (gg::check_params(family, n32, pa, pb, t0, t1) != nullptr || gg::workspace_words(n32) > p.ws_words ||
      p.graph_ptr[gi + 1] - n0 != n32 || p.bit_ptr[gi + 1] - b0 != gg::bitset_words(n32) || n0 < 0 || b0 < 0 ||
      n0 + n32 > p.num_nodes || b0 + gg::bitset_words(n32) > p.num_bit_words) {
    if (tid == 0) p.status[gi] = -1;               // (uniform) not this launch's: no LDS is touched
    return;
  }
  const int n = n32;
  const int64_t words = gg::workspace_words(n);
  gg::Graph g(gg_lds, n);
  int* ctl = reinterpret_cast<int*>(gg_lds + words - 4);         // the workspace's last four words
  const uint32_t graph = (uint32_t)(p.graph_base + gi);
  const int rw = g.rw;
  clear_parallel<THREADS>(gg_lds, words);

  int tries = 0;
  if (n > 1) {
    if (family == gg::kER) {
      const int64_t pairs = (int64_t)n * (n - 1) / 2;
      for (int64_t q = tid; 4 * q < pairs; q += THREADS) {
        uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), graph, (uint32_t)gg::kBody};
        null_model::philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
        // the pair (u < v) of index 4 q: v = the largest v with v (v - 1) / 2 <= index
        int64_t v = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)(4 * q))) * 0.5);
        while (v * (v - 1) / 2 > 4 * q) --v;
        while ((v + 1) * v / 2 <= 4 * q) ++v;
        int64_t u = 4 * q - v * (v - 1) / 2;
        for (int k = 0; k < 4 && 4 * q + k < pairs; ++k) {
          if ((uint64_t)c[k] < t0) {
            atomicOr(&g.adj[v * rw + (u >> 5)], 1u << (u & 31));
            atomicOr(&g.adj[u * rw + (v >> 5)], 1u << (v & 31));
          }
          if (++u == v) u = 0, ++v;
        }
      }
      __syncthreads();
      for (int v = tid; v < n; v += THREADS) {
        uint32_t d = 0;
        for (int j = 0; j < rw; ++j) d += (uint32_t)__builtin_popcount(g.adj[v * rw + j]);
        g.D[v] = d;
      }
    } else if (family == gg::kWS) {
      const int h = (int)(pa / 2);
      tries = gg::kFellBack;
      for (int attempt = 0; h > 0 && attempt < gg::kWsTries; ++attempt) {      // (uniform: h and the count are)
        if (attempt) clear_parallel<THREADS>(gg_lds, words);
        if (tid < 64) gg::ws_try(g, p.seed, graph, attempt, h, t0);
        __syncthreads();
        if (components_parallel<THREADS>(g, ctl) == 1) {
          tries = attempt + 1;
          break;
        }
      }
      if (tries == gg::kFellBack) {
        __syncthreads();
        clear_parallel<THREADS>(gg_lds, words);
        if (tid < 64) gg::random_body(g, p.seed, graph, pb);
      }
    } else if (tid < 64) {
      if (family == gg::kRandom) gg::random_body(g, p.seed, graph, pa);
      else if (family == gg::kBA) gg::ba_body(g, p.seed, graph, (int)pa);
      else if (family == gg::kEBA) gg::eba_body(g, p.seed, graph, (int)pa, t0, t1);
      else gg::power_body(g, p.seed, graph, (int)pa, t0);
    }
  }
  __syncthreads();

  // ---- connection ---------------------------------------------------------------------------------------------------
  int added = 0;
  if (!(p.flags & DESCO_GRAPH_GEN_NO_CONNECT)) {                 // (uniform)
    components_parallel<THREADS>(g, ctl);
    if (tid < 64) ctl[2] = gg::connect(g, p.seed, graph);
    __syncthreads();
    added = ctl[2];
  }

  // ---- relabel: A = rank, B = its inverse ---------------------------------------------------------------------------
  for (int v = tid; v < n; v += THREADS) g.C[v] = (p.flags & DESCO_GRAPH_GEN_NO_RELABEL) ? 0u : gg::relabel_key(p.seed, graph, v);
  __syncthreads();
  for (int v = tid; v < n; v += THREADS) {
    const uint32_t key = g.C[v];
    uint32_t rank = 0;
    for (int u = 0; u < n; ++u) {
      const uint32_t ku = g.C[u];
      rank += ku < key || (ku == key && u < v);
    }
    g.A[v] = rank;
  }
  __syncthreads();
  for (int v = tid; v < n; v += THREADS) g.B[g.A[v]] = (uint32_t)v;          // (ranks are a permutation of 0 .. n - 1)
  __syncthreads();

  // ---- output -------------------------------------------------------------------------------------------------------
  uint32_t* __restrict__ bits = p.bits + b0;
  int32_t* __restrict__ deg = p.deg + n0;
  for (int a = tid; a < n; a += THREADS) {
    const int v = (int)g.B[a];
    deg[a] = (int32_t)g.D[v];
    const uint32_t* row = g.adj + v * rw;
    for (int j = 0; j < rw; ++j) {
      uint32_t w = 0;
      const int hi = 32 * j + 32 < n ? 32 * j + 32 : n;
      for (int b = 32 * j; b < hi; ++b) {
        const uint32_t u = g.B[b];
        w |= ((row[u >> 5] >> (u & 31)) & 1u) << (b & 31);
      }
      bits[(int64_t)a * rw + j] = w;
    }
  }
  if (tid == 0) p.status[gi] = (int32_t)(tries | (added << 8));
}

struct ExpandArgs {
  const int64_t* graph_ptr;
  const int64_t* bit_ptr;
  const uint32_t* bits;
  const int64_t* rowptr;
  int64_t num_graphs, num_nodes, num_bit_words, num_entries;
  int32_t* col;
};

// a lane per node of the workgroup's graph: its bitset row becomes its ascending col row.  A row whose popcount is not
// its rowptr span, or which ends beyond col, is not written.
__global__ __launch_bounds__(256) void graph_gen_expand_kernel(ExpandArgs p) {
  const int64_t gi = blockIdx.x;
  if (gi >= p.num_graphs) return;
  const int64_t n0 = p.graph_ptr[gi], n = p.graph_ptr[gi + 1] - n0, b0 = p.bit_ptr[gi];
  const int64_t rw = gg::row_words(n);
  if (n <= 0 || n0 < 0 || b0 < 0 || n0 + n > p.num_nodes || b0 + n * rw > p.num_bit_words) return;
  for (int64_t v = threadIdx.x; v < n; v += 256) {
    const uint32_t* row = p.bits + b0 + v * rw;
    int64_t e = p.rowptr[n0 + v];
    const int64_t e1 = p.rowptr[n0 + v + 1];
    int64_t count = 0;
    for (int64_t j = 0; j < rw; ++j) count += __builtin_popcount(row[j]);
    if (e < 0 || e1 - e != count || e1 > p.num_entries) continue;
    for (int64_t j = 0; j < rw; ++j)
      for (uint32_t w = row[j]; w; w &= w - 1) p.col[e++] = (int32_t)(n0 + 32 * j + __builtin_ctz(w));
  }
}

template <int THREADS>
int launch(const GraphGenArgs& a, int64_t num_ids, hipStream_t stream) {
  const hipError_t e = size_dynamic_lds<graph_gen_kernel<THREADS>>(4 * DESCO_GRAPH_GEN_DEV_MAX_WORDS);
  if (e != hipSuccess) return fail((int)e, "desco_graph_gen_dev: cannot size LDS");
  hipLaunchKernelGGL(graph_gen_kernel<THREADS>, dim3((unsigned)num_ids), dim3(THREADS), (size_t)(4 * a.ws_words),
                     stream, a);
  return launch_status("desco_graph_gen_dev");
}

}  // namespace desco

using namespace desco;

extern "C" int desco_graph_gen_dev(const int32_t* family, const int32_t* n, const int64_t* param,
                                   const uint64_t* threshold, int64_t num_graphs, const int64_t* graph_ids,
                                   int64_t num_ids, int64_t graph_base, uint64_t seed, const int64_t* graph_ptr,
                                   const int64_t* bit_ptr, int64_t num_nodes, int64_t num_bit_words, int64_t max_words, int waves, int flags, uint32_t* bits,
                                   int32_t* deg,
                                   int32_t* status, desco_stream_t stream) {
  if (num_graphs < 0 || num_ids < 0 || graph_base < 0 || num_nodes < 0 || num_bit_words < 0)
    return fail(DESCO_EINVAL,
                "desco_graph_gen_dev: negative num_graphs, num_ids, graph_base, num_nodes or num_bit_words");
  if (max_words < 0) return fail(DESCO_EINVAL, "desco_graph_gen_dev: negative max_words");
  if (waves != 0 && waves != 1 && waves != 4) return fail(DESCO_EINVAL, "desco_graph_gen_dev: waves is not 0, 1 or 4");
  if (flags & ~(DESCO_GRAPH_GEN_NO_CONNECT | DESCO_GRAPH_GEN_NO_RELABEL))
    return fail(DESCO_EINVAL, "desco_graph_gen_dev: unknown flags");
  if (!graph_ids) num_ids = num_graphs;
  if (num_ids == 0) return 0;
  if (max_words > DESCO_GRAPH_GEN_DEV_MAX_WORDS)
    return fail(DESCO_EINVAL,
                "desco_graph_gen_dev: a graph's workspace, n * (ceil(n / 32) | 1) + 4 n + 4 words, exceeds "
                "DESCO_GRAPH_GEN_DEV_MAX_WORDS (40960); use desco_graph_gen for it");
  if (num_ids > INT32_MAX) return fail(DESCO_EINVAL, "desco_graph_gen_dev: num_ids is above 2^31 - 1");
  if (!family || !n || !param || !threshold || !graph_ptr || !bit_ptr || !bits || !deg || !status)
    return fail(DESCO_EINVAL, "desco_graph_gen_dev: a null pointer with non-empty input");
  if (mis8(param) || mis8(threshold) || mis8(graph_ptr) || mis8(bit_ptr) || mis8(graph_ids))
    return fail(DESCO_EINVAL, "desco_graph_gen_dev: a 64-bit array is not 8-byte aligned");
  GraphGenArgs a;
  a.family = family, a.n = n, a.param = param, a.threshold = threshold, a.graph_ptr = graph_ptr, a.bit_ptr = bit_ptr;
  a.graph_ids = graph_ids;
  a.num_graphs = num_graphs, a.num_nodes = num_nodes, a.num_bit_words = num_bit_words;
  a.ws_words = max_words < 8 ? 8 : (max_words + 3) & ~(int64_t)3;
  a.seed = seed, a.graph_base = graph_base, a.flags = flags;
  a.bits = bits, a.deg = deg, a.status = status;
  // one wave per graph where the launch's graphs are small (DESCO_GRAPH_GEN_WAVE_WORDS), four above
  const bool one = waves == 1 || (waves == 0 && a.ws_words <= DESCO_GRAPH_GEN_WAVE_WORDS);
  return one ? launch<64>(a, num_ids, (hipStream_t)stream) : launch<256>(a, num_ids, (hipStream_t)stream);
}

extern "C" int desco_graph_gen_expand_dev(const int64_t* graph_ptr, const int64_t* bit_ptr, const uint32_t* bits,
                                          const int64_t* rowptr, int64_t num_graphs, int64_t num_nodes,
                                          int64_t num_bit_words, int64_t num_entries, int32_t* col,
                                          desco_stream_t stream) {
  if (num_graphs < 0 || num_nodes < 0 || num_bit_words < 0 || num_entries < 0)
    return fail(DESCO_EINVAL, "desco_graph_gen_expand_dev: a negative count");
  if (num_graphs == 0 || num_entries == 0) return 0;
  if (num_graphs > INT32_MAX) return fail(DESCO_EINVAL, "desco_graph_gen_expand_dev: num_graphs is above 2^31 - 1");
  if (!graph_ptr || !bit_ptr || !bits || !rowptr || !col)
    return fail(DESCO_EINVAL, "desco_graph_gen_expand_dev: a null pointer with non-empty input");
  if (mis8(graph_ptr) || mis8(bit_ptr) || mis8(rowptr))
    return fail(DESCO_EINVAL, "desco_graph_gen_expand_dev: a 64-bit array is not 8-byte aligned");
  ExpandArgs a{graph_ptr, bit_ptr, bits, rowptr, num_graphs, num_nodes, num_bit_words, num_entries, col};
  hipLaunchKernelGGL(graph_gen_expand_kernel, dim3((unsigned)num_graphs), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("desco_graph_gen_expand_dev");
}
