// The synthetic graph generators' definition, as the host twin (graph_gen.cpp) and the gfx950 kernel
// (graph_gen_dev.hip) share it.  See include/desco_hip.h, "GRAPH GENERATORS", for the definition in words; this file
// is that definition as code, compiled by both compilers, so the two sides cannot drift apart.
//
// A graph lives in a workspace of 32-bit words: the adjacency bitset (n rows of ceil(n / 32) | 1 words) and four arrays
// of n words, A B C D.  D is the degree throughout; the others change hands between the phases:
//                A               B                     C
//   BA           chosen mark     -                     the new node's targets
//   EBA          chosen mark     eligibility flag      the new node's targets
//   Power        weight          chosen mark           the new node's targets, in draw order
//   connection   tree degree     component of a node   smallest member -> component, then the Pruefer sequence
//   relabel      rank            inverse of the rank   key
//
// THE EBA WEIGHT INVARIANT.  The extended Barabasi-Albert model keeps a list in which a node appears once when it is
// created and once more for every edge end it gains; a rewiring takes one entry of the end that loses the edge and
// gives one to the end that gains it, and the pivot keeps its degree.  A node created by the growth step gets m edges
// and m + 1 entries.  By induction over the three steps every node appears deg + 1 times, so a uniform choice from the
// list IS a choice with weight deg + 1, and "a choice among the entries that are not in a prohibited set" is that
// choice with the prohibited nodes' weights zeroed.  No list is kept.
// WHERE THE LIST WOULD BE EMPTY (no eligible node, or no node outside the prohibited set) the textbook model fails; here
// the remaining iterations of that step are skipped and the growth step follows.
#pragma once
#include <stdint.h>

#include "null_model.hpp"

#if defined(__HIPCC__)
#define DESCO_GG_HD __host__ __device__ __forceinline__
#else
#define DESCO_GG_HD inline
#endif

namespace desco {
namespace graph_gen {

enum Family : int32_t { kER = 0, kWS = 1, kRandom = 2, kBA = 3, kEBA = 4, kPower = 5, kFamilies = 6 };
// the fourth counter word: which phase draws
enum Stream : uint32_t { kBody = 0, kRandomBody = 1, kConnect = 2, kRelabel = 3, kWsTry = 16 };
constexpr int kWsTries = 100;
constexpr int kFellBack = kWsTries + 1;          // "tries" of a WS graph that ended in the Random family

DESCO_GG_HD int64_t row_words(int64_t n) { return null_model::row_words(n); }
DESCO_GG_HD int64_t bitset_words(int64_t n) { return n * row_words(n); }
// (the last four words are the kernel's control words)
DESCO_GG_HD int64_t workspace_words(int64_t n) { return bitset_words(n) + 4 * n + 4; }

// word i of the sequence (graph, stream): word i & 3 of the Philox call with counter t = i >> 2
DESCO_GG_HD uint32_t word(uint64_t seed, uint32_t graph, uint32_t stream, uint64_t i) {
  const uint64_t t = i >> 2;
  uint32_t c[4] = {(uint32_t)t, (uint32_t)(t >> 32), graph, stream};
  null_model::philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return c[i & 3];
}

// the words of one (graph, stream) sequence in order
struct Rng {
  uint64_t seed, i;
  uint32_t graph, stream, buf[4];
  DESCO_GG_HD Rng(uint64_t seed_, uint32_t graph_, uint32_t stream_) : seed(seed_), i(0), graph(graph_), stream(stream_) {}
  DESCO_GG_HD uint32_t next() {
    if ((i & 3) == 0) {
      const uint64_t t = i >> 2;
      buf[0] = (uint32_t)t, buf[1] = (uint32_t)(t >> 32), buf[2] = graph, buf[3] = stream;
      null_model::philox4x32_10(buf, (uint32_t)seed, (uint32_t)(seed >> 32));
    }
    return buf[i++ & 3];
  }
  DESCO_GG_HD uint32_t below(uint32_t w) { return (uint32_t)(((uint64_t)next() * w) >> 32); }       // uniform in [0, w)
  DESCO_GG_HD bool bernoulli(uint64_t threshold) { return (uint64_t)next() < threshold; }
};

struct Graph {
  uint32_t *adj, *A, *B, *C, *D;
  int n, rw;
  DESCO_GG_HD Graph(uint32_t* ws, int n_) : n(n_), rw((int)row_words(n_)) {
    adj = ws;
    A = ws + bitset_words(n_), B = A + n_, C = B + n_, D = C + n_;
  }
  DESCO_GG_HD bool has(int u, int v) const { return (adj[u * rw + (v >> 5)] >> (v & 31)) & 1u; }
  DESCO_GG_HD void add(int u, int v) {
    adj[u * rw + (v >> 5)] |= 1u << (v & 31), adj[v * rw + (u >> 5)] |= 1u << (u & 31);
    ++D[u], ++D[v];
  }
  DESCO_GG_HD void del(int u, int v) {
    adj[u * rw + (v >> 5)] &= ~(1u << (v & 31)), adj[v * rw + (u >> 5)] &= ~(1u << (u & 31));
    --D[u], --D[v];
  }
  DESCO_GG_HD void clear() {
    const int64_t words = workspace_words(n);
    for (int64_t i = 0; i < words; ++i) adj[i] = 0;
  }
};

DESCO_GG_HD int kth_bit(uint32_t w, int k) {          // position of the k-th set bit of w, k < popcount(w)
  for (; k > 0; --k) w &= w - 1;
  return __builtin_ctz(w);
}

// THE WAVE FORMS.  On the device the sequential bodies below are run by ALL 64 LANES OF ONE WAVEFRONT with equal
// arguments: every lane executes the whole chain and writes the same words.  The searches over n nodes -- the k-th
// marked node, a sum of weights, the preferential choice, the rebuild of the flags -- then split the nodes over the
// lanes and exchange through ballots and shuffles; they return, in every lane, the integer the sequential loop returns.
// WHAT THIS RESTS ON.  The 64 lanes do plain, non-atomic read-modify-writes on the same LDS words (++D[u], the bitset's
// |= and &=).  Between independent threads that would be a data race; it is correct here only because a wave64 of
// gfx950 executes one instruction stream in lockstep -- every lane has finished a load before any lane issues the store
// that follows it, and all lanes store the same value -- and because the LDS serves a wave's accesses in issue order.
// So: (1) these bodies may only be entered by a whole wavefront, all 64 lanes active (the kernel's `tid < 64`, never a
// narrower or a lane-dependent condition); (2) NO DIVERGENT BRANCH may ever be added to them: every condition has to
// be computed from values that are equal in all lanes (draws, graph state, uniform arguments), the lane-dependent
// work stays inside the wave_* helpers, which return uniform values; (3) they must not be split over several waves.
// A word that one lane alone writes (set_flags) is fenced at wavefront scope before any other lane reads it.
#if defined(__HIP_DEVICE_COMPILE__)
#define DESCO_GG_WAVE 1
__device__ __forceinline__ int wave_lane() { return (int)(threadIdx.x & 63u); }
// position of the k-th set bit of a ballot, k < popcount
__device__ __forceinline__ int kth_bit64(uint64_t b, uint32_t k) {
  for (; k > 0; --k) b &= b - 1;
  return __builtin_ctzll(b);
}
// the k-th v < cnt with pred(v), or cnt
template <class Pred>
__device__ __forceinline__ int wave_kth(int cnt, uint32_t k, Pred pred) {
  const int lane = wave_lane();
  for (int base = 0; base < cnt; base += 64) {
    const int v = base + lane;
    const uint64_t b = __ballot(v < cnt && pred(v));
    const uint32_t c = (uint32_t)__builtin_popcountll(b);
    if (k < c) return base + kth_bit64(b, k);
    k -= c;
  }
  return cnt;
}
template <class Pred>
__device__ __forceinline__ uint32_t wave_count(int cnt, Pred pred) {
  const int lane = wave_lane();
  uint32_t c = 0;
  for (int base = 0; base < cnt; base += 64) c += (uint32_t)__builtin_popcountll(__ballot(base + lane < cnt && pred(base + lane)));
  return c;
}
#endif

// flag[v] = pred(v) for every v < cnt; returns how many are set
template <class Pred>
DESCO_GG_HD int set_flags(uint32_t* flag, int cnt, Pred pred) {
#if defined(DESCO_GG_WAVE)
  const int lane = wave_lane();
  int c = 0;
  for (int base = 0; base < cnt; base += 64) {
    const int v = base + lane;
    const bool on = v < cnt && pred(v);
    if (v < cnt) flag[v] = on;
    c += __builtin_popcountll(__ballot(on));
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // a lane's words, before the other lanes read them
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return c;
#else
  int c = 0;
  for (int v = 0; v < cnt; ++v) c += (int)(flag[v] = pred(v));
  return c;
#endif
}
// the k-th node v < cnt with flag[v] != 0 in id order; cnt when there are k or fewer
DESCO_GG_HD int kth_flagged(const uint32_t* flag, int cnt, uint32_t k) {
#if defined(DESCO_GG_WAVE)
  return wave_kth(cnt, k, [&](int v) { return flag[v] != 0; });
#else
  for (int v = 0; v < cnt; ++v)
    if (flag[v] && k-- == 0) return v;
  return cnt;
#endif
}
// the k-th node v < n with value[v] == x
DESCO_GG_HD int kth_equal(const uint32_t* value, int n, uint32_t x, uint32_t k) {
#if defined(DESCO_GG_WAVE)
  return wave_kth(n, k, [&](int v) { return value[v] == x; });
#else
  for (int v = 0; v < n; ++v)
    if (value[v] == x && k-- == 0) return v;
  return n;
#endif
}
// the number of nodes v < n with value[v] == x
DESCO_GG_HD uint32_t count_equal(const uint32_t* value, int n, uint32_t x) {
#if defined(DESCO_GG_WAVE)
  return wave_count(n, [&](int v) { return value[v] == x; });
#else
  uint32_t c = 0;
  for (int v = 0; v < n; ++v) c += value[v] == x;
  return c;
#endif
}
// the k-th neighbour of u in id order, k < deg(u)
DESCO_GG_HD int kth_neighbour(const Graph& g, int u, uint32_t k) {
  for (int j = 0; j < g.rw; ++j) {
    const uint32_t w = g.adj[u * g.rw + j];
    const uint32_t c = (uint32_t)__builtin_popcount(w);
    if (k < c) return 32 * j + kth_bit(w, (int)k);
    k -= c;
  }
  return g.n;
}

// PREFERENTIAL CHOICE: the node whose interval of the prefix weights, in id order over the nodes below cnt, holds r.
//   mode 0  weight = degree;  mode 1  weight = A[v];  mode 2  weight = degree + 1, 0 for `excl` and its neighbours
//   (excl < 0: nobody is excluded).  total() is the sum of the same weights.
DESCO_GG_HD uint32_t weight(const Graph& g, int mode, int excl, int v) {
  if (mode == 0) return g.D[v];
  if (mode == 1) return g.A[v];
  return excl >= 0 && (v == excl || g.has(excl, v)) ? 0u : g.D[v] + 1u;
}
DESCO_GG_HD uint32_t total(const Graph& g, int cnt, int mode, int excl) {
  uint32_t s = 0;
#if defined(DESCO_GG_WAVE)
  for (int v = wave_lane(); v < cnt; v += 64) s += weight(g, mode, excl, v);
  for (int d = 32; d > 0; d >>= 1) s += (uint32_t)__shfl_xor((int)s, d);
#else
  for (int v = 0; v < cnt; ++v) s += weight(g, mode, excl, v);
#endif
  return s;
}
DESCO_GG_HD int pick(const Graph& g, int cnt, int mode, int excl, uint32_t r) {
  uint32_t acc = 0;
#if defined(DESCO_GG_WAVE)
  const int lane = wave_lane();
  for (int base = 0; base < cnt; base += 64) {     // a wave prefix sum over 64 nodes, then the first lane past r
    const int v = base + lane;
    uint32_t incl = v < cnt ? weight(g, mode, excl, v) : 0u;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += up;
    }
    const uint32_t chunk = (uint32_t)__shfl((int)incl, 63);
    if (r < acc + chunk) return base + __builtin_ctzll(__ballot(r < acc + incl));
    acc += chunk;
  }
#else
  for (int v = 0; v < cnt; ++v) {
    acc += weight(g, mode, excl, v);
    if (r < acc) return v;
  }
#endif
  return cnt - 1;                                  // (r < total: not reached)
}
// m distinct nodes below cnt by preferential draws of total weight w, into C[0 .. m) in draw order; `mark` is all zero
// before and after
DESCO_GG_HD void distinct_targets(Graph& g, Rng& r, int cnt, int m, int mode, uint32_t w, uint32_t* mark) {
  for (int have = 0; have < m;) {
    const int x = pick(g, cnt, mode, -1, r.below(w));
    if (!mark[x]) mark[x] = 1, g.C[have++] = (uint32_t)x;
  }
  for (int i = 0; i < m; ++i) mark[g.C[i]] = 0;
}

// ---- the families' sequential parts (ER's pairs are independent: see er_pair) ---------------------------------------

// pair index of (u < v) and back
DESCO_GG_HD uint64_t pair_index(uint32_t u, uint32_t v) { return (uint64_t)v * (v - 1) / 2 + u; }
DESCO_GG_HD void er_body(Graph& g, uint64_t seed, uint32_t graph, uint64_t threshold) {
  Rng r(seed, graph, kBody);                           // (the pair index counts up in this order of the loops)
  for (int v = 1; v < g.n; ++v)
    for (int u = 0; u < v; ++u)
      if (r.bernoulli(threshold)) g.add(u, v);
}

DESCO_GG_HD void complete(Graph& g) {
  for (int v = 1; v < g.n; ++v)
    for (int u = 0; u < v; ++u) g.add(u, v);
}

// G(n, m) on the empty graph g
DESCO_GG_HD void random_body(Graph& g, uint64_t seed, uint32_t graph, int64_t m) {
  const int64_t room = (int64_t)g.n * (g.n - 1) / 2;
  if (m >= room) return complete(g);
  Rng r(seed, graph, kRandomBody);
  for (int64_t e = 0; e < m;) {
    const int u = (int)r.below((uint32_t)g.n), v = (int)r.below((uint32_t)g.n);
    if (u == v || g.has(u, v)) continue;
    g.add(u, v), ++e;
  }
}

// one Watts-Strogatz try on the empty graph g, h = k / 2 >= 1 neighbours per side
DESCO_GG_HD void ws_try(Graph& g, uint64_t seed, uint32_t graph, int attempt, int h, uint64_t threshold) {
  const int n = g.n;
  for (int j = 1; j <= h; ++j)
    for (int u = 0; u < n; ++u) {
      const int v = u + j < n ? u + j : u + j - n;
      if (!g.has(u, v)) g.add(u, v);
    }
  Rng r(seed, graph, kWsTry + (uint32_t)attempt);
  for (int j = 1; j <= h; ++j)
    for (int u = 0; u < n; ++u) {
      if (!r.bernoulli(threshold)) continue;
      if ((int)g.D[u] >= n - 1) continue;
      const int v = u + j < n ? u + j : u + j - n;
      int w;
      do w = (int)r.below((uint32_t)n);
      while (w == u || g.has(u, w));
      g.del(u, v), g.add(u, w);
    }
}

DESCO_GG_HD void ba_body(Graph& g, uint64_t seed, uint32_t graph, int m) {
  for (int v = 1; v <= m; ++v) g.add(0, v);
  Rng r(seed, graph, kBody);
  uint32_t w = 2u * (uint32_t)m;
  for (int s = m + 1; s < g.n; ++s) {
    distinct_targets(g, r, s, m, 0, w, g.A);
    for (int i = 0; i < m; ++i) g.add(s, (int)g.C[i]);
    w += 2u * (uint32_t)m;
  }
}

DESCO_GG_HD void eba_body(Graph& g, uint64_t seed, uint32_t graph, int m, uint64_t t_add, uint64_t t_rewire) {
  Rng r(seed, graph, kBody);
  int64_t edges = 0;
  for (int s = m; s < g.n; ++s) {
    const int cnt = s, full = s - 1;                       // existing nodes; the degree of a saturated one
    const int64_t room = (int64_t)cnt * full / 2;
    const uint64_t a = r.next();
    if (a < t_add) {
      if (edges + m <= room) {                             // add m edges between existing nodes
        int flagged = set_flags(g.B, cnt, [&](int v) { return (int)g.D[v] < full; });
        for (int i = 0; i < m && flagged > 0; ++i) {
          const int src = kth_flagged(g.B, cnt, r.below((uint32_t)flagged));
          const uint32_t w = total(g, cnt, 2, src);
          if (w == 0) break;
          const int dst = pick(g, cnt, 2, src, r.below(w));
          g.add(src, dst), ++edges;
          if ((int)g.D[src] == full) g.B[src] = 0, --flagged;
          if ((int)g.D[dst] == full && g.B[dst]) g.B[dst] = 0, --flagged;
        }
      }
    } else if (a < t_rewire) {
      if (m <= edges && edges < room) {                    // rewire m edges
        int flagged = set_flags(g.B, cnt, [&](int v) { return g.D[v] > 0 && (int)g.D[v] < full; });
        for (int i = 0; i < m && flagged > 0; ++i) {
          const int node = kth_flagged(g.B, cnt, r.below((uint32_t)flagged));
          if (g.D[node] == 0) break;
          const int old = kth_neighbour(g, node, r.below(g.D[node]));
          const uint32_t w = total(g, cnt, 2, node);
          if (w == 0) break;
          const int dst = pick(g, cnt, 2, node, r.below(w));
          g.del(node, old), g.add(node, dst);
          if (g.D[old] == 0 && g.B[old]) g.B[old] = 0, --flagged;
          if (g.B[dst]) {
            if ((int)g.D[dst] == full) g.B[dst] = 0, --flagged;
          } else if (g.D[dst] == 1) {
            g.B[dst] = 1, ++flagged;                       // (a node that merely leaves saturation is not flagged again)
          }
        }
      }
    }
    distinct_targets(g, r, cnt, m, 2, (uint32_t)(2 * edges + cnt), g.A);
    for (int i = 0; i < m; ++i) g.add(s, (int)g.C[i]);
    edges += m;
  }
}

// THE OPEN NEIGHBOURS of `target` for the new node s: target's neighbours that are neither s nor joined to s, as bitset
// words; their number, and the k-th of them in id order (k < their number)
DESCO_GG_HD uint32_t open_word(const Graph& g, int target, int s, int j) {
  return g.adj[target * g.rw + j] & ~g.adj[s * g.rw + j] & ~(j == (s >> 5) ? 1u << (s & 31) : 0u);
}
DESCO_GG_HD int open_count(const Graph& g, int target, int s) {
  int open = 0;
#if defined(DESCO_GG_WAVE)
  for (int j = wave_lane(); j < g.rw; j += 64) open += __builtin_popcount(open_word(g, target, s, j));
  for (int d = 32; d > 0; d >>= 1) open += __shfl_xor(open, d);
#else
  for (int j = 0; j < g.rw; ++j) open += __builtin_popcount(open_word(g, target, s, j));
#endif
  return open;
}
DESCO_GG_HD int open_kth(const Graph& g, int target, int s, uint32_t k) {
#if defined(DESCO_GG_WAVE)
  const int lane = wave_lane();
  for (int base = 0; base < g.rw; base += 64) {          // a word per lane, a wave prefix sum over their populations
    const int j = base + lane;
    const uint32_t c = j < g.rw ? open_word(g, target, s, j) : 0u;
    const uint32_t pc = (uint32_t)__builtin_popcount(c);
    uint32_t incl = pc;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += up;
    }
    const uint32_t chunk = (uint32_t)__shfl((int)incl, 63);
    if (k < chunk) {
      const int at = __builtin_ctzll(__ballot(k < incl));
      const uint32_t word_at = (uint32_t)__shfl((int)c, at), before = (uint32_t)__shfl((int)(incl - pc), at);
      return 32 * (base + at) + kth_bit(word_at, (int)(k - before));
    }
    k -= chunk;
  }
#else
  for (int j = 0; j < g.rw; ++j) {
    const uint32_t c = open_word(g, target, s, j);
    const uint32_t pc = (uint32_t)__builtin_popcount(c);
    if (k < pc) return 32 * j + kth_bit(c, (int)k);
    k -= pc;
  }
#endif
  return g.n;                                           // (k < the count: not reached)
}

DESCO_GG_HD void power_body(Graph& g, uint64_t seed, uint32_t graph, int m, uint64_t threshold) {
  Rng r(seed, graph, kBody);
  for (int v = 0; v < m; ++v) g.A[v] = 1;
  uint32_t w = (uint32_t)m;
  for (int s = m; s < g.n; ++s) {
    distinct_targets(g, r, s, m, 1, w, g.B);
    int next = 0, target = (int)g.C[next++];
    if (!g.has(s, target)) g.add(s, target);
    ++g.A[target], ++w;
    for (int count = 1; count < m;) {
      if (r.bernoulli(threshold)) {                        // a neighbour of the last target that s does not touch yet
        const int open = open_count(g, target, s);
        if (open > 0) {
          const int nb = open_kth(g, target, s, r.below((uint32_t)open));
          g.add(s, nb);
          ++g.A[nb], ++w;
          continue;                                        // (a triangle edge does not count towards m)
        }
      }
      target = (int)g.C[next++];
      if (!g.has(s, target)) g.add(s, target);
      ++g.A[target], ++w, ++count;                         // (counted even where the edge stood already)
    }
    g.A[s] += (uint32_t)m, w += (uint32_t)m;
  }
}

// ---- components, connection, relabel --------------------------------------------------------------------------------

// B[v] = the smallest member of v's component (sequential: a walk from every unlabelled node in ascending order, the
// stack in C); returns the number of components
DESCO_GG_HD int components(Graph& g) {
  const uint32_t none = 0xffffffffu;
  for (int v = 0; v < g.n; ++v) g.B[v] = none;
  int c = 0;
  for (int s = 0; s < g.n; ++s) {
    if (g.B[s] != none) continue;
    ++c;
    int top = 0;
    g.C[top++] = (uint32_t)s, g.B[s] = (uint32_t)s;
    while (top > 0) {
      const int v = (int)g.C[--top];
      for (int j = 0; j < g.rw; ++j)
        for (uint32_t w = g.adj[v * g.rw + j]; w; w &= w - 1) {
          const int u = 32 * j + __builtin_ctz(w);
          if (g.B[u] == none) g.B[u] = (uint32_t)s, g.C[top++] = (uint32_t)u;
        }
    }
  }
  return c;
}

// With B = the smallest member of every node's component: joins the c components by a uniform random labelled tree;
// returns the edges added, c - 1
DESCO_GG_HD int connect(Graph& g, uint64_t seed, uint32_t graph) {
  int c = 0;
  for (int v = 0; v < g.n; ++v) {                          // components numbered by their smallest member
    if ((int)g.B[v] == v) g.C[v] = (uint32_t)c++;
    g.B[v] = g.C[g.B[v]];
  }
  if (c <= 1) return 0;
  Rng r(seed, graph, kConnect);
  auto join = [&](uint32_t i, uint32_t j) {
    const uint32_t si = count_equal(g.B, g.n, i), sj = count_equal(g.B, g.n, j);
    const int a = kth_equal(g.B, g.n, i, r.below(si));
    const int b = kth_equal(g.B, g.n, j, r.below(sj));
    g.add(a, b);
  };
  for (int i = 0; i < c; ++i) g.A[i] = 1;
  for (int i = 0; i < c - 2; ++i) g.C[i] = r.below((uint32_t)c), ++g.A[g.C[i]];
  // Pruefer decoding: every entry x is joined to the smallest node that is a leaf by then
  int ptr = 0;
  while (g.A[ptr] != 1) ++ptr;
  int leaf = ptr;
  for (int i = 0; i < c - 2; ++i) {
    const int x = (int)g.C[i];
    join((uint32_t)leaf, (uint32_t)x);
    if (--g.A[x] == 1 && x < ptr) {
      leaf = x;
    } else {
      do ++ptr;
      while (g.A[ptr] != 1);
      leaf = ptr;
    }
  }
  join((uint32_t)leaf, (uint32_t)(c - 1));
  return c - 1;
}

// the key of node v in the relabelling; the new id of v is the rank of (key, v)
DESCO_GG_HD uint32_t relabel_key(uint64_t seed, uint32_t graph, int v) { return word(seed, graph, kRelabel, (uint64_t)v); }

// what is wrong with a graph's parameters, or nullptr.  n == 1 is the single node whatever the parameters say.
DESCO_GG_HD const char* check_params(int32_t family, int32_t n, int64_t a, int64_t b, uint64_t t0, uint64_t t1) {
  if (family < 0 || family >= kFamilies) return "unknown family";
  if (n < 1) return "n < 1";
  if (t0 > ((uint64_t)1 << 32) || t1 > ((uint64_t)1 << 32)) return "a threshold above 2^32";
  if (n == 1) return nullptr;
  switch (family) {
    case kWS: return a < 0 || a > n - 1 || b < 0 ? "WS needs 0 <= k <= n - 1 and an edge target >= 0 (m outside the family's range)" : nullptr;
    case kRandom: return a < 0 ? "Random needs m >= 0 (m outside the family's range)" : nullptr;
    case kBA: return a < 1 || a >= n ? "BA needs 1 <= m < n (m outside the family's range)" : nullptr;
    case kEBA: return a < 1 || a >= n ? "EBA needs 1 <= m < n (m outside the family's range)"
                      : t0 > t1 ? "EBA needs threshold 0 <= threshold 1" : nullptr;
    case kPower: return a < 1 || a > n ? "Power needs 1 <= m <= n (m outside the family's range)" : nullptr;
    default: return nullptr;
  }
}

}  // namespace graph_gen
}  // namespace desco
