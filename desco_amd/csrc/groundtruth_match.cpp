// Exact canonical ground-truth counts of LARGE queries (C ABI: desco_canonical_match_plan_size,
// desco_canonical_match_plan, desco_canonical_counts_match).  Same definition as groundtruth.cpp:
//
//   count[v][q] = #{ node subsets S : max(S) = v, G[S] isomorphic to query q }      (induced)
//
// but where ESU visits every connected subset of up to k nodes and looks its adjacency mask up in a table of
// 2^(k(k-1)/2) entries (2 M at k = 7, 268 M at k = 8), this is a pattern-guided induced-subgraph matcher: its work
// follows the query.  Every query is compiled into a PLAN (groundtruth_match.hpp) of anchors -- the query node
// that lands on the root v, one per orbit of Aut(q) -- each with a connected matching order, the earlier position
// whose image's adjacency row supplies the candidates of a position, the exact adjacency / non-adjacency mask
// against the earlier positions, and order constraints between images that break the remaining symmetry.
//
// Exactness.  Fix S with max(S) = v and G[S] isomorphic to q.  The isomorphisms q -> G[S] number |Aut(q)|, the
// preimages of v run through exactly one orbit O of Aut(q), and those with f(a) = v for the orbit's
// representative a form one coset of Stab(a).  Inside Stab(a) the symmetry is broken as in Grochow and Kellis
// ("Network motif discovery using subgraph enumeration and symmetry-breaking", RECOMB 2007): while the group H
// (at first Stab(a)) moves some node x, require f(x) < f(y) for every other y of x's orbit under H and replace H
// by the stabiliser of x in H.  The images are distinct integers, so exactly one map of the coset meets all
// constraints: every subset is visited ONCE, no division is needed (a star K1,6 does not carry its 720
// automorphisms), and GTM_DIVISOR is 1.  Automorphisms are never listed (K1,15 has 15! of them): orbits come
// from a backtracking search for ONE automorphism that fixes the chosen nodes and maps x to y.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/desco_hip.h"
#include "common_host.hpp"
#include "groundtruth_match.hpp"

namespace {

using namespace desco;

struct Query {
  int k = 0;
  uint32_t adj[GTM_KMAX] = {0};        // adjacency row bitmasks
  int deg(int a) const { return __builtin_popcount(adj[a]); }
  bool has(int a, int b) const { return adj[a] >> b & 1; }
};

const char* kQueryLimit =
    ": queries must be connected and loop-free with 2..16 nodes (backend=\"vf2\" takes larger ones)";

// Reads and validates query q.  Returns nullptr or the message's tail.
const char* read_query(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges, int q, Query& out) {
  const int k = q_nodes[q];
  if (k < 2 || k > GTM_KMAX) return kQueryLimit;
  out = Query();
  out.k = k;
  if (q_edge_ptr[q + 1] < q_edge_ptr[q] || (q_edge_ptr[q + 1] > q_edge_ptr[q] && !q_edges)) return ": bad query edge";
  for (int e = q_edge_ptr[q]; e < q_edge_ptr[q + 1]; ++e) {
    const int a = q_edges[2 * e], b = q_edges[2 * e + 1];
    if (a < 0 || b < 0 || a >= k || b >= k) return ": bad query edge";
    if (a == b) return kQueryLimit;
    out.adj[a] |= 1u << b;
    out.adj[b] |= 1u << a;
  }
  uint32_t seen = 1, front = 1;
  while (front) {
    uint32_t next = 0;
    for (int a = 0; a < k; ++a)
      if (front >> a & 1) next |= out.adj[a];
    front = next & ~seen;
    seen |= front;
  }
  if (seen != (1u << k) - 1u) return kQueryLimit;
  return nullptr;
}

// Is there an automorphism g of q with g(src[t]) = dst[t] for t < m?  Backtracking over a connected order.
struct AutoSearch {
  const Query& q;
  int order[GTM_KMAX], img[GTM_KMAX], m;
  uint32_t used = 0;

  AutoSearch(const Query& q_, const int* src, const int* dst, int m_) : q(q_), m(m_) {
    uint32_t placed = 0;
    int n = 0;
    for (int t = 0; t < m; ++t) {
      order[n++] = src[t];
      placed |= 1u << src[t];
      img[t] = dst[t];
    }
    while (n < q.k) {                  // next: a node adjacent to a placed one (any node when nothing is placed)
      int pick = -1;
      for (int a = 0; a < q.k && pick < 0; ++a)
        if (!(placed >> a & 1) && (q.adj[a] & placed)) pick = a;
      for (int a = 0; a < q.k && pick < 0; ++a)
        if (!(placed >> a & 1)) pick = a;
      order[n++] = pick;
      placed |= 1u << pick;
    }
  }
  bool fits(int t, int y) const {
    if ((used >> y & 1) || q.deg(order[t]) != q.deg(y)) return false;
    for (int s = 0; s < t; ++s)
      if (q.has(order[s], order[t]) != q.has(img[s], y)) return false;
    return true;
  }
  bool go(int t) {
    if (t == q.k) return true;
    if (t < m) {
      const int y = img[t];
      if (!fits(t, y)) return false;
      used |= 1u << y;
      const bool ok = go(t + 1);
      used &= ~(1u << y);
      return ok;
    }
    for (int y = 0; y < q.k; ++y) {
      if (!fits(t, y)) continue;
      img[t] = y;
      used |= 1u << y;
      const bool ok = go(t + 1);
      used &= ~(1u << y);
      if (ok) return true;
    }
    return false;
  }
};

// orbit of x (as a bitmask) under the automorphisms that fix every node of fixed[0..m-1]
uint32_t orbit_of(const Query& q, const int* fixed, int m, int x) {
  int src[GTM_KMAX + 1], dst[GTM_KMAX + 1];
  for (int t = 0; t < m; ++t) src[t] = dst[t] = fixed[t];
  uint32_t orb = 1u << x;
  src[m] = x;
  for (int y = 0; y < q.k; ++y) {
    if (y == x || q.deg(y) != q.deg(x)) continue;
    bool is_fixed = false;
    for (int t = 0; t < m; ++t) is_fixed |= fixed[t] == y;
    if (is_fixed) continue;
    dst[m] = y;
    AutoSearch s(q, src, dst, m + 1);
    if (s.go(0)) orb |= 1u << y;
  }
  return orb;
}

// Appends the records of query `qi` to `plan` (one per orbit of Aut(q)).
void plan_query(const Query& q, int qi, std::vector<int32_t>& plan) {
  const int k = q.k;
  uint32_t covered = 0;
  for (int a = 0; a < k; ++a) {
    if (covered >> a & 1) continue;
    covered |= orbit_of(q, nullptr, 0, a);                       // a = the smallest node of its orbit

    // symmetry breaking inside Stab(a): less[x] = nodes y with the constraint image(x) < image(y)
    uint32_t less[GTM_KMAX] = {0};
    int fixed[GTM_KMAX], m = 0;
    fixed[m++] = a;
    for (bool moved = true; moved;) {
      moved = false;
      uint32_t is_fixed = 0;
      for (int t = 0; t < m; ++t) is_fixed |= 1u << fixed[t];
      for (int x = 0; x < k && !moved; ++x) {
        if (is_fixed >> x & 1) continue;
        const uint32_t orb = orbit_of(q, fixed, m, x);
        if (orb == (1u << x)) continue;
        less[x] |= orb & ~(1u << x);
        fixed[m++] = x;
        moved = true;
      }
    }

    // connected matching order from a: next = the node with the most placed neighbours (then the highest degree,
    // then the smallest id), so that the adjacency constraints bite as early as possible
    int node[GTM_KMAX];
    uint32_t placed = 1u << a;
    node[0] = a;
    for (int i = 1; i < k; ++i) {
      int pick = -1, best = 0;
      for (int c = 0; c < k; ++c) {
        if (placed >> c & 1) continue;
        const int back = __builtin_popcount(q.adj[c] & placed);
        if (!back) continue;
        const int score = back * 64 + q.deg(c);
        if (score > best) best = score, pick = c;
      }
      node[i] = pick;                                            // (exists: the query is connected)
      placed |= 1u << pick;
    }

    const size_t r = plan.size();
    plan.resize(r + GTM_REC, 0);
    int32_t* rec = plan.data() + r;
    rec[GTM_QUERY] = qi;
    rec[GTM_K] = k;
    rec[GTM_ANCHOR] = a;
    rec[GTM_DIVISOR] = 1;
    for (int i = 0; i < k; ++i) {
      const int x = node[i];
      uint32_t adj = 0, lt = 0, gt = 0;
      int parent = 0;
      for (int j = 0; j < i; ++j) {
        const int y = node[j];
        if (q.has(x, y)) adj |= 1u << j, parent = j;             // the latest adjacent earlier position
        if (less[x] >> y & 1) lt |= 1u << j;
        if (less[y] >> x & 1) gt |= 1u << j;
      }
      rec[GTM_NODE + i] = x;
      rec[GTM_PARENT + i] = parent;
      rec[GTM_ADJ + i] = (int32_t)adj;
      rec[GTM_LT + i] = (int32_t)lt;
      rec[GTM_GT + i] = (int32_t)gt;
    }
  }
}

int build_plan(const char* who, const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
               int num_queries, std::vector<int32_t>& plan) {
  if (!q_nodes || !q_edge_ptr || num_queries < 0)
    return fail(DESCO_EINVAL, (std::string(who) + ": bad argument").c_str());
  plan.assign(GTM_HEAD, 0);
  for (int q = 0; q < num_queries; ++q) {
    Query qq;
    if (const char* why = read_query(q_nodes, q_edge_ptr, q_edges, q, qq))
      return fail(DESCO_EINVAL, (std::string(who) + why).c_str());
    plan_query(qq, q, plan);
  }
  plan[0] = num_queries;
  plan[1] = (int32_t)((plan.size() - GTM_HEAD) / GTM_REC);
  return 0;
}

// One graph's matcher state.
struct Matcher {
  int64_t base;
  const int64_t* rowptr;
  const int32_t* col;
  const uint64_t* bits;
  int words, v;
  const int32_t* rec;
  int k;
  int img[GTM_KMAX];
  int64_t found;

  bool adj(int a, int b) const { return bits[(size_t)a * words + (b >> 6)] >> (b & 63) & 1; }

  bool fits(int level, int u) const {
    const uint32_t want = (uint32_t)rec[GTM_ADJ + level], lt = (uint32_t)rec[GTM_LT + level],
                   gt = (uint32_t)rec[GTM_GT + level];
    for (int j = 0; j < level; ++j) {
      const int w = img[j];
      if (u == w || adj(u, w) != (want >> j & 1)) return false;
      if ((lt >> j & 1) && !(u < w)) return false;
      if ((gt >> j & 1) && !(u > w)) return false;
    }
    return true;
  }

  void extend(int level) {
    const int64_t p = base + img[rec[GTM_PARENT + level]];
    for (int64_t e = rowptr[p]; e < rowptr[p + 1]; ++e) {
      const int u = (int)(col[e] - base);
      if (u >= v) break;                       // rows ascend: every image but the anchor's is below the root
      if (!fits(level, u)) continue;
      if (level + 1 == k) {
        ++found;
      } else {
        img[level] = u;
        extend(level + 1);
      }
    }
  }
};

}  // namespace

extern "C" int64_t desco_canonical_match_plan_size(const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                                   const int32_t* q_edges, int num_queries) {
  try {
    std::vector<int32_t> plan;
    if (build_plan("desco_canonical_match_plan_size", q_nodes, q_edge_ptr, q_edges, num_queries, plan)) return -1;
    return (int64_t)plan.size();
  } catch (const std::bad_alloc&) {
    fail(DESCO_ENOMEM, "desco_canonical_match_plan_size: out of memory");
    return -1;
  }
}

extern "C" int desco_canonical_match_plan(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                                          int num_queries, int32_t* plan, int64_t plan_entries) {
  try {
    std::vector<int32_t> p;
    if (const int rc = build_plan("desco_canonical_match_plan", q_nodes, q_edge_ptr, q_edges, num_queries, p))
      return rc;
    if (!plan || plan_entries != (int64_t)p.size())
      return fail(DESCO_EINVAL, "desco_canonical_match_plan: plan_entries is not desco_canonical_match_plan_size");
    std::memcpy(plan, p.data(), p.size() * sizeof(int32_t));
    return 0;
  } catch (const std::bad_alloc&) {
    return fail(DESCO_ENOMEM, "desco_canonical_match_plan: out of memory");
  }
}

// Structural check of a plan handed back by a caller (both matchers index with its fields).
int desco::match_plan_check(const char* who, const int32_t* plan, int64_t plan_entries, int num_queries) {
  const std::string w(who);
  if (!plan || plan_entries < GTM_HEAD || plan[0] != num_queries || plan[1] < 0 ||
      plan_entries != GTM_HEAD + (int64_t)plan[1] * GTM_REC)
    return fail(DESCO_EINVAL, (w + ": not a plan of desco_canonical_match_plan for these queries").c_str());
  for (int a = 0; a < plan[1]; ++a) {
    const int32_t* rec = plan + GTM_HEAD + (int64_t)a * GTM_REC;
    const int k = rec[GTM_K];
    bool ok = rec[GTM_QUERY] >= 0 && rec[GTM_QUERY] < num_queries && k >= 2 && k <= GTM_KMAX && rec[GTM_DIVISOR] == 1;
    for (int i = 1; ok && i < k; ++i) {
      const uint32_t below = (1u << i) - 1u;
      const int p = rec[GTM_PARENT + i];
      ok = p >= 0 && p < i && ((uint32_t)rec[GTM_ADJ + i] >> p & 1) && !((uint32_t)rec[GTM_ADJ + i] & ~below) &&
           !((uint32_t)rec[GTM_LT + i] & ~below) && !((uint32_t)rec[GTM_GT + i] & ~below);
    }
    if (!ok) return fail(DESCO_EINVAL, (w + ": malformed plan record").c_str());
  }
  return 0;
}

extern "C" int desco_canonical_counts_match(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                            const int32_t* col, const int32_t* plan, int64_t plan_entries,
                                            int num_queries, int num_threads, int64_t* out) {
  if (!graph_ptr || !rowptr || !out || num_graphs < 0 || num_queries < 0)
    return fail(DESCO_EINVAL, "desco_canonical_counts_match: bad argument");
  if (const int rc = match_plan_check("desco_canonical_counts_match", plan, plan_entries, num_queries)) return rc;
  try {
    const int64_t total = graph_ptr[num_graphs];
    std::memset(out, 0, sizeof(int64_t) * (size_t)total * (size_t)num_queries);
    const int num_anchors = plan[1];
    if (num_queries == 0 || num_anchors == 0) return 0;
#ifdef _OPENMP
    const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
    const int nt = 1;
    (void)num_threads;
#endif
    bool oom = false;
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
    for (int64_t g = 0; g < num_graphs; ++g) {
      const int64_t base = graph_ptr[g], n = graph_ptr[g + 1] - base;
      const int words = (int)((n + 63) / 64);
      std::vector<uint64_t> bits;
      try {
        bits.assign((size_t)n * words, 0);
      } catch (const std::bad_alloc&) {
#pragma omp atomic write
        oom = true;
        continue;
      }
      for (int64_t u = 0; u < n; ++u)
        for (int64_t e = rowptr[base + u]; e < rowptr[base + u + 1]; ++e) {
          const int w = (int)(col[e] - base);
          bits[(size_t)u * words + (w >> 6)] |= (uint64_t)1 << (w & 63);
        }
      Matcher m;
      m.base = base;
      m.rowptr = rowptr;
      m.col = col;
      m.bits = bits.data();
      m.words = words;
      for (int v = 1; v < (int)n; ++v) {
        if (rowptr[base + v] == rowptr[base + v + 1]) continue;
        m.v = v;
        m.img[0] = v;
        for (int a = 0; a < num_anchors; ++a) {
          m.rec = plan + GTM_HEAD + (int64_t)a * GTM_REC;
          m.k = m.rec[GTM_K];
          m.found = 0;
          m.extend(1);
          out[(base + v) * num_queries + m.rec[GTM_QUERY]] += m.found;
        }
      }
    }
    if (oom) return fail(DESCO_ENOMEM, "desco_canonical_counts_match: out of memory");
    return 0;
  } catch (const std::bad_alloc&) {
    return fail(DESCO_ENOMEM, "desco_canonical_counts_match: out of memory");
  }
}
