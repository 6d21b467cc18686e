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
//
// LABELLED queries (--use_node_feature; desco_canonical_match_plan_labelled_size, desco_canonical_match_plan_labelled,
// desco_canonical_counts_match_labelled): every node carries an int32 label id and a map must preserve it.  The same
// argument holds with Aut(q) replaced by the LABEL-PRESERVING automorphisms: anchors are one per orbit of that
// (smaller) group and the order constraints break only it, so an asymmetrically labelled P7 has 7 anchors and no
// constraint, and an all-equal labelling gives the unlabelled records.  The reference's expansion of a query into
// F^k labelled copies is full of copies isomorphic to each other, so the labelled plan is built over labelled
// isomorphism CLASSES (numbered by first query; the caller expands out[:, class_of_query]), its records carry the
// label of every position and are sorted by (label of position 0, label of position 1) with a bucket table behind
// them (groundtruth_match.hpp): a root and its first neighbour select the one bucket whose records can match.
//
// NON-INDUCED mode (desco_canonical_counts_match_mode, desco_canonical_counts_match_labelled_mode with induced = 0):
//
//   count[v][q] = #{ injective f : {f(a), f(b)} in E(G) for every {a, b} in E(q), max(im f) = v } / |Aut(q)|
//
// i.e. occurrences of q as a not necessarily induced subgraph (monomorphisms), rooted at the largest image.  The plan
// is the same, byte for byte: anchors, matching order and order constraints depend on Aut(q) alone, and Aut(q) acts
// freely on monomorphisms by pre-composition exactly as on induced embeddings, so the argument above holds word for
// word with "isomorphisms q -> G[S]" replaced by "the |Aut(q)| monomorphisms with one image (node AND edge set)".  Only
// the reading of rec[GTM_ADJ] differs: a set bit still means "adjacent", a clear bit means nothing.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "groundtruth_esu.hpp"
#include "groundtruth_match.hpp"
#include "occurrences.hpp"

namespace {

using namespace desco;

struct Query {
  int k = 0;
  uint32_t adj[GTM_KMAX] = {0};        // adjacency row bitmasks
  int32_t lab[GTM_KMAX] = {0};         // label ids (all 0: an unlabelled query)
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

// Is there an isomorphism g from q onto p (edges and labels preserved; p = q: an automorphism) with g(src[t]) = dst[t]
// for t < m?  Backtracking over a connected order.  q and p have the same number of nodes.
struct AutoSearch {
  const Query& q;
  const Query& p;
  int order[GTM_KMAX], img[GTM_KMAX], m;
  uint32_t used = 0;

  AutoSearch(const Query& q_, const Query& p_, const int* src, const int* dst, int m_) : q(q_), p(p_), m(m_) {
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
    if ((used >> y & 1) || q.deg(order[t]) != p.deg(y) || q.lab[order[t]] != p.lab[y]) return false;
    for (int s = 0; s < t; ++s)
      if (q.has(order[s], order[t]) != p.has(img[s], y)) return false;
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

// orbit of x (as a bitmask) under the (label-preserving) automorphisms that fix every node of fixed[0..m-1]
uint32_t orbit_of(const Query& q, const int* fixed, int m, int x) {
  int src[GTM_KMAX + 1], dst[GTM_KMAX + 1];
  for (int t = 0; t < m; ++t) src[t] = dst[t] = fixed[t];
  uint32_t orb = 1u << x;
  src[m] = x;
  for (int y = 0; y < q.k; ++y) {
    if (y == x || q.deg(y) != q.deg(x) || q.lab[y] != q.lab[x]) continue;
    bool is_fixed = false;
    for (int t = 0; t < m; ++t) is_fixed |= fixed[t] == y;
    if (is_fixed) continue;
    dst[m] = y;
    AutoSearch s(q, q, src, dst, m + 1);
    if (s.go(0)) orb |= 1u << y;
  }
  return orb;
}

// Appends the records of query `qi` to `plan` (one per orbit of Aut(q)), `rec_size` entries each: GTM_REC, or
// GTML_REC with the label of every position.
void plan_query(const Query& q, int qi, std::vector<int32_t>& plan, int rec_size = GTM_REC) {
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
    plan.resize(r + rec_size, 0);
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
      if (rec_size == GTML_REC) rec[GTML_LABEL + i] = q.lab[x];
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

const char* kLabelLimit = ": label ids must be non-negative";

// Invariant of a labelled query under isomorphism: equal for isomorphic queries (the filter in front of AutoSearch).
uint64_t mix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
uint64_t invariant(const Query& q) {
  uint64_t own[GTM_KMAX], sum = mix64((uint64_t)q.k);
  for (int a = 0; a < q.k; ++a) own[a] = mix64(((uint64_t)(uint32_t)q.lab[a] << 8) | (uint64_t)q.deg(a));
  for (int a = 0; a < q.k; ++a) {
    uint64_t around = 0;
    for (int b = 0; b < q.k; ++b)
      if (q.has(a, b)) around += own[b];
    sum += mix64(own[a] ^ mix64(around));                        // (sums: independent of the node numbering)
  }
  return sum;
}

bool isomorphic(const Query& a, const Query& b) {
  if (a.k != b.k) return false;
  AutoSearch s(a, b, nullptr, nullptr, 0);
  return s.go(0);
}

// The labelled plan (groundtruth_match.hpp) of the queries, class_of_query and the number of classes.
int build_plan_labelled(const char* who, const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                        const int32_t* q_labels, int num_queries, std::vector<int32_t>& plan,
                        std::vector<int32_t>& class_of_query) {
  if (!q_nodes || !q_edge_ptr || num_queries < 0 || (num_queries > 0 && !q_labels))
    return fail(DESCO_EINVAL, (std::string(who) + ": bad argument").c_str());
  std::vector<Query> reps;                                       // the first query of every class
  std::vector<uint64_t> rep_inv;
  class_of_query.assign((size_t)num_queries, 0);
  int64_t off = 0;
  for (int q = 0; q < num_queries; ++q) {
    Query qq;
    if (const char* why = read_query(q_nodes, q_edge_ptr, q_edges, q, qq))
      return fail(DESCO_EINVAL, (std::string(who) + why).c_str());
    for (int a = 0; a < qq.k; ++a) {
      qq.lab[a] = q_labels[off + a];
      if (qq.lab[a] < 0) return fail(DESCO_EINVAL, (std::string(who) + kLabelLimit).c_str());
    }
    off += qq.k;
    const uint64_t inv = invariant(qq);
    int c = -1;
    for (size_t r = 0; r < reps.size() && c < 0; ++r)
      if (rep_inv[r] == inv && isomorphic(qq, reps[r])) c = (int)r;
    if (c < 0) {
      c = (int)reps.size();
      reps.push_back(qq);
      rep_inv.push_back(inv);
    }
    class_of_query[q] = c;
  }
  std::vector<int32_t> recs;
  for (size_t c = 0; c < reps.size(); ++c) plan_query(reps[c], (int)c, recs, GTML_REC);
  const int num_recs = (int)(recs.size() / GTML_REC);
  std::vector<int> order((size_t)num_recs);
  for (int a = 0; a < num_recs; ++a) order[a] = a;
  auto key = [&](int a) {
    const int32_t* rec = recs.data() + (size_t)a * GTML_REC;
    return ((int64_t)rec[GTML_LABEL] << 32) | (int64_t)rec[GTML_LABEL + 1];
  };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key(a) < key(b); });
  plan.assign(GTML_HEAD, 0);
  std::vector<int32_t> buckets;
  int largest = 0;
  for (int i = 0; i < num_recs; ++i) {
    const int32_t* rec = recs.data() + (size_t)order[i] * GTML_REC;
    plan.insert(plan.end(), rec, rec + GTML_REC);
    if (i == 0 || key(order[i]) != key(order[i - 1])) {
      const int32_t b[GTML_BUCKET] = {rec[GTML_LABEL], rec[GTML_LABEL + 1], i, i};
      buckets.insert(buckets.end(), b, b + GTML_BUCKET);
    }
    int32_t* b = buckets.data() + buckets.size() - GTML_BUCKET;
    b[3] = i + 1;
    largest = std::max(largest, b[3] - b[2]);
  }
  plan.insert(plan.end(), buckets.begin(), buckets.end());
  plan[0] = (int32_t)reps.size();
  plan[1] = num_recs;
  plan[2] = (int32_t)(buckets.size() / GTML_BUCKET);
  plan[3] = largest;
  return 0;
}

// One graph's matcher state.  LAB: the labelled matcher, which tests a candidate's label before its adjacency bits.
// IND: induced matching (a clear GTM_ADJ bit means NOT adjacent); else a clear bit asks nothing.
// LIST (desco_list_occurrences): the first `room` maps found are also stored, in query-node order and with global
// ids, as rows dst[found * k ...]; the caller compares `found` with `room` afterwards.
template <bool LAB, bool IND, bool LIST = false>
struct Matcher {
  GraphBits g;
  const int64_t* rowptr;
  const int32_t* col;
  int v;
  const int32_t* rec;
  const int32_t* lab;                  // LAB: this graph's node labels
  int k;
  int img[GTM_KMAX];
  int64_t found;
  int32_t* dst = nullptr;              // LIST
  int64_t room = 0;

  void emit(int last) {
    if (found >= room) return;
    int32_t* row = dst + found * k;
    for (int i = 0; i + 1 < k; ++i) row[rec[GTM_NODE + i]] = (int32_t)(g.base + img[i]);
    row[rec[GTM_NODE + k - 1]] = (int32_t)(g.base + last);
  }

  bool fits(int level, int u) const {
    if (LAB && lab[u] != rec[GTML_LABEL + level]) return false;
    const uint32_t want = (uint32_t)rec[GTM_ADJ + level], lt = (uint32_t)rec[GTM_LT + level],
                   gt = (uint32_t)rec[GTM_GT + level];
    for (int j = 0; j < level; ++j) {
      const int w = img[j];
      if (u == w) return false;
      if (IND ? g.adj(u, w) != (want >> j & 1) : (want >> j & 1) && !g.adj(u, w)) return false;
      if ((lt >> j & 1) && !(u < w)) return false;
      if ((gt >> j & 1) && !(u > w)) return false;
    }
    return true;
  }

  void extend(int level) {
    const int64_t p = g.base + img[rec[GTM_PARENT + level]];
    for (int64_t e = rowptr[p]; e < rowptr[p + 1]; ++e) {
      const int u = (int)(col[e] - g.base);
      if (u >= v) break;                       // rows ascend: every image but the anchor's is below the root
      if (!fits(level, u)) continue;
      if (level + 1 == k) {
        if (LIST) emit(u);
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

extern "C" int64_t desco_canonical_match_plan_labelled_size(const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                                            const int32_t* q_edges, const int32_t* q_labels,
                                                            int num_queries) {
  try {
    std::vector<int32_t> plan, coq;
    if (build_plan_labelled("desco_canonical_match_plan_labelled_size", q_nodes, q_edge_ptr, q_edges, q_labels,
                            num_queries, plan, coq))
      return -1;
    return (int64_t)plan.size();
  } catch (const std::bad_alloc&) {
    fail(DESCO_ENOMEM, "desco_canonical_match_plan_labelled_size: out of memory");
    return -1;
  }
}

extern "C" int desco_canonical_match_plan_labelled(const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                                   const int32_t* q_edges, const int32_t* q_labels, int num_queries,
                                                   int32_t* plan, int64_t plan_entries, int32_t* class_of_query,
                                                   int* num_classes) {
  try {
    std::vector<int32_t> p, coq;
    if (const int rc = build_plan_labelled("desco_canonical_match_plan_labelled", q_nodes, q_edge_ptr, q_edges,
                                           q_labels, num_queries, p, coq))
      return rc;
    if (!num_classes || (num_queries > 0 && !class_of_query))
      return fail(DESCO_EINVAL, "desco_canonical_match_plan_labelled: bad argument");
    if (!plan || plan_entries != (int64_t)p.size())
      return fail(DESCO_EINVAL,
                  "desco_canonical_match_plan_labelled: plan_entries is not desco_canonical_match_plan_labelled_size");
    std::memcpy(plan, p.data(), p.size() * sizeof(int32_t));
    if (num_queries > 0) std::memcpy(class_of_query, coq.data(), coq.size() * sizeof(int32_t));
    *num_classes = p[0];
    return 0;
  } catch (const std::bad_alloc&) {
    return fail(DESCO_ENOMEM, "desco_canonical_match_plan_labelled: out of memory");
  }
}

// The same for a labelled plan: head, record fields, labels, the sort by (label 0, label 1) and the bucket table, which
// must be exactly the runs of equal (label 0, label 1) in the records.
int desco::match_plan_labelled_check(const char* who, const int32_t* plan, int64_t plan_entries, int num_classes) {
  const std::string w(who);
  if (!plan || plan_entries < GTML_HEAD || plan[0] != num_classes || plan[1] < 0 || plan[2] < 0 || plan[2] > plan[1] ||
      plan_entries != GTML_HEAD + (int64_t)plan[1] * GTML_REC + (int64_t)plan[2] * GTML_BUCKET)
    return fail(DESCO_EINVAL, (w + ": not a plan of desco_canonical_match_plan_labelled for these queries").c_str());
  const int32_t* buckets = plan + GTML_HEAD + (int64_t)plan[1] * GTML_REC;
  int b = -1, largest = 0;
  for (int a = 0; a < plan[1]; ++a) {
    const int32_t* rec = plan + GTML_HEAD + (int64_t)a * GTML_REC;
    const int k = rec[GTM_K];
    bool ok = rec[GTM_QUERY] >= 0 && rec[GTM_QUERY] < num_classes && k >= 2 && k <= GTM_KMAX && rec[GTM_DIVISOR] == 1;
    for (int i = 0; ok && i < k; ++i) ok = rec[GTML_LABEL + i] >= 0;
    for (int i = 1; ok && i < k; ++i) {
      const uint32_t below = (1u << i) - 1u;
      const int p = rec[GTM_PARENT + i];
      ok = p >= 0 && p < i && ((uint32_t)rec[GTM_ADJ + i] >> p & 1) && !((uint32_t)rec[GTM_ADJ + i] & ~below) &&
           !((uint32_t)rec[GTM_LT + i] & ~below) && !((uint32_t)rec[GTM_GT + i] & ~below);
    }
    if (ok) {                                                    // the bucket this record belongs to
      const int32_t l0 = rec[GTML_LABEL], l1 = rec[GTML_LABEL + 1];
      if (b < 0 || buckets[b * GTML_BUCKET] != l0 || buckets[b * GTML_BUCKET + 1] != l1) {
        ++b;
        const int32_t* nb = buckets + (int64_t)b * GTML_BUCKET;
        ok = b < plan[2] && nb[0] == l0 && nb[1] == l1 && nb[2] == a && nb[3] > a && nb[3] <= plan[1] &&
             (b == 0 || nb[-GTML_BUCKET] < l0 || (nb[-GTML_BUCKET] == l0 && nb[-GTML_BUCKET + 1] < l1)) &&
             (b == 0 || nb[-GTML_BUCKET + 3] == a);
        if (ok) largest = std::max(largest, nb[3] - nb[2]);
      } else {
        ok = a < buckets[b * GTML_BUCKET + 3];
      }
    }
    if (!ok) return fail(DESCO_EINVAL, (w + ": malformed plan record").c_str());
  }
  if (b + 1 != plan[2] || largest != plan[3] || (b >= 0 && buckets[b * GTML_BUCKET + 3] != plan[1]))
    return fail(DESCO_EINVAL, (w + ": malformed plan buckets").c_str());
  return 0;
}

namespace {

template <bool IND>
int counts_match(const std::string& who, const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                 const int32_t* col, const int32_t* plan, int64_t plan_entries, int num_queries, int num_threads,
                 int64_t* out) {
  if (!graph_ptr || !rowptr || !out || num_graphs < 0 || num_queries < 0)
    return fail(DESCO_EINVAL, (who + ": bad argument").c_str());
  if (const int rc = match_plan_check(who.c_str(), plan, plan_entries, num_queries)) return rc;
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
    for (int64_t gi = 0; gi < num_graphs; ++gi) {
      Matcher<false, IND> m;
      try {
        m.g.build(graph_ptr, gi, rowptr, col);
      } catch (const std::bad_alloc&) {
#pragma omp atomic write
        oom = true;
        continue;
      }
      const int64_t base = m.g.base, n = m.g.n;
      m.rowptr = rowptr;
      m.col = col;
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
    if (oom) return fail(DESCO_ENOMEM, (who + ": out of memory").c_str());
    return 0;
  } catch (const std::bad_alloc&) {
    return fail(DESCO_ENOMEM, (who + ": out of memory").c_str());
  }
}

template <bool IND>
int counts_match_labelled(const std::string& who, const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                          const int32_t* col, const int32_t* labels, const int32_t* plan, int64_t plan_entries,
                          int num_classes, int num_threads, int64_t* out) {
  if (!graph_ptr || !rowptr || !out || num_graphs < 0 || num_classes < 0 || (graph_ptr[num_graphs] > 0 && !labels))
    return fail(DESCO_EINVAL, (who + ": bad argument").c_str());
  if (const int rc = match_plan_labelled_check(who.c_str(), plan, plan_entries, num_classes)) return rc;
  try {
    const int64_t total = graph_ptr[num_graphs];
    std::memset(out, 0, sizeof(int64_t) * (size_t)total * (size_t)num_classes);
    const int num_recs = plan[1];
    if (num_classes == 0 || num_recs == 0) return 0;
#ifdef _OPENMP
    const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
    const int nt = 1;
    (void)num_threads;
#endif
    bool oom = false;
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
    for (int64_t gi = 0; gi < num_graphs; ++gi) {
      Matcher<true, IND> m;
      try {
        m.g.build(graph_ptr, gi, rowptr, col);
      } catch (const std::bad_alloc&) {
#pragma omp atomic write
        oom = true;
        continue;
      }
      const int64_t base = m.g.base, n = m.g.n;
      m.rowptr = rowptr;
      m.col = col;
      m.lab = labels + base;
      for (int v = 1; v < (int)n; ++v) {
        if (rowptr[base + v] == rowptr[base + v + 1]) continue;
        m.v = v;
        m.img[0] = v;
        for (int a = 0; a < num_recs; ++a) {
          m.rec = plan + GTML_HEAD + (int64_t)a * GTML_REC;
          if (m.rec[GTML_LABEL] != m.lab[v]) continue;           // the root's label retires the record at once
          m.k = m.rec[GTM_K];
          m.found = 0;
          m.extend(1);
          out[(base + v) * num_classes + m.rec[GTM_QUERY]] += m.found;
        }
      }
    }
    if (oom) return fail(DESCO_ENOMEM, (who + ": out of memory").c_str());
    return 0;
  } catch (const std::bad_alloc&) {
    return fail(DESCO_ENOMEM, (who + ": out of memory").c_str());
  }
}

}  // namespace

extern "C" int desco_canonical_counts_match(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                            const int32_t* col, const int32_t* plan, int64_t plan_entries,
                                            int num_queries, int num_threads, int64_t* out) {
  return counts_match<true>("desco_canonical_counts_match", graph_ptr, num_graphs, rowptr, col, plan, plan_entries,
                            num_queries, num_threads, out);
}

extern "C" int desco_canonical_counts_match_mode(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                                 const int32_t* col, const int32_t* plan, int64_t plan_entries,
                                                 int num_queries, int induced, int num_threads, int64_t* out) {
  const char* who = "desco_canonical_counts_match_mode";
  if (induced != 0 && induced != 1) return fail(DESCO_EINVAL, "desco_canonical_counts_match_mode: induced must be 0 or 1");
  return induced ? counts_match<true>(who, graph_ptr, num_graphs, rowptr, col, plan, plan_entries, num_queries,
                                      num_threads, out)
                 : counts_match<false>(who, graph_ptr, num_graphs, rowptr, col, plan, plan_entries, num_queries,
                                       num_threads, out);
}

extern "C" int desco_canonical_counts_match_labelled(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                                     const int32_t* col, const int32_t* labels, const int32_t* plan,
                                                     int64_t plan_entries, int num_classes, int num_threads,
                                                     int64_t* out) {
  return counts_match_labelled<true>("desco_canonical_counts_match_labelled", graph_ptr, num_graphs, rowptr, col,
                                     labels, plan, plan_entries, num_classes, num_threads, out);
}

extern "C" int desco_canonical_counts_match_labelled_mode(const int64_t* graph_ptr, int64_t num_graphs,
                                                          const int64_t* rowptr, const int32_t* col,
                                                          const int32_t* labels, const int32_t* plan,
                                                          int64_t plan_entries, int num_classes, int induced,
                                                          int num_threads, int64_t* out) {
  const char* who = "desco_canonical_counts_match_labelled_mode";
  if (induced != 0 && induced != 1)
    return fail(DESCO_EINVAL, "desco_canonical_counts_match_labelled_mode: induced must be 0 or 1");
  return induced ? counts_match_labelled<true>(who, graph_ptr, num_graphs, rowptr, col, labels, plan, plan_entries,
                                               num_classes, num_threads, out)
                 : counts_match_labelled<false>(who, graph_ptr, num_graphs, rowptr, col, labels, plan, plan_entries,
                                                num_classes, num_threads, out);
}

// ---- OCCURRENCE LISTING (include/desco_hip.h): the matcher's maps written out instead of counted ----------------------

int desco::list_plan_check(const char* who, const int32_t* plan, int64_t plan_entries) {
  const std::string w(who);
  if (!plan || plan_entries < GTM_HEAD || plan[0] != 1)
    return fail(DESCO_EINVAL, (w + ": one query per call (plan[0] must be 1)").c_str());
  if (const int rc = match_plan_check(who, plan, plan_entries, 1)) return rc;
  for (int a = 0; a < plan[1]; ++a) {
    const int32_t* rec = plan + GTM_HEAD + (int64_t)a * GTM_REC;
    const int k = rec[GTM_K];
    uint32_t seen = 0;
    for (int i = 0; i < k; ++i)
      if (rec[GTM_NODE + i] >= 0 && rec[GTM_NODE + i] < k) seen |= 1u << rec[GTM_NODE + i];
    if (seen != (1u << k) - 1u || rec[GTM_NODE] != rec[GTM_ANCHOR] || k != plan[GTM_HEAD + GTM_K])
      return fail(DESCO_EINVAL, (w + ": malformed plan record (positions must permute the query's nodes)").c_str());
  }
  return 0;
}

namespace {

template <bool IND>
int list_occurrences(const std::string& who, const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                     const int32_t* col, const int32_t* plan, int num_threads, int64_t node_begin, int64_t node_end,
                     const int64_t* ptr, int32_t* rows) {
  const int num_anchors = plan[1];
  const int k = num_anchors ? plan[GTM_HEAD + GTM_K] : 0;
  // the graphs that hold a node of [node_begin, node_end)
  const int64_t g0 = std::upper_bound(graph_ptr, graph_ptr + num_graphs + 1, node_begin) - graph_ptr - 1;
  const int64_t g1 = std::lower_bound(graph_ptr, graph_ptr + num_graphs + 1, node_end) - graph_ptr;
#ifdef _OPENMP
  const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
  const int nt = 1;
  (void)num_threads;
#endif
  bool oom = false;
  int64_t bad = -1;                                // a node whose segment is not the number of its maps
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
  for (int64_t gi = g0; gi < g1; ++gi) {
    Matcher<false, IND, true> m;
    std::vector<int64_t> order;
    std::vector<int32_t> tmp;
    try {
      m.g.build(graph_ptr, gi, rowptr, col);
      const int64_t base = m.g.base, n = m.g.n;
      m.rowptr = rowptr;
      m.col = col;
      const int64_t v0 = std::max<int64_t>(node_begin - base, 0), v1 = std::min<int64_t>(node_end - base, n);
      for (int v = (int)v0; v < (int)v1; ++v) {
        const int64_t seg = ptr[base + v + 1] - ptr[base + v];
        m.v = v;
        m.img[0] = v;
        m.found = 0;
        m.room = seg;
        m.dst = rows + (ptr[base + v] - ptr[node_begin]) * k;
        if (v > 0 && rowptr[base + v] != rowptr[base + v + 1])
          for (int a = 0; a < num_anchors; ++a) {
            m.rec = plan + GTM_HEAD + (int64_t)a * GTM_REC;
            m.k = k;
            m.extend(1);
          }
        if (m.found != seg) {
#pragma omp critical(desco_list_occurrences_bad)
          if (bad < 0 || base + v < bad) bad = base + v;
          continue;
        }
        if (seg < 2) continue;
        // the segment in ascending lexicographic order of its rows
        order.resize((size_t)seg);
        for (int64_t r = 0; r < seg; ++r) order[(size_t)r] = r;
        const int32_t* d = m.dst;
        std::sort(order.begin(), order.end(), [d, k](int64_t x, int64_t y) {
          return std::lexicographical_compare(d + x * k, d + x * k + k, d + y * k, d + y * k + k);
        });
        tmp.assign(d, d + seg * k);
        for (int64_t r = 0; r < seg; ++r)
          std::memcpy(m.dst + r * k, tmp.data() + order[(size_t)r] * k, sizeof(int32_t) * (size_t)k);
      }
    } catch (const std::bad_alloc&) {
#pragma omp atomic write
      oom = true;
    }
  }
  if (oom) return fail(DESCO_ENOMEM, (who + ": out of memory").c_str());
  if (bad >= 0)
    return fail(DESCO_EINVAL, (who + ": ptr is not the scan of this query's canonical counts (first at node " +
                               std::to_string(bad) + ")").c_str());
  return 0;
}

}  // namespace

extern "C" int desco_list_occurrences(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                      const int32_t* col, const int32_t* plan, int64_t plan_entries, int induced,
                                      int num_threads, int64_t node_begin, int64_t node_end, const int64_t* ptr,
                                      int64_t rows_capacity, int32_t* rows) {
  const std::string who = "desco_list_occurrences";
  if (num_graphs < 0 || rows_capacity < 0) return fail(DESCO_EINVAL, (who + ": negative size").c_str());
  if (!graph_ptr || !rowptr || !ptr || (rows_capacity > 0 && !rows))
    return fail(DESCO_EINVAL, (who + ": null pointer").c_str());
  if (induced != 0 && induced != 1) return fail(DESCO_EINVAL, (who + ": induced must be 0 or 1").c_str());
  if (const int rc = list_plan_check(who.c_str(), plan, plan_entries)) return rc;
  const int64_t total = graph_ptr[num_graphs];
  if (node_begin < 0 || node_end < node_begin || node_end > total)
    return fail(DESCO_EINVAL, (who + ": node range outside [0, num_nodes]").c_str());
  if (rowptr[total] > 0 && !col) return fail(DESCO_EINVAL, (who + ": null pointer").c_str());
  for (int64_t v = node_begin; v < node_end; ++v)                // every segment lies inside rows: no store outside it
    if (ptr[v + 1] < ptr[v]) return fail(DESCO_EINVAL, (who + ": ptr must not descend").c_str());
  if (ptr[node_end] - ptr[node_begin] > rows_capacity)
    return fail(DESCO_EINVAL, (who + ": rows_capacity is below ptr[node_end] - ptr[node_begin]").c_str());
  try {
    return induced ? list_occurrences<true>(who, graph_ptr, num_graphs, rowptr, col, plan, num_threads, node_begin,
                                            node_end, ptr, rows)
                   : list_occurrences<false>(who, graph_ptr, num_graphs, rowptr, col, plan, num_threads, node_begin,
                                             node_end, ptr, rows);
  } catch (const std::bad_alloc&) {
    return fail(DESCO_ENOMEM, (who + ": out of memory").c_str());
  }
}
