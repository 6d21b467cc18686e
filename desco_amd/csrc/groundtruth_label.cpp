// Exact canonical ground-truth counts of LABELLED queries (--use_node_feature), host side:
//
//   count[v][c] = #{ node subsets S : max(S) = v, G[S] connected, and G[S] with its node labels
//                    isomorphic to the labelled queries of class c }
//
// -- what the reference gets from networkx VF2 with node_match on the feature (workload.py:327-348, keyed by
// max(vmap.keys())) divided by the labelled symmetry factor (data.py:61-68).  The reference's expansion
// (add_node_feat_to_networkx, utils.py:258-272) yields labelled copies that are isomorphic to each other, so queries
// are first grouped into labelled isomorphism classes and counted once per class.
//
// A labelled pattern on k nodes is the pair (adjacency mask, k label ids); its class is named by the smallest code
// over all k! relabelings.  This file holds
//   desco_canonical_label_classes     queries -> class_of_query, number of classes           (2..6 nodes)
//   desco_canonical_label_table[_size] the direct lookup table the device kernel classifies with (2..5 nodes)
//   desco_canonical_counts_labelled   the ESU enumerator of groundtruth.cpp with labels      (2..6 nodes)
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/desco_hip.h"
#include "common_host.hpp"
#include "groundtruth_label.hpp"

namespace {

using desco::GTL_AMAX_DEV;
using desco::GTL_AMAX_HOST;
using desco::GTL_KMAX_DEV;
using desco::GTL_KMAX_HOST;
constexpr int KMAX = GTL_KMAX_HOST;

inline int pair_bit(int a, int b) { return b * (b - 1) / 2 + a; }   // a < b

// 64-bit code of a labelled pattern on k nodes: the mask in bits 0..14, label j in bits 15 + 8j (codes of different
// k live in different maps)
using ClassMap = std::unordered_map<uint64_t, int32_t>;

inline uint64_t make_code(int k, uint32_t mask, const int* lab) {
  uint64_t c = mask;
  for (int j = 0; j < k; ++j) c |= (uint64_t)lab[j] << (15 + 8 * j);
  return c;
}

// every permutation of k positions, with the pair bit each pair bit moves to
struct Perms {
  std::vector<std::vector<int>> p;          // p[i][a] = new position of node a
  std::vector<std::vector<int>> bit;        // bit[i][old pair bit] = new pair bit
  explicit Perms(int k) {
    std::vector<int> perm(k);
    for (int i = 0; i < k; ++i) perm[i] = i;
    do {
      std::vector<int> b(k * (k - 1) / 2);
      for (int y = 1; y < k; ++y)
        for (int x = 0; x < y; ++x)
          b[pair_bit(x, y)] = pair_bit(std::min(perm[x], perm[y]), std::max(perm[x], perm[y]));
      p.push_back(perm);
      bit.push_back(b);
    } while (std::next_permutation(perm.begin(), perm.end()));
  }
};

const Perms& perms_of(int k) {
  static const Perms tab[KMAX + 1] = {Perms(0), Perms(1), Perms(2), Perms(3), Perms(4), Perms(5), Perms(6)};
  return tab[k];
}

inline void relabel(const Perms& P, size_t i, int k, uint32_t mask, const int* lab, uint32_t* mask2, int* lab2) {
  uint32_t r = 0;
  for (int b = 0; b < k * (k - 1) / 2; ++b)
    if (mask >> b & 1) r |= 1u << P.bit[i][b];
  for (int a = 0; a < k; ++a) lab2[P.p[i][a]] = lab[a];
  *mask2 = r;
}

uint64_t canonical_code(int k, uint32_t mask, const int* lab) {
  const Perms& P = perms_of(k);
  uint64_t best = ~(uint64_t)0;
  int lab2[KMAX];
  uint32_t m2;
  for (size_t i = 0; i < P.p.size(); ++i) {
    relabel(P, i, k, mask, lab, &m2, lab2);
    best = std::min(best, make_code(k, m2, lab2));
  }
  return best;
}

struct Queries {
  std::vector<uint32_t> mask;
  std::vector<int64_t> lab_off;       // first label of query q in q_labels
};

// validates the queries (sizes kmin..kmax_allowed, edges, label ids) and extracts their masks
int read_queries(const char* who, const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                 const int32_t* q_labels, int num_queries, int num_labels, int k_allowed, Queries* out, int* kmax) {
  auto bad = [&](const char* what) {
    return desco::fail(DESCO_EINVAL, (std::string(who) + ": " + what).c_str());
  };
  out->mask.assign((size_t)num_queries, 0);
  out->lab_off.assign((size_t)num_queries + 1, 0);
  *kmax = 0;
  for (int q = 0; q < num_queries; ++q) {
    const int k = q_nodes[q];
    if (k < 2 || k > k_allowed)
      return bad(k_allowed == KMAX ? "queries must have 2..6 nodes" : "the device path takes queries of 2..5 nodes");
    *kmax = std::max(*kmax, k);
    out->lab_off[q + 1] = out->lab_off[q] + k;
    for (int j = 0; j < k; ++j) {
      const int l = q_labels[out->lab_off[q] + j];
      if (l < 0 || l >= num_labels) return bad("query label id outside 0..num_labels-1");
    }
    if (q_edge_ptr[q + 1] < q_edge_ptr[q]) return bad("q_edge_ptr must not decrease");
    uint32_t m = 0;
    for (int e = q_edge_ptr[q]; e < q_edge_ptr[q + 1]; ++e) {
      int a = q_edges[2 * e], b = q_edges[2 * e + 1];
      if (a == b || a < 0 || b < 0 || a >= k || b >= k) return bad("bad query edge");
      if (a > b) std::swap(a, b);
      m |= 1u << pair_bit(a, b);
    }
    out->mask[q] = m;
  }
  return 0;
}

inline bool queries_null(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                         const int32_t* q_labels, int num_queries) {
  if (!q_nodes || !q_edge_ptr || !q_labels) return true;
  return !q_edges && q_edge_ptr[num_queries] > q_edge_ptr[0];
}

struct Ctx {
  int64_t base, n;
  const int64_t* rowptr;
  const int32_t* col;
  const int32_t* labels;
  int kmax;
  bool used[KMAX + 1];
  const ClassMap* classes;            // [k]: canonical code -> class
  ClassMap memo[KMAX + 1];            // [k]: code as found -> class or -1
  std::vector<uint64_t> bits;
  int words;
  std::vector<uint8_t> seen;
  int64_t* out;
  int64_t num_c;
  bool adj(int a, int b) const { return bits[(size_t)a * words + (b >> 6)] >> (b & 63) & 1; }
};

void classify(Ctx& c, const int* sub, int k, int v) {
  if (!c.used[k]) return;
  uint32_t m = 0;
  int lab[KMAX];
  for (int b = 0; b < k; ++b) {
    lab[b] = c.labels[c.base + sub[b]];
    for (int a = 0; a < b; ++a)
      if (c.adj(sub[a], sub[b])) m |= 1u << pair_bit(a, b);
  }
  const uint64_t code = make_code(k, m, lab);
  auto it = c.memo[k].find(code);
  if (it == c.memo[k].end()) {
    auto cl = c.classes[k].find(canonical_code(k, m, lab));
    it = c.memo[k].emplace(code, cl == c.classes[k].end() ? -1 : cl->second).first;
  }
  if (it->second >= 0) c.out[(c.base + v) * c.num_c + it->second] += 1;
}

// ESU, as in groundtruth.cpp
void extend(Ctx& c, int* sub, int nsub, std::vector<int>& ext, int v) {
  classify(c, sub, nsub, v);
  if (nsub == c.kmax) return;
  std::vector<int> newly, ext2;
  while (!ext.empty()) {
    const int w = ext.back();
    ext.pop_back();
    newly.clear();
    const int64_t gw = c.base + w;
    for (int64_t e = c.rowptr[gw]; e < c.rowptr[gw + 1]; ++e) {
      const int u = (int)(c.col[e] - c.base);
      if (u >= v) break;                       // rows sorted ascending; only ids below the root
      if (!c.seen[u]) {
        c.seen[u] = 1;
        newly.push_back(u);
      }
    }
    ext2 = ext;
    ext2.insert(ext2.end(), newly.begin(), newly.end());
    sub[nsub] = w;
    extend(c, sub, nsub + 1, ext2, v);
    for (int u : newly) c.seen[u] = 0;
  }
}

}  // namespace

extern "C" int desco_canonical_label_classes(const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                             const int32_t* q_edges, const int32_t* q_labels, int num_queries,
                                             int num_labels, int32_t* class_of_query, int* num_classes,
                                             int* kmax_out) {
  if (num_queries < 0 || !num_classes || !kmax_out || num_labels < 1 || num_labels > GTL_AMAX_HOST ||
      (num_queries > 0 && (!class_of_query || queries_null(q_nodes, q_edge_ptr, q_edges, q_labels, num_queries))))
    return desco::fail(DESCO_EINVAL, "desco_canonical_label_classes: bad argument (1..256 label ids)");
  try {
    Queries qs;
    int kmax = 0;
    if (const int rc = read_queries("desco_canonical_label_classes", q_nodes, q_edge_ptr, q_edges, q_labels,
                                    num_queries, num_labels, KMAX, &qs, &kmax))
      return rc;
    ClassMap classes[KMAX + 1];
    int32_t count = 0;                       // classes are numbered in the order of their first query
    for (int q = 0; q < num_queries; ++q) {
      int lab[KMAX];
      for (int j = 0; j < q_nodes[q]; ++j) lab[j] = q_labels[qs.lab_off[q] + j];
      auto r = classes[q_nodes[q]].emplace(canonical_code(q_nodes[q], qs.mask[q], lab), count);
      count += r.second;
      class_of_query[q] = r.first->second;
    }
    *num_classes = count;
    *kmax_out = kmax;
    return 0;
  } catch (const std::bad_alloc&) {
    return desco::fail(DESCO_ENOMEM, "desco_canonical_label_classes: out of memory");
  }
}

extern "C" int64_t desco_canonical_label_table_size(int kmax, int num_labels) {
  if (kmax < 2 || kmax > GTL_KMAX_DEV || num_labels < 1 || num_labels > GTL_AMAX_DEV) {
    desco::fail(DESCO_EINVAL, "desco_canonical_label_table_size: the device path takes queries of 2..5 nodes and "
                              "1..16 label ids");
    return -1;
  }
  return desco::gtl_layout(kmax, num_labels).off[kmax + 1];
}

extern "C" int desco_canonical_label_table(const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                           const int32_t* q_edges, const int32_t* q_labels, int num_queries,
                                           int num_labels, const int32_t* class_of_query, int num_classes,
                                           int kmax, int32_t* table, int64_t table_entries) {
  if (num_queries < 0 || num_classes < 0 || num_labels < 1 || num_labels > GTL_AMAX_DEV || kmax < 2 ||
      kmax > GTL_KMAX_DEV || !table ||
      (num_queries > 0 && (!class_of_query || queries_null(q_nodes, q_edge_ptr, q_edges, q_labels, num_queries))))
    return desco::fail(DESCO_EINVAL, "desco_canonical_label_table: bad argument (queries of 2..5 nodes, 1..16 "
                                     "label ids)");
  const desco::GtlLayout lay = desco::gtl_layout(kmax, num_labels);
  if (table_entries != lay.off[kmax + 1])
    return desco::fail(DESCO_EINVAL, "desco_canonical_label_table: table_entries is not "
                                     "desco_canonical_label_table_size(kmax, num_labels)");
  try {
    Queries qs;
    int kq = 0;
    if (const int rc = read_queries("desco_canonical_label_table", q_nodes, q_edge_ptr, q_edges, q_labels,
                                    num_queries, num_labels, GTL_KMAX_DEV, &qs, &kq))
      return rc;
    if (kq > kmax) return desco::fail(DESCO_EINVAL, "desco_canonical_label_table: a query has more than kmax nodes");
    for (int q = 0; q < num_queries; ++q)
      if (class_of_query[q] < 0 || class_of_query[q] >= num_classes)
        return desco::fail(DESCO_EINVAL, "desco_canonical_label_table: class_of_query outside 0..num_classes-1");
    std::fill(table, table + table_entries, (int32_t)-1);
    std::vector<uint8_t> done((size_t)num_classes, 0);
    for (int q = 0; q < num_queries; ++q) {
      const int c = class_of_query[q], k = q_nodes[q];
      if (done[c]) continue;                 // every relabeling of one member covers the class
      done[c] = 1;
      int lab[KMAX], lab2[KMAX];
      for (int j = 0; j < k; ++j) lab[j] = q_labels[qs.lab_off[q] + j];
      const Perms& P = perms_of(k);
      for (size_t i = 0; i < P.p.size(); ++i) {
        uint32_t m2;
        relabel(P, i, k, qs.mask[q], lab, &m2, lab2);
        int64_t idx = lay.off[k] + (int64_t)m2 * lay.apow[k];
        for (int j = 0; j < k; ++j) idx += lab2[j] * lay.apow[j];
        if (table[idx] >= 0 && table[idx] != c)
          return desco::fail(DESCO_EINVAL, "desco_canonical_label_table: class_of_query puts isomorphic queries "
                                           "into different classes");
        table[idx] = c;
      }
    }
    return 0;
  } catch (const std::bad_alloc&) {
    return desco::fail(DESCO_ENOMEM, "desco_canonical_label_table: out of memory");
  }
}

extern "C" int desco_canonical_counts_labelled(const int64_t* graph_ptr, int64_t num_graphs, const int64_t* rowptr,
                                               const int32_t* col, const int32_t* labels, int num_labels,
                                               const int32_t* q_nodes, const int32_t* q_edge_ptr,
                                               const int32_t* q_edges, const int32_t* q_labels, int num_queries,
                                               const int32_t* class_of_query, int num_classes, int num_threads,
                                               int64_t* out) {
  const char* who = "desco_canonical_counts_labelled";
  if (!graph_ptr || num_graphs < 0 || num_queries < 0 || num_classes < 0 || num_classes > num_queries ||
      num_labels < 1 || num_labels > GTL_AMAX_HOST)
    return desco::fail(DESCO_EINVAL, "desco_canonical_counts_labelled: bad argument (1..256 label ids)");
  const int64_t total = graph_ptr[num_graphs];
  if (total == 0 || num_queries == 0) return 0;
  if (!rowptr || !labels || !out || !class_of_query || (rowptr[total] > 0 && !col) ||
      queries_null(q_nodes, q_edge_ptr, q_edges, q_labels, num_queries))
    return desco::fail(DESCO_EINVAL, "desco_canonical_counts_labelled: null argument");
  try {
    Queries qs;
    int kmax = 0;
    if (const int rc = read_queries(who, q_nodes, q_edge_ptr, q_edges, q_labels, num_queries, num_labels, KMAX, &qs,
                                    &kmax))
      return rc;
    for (int64_t v = 0; v < total; ++v)
      if (labels[v] < 0 || labels[v] >= num_labels)
        return desco::fail(DESCO_EINVAL, "desco_canonical_counts_labelled: node label id outside 0..num_labels-1");
    ClassMap classes[KMAX + 1];
    bool used[KMAX + 1] = {false};
    for (int q = 0; q < num_queries; ++q) {
      if (class_of_query[q] < 0 || class_of_query[q] >= num_classes)
        return desco::fail(DESCO_EINVAL, "desco_canonical_counts_labelled: class_of_query outside 0..num_classes-1");
      int lab[KMAX];
      for (int j = 0; j < q_nodes[q]; ++j) lab[j] = q_labels[qs.lab_off[q] + j];
      used[q_nodes[q]] = true;
      auto r = classes[q_nodes[q]].emplace(canonical_code(q_nodes[q], qs.mask[q], lab), class_of_query[q]);
      if (r.first->second != class_of_query[q])
        return desco::fail(DESCO_EINVAL, "desco_canonical_counts_labelled: class_of_query puts isomorphic queries "
                                         "into different classes");
    }
    std::memset(out, 0, sizeof(int64_t) * (size_t)total * (size_t)num_classes);
#ifdef _OPENMP
    const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#else
    const int nt = 1;
    (void)num_threads;
#endif
    bool oom = false;
#pragma omp parallel num_threads(nt)
    {
      Ctx c;
      {
        c.rowptr = rowptr;
        c.col = col;
        c.labels = labels;
        c.kmax = kmax;
        std::copy(used, used + KMAX + 1, c.used);
        c.classes = classes;
        c.out = out;
        c.num_c = num_classes;
#pragma omp for schedule(dynamic, 1)
        for (int64_t g = 0; g < num_graphs; ++g) try {
          c.base = graph_ptr[g];
          c.n = graph_ptr[g + 1] - c.base;
          c.words = (int)((c.n + 63) / 64);
          c.bits.assign((size_t)c.n * c.words, 0);
          for (int64_t u = 0; u < c.n; ++u)
            for (int64_t e = rowptr[c.base + u]; e < rowptr[c.base + u + 1]; ++e) {
              const int w = (int)(col[e] - c.base);
              c.bits[(size_t)u * c.words + (w >> 6)] |= (uint64_t)1 << (w & 63);
            }
          c.seen.assign((size_t)c.n, 0);
          int sub[KMAX];
          std::vector<int> ext;
          for (int v = 0; v < (int)c.n; ++v) {
            ext.clear();
            c.seen[v] = 1;
            const int64_t gv = c.base + v;
            for (int64_t e = rowptr[gv]; e < rowptr[gv + 1]; ++e) {
              const int u = (int)(col[e] - c.base);
              if (u >= v) break;
              c.seen[u] = 1;
              ext.push_back(u);
            }
            std::vector<int> marked = ext;
            sub[0] = v;
            extend(c, sub, 1, ext, v);
            for (int u : marked) c.seen[u] = 0;
            c.seen[v] = 0;
          }
        } catch (const std::bad_alloc&) {
#pragma omp atomic write
          oom = true;
        }
      }
    }
    if (oom) return desco::fail(DESCO_ENOMEM, "desco_canonical_counts_labelled: out of memory");
    return 0;
  } catch (const std::bad_alloc&) {
    return desco::fail(DESCO_ENOMEM, "desco_canonical_counts_labelled: out of memory");
  }
}
