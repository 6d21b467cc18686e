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
//   desco_canonical_counts_labelled   a visitor with labels over the ESU walk of groundtruth_esu.hpp (2..6 nodes)
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

#include "groundtruth_esu.hpp"
#include "groundtruth_label.hpp"

namespace {

using desco::GTL_AMAX_DEV;
using desco::GTL_AMAX_HOST;
using desco::GTL_KMAX_DEV;
using desco::GTL_KMAX_HOST;
using desco::GraphBits;
using desco::pair_bit;
constexpr int KMAX = GTL_KMAX_HOST;
static_assert(KMAX == desco::ESU_KMAX_HOST, "the labelled enumerator walks with the shared ESU");

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
    if (const int rc = desco::query_mask(who, q_edge_ptr, q_edges, q, k, &out->mask[q])) return rc;
  }
  return 0;
}

inline bool queries_null(const int32_t* q_nodes, const int32_t* q_edge_ptr, const int32_t* q_edges,
                         const int32_t* q_labels, int num_queries) {
  if (!q_nodes || !q_edge_ptr || !q_labels) return true;
  return !q_edges && q_edge_ptr[num_queries] > q_edge_ptr[0];
}

// the ESU visitor: one per thread, with its memo of the codes it has met
struct LabelVisitor {
  const int32_t* labels;
  const bool* used;                   // [k]: a query has k nodes
  const ClassMap* classes;            // [k]: canonical code -> class
  int64_t* out;
  int64_t num_c;
  ClassMap memo[KMAX + 1];            // [k]: code as found -> class or -1

  void operator()(const GraphBits& g, const int* sub, int k, int v) {
    if (!used[k]) return;
    int lab[KMAX];
    for (int b = 0; b < k; ++b) lab[b] = labels[g.base + sub[b]];
    const uint32_t m = g.mask_of(sub, k);
    const uint64_t code = make_code(k, m, lab);
    auto it = memo[k].find(code);
    if (it == memo[k].end()) {
      auto cl = classes[k].find(canonical_code(k, m, lab));
      it = memo[k].emplace(code, cl == classes[k].end() ? -1 : cl->second).first;
    }
    if (it->second >= 0) out[(g.base + v) * num_c + it->second] += 1;
  }
};

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
    const bool ok = desco::esu_enumerate_graphs(graph_ptr, num_graphs, rowptr, col, kmax, num_threads, [&] {
      return LabelVisitor{labels, used, classes, out, num_classes, {}};
    });
    if (!ok) return desco::fail(DESCO_ENOMEM, "desco_canonical_counts_labelled: out of memory");
    return 0;
  } catch (const std::bad_alloc&) {
    return desco::fail(DESCO_ENOMEM, "desco_canonical_counts_labelled: out of memory");
  }
}
