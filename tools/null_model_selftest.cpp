// Stand-alone check of the host null-model routine (desco_amd/csrc/null_model.cpp) on the ladder of small graphs the
// tests use, meant to be built with the host sanitizers -- it links no HIP and loads nothing into Python:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/null_model_selftest.cpp desco_amd/csrc/null_model.cpp -o null_model_selftest
//   ./null_model_selftest                (exit code 0 and "ok" when every expectation holds)
//
// Expectations: degrees kept, rows strictly ascending, symmetric and loop-free; K3 / K4 / K1,3 unchanged with nothing
// accepted; 1 thread equal to 8 threads; a slice with graph_base and a chunk with replica_base equal to the whole call;
// bad input refused by name.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../include/desco_hip.h"

// the library's error plumbing (capi.hip), restated for a program without the library
namespace desco {
std::string& last_error_ref() {
  static thread_local std::string e;
  return e;
}
int fail(int code, const char* msg) {
  last_error_ref() = msg;
  return code;
}
}  // namespace desco

namespace {

using Edges = std::vector<std::pair<int, int>>;

struct Set {
  std::vector<int64_t> graph_ptr{0}, rowptr{0};
  std::vector<int32_t> col;
  void add(int n, const Edges& edges) {
    const int64_t n0 = graph_ptr.back();
    std::vector<std::vector<int32_t>> adj(n);
    for (auto [a, b] : edges) {
      adj[a].push_back((int32_t)(n0 + b));
      adj[b].push_back((int32_t)(n0 + a));
    }
    for (auto& r : adj) {
      std::sort(r.begin(), r.end());
      col.insert(col.end(), r.begin(), r.end());
      rowptr.push_back((int64_t)col.size());
    }
    graph_ptr.push_back(n0 + n);
  }
  int64_t graphs() const { return (int64_t)graph_ptr.size() - 1; }
};

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++failures;
  }
}

struct Result {
  std::vector<int32_t> col, accepted;
  int rc;
};

Result run(const Set& s, int64_t g0, int64_t g1, int64_t graph_base, int replicas, int64_t replica_base, int64_t spe,
           uint64_t seed, int threads) {
  // graphs [g0, g1) as a set of their own (re-based), as GraphSet.subset makes it
  Set sub;
  const int64_t n0 = s.graph_ptr[g0], e0 = s.rowptr[n0];
  for (int64_t g = g0; g < g1; ++g) sub.graph_ptr.push_back(s.graph_ptr[g + 1] - n0);
  for (int64_t v = n0; v < s.graph_ptr[g1]; ++v) sub.rowptr.push_back(s.rowptr[v + 1] - e0);
  for (int64_t e = e0; e < s.rowptr[s.graph_ptr[g1]]; ++e) sub.col.push_back((int32_t)(s.col[e] - n0));
  Result r;
  r.col.assign((size_t)replicas * sub.col.size(), -7);
  r.accepted.assign((size_t)replicas * (g1 - g0), -7);
  r.rc = desco_null_model_rewire(sub.graph_ptr.data(), sub.rowptr.data(), sub.col.data(), g1 - g0, graph_base, replicas,
                                 replica_base, spe, seed, threads, r.col.data(), r.accepted.data());
  for (auto& c : r.col) c += (int32_t)n0;
  return r;
}

void check_invariants(const Set& s, const Result& r, int replicas) {
  const int64_t N = s.graph_ptr.back(), E = (int64_t)s.col.size();
  for (int k = 0; k < replicas; ++k) {
    const int32_t* c = r.col.data() + (int64_t)k * E;
    bool sorted = true, inside = true, symmetric = true;
    int64_t g = 0;
    for (int64_t v = 0; v < N; ++v) {
      while (s.graph_ptr[g + 1] <= v) ++g;
      for (int64_t e = s.rowptr[v]; e < s.rowptr[v + 1]; ++e) {
        inside = inside && c[e] >= s.graph_ptr[g] && c[e] < s.graph_ptr[g + 1] && c[e] != v;
        sorted = sorted && (e == s.rowptr[v] || c[e - 1] < c[e]);
      }
    }
    expect(inside, "entries inside the graph, loop-free");
    expect(sorted, "rows strictly ascending");
    if (inside)
      for (int64_t v = 0; v < N; ++v)
        for (int64_t e = s.rowptr[v]; e < s.rowptr[v + 1]; ++e)
          symmetric = symmetric && std::binary_search(c + s.rowptr[c[e]], c + s.rowptr[c[e] + 1], (int32_t)v);
    expect(symmetric, "symmetric");
  }
  for (int32_t a : r.accepted) expect(a >= 0, "accepted is not negative");
}

}  // namespace

int main() {
  Set s;
  s.add(3, {});                                                        // m = 0, 1, 2, 3
  s.add(2, {{0, 1}});
  s.add(4, {{0, 1}, {2, 3}});
  s.add(5, {{0, 1}, {1, 2}, {3, 4}});
  const int64_t fixed0 = s.graphs();
  s.add(3, {{0, 1}, {1, 2}, {0, 2}});                                  // K3, K4, K1,3: nothing can be accepted
  s.add(4, {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}});
  s.add(4, {{0, 1}, {0, 2}, {0, 3}});
  const int64_t fixed1 = s.graphs();
  s.add(4, {{0, 1}, {1, 2}, {2, 3}});                                  // P4, C6, two triangles sharing a node
  s.add(6, {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 0}});
  s.add(5, {{0, 1}, {1, 2}, {0, 2}, {2, 3}, {3, 4}, {2, 4}});
  {                                                                    // a 40-node graph of 100 edges, a hub graph
    Edges e;
    uint64_t x = 88172645463325252ull;
    std::vector<char> have(40 * 40, 0);
    while (e.size() < 100) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      const int a = (int)(x % 40), b = (int)((x >> 20) % 40);
      if (a != b && !have[a * 40 + b]) have[a * 40 + b] = have[b * 40 + a] = 1, e.push_back({a, b});
    }
    s.add(40, e);
    Edges h;
    for (int v = 1; v < 70; ++v) h.push_back({0, v});
    for (int v = 1; v < 69; ++v) h.push_back({v, v + 1});
    s.add(70, h);
  }
  const int64_t G = s.graphs(), E = (int64_t)s.col.size();
  for (int64_t spe : {0, 1, 20}) {
    const Result whole = run(s, 0, G, 0, 4, 0, spe, 42, 8);
    expect(whole.rc == 0, "the whole call succeeds");
    check_invariants(s, whole, 4);
    for (int k = 0; k < 4; ++k) {
      expect(std::equal(s.col.begin(), s.col.begin() + s.rowptr[s.graph_ptr[2]], whole.col.begin() + k * E),
             "m < 2 comes back unchanged");
      for (int64_t g = fixed0; g < fixed1; ++g) {
        expect(whole.accepted[k * G + g] == 0, "K3 / K4 / K1,3 accept nothing");
        expect(std::equal(s.col.begin() + s.rowptr[s.graph_ptr[g]], s.col.begin() + s.rowptr[s.graph_ptr[g + 1]],
                          whole.col.begin() + k * E + s.rowptr[s.graph_ptr[g]]), "K3 / K4 / K1,3 unchanged");
      }
      if (spe == 20) expect(whole.accepted[k * G + G - 1] > 0 && whole.accepted[k * G + G - 2] > 0, "chains move");
      if (spe == 0) expect(std::equal(s.col.begin(), s.col.end(), whole.col.begin() + k * E), "no attempts: unchanged");
    }
    const Result one = run(s, 0, G, 0, 4, 0, spe, 42, 1);
    expect(one.col == whole.col && one.accepted == whole.accepted, "1 thread equals 8 threads");
    const Result slice = run(s, 7, G, 7, 4, 0, spe, 42, 3);
    const int64_t e7 = s.rowptr[s.graph_ptr[7]];
    bool same = true;
    for (int k = 0; k < 4; ++k) {
      same = same && std::equal(slice.col.begin() + k * (E - e7), slice.col.begin() + (k + 1) * (E - e7),
                                whole.col.begin() + k * E + e7);
      same = same && std::equal(slice.accepted.begin() + k * (G - 7), slice.accepted.begin() + (k + 1) * (G - 7),
                                whole.accepted.begin() + k * G + 7);
    }
    expect(same, "a slice with graph_base equals the whole call");
    const Result chunk = run(s, 0, G, 0, 2, 2, spe, 42, 2);
    expect(std::equal(chunk.col.begin(), chunk.col.end(), whole.col.begin() + 2 * E) &&
               std::equal(chunk.accepted.begin(), chunk.accepted.end(), whole.accepted.begin() + 2 * G),
           "a chunk with replica_base equals the whole call");
  }
  // refusals
  std::vector<int32_t> out(s.col.size()), acc(G);
  auto refused = [&](int rc, const char* word) {
    expect(rc == DESCO_EINVAL && desco::last_error_ref().find("desco_null_model_rewire") != std::string::npos &&
               desco::last_error_ref().find(word) != std::string::npos, word);
  };
  refused(desco_null_model_rewire(s.graph_ptr.data(), s.rowptr.data(), s.col.data(), -1, 0, 1, 0, 1, 0, 1, out.data(),
                                  acc.data()), "negative");
  refused(desco_null_model_rewire(s.graph_ptr.data(), s.rowptr.data(), s.col.data(), G, 0, 1, 0, -1, 0, 1, out.data(),
                                  acc.data()), "swaps_per_edge");
  refused(desco_null_model_rewire(s.graph_ptr.data(), s.rowptr.data(), nullptr, G, 0, 1, 0, 1, 0, 1, out.data(),
                                  acc.data()), "col is null");
  std::vector<int32_t> bad = s.col;
  std::swap(bad[s.rowptr[s.graph_ptr[G - 1]]], bad[s.rowptr[s.graph_ptr[G - 1]] + 1]);
  refused(desco_null_model_rewire(s.graph_ptr.data(), s.rowptr.data(), bad.data(), G, 0, 1, 0, 1, 0, 1, out.data(),
                                  acc.data()), "unsorted");
  bad = s.col;
  bad[s.rowptr[s.graph_ptr[G - 1] + 5] + 2] = (int32_t)(s.graph_ptr[G - 1] + 7);  // row 5 of the hub: 0 4 6 -> 0 4 7
  refused(desco_null_model_rewire(s.graph_ptr.data(), s.rowptr.data(), bad.data(), G, 0, 1, 0, 1, 0, 1, out.data(),
                                  acc.data()), "asymmetric");
  refused(desco_null_model_rewire(s.graph_ptr.data(), s.rowptr.data(), s.col.data(), G, 0, 1, 0, INT64_MAX / 2, 0, 1,
                                  out.data(), acc.data()), "2^63");
  int64_t d[3];
  expect(desco_null_model_draw(1, 2, 3, 1ull << 40, 1 << 20, d) == 0 && d[0] >= 0 && d[0] < (1 << 20) && d[1] >= 0 &&
             d[1] < (1 << 20) && (d[2] == 0 || d[2] == 1), "a draw lies in its ranges");
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
