// Stand-alone check of the host k-core / k-truss routine (desco_amd/csrc/core_truss.cpp) on the named families of the
// tests and a seeded random set, against a naive peel inside this program; meant to be built with the host sanitizers
// -- it links no HIP and loads nothing into Python:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/decomposition_selftest.cpp desco_amd/csrc/core_truss.cpp -o decomposition_selftest
//   ./decomposition_selftest             (exit code 0 and "ok" when every expectation holds)
//
// Expectations: core, support and truss numbers equal to the naive peel; 1 thread equal to 8 threads; each output alone
// (the others NULL) equal to the full call; bad input refused by name with nothing written.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
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
  std::vector<std::pair<int, Edges>> lists;
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
    lists.emplace_back(n, edges);
  }
  int64_t graphs() const { return (int64_t)graph_ptr.size() - 1; }
  int64_t nodes() const { return graph_ptr.back(); }
  int64_t edges() const { return (int64_t)col.size() / 2; }
};

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++failures;
  }
}

// the naive peels: remove what is at or below the level, one at a time, recounting from the sets
void naive(int n, const Edges& edges, std::vector<int32_t>& core, std::vector<int32_t>& truss,
           std::vector<int32_t>& support) {
  std::vector<std::set<int>> adj(n);
  for (auto [a, b] : edges) adj[a].insert(b), adj[b].insert(a);
  {
    auto live = adj;
    std::vector<int> out(n, -1);
    int left = n, k = 0;
    while (left) {
      bool any = false;
      for (int v = 0; v < n; ++v)
        if (out[v] < 0 && (int)live[v].size() <= k) {
          out[v] = k, --left, any = true;
          for (int u : live[v]) live[u].erase(v);
          live[v].clear();
        }
      if (!any) ++k;
    }
    core.insert(core.end(), out.begin(), out.end());
  }
  auto common = [&](const std::vector<std::set<int>>& g, int a, int b) {
    int c = 0;
    for (int w : g[a]) c += (int)g[b].count(w);
    return c;
  };
  std::map<std::pair<int, int>, int> number;             // keyed (v, u), u < v: the order of the rows
  for (auto [a, b] : edges) number[{std::max(a, b), std::min(a, b)}] = 0;
  for (auto& [key, value] : number) support.push_back(common(adj, key.first, key.second));
  auto live = adj;
  size_t left = number.size();
  int k = 2;
  while (left) {
    bool any = false;
    for (auto& [key, value] : number)
      if (value == 0 && common(live, key.first, key.second) <= k - 2) {
        value = k, --left, any = true;
        live[key.first].erase(key.second), live[key.second].erase(key.first);
      }
    if (!any) ++k;
  }
  for (auto& [key, value] : number) truss.push_back(value);
}

struct Out {
  std::vector<int32_t> core, truss, support;
  int rc;
};

Out run(const Set& s, int threads, bool c = true, bool t = true, bool u = true) {
  Out o;
  o.core.assign((size_t)s.nodes(), -7), o.truss.assign((size_t)s.edges(), -7), o.support.assign((size_t)s.edges(), -7);
  o.rc = desco_core_truss(s.graph_ptr.data(), s.rowptr.data(), s.col.data(), s.graphs(), threads,
                          c ? o.core.data() : nullptr, t ? o.truss.data() : nullptr, u ? o.support.data() : nullptr);
  return o;
}

Edges clique(int k, int base = 0) {
  Edges e;
  for (int a = 0; a < k; ++a)
    for (int b = a + 1; b < k; ++b) e.push_back({base + a, base + b});
  return e;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uniform() {                                       // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}
Edges gnp(int n, double p) {
  Edges e;
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b)
      if (uniform() < p) e.push_back({a, b});
  return e;
}

void check(const Set& s, const char* what) {
  std::vector<int32_t> core, truss, support;
  for (auto& [n, edges] : s.lists) naive(n, edges, core, truss, support);
  const Out a = run(s, 1), b = run(s, 8);
  expect(a.rc == 0 && b.rc == 0, what);
  expect(a.core == core && a.truss == truss && a.support == support, what);
  expect(b.core == a.core && b.truss == a.truss && b.support == a.support, "1 thread equals 8 threads");
  const Out c = run(s, 2, true, false, false), t = run(s, 2, false, true, false), u = run(s, 2, false, false, true);
  const std::vector<int32_t> nodes_untouched((size_t)s.nodes(), -7), edges_untouched((size_t)s.edges(), -7);
  expect(c.core == core && c.truss == edges_untouched && c.support == edges_untouched, "core alone");
  expect(t.truss == truss && t.core == nodes_untouched && t.support == edges_untouched, "truss alone");
  expect(u.support == support && u.core == nodes_untouched && u.truss == edges_untouched, "support alone");
}

}  // namespace

int main() {
  Set fam;
  for (int k = 2; k <= 6; ++k) fam.add(k, clique(k));
  {
    Edges e = clique(5);
    e.erase(e.begin());
    fam.add(5, e);                                       // K5 minus an edge
  }
  {
    Edges path, cycle;
    for (int i = 0; i < 6; ++i) path.push_back({i, i + 1});
    for (int i = 0; i < 7; ++i) cycle.push_back({i, (i + 1) % 7});
    fam.add(7, path), fam.add(7, cycle);
  }
  fam.add(5, {}), fam.add(1, {});
  {
    Edges e = clique(3, 1);
    e.push_back({5, 6}), e.push_back({6, 7});
    fam.add(9, e);                                       // isolated nodes between components
  }
  fam.add(6, {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}, {0, 4}, {0, 5}, {1, 4}, {1, 5}, {4, 5}});   // two K4 on an edge
  {
    Edges e = clique(5);                                 // two K5 sharing the triangle 0 1 2
    for (int a : {0, 1, 2, 5}) e.push_back({a, 6});
    for (int a : {0, 1, 2}) e.push_back({a, 5});
    fam.add(7, e);
  }
  {
    Edges e;
    for (int a = 0; a < 3; ++a)
      for (int b = 3; b < 6; ++b) e.push_back({a, b});
    e.push_back({0, 1});
    fam.add(6, e);                                       // K3,3 plus an edge
  }
  {
    Edges strip, wheel, windmill, star;
    for (int i = 0; i < 41; ++i) strip.push_back({i, i + 1});
    for (int i = 0; i < 40; ++i) strip.push_back({i, i + 2});
    for (int v = 1; v < 8; ++v) wheel.push_back({0, v}), wheel.push_back({v, v % 7 + 1});
    for (int t = 0; t < 150; ++t)
      windmill.push_back({0, 2 * t + 1}), windmill.push_back({0, 2 * t + 2}), windmill.push_back({2 * t + 1, 2 * t + 2});
    for (int v = 1; v <= 300; ++v) star.push_back({0, v});
    fam.add(42, strip), fam.add(8, wheel), fam.add(301, windmill), fam.add(301, star);
  }
  fam.add(120, gnp(120, 0.5));
  check(fam, "the families equal the naive peel");

  Set random;
  for (int i = 0; i < 40; ++i) {
    const int n = 5 + (int)(uniform() * 36);
    random.add(n, gnp(n, 0.1 + 0.6 * uniform()));
  }
  check(random, "the random set equals the naive peel");
  check(Set(), "the empty set");

  // refusals, by name, with nothing written
  Set s;
  s.add(4, {{0, 1}, {1, 2}, {2, 3}});
  std::vector<int32_t> out(8, -7);
  auto refused = [&](int rc, const char* word) {
    expect(rc == DESCO_EINVAL && desco::last_error_ref().find("desco_core_truss") != std::string::npos &&
               desco::last_error_ref().find(word) != std::string::npos, word);
    expect(std::count(out.begin(), out.end(), -7) == 8, "a refused call writes nothing");
    desco::last_error_ref().clear();
  };
  auto call = [&](const int64_t* gp, const int64_t* rp, const int32_t* c, int64_t G) {
    return desco_core_truss(gp, rp, c, G, 2, out.data(), out.data() + 4, out.data() + 4);
  };
  refused(call(s.graph_ptr.data(), s.rowptr.data(), s.col.data(), -1), "negative");
  refused(call(nullptr, s.rowptr.data(), s.col.data(), 1), "graph_ptr is null");
  refused(call(s.graph_ptr.data(), nullptr, s.col.data(), 1), "rowptr is null");
  refused(call(s.graph_ptr.data(), s.rowptr.data(), nullptr, 1), "col is null");
  const std::vector<int64_t> bad_gp{0, 5, 4}, bad_rp{0, 2, 1, 5, 6};
  refused(call(bad_gp.data(), s.rowptr.data(), s.col.data(), 2), "graph_ptr is not monotone");
  refused(call(s.graph_ptr.data(), bad_rp.data(), s.col.data(), 1), "rowptr is not monotone");
  const std::vector<int32_t> unsorted{1, 2, 0, 1, 3, 2}, asym{1, 0, 3, 1, 3, 2}, loop{1, 0, 2, 1, 3, 3},
      outside{1, 0, 2, 1, 4, 2};
  refused(call(s.graph_ptr.data(), s.rowptr.data(), unsorted.data(), 1), "unsorted");
  refused(call(s.graph_ptr.data(), s.rowptr.data(), asym.data(), 1), "asymmetric");
  refused(call(s.graph_ptr.data(), s.rowptr.data(), loop.data(), 1), "loop");
  refused(call(s.graph_ptr.data(), s.rowptr.data(), outside.data(), 1), "outside");

  if (failures) {
    std::printf("%d expectation(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
