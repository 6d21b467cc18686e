// Stand-alone check of the clique census host twins (desco_peel_order, desco_clique_census) for sanitizer builds: the
// closed-form families, and a naive subset enumerator on small random graphs.  Links clique_census.cpp directly; loads
// nothing else.
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tools/clique_census_selftest.cpp desco_amd/csrc/clique_census.cpp -o clique_census_selftest && ./clique_census_selftest
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../include/desco_hip.h"

namespace desco {                              // the error plumbing the library's capi.hip provides
std::string& last_error_ref() {
  static thread_local std::string s;
  return s;
}
int fail(int code, const char* msg) {
  last_error_ref() = msg;
  return code;
}
}  // namespace desco

namespace {

int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

struct Set {
  std::vector<int64_t> graph_ptr{0}, rowptr{0};
  std::vector<int32_t> col;
  void add(int n, const std::vector<std::pair<int, int>>& edges) {
    const int64_t n0 = graph_ptr.back();
    std::vector<std::vector<int32_t>> adj((size_t)n);
    for (const auto& e : edges) adj[e.first].push_back(e.second), adj[e.second].push_back(e.first);
    for (int v = 0; v < n; ++v) {
      std::vector<char> seen((size_t)n, 0);
      for (const int32_t u : adj[v]) seen[u] = 1;
      for (int u = 0; u < n; ++u)
        if (seen[u]) col.push_back((int32_t)(n0 + u));
      rowptr.push_back((int64_t)col.size());
    }
    graph_ptr.push_back(n0 + n);
  }
  int64_t graphs() const { return (int64_t)graph_ptr.size() - 1; }
  int64_t nodes() const { return graph_ptr.back(); }
};

uint64_t binom(int n, int k) {                 // mod 2^64, by Pascal's rule
  if (k < 0 || k > n) return 0;
  std::vector<uint64_t> row((size_t)n + 1, 0);
  row[0] = 1;
  for (int i = 1; i <= n; ++i)
    for (int j = i; j >= 1; --j) row[j] += row[j - 1];
  return row[k];
}

std::vector<std::pair<int, int>> multipartite(const std::vector<int>& parts) {
  std::vector<int> part;
  for (size_t i = 0; i < parts.size(); ++i) part.insert(part.end(), (size_t)parts[i], (int)i);
  std::vector<std::pair<int, int>> e;
  for (size_t a = 0; a < part.size(); ++a)
    for (size_t b = a + 1; b < part.size(); ++b)
      if (part[a] != part[b]) e.emplace_back((int)a, (int)b);
  return e;
}

struct Result {
  std::vector<int64_t> graph, node;
  std::vector<int32_t> omega, key, core;
};

Result run(const Set& s, int kmax, int threads, const int32_t* key = nullptr) {
  Result r;
  r.graph.assign((size_t)(s.graphs() * kmax), -7), r.node.assign((size_t)(s.nodes() * kmax), -7);
  r.omega.assign((size_t)s.graphs(), -7), r.key.assign((size_t)s.nodes(), -7), r.core.assign((size_t)s.nodes(), -7);
  CHECK(desco_peel_order(s.graph_ptr.data(), s.rowptr.data(), s.col.data(), s.graphs(), threads, r.key.data(),
                         r.core.data()) == 0);
  CHECK(desco_clique_census(s.graph_ptr.data(), s.rowptr.data(), s.col.data(), s.graphs(), key, kmax, threads,
                            r.graph.data(), r.node.data(), r.omega.data()) == 0);
  return r;
}

void families() {
  Set s;
  const int sizes[] = {1, 2, 5, 33, 65, 70};
  for (const int n : sizes) {
    std::vector<std::pair<int, int>> e;
    for (int a = 0; a < n; ++a)
      for (int b = a + 1; b < n; ++b) e.emplace_back(a, b);
    s.add(n, e);
  }
  s.add(21, multipartite(std::vector<int>(7, 3)));
  s.add(24, multipartite(std::vector<int>(12, 2)));
  s.add(0, {});
  s.add(3, {});
  const int kmax = 64;
  const Result r = run(s, kmax, 3);
  for (int g = 0; g < 6; ++g) {
    const int n = sizes[g];
    CHECK(r.omega[g] == n);
    for (int k = 1; k <= kmax; ++k) {
      CHECK((uint64_t)r.graph[(size_t)g * kmax + k - 1] == binom(n, k));
      for (int64_t v = s.graph_ptr[g]; v < s.graph_ptr[g + 1]; ++v)
        CHECK((uint64_t)r.node[(size_t)v * kmax + k - 1] == binom(n - 1, k - 1));
    }
  }
  CHECK((uint64_t)r.graph[5 * kmax + 34] == binom(70, 35));             // C(70, 35) > 2^64: the sums wrap around
  for (int k = 1; k <= kmax; ++k) {            // K_{3x7}: C(7, k) 3^k; K_{2x12}: C(12, k) 2^k
    uint64_t p3 = 1, p2 = 1;
    for (int i = 0; i < k; ++i) p3 *= 3, p2 *= 2;
    CHECK((uint64_t)r.graph[6 * kmax + k - 1] == binom(7, k) * p3);
    CHECK((uint64_t)r.graph[7 * kmax + k - 1] == binom(12, k) * p2);
  }
  CHECK(r.omega[6] == 7 && r.omega[7] == 12 && r.omega[8] == 0 && r.omega[9] == 1);
  CHECK(r.graph[8 * kmax] == 0 && r.graph[9 * kmax] == 3 && r.graph[9 * kmax + 1] == 0);
  for (int64_t v = 0; v < s.nodes(); ++v) CHECK(r.key[v] >= 0 && r.core[v] >= 0);
}

void random_graphs() {
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return state;
  };
  Set s;
  std::vector<std::vector<uint32_t>> adjs;
  for (int t = 0; t < 24; ++t) {
    const int n = 3 + (int)(next() % 14);      // up to 16 nodes: 2^16 subsets
    const uint64_t cut = (next() % 90 + 8) * (UINT64_MAX / 100);
    std::vector<std::pair<int, int>> e;
    std::vector<uint32_t> adj((size_t)n, 0);
    for (int a = 0; a < n; ++a)
      for (int b = a + 1; b < n; ++b)
        if (next() < cut) e.emplace_back(a, b), adj[a] |= 1u << b, adj[b] |= 1u << a;
    s.add(n, e);
    adjs.push_back(adj);
  }
  const int kmax = 9;
  const Result one = run(s, kmax, 1), four = run(s, kmax, 4);
  CHECK(one.graph == four.graph && one.node == four.node && one.omega == four.omega && one.key == four.key);
  std::vector<int32_t> other((size_t)s.nodes());
  for (auto& k : other) k = (int32_t)(next() % 5);
  const Result keyed = run(s, kmax, 2, other.data());
  CHECK(keyed.graph == one.graph && keyed.node == one.node && keyed.omega == one.omega);
  for (int64_t g = 0; g < s.graphs(); ++g) {
    const int n = (int)(s.graph_ptr[g + 1] - s.graph_ptr[g]);
    const std::vector<uint32_t>& adj = adjs[(size_t)g];
    std::vector<uint64_t> total((size_t)kmax, 0), node((size_t)n * kmax, 0);
    int omega = 0;
    for (uint32_t m = 1; m < (1u << n); ++m) {
      bool clique = true;
      for (int v = 0; v < n && clique; ++v)
        if (m >> v & 1) clique = ((m & ~(1u << v)) & ~adj[v]) == 0;
      if (!clique) continue;
      const int k = __builtin_popcount(m);
      omega = k > omega ? k : omega;
      if (k > kmax) continue;
      ++total[k - 1];
      for (int v = 0; v < n; ++v)
        if (m >> v & 1) ++node[(size_t)v * kmax + k - 1];
    }
    CHECK(one.omega[g] == omega);
    for (int k = 0; k < kmax; ++k) {
      CHECK((uint64_t)one.graph[(size_t)g * kmax + k] == total[k]);
      for (int v = 0; v < n; ++v)
        CHECK((uint64_t)one.node[(size_t)(s.graph_ptr[g] + v) * kmax + k] == node[(size_t)v * kmax + k]);
    }
    // the out-degree under the peel key is at most the core number
    for (int v = 0; v < n; ++v) {
      int out = 0;
      const int64_t a = s.graph_ptr[g] + v;
      for (int u = 0; u < n; ++u)
        if (adj[v] >> u & 1) {
          const int64_t b = s.graph_ptr[g] + u;
          out += one.key[b] > one.key[a] || (one.key[b] == one.key[a] && b > a);
        }
      CHECK(out <= one.core[a]);
    }
  }
}

void refusals() {
  Set s;
  s.add(4, {{0, 1}, {1, 2}, {2, 3}});
  std::vector<int64_t> g(3, -7), nd(12, -7);
  std::vector<int32_t> om(1, -7), key(4, -7);
  auto census = [&](const int32_t* col, int kmax, const int32_t* k) {
    return desco_clique_census(s.graph_ptr.data(), s.rowptr.data(), col, 1, k, kmax, 1, g.data(), nd.data(), om.data());
  };
  const int32_t loop[] = {1, 0, 2, 1, 3, 3}, outside[] = {1, 0, 2, 1, 4, 2}, unsorted[] = {1, 2, 0, 1, 3, 2};
  const int32_t negative[] = {0, 1, -1, 0};
  CHECK(census(loop, 3, nullptr) == DESCO_EINVAL && census(outside, 3, nullptr) == DESCO_EINVAL);
  CHECK(census(unsorted, 3, nullptr) == DESCO_EINVAL && census(s.col.data(), 0, nullptr) == DESCO_EINVAL);
  CHECK(census(s.col.data(), 65, nullptr) == DESCO_EINVAL && census(s.col.data(), 3, negative) == DESCO_EINVAL);
  CHECK(desco::last_error_ref().find("desco_clique_census") == 0);
  CHECK(desco_peel_order(s.graph_ptr.data(), s.rowptr.data(), loop, 1, 1, key.data(), nullptr) == DESCO_EINVAL);
  for (const int64_t x : g) CHECK(x == -7);
  for (const int64_t x : nd) CHECK(x == -7);
  CHECK(om[0] == -7 && key[0] == -7);
}

}  // namespace

int main() {
  families();
  random_graphs();
  refusals();
  std::printf(failures ? "clique_census_selftest: %d check(s) FAILED\n" : "clique_census_selftest: all checks passed\n",
              failures);
  return failures ? 1 : 0;
}
