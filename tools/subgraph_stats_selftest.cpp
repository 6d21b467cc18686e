// Stand-alone check of the host statistics routine (desco_amd/csrc/subgraph_stats.cpp) on closed-form inputs, meant to
// be built with the host sanitizers -- it links no HIP and loads nothing into Python:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/subgraph_stats_selftest.cpp desco_amd/csrc/subgraph_stats.cpp -o subgraph_stats_selftest
//   ./subgraph_stats_selftest            (exit code 0 and "ok" when every expectation holds)
#include <algorithm>
#include <cstdint>
#include <cstdio>
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

struct Problem {
  std::vector<int64_t> rowptr{0}, set_ptr{0};
  std::vector<int32_t> col, set_nodes;
  int64_t nodes = 0;
  // one graph of n nodes with the given edges, and the set `members` (local ids, ascending) of it
  void add(int n, const std::vector<std::pair<int, int>>& edges, const std::vector<int>& members) {
    std::vector<std::vector<int32_t>> adj(n);
    for (auto [a, b] : edges) {
      adj[a].push_back((int32_t)(nodes + b));
      adj[b].push_back((int32_t)(nodes + a));
    }
    for (auto& r : adj) {
      std::sort(r.begin(), r.end());
      col.insert(col.end(), r.begin(), r.end());
      rowptr.push_back((int64_t)col.size());
    }
    for (int v : members) set_nodes.push_back((int32_t)(nodes + v));
    set_ptr.push_back((int64_t)set_nodes.size());
    nodes += n;
  }
};

std::vector<int> iota(int n) {
  std::vector<int> v(n);
  for (int i = 0; i < n; ++i) v[i] = i;
  return v;
}

int failures = 0;
void expect(const char* name, const int64_t* got, double gotf, std::vector<int64_t> want, double wantf) {
  bool ok = gotf == wantf;
  for (int k = 0; k < 6; ++k) ok = ok && got[k] == want[k];
  if (!ok) {
    ++failures;
    std::printf("FAIL %s: got %lld %lld %lld %lld %lld %lld %.17g\n", name, (long long)got[0], (long long)got[1],
                (long long)got[2], (long long)got[3], (long long)got[4], (long long)got[5], gotf);
  }
}

}  // namespace

int main() {
  Problem p;
  std::vector<std::pair<int, int>> e;
  for (int v = 0; v + 1 < 130; ++v) e.push_back({v, v + 1});
  p.add(130, e, iota(130));                                     // 0: path
  e.clear();
  for (int v = 0; v < 65; ++v) e.push_back({v, (v + 1) % 65});
  p.add(65, e, iota(65));                                       // 1: cycle
  e.clear();
  for (int v = 0; v < 65; ++v)
    if (v != 30) e.push_back({30, v});
  p.add(65, e, iota(65));                                       // 2: star
  e.clear();
  for (int a = 0; a < 65; ++a)
    for (int b = a + 1; b < 65; ++b) e.push_back({a, b});
  p.add(65, e, iota(65));                                       // 3: clique
  p.add(9, {{0, 2}, {2, 4}, {4, 6}, {1, 3}, {3, 5}, {1, 5}, {5, 7}}, iota(9));   // 4: two components of 4: the tie
  p.add(12, {{0, 1}, {2, 3}, {4, 5}}, {2, 4, 7, 9});            // 5: isolated members
  p.add(3, {{0, 1}}, {});                                       // 6: the empty set
  e.clear();
  for (int v = 0; v + 1 < 5000; ++v) e.push_back({v, v + 1});
  p.add(5000, e, iota(5000));                                   // 7: above the inner threshold (OpenMP over sources)

  const int64_t S = (int64_t)p.set_ptr.size() - 1;
  std::vector<int64_t> oi(6 * S, -7);
  std::vector<double> of(S, -7.0);
  for (int threads : {1, 4}) {
    int rc = desco_subgraph_stats(p.rowptr.data(), p.col.data(), p.nodes, p.set_ptr.data(), p.set_nodes.data(), S,
                                  threads, oi.data(), of.data());
    if (rc != 0) {
      std::printf("FAIL rc %d: %s\n", rc, desco::last_error_ref().c_str());
      return 1;
    }
    expect("path130", &oi[0], of[0], {130, 130, 129, 129, 130LL * 129 * 131 / 3, 0}, 0.0);
    expect("cycle65", &oi[6], of[1], {65, 65, 65, 32, 65LL * 2 * (32 * 33 / 2), 0}, 0.0);
    expect("star64", &oi[12], of[2], {65, 65, 64, 2, 2 * 64 + 64 * 63 * 2, 0}, 0.0);
    expect("k65", &oi[18], of[3], {65, 65, 65 * 64 / 2, 1, 65 * 64, 65 * 64 * 63 / 6}, 65.0);
    expect("tie", &oi[24], of[4], {9, 4, 3, 3, 20, 0}, 0.0);
    expect("isolated", &oi[30], of[5], {4, 1, 0, 0, 0, 0}, 0.0);
    expect("empty", &oi[36], of[6], {0, 0, 0, 0, 0, 0}, 0.0);
    expect("path5000", &oi[42], of[7], {5000, 5000, 4999, 4999, 5000LL * 4999 * 5001 / 3, 0}, 0.0);
  }
  // refusals return before any work
  if (desco_subgraph_stats(p.rowptr.data(), p.col.data(), p.nodes, nullptr, p.set_nodes.data(), S, 1, oi.data(),
                           of.data()) == 0)
    ++failures;
  std::vector<int32_t> unsorted = p.set_nodes;
  std::swap(unsorted[3], unsorted[4]);
  if (desco_subgraph_stats(p.rowptr.data(), p.col.data(), p.nodes, p.set_ptr.data(), unsorted.data(), S, 1, oi.data(),
                           of.data()) == 0)
    ++failures;
  if (desco_subgraph_stats(nullptr, nullptr, 0, nullptr, nullptr, 0, 1, nullptr, nullptr) != 0) ++failures;
  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
