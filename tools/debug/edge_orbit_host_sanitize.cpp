// Stand-alone sanitizer pass over the HOST edge-orbit enumerator (csrc/groundtruth.cpp: desco_edge_orbit_table,
// desco_edge_orbit_counts).  Build and run from the repository root (no GPU, no Python):
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/debug/edge_orbit_host_sanitize.cpp desco_amd/csrc/groundtruth.cpp -o /tmp/edge_orbit_host_sanitize \
//       && /tmp/edge_orbit_host_sanitize
// Graphs: a star, a clique, a path, a graph with isolated nodes, an edgeless and an empty graph, seeded random graphs
// (all below 1024 nodes: the dense edge-row table) and a sparse graph of 1100 nodes (the bisection).  Queries: every
// connected graph of 2..4 nodes and some of 5.  Checks the number of columns, the single-edge column (1), the triangle
// column (common neighbours), that 1 and 4 threads agree and that refusals return an error; the counts themselves are
// the tests' business (tests/edge_orbit_reference.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/desco_hip.h"

namespace desco {                                  // the library's error plumbing (capi.hip), for this program
std::string& last_error_ref() { static std::string s; return s; }
int fail(int code, const char* msg) { last_error_ref() = msg; return code ? -1 : 0; }
}  // namespace desco

struct Graphs {
  std::vector<int64_t> graph_ptr{0}, rowptr{0};
  std::vector<int32_t> col;
  void add(int n, const std::vector<std::pair<int, int>>& edges) {
    const int64_t base = graph_ptr.back();
    std::vector<std::vector<int>> adj(n);
    for (auto [a, b] : edges) { adj[a].push_back(b); adj[b].push_back(a); }
    for (int v = 0; v < n; ++v) {
      std::vector<char> seen(n, 0);
      for (int u : adj[v]) seen[u] = 1;
      for (int u = 0; u < n; ++u) if (seen[u] && u != v) col.push_back((int32_t)(base + u));   // ascending, no duplicates
      rowptr.push_back((int64_t)col.size());
    }
    graph_ptr.push_back(base + n);
  }
};

int main() {
  Graphs g;
  std::vector<std::pair<int, int>> e;
  for (int i = 1; i <= 70; ++i) e.push_back({0, i});
  e.push_back({3, 4});
  g.add(71, e);                                                             // star with a chord
  e.clear();
  for (int a = 0; a < 9; ++a) for (int b = a + 1; b < 9; ++b) e.push_back({a, b});
  g.add(9, e);                                                              // clique
  e.clear();
  for (int i = 0; i + 1 < 12; ++i) e.push_back({i, i + 1});
  g.add(12, e);                                                             // path
  g.add(7, {{0, 3}, {3, 5}, {5, 0}});                                       // isolated nodes
  g.add(4, {});                                                             // edgeless
  g.add(0, {});                                                             // no nodes
  uint32_t state = 12345;
  auto rnd = [&] { state = state * 1664525u + 1013904223u; return state >> 8; };
  for (int t = 0; t < 6; ++t) {
    const int n = 5 + (int)(rnd() % 60);
    e.clear();
    for (int a = 0; a < n; ++a) for (int b = a + 1; b < n; ++b) if (rnd() % 100 < 12u) e.push_back({a, b});
    g.add(n, e);
  }
  e.clear();
  for (int i = 0; i + 1 < 1100; ++i) e.push_back({i, i + 1});               // above the dense table's limit: bisection
  for (int i = 0; i + 2 < 1100; i += 3) e.push_back({i, i + 2});
  for (int t = 0; t < 300; ++t) {
    const int a = (int)(rnd() % 1100), b = (int)(rnd() % 1100);
    if (a != b) e.push_back({a, b});
  }
  g.add(1100, e);
  // queries: edge; P3, triangle; the six connected 4-node graphs; 5-star, 5-path, 5-cycle, K5
  const std::vector<std::pair<int, std::vector<std::pair<int, int>>>> qs = {
      {2, {{0, 1}}}, {3, {{0, 1}, {1, 2}}}, {3, {{0, 1}, {1, 2}, {0, 2}}},
      {4, {{0, 1}, {0, 2}, {0, 3}}}, {4, {{0, 1}, {1, 2}, {2, 3}}}, {4, {{0, 1}, {1, 2}, {0, 2}, {2, 3}}},
      {4, {{0, 1}, {1, 2}, {2, 3}, {3, 0}}}, {4, {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {0, 2}}},
      {4, {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}}},
      {5, {{0, 1}, {0, 2}, {0, 3}, {0, 4}}}, {5, {{0, 1}, {1, 2}, {2, 3}, {3, 4}}},
      {5, {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 0}}},
      {5, {{0, 1}, {0, 2}, {0, 3}, {0, 4}, {1, 2}, {1, 3}, {1, 4}, {2, 3}, {2, 4}, {3, 4}}}};
  std::vector<int32_t> q_nodes, q_edge_ptr{0}, q_edges;
  for (const auto& q : qs) {
    q_nodes.push_back(q.first);
    for (auto [a, b] : q.second) { q_edges.push_back(a); q_edges.push_back(b); }
    q_edge_ptr.push_back((int32_t)(q_edges.size() / 2));
  }
  std::vector<int16_t> table(1098 * 10);
  int cols = 0, kmax = 0;
  if (desco_edge_orbit_table(q_nodes.data(), q_edge_ptr.data(), q_edges.data(), (int)qs.size(), table.data(), &cols,
                             &kmax)) {
    std::printf("table: %s\n", desco::last_error_ref().c_str());
    return 1;
  }
  if (cols != 1 + 1 + 1 + 1 + 2 + 3 + 1 + 2 + 1 + 1 + 2 + 1 + 1 || kmax != 5) {
    std::printf("unexpected shape: %d columns, kmax %d\n", cols, kmax);
    return 1;
  }
  const int64_t N = g.graph_ptr.back();
  const int G = (int)g.graph_ptr.size() - 1;
  std::vector<std::pair<int64_t, int64_t>> rows;                            // (v, u), u < v, in CSR order
  for (int64_t v = 0; v < N; ++v)
    for (int64_t i = g.rowptr[v]; i < g.rowptr[v + 1]; ++i)
      if (g.col[i] < v) rows.push_back({v, g.col[i]});
  const int64_t M = (int64_t)rows.size();
  std::vector<int64_t> a((size_t)M * cols, -1), b((size_t)M * cols, -1);
  for (auto* out : {&a, &b})
    if (desco_edge_orbit_counts(g.graph_ptr.data(), G, g.rowptr.data(), g.col.data(), q_nodes.data(), q_edge_ptr.data(),
                                q_edges.data(), (int)qs.size(), out == &a ? 1 : 4, out->data())) {
      std::printf("counts: %s\n", desco::last_error_ref().c_str());
      return 1;
    }
  if (a != b) { std::printf("1 and 4 threads differ\n"); return 1; }
  int64_t cells = 0;
  for (int64_t r = 0; r < M; ++r) {
    const auto [v, u] = rows[r];
    int64_t common = 0;                                                     // merge of the two ascending rows
    for (int64_t i = g.rowptr[v], j = g.rowptr[u]; i < g.rowptr[v + 1] && j < g.rowptr[u + 1];) {
      if (g.col[i] == g.col[j]) { ++common; ++i; ++j; }
      else if (g.col[i] < g.col[j]) ++i;
      else ++j;
    }
    if (a[(size_t)r * cols] != 1 || a[(size_t)r * cols + 2] != common) {
      std::printf("edge or triangle column wrong at row %lld\n", (long long)r);
      return 1;
    }
    for (int c = 0; c < cols; ++c) cells += a[(size_t)r * cols + c];
  }
  // refusals leave a message and touch nothing
  const int32_t six = 6, ptr0[2] = {0, 0};
  if (desco_edge_orbit_table(&six, ptr0, nullptr, 1, table.data(), &cols, &kmax) != -1) return 1;
  const int32_t four = 4, ptr1[2] = {0, 2}, split[4] = {0, 1, 2, 3};
  if (desco_edge_orbit_table(&four, ptr1, split, 1, table.data(), &cols, &kmax) != -1) return 1;
  std::printf("edge orbit host sanitize ok: %lld edges, %lld cell updates\n", (long long)M, (long long)cells);
  return 0;
}
