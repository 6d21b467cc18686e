// Stand-alone check of the host twin of the sampled counts (desco_amd/csrc/sampled_counts.cpp); meant to be built with
// the host sanitizers -- it links no HIP and loads nothing into Python:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/sampled_counts_selftest.cpp desco_amd/csrc/sampled_counts.cpp -o sampled_counts_selftest
//   ./sampled_counts_selftest            (exit code 0 and "ok" when every expectation holds)
//
// Expectations: with every threshold 2^32 the tallies of K8 and of a 12-leaf star are the binomial coefficients, for
// 2..6 nodes; a sampled walk never exceeds them, is the same on 1 and on 8 threads, per graph equals the sum of its node
// rows, and a slice with graph_base / replica_base equals its part of the whole call; bad input is refused by name.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
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

int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

struct Set {
  std::vector<int64_t> graph_ptr{0}, rowptr{0};
  std::vector<int32_t> col;
  // appends a graph given by its adjacency test
  template <class Adj>
  void add(int n, Adj adj) {
    const int64_t base = graph_ptr.back();
    for (int a = 0; a < n; ++a) {
      for (int b = 0; b < n; ++b)
        if (a != b && adj(a, b)) col.push_back((int32_t)(base + b));
      rowptr.push_back((int64_t)col.size());
    }
    graph_ptr.push_back(base + n);
  }
  int64_t G() const { return (int64_t)graph_ptr.size() - 1; }
  int64_t N() const { return graph_ptr.back(); }
};

// one query per size: the clique (K8's subsets) and the star (the star's subsets), 2..6 nodes
struct Queries {
  std::vector<int32_t> nodes, edge_ptr{0}, edges;
  void add(int k, bool clique) {
    nodes.push_back(k);
    for (int b = 1; b < k; ++b)
      for (int a = 0; a < (clique ? b : 1); ++a) {
        edges.push_back(a);
        edges.push_back(b);
      }
    edge_ptr.push_back((int32_t)edges.size() / 2);
  }
};

int64_t choose(int n, int k) {
  int64_t c = 1;
  for (int i = 0; i < k; ++i) c = c * (n - i) / (i + 1);
  return c;
}

int run(const Set& s, const Queries& q, const int64_t* thr, uint64_t seed, int64_t gb, int64_t rb, int R, int per_graph,
        int nt, std::vector<int64_t>& out) {
  out.assign((size_t)(R > 0 ? R : 1) * (size_t)(per_graph == 1 ? s.G() : s.N()) * q.nodes.size(), -1);
  return desco_sampled_counts(s.graph_ptr.data(), s.G(), s.rowptr.data(), s.col.data(), q.nodes.data(),
                              q.edge_ptr.data(), q.edges.data(), (int)q.nodes.size(), 6, thr, seed, gb, rb, R, per_graph,
                              nt, out.data());
}

}  // namespace

int main() {
  const int64_t ONE = (int64_t)1 << 32;
  Set s;
  s.add(8, [](int, int) { return true; });                                   // K8
  s.add(13, [](int a, int b) { return a == 5 || b == 5; });                  // a 12-leaf star
  s.add(9, [](int a, int b) { return (a + 1) % 9 == b || (b + 1) % 9 == a; });   // a 9-cycle
  s.add(3, [](int, int) { return false; });                                  // no edges
  s.add(1, [](int, int) { return false; });                                  // a single node
  Queries q;                              // columns: P2, then clique and star of 3..6 nodes (the triangle / P3 first)
  q.add(2, true);
  for (int k = 3; k <= 6; ++k) q.add(k, true), q.add(k, false);
  const int Q = (int)q.nodes.size();
  std::vector<int64_t> exact, a, b;
  const int64_t all[7] = {0, 0, ONE, ONE, ONE, ONE, ONE};
  EXPECT(run(s, q, all, 1, 0, 0, 2, 1, 0, exact) == 0);
  for (int r = 0; r < 2; ++r) {
    const int64_t* k8 = exact.data() + ((size_t)r * s.G() + 0) * Q;
    const int64_t* star = exact.data() + ((size_t)r * s.G() + 1) * Q;
    EXPECT(k8[0] == 28 && star[0] == 12);
    for (int k = 3; k <= 6; ++k) {
      EXPECT(k8[2 * k - 5] == choose(8, k) && k8[2 * k - 4] == 0);
      EXPECT(star[2 * k - 5] == 0 && star[2 * k - 4] == choose(12, k - 1));
    }
    const int64_t* rest = exact.data() + ((size_t)r * s.G() + 3) * Q;
    for (int i = 0; i < 2 * Q; ++i) EXPECT(rest[i] == 0);
  }
  const int64_t thr[7] = {0, 0, ONE, ONE / 2, (ONE / 4) * 3, ONE / 3, ONE / 2};
  EXPECT(run(s, q, thr, 7, 0, 0, 5, 0, 1, a) == 0);
  EXPECT(run(s, q, thr, 7, 0, 0, 5, 0, 8, b) == 0);
  EXPECT(a == b);
  int64_t kept = 0;
  for (int64_t x : a) {
    kept += x;
    EXPECT(x >= 0);
  }
  EXPECT(kept > 0);
  std::vector<int64_t> pg;
  EXPECT(run(s, q, thr, 7, 0, 0, 5, 1, 3, pg) == 0);
  for (int r = 0; r < 5; ++r)
    for (int64_t g = 0; g < s.G(); ++g)
      for (int c = 0; c < Q; ++c) {
        int64_t sum = 0;
        for (int64_t v = s.graph_ptr[g]; v < s.graph_ptr[g + 1]; ++v) sum += a[((size_t)r * s.N() + v) * Q + c];
        EXPECT(sum == pg[((size_t)r * s.G() + g) * Q + c]);
        EXPECT(sum <= exact[(size_t)g * Q + c]);
      }
  // graphs [1, 3) and replicas [2, 4) reproduce their part of the whole call
  Set part;
  part.add(13, [](int x, int y) { return x == 5 || y == 5; });
  part.add(9, [](int x, int y) { return (x + 1) % 9 == y || (y + 1) % 9 == x; });
  EXPECT(run(part, q, thr, 7, 1, 2, 2, 1, 2, b) == 0);
  for (int r = 0; r < 2; ++r)
    for (int g = 0; g < 2; ++g)
      for (int c = 0; c < Q; ++c) EXPECT(b[((size_t)r * 2 + g) * Q + c] == pg[((size_t)(r + 2) * s.G() + g + 1) * Q + c]);
  // refusals, by name
  const int64_t high[7] = {0, 0, ONE + 1, ONE, ONE, ONE, ONE}, low[7] = {0, 0, ONE, -1, ONE, ONE, ONE};
  EXPECT(run(s, q, high, 0, 0, 0, 1, 0, 1, b) == DESCO_EINVAL);
  EXPECT(desco::last_error_ref().find("desco_sampled_counts: a threshold") == 0);
  EXPECT(run(s, q, low, 0, 0, 0, 1, 0, 1, b) == DESCO_EINVAL);
  EXPECT(run(s, q, all, 0, -1, 0, 1, 0, 1, b) == DESCO_EINVAL);
  EXPECT(run(s, q, all, 0, 0, 0, -1, 0, 1, b) == DESCO_EINVAL);
  EXPECT(run(s, q, all, 0, 0, 0, 1, 2, 1, b) == DESCO_EINVAL);
  EXPECT(desco_sampled_counts(s.graph_ptr.data(), s.G(), s.rowptr.data(), s.col.data(), q.nodes.data(),
                              q.edge_ptr.data(), q.edges.data(), Q, 5, all, 0, 0, 0, 1, 0, 1, b.data()) == DESCO_EINVAL);
  EXPECT(desco::last_error_ref().find("desco_sampled_counts: queries must have") == 0);
  std::printf(failures ? "%d expectation(s) failed\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
