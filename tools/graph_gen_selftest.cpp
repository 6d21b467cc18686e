// Stand-alone check of the host graph generators (desco_amd/csrc/graph_gen.cpp) on every family at the edge shapes of
// the tests; meant to be built with the host sanitizers -- it links no HIP and loads nothing into Python:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/graph_gen_selftest.cpp desco_amd/csrc/graph_gen.cpp -o graph_gen_selftest
//   ./graph_gen_selftest                 (exit code 0 and "ok" when every expectation holds)
//
// Expectations: every graph simple, symmetric, rows ascending, connected, with the edge count its family fixes; 1 thread
// equal to 8 threads; a slice with graph_base equal to its part of the whole call; bad input refused by name with
// nothing written.
#include <algorithm>
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

constexpr uint64_t T32 = (uint64_t)1 << 32;

struct Spec {
  std::vector<int32_t> family, n;
  std::vector<int64_t> param;
  std::vector<uint64_t> thr;
  void add(int f, int nn, int64_t a, int64_t b, uint64_t t0, uint64_t t1) {
    family.push_back(f), n.push_back(nn);
    param.push_back(a), param.push_back(b);
    thr.push_back(t0), thr.push_back(t1);
  }
  int64_t size() const { return (int64_t)n.size(); }
};

struct Out {
  std::vector<int64_t> graph_ptr, bit_ptr, rowptr;
  std::vector<uint32_t> bits;
  std::vector<int32_t> deg, status, col;
  int rc = 0;
};

int64_t row_words(int64_t n) { return ((n + 31) >> 5) | 1; }

Out run(const Spec& s, int64_t first, int64_t count, int64_t base, int threads, uint64_t seed = 5) {
  Out o;
  o.graph_ptr.assign(1, 0), o.bit_ptr.assign(1, 0);
  for (int64_t g = first; g < first + count; ++g) {
    o.graph_ptr.push_back(o.graph_ptr.back() + s.n[g]);
    o.bit_ptr.push_back(o.bit_ptr.back() + s.n[g] * row_words(s.n[g]));
  }
  o.bits.assign((size_t)o.bit_ptr.back() + 1, 0), o.deg.assign((size_t)o.graph_ptr.back() + 1, 0);
  o.status.assign((size_t)count + 1, 0);
  o.rc = desco_graph_gen(s.family.data() + first, s.n.data() + first, s.param.data() + 2 * first,
                         s.thr.data() + 2 * first, count, base, seed, threads, 0, o.graph_ptr.data(), o.bit_ptr.data(),
                         o.bits.data(), o.deg.data(), o.status.data());
  if (o.rc) return o;
  o.rowptr.assign(1, 0);
  for (int64_t v = 0; v < o.graph_ptr.back(); ++v) o.rowptr.push_back(o.rowptr.back() + o.deg[v]);
  o.col.assign((size_t)o.rowptr.back() + 1, -1);
  o.rc = desco_graph_gen_expand(o.graph_ptr.data(), o.bit_ptr.data(), o.bits.data(), o.rowptr.data(), count, threads,
                                o.col.data());
  return o;
}

void check_graphs(const Spec& s, const Out& o) {
  for (int64_t g = 0; g < s.size(); ++g) {
    const int64_t n0 = o.graph_ptr[g], n = s.n[g];
    std::vector<int> seen((size_t)n, 0), stack{0};
    seen[0] = 1;
    int64_t reached = 1, entries = o.rowptr[n0 + n] - o.rowptr[n0];
    for (int64_t v = 0; v < n; ++v)
      for (int64_t e = o.rowptr[n0 + v]; e < o.rowptr[n0 + v + 1]; ++e) {
        const int64_t u = o.col[e] - n0;
        EXPECT(u >= 0 && u < n && u != v);
        EXPECT(e == o.rowptr[n0 + v] || o.col[e - 1] < o.col[e]);
        if (u < 0 || u >= n) continue;
        EXPECT(std::binary_search(o.col.begin() + o.rowptr[n0 + u], o.col.begin() + o.rowptr[n0 + u + 1],
                                  (int32_t)(n0 + v)));
      }
    while (!stack.empty()) {
      const int v = stack.back();
      stack.pop_back();
      for (int64_t e = o.rowptr[n0 + v]; e < o.rowptr[n0 + v + 1]; ++e) {
        const int u = (int)(o.col[e] - n0);
        if (u >= 0 && u < n && !seen[u]) seen[u] = 1, ++reached, stack.push_back(u);
      }
    }
    EXPECT(reached == n);
    const int64_t m = s.param[2 * g], added = o.status[g] >> 8, tries = o.status[g] & 0xff;
    if (n > 1 && s.family[g] == 3) EXPECT(entries / 2 == m * (n - m) && added == 0);
    if (n > 1 && s.family[g] == 2) EXPECT(entries / 2 == std::min(m, n * (n - 1) / 2) + added);
    if (n > 1 && s.family[g] == 1 && tries >= 1 && tries <= 100) EXPECT(entries / 2 == n * (m / 2) && added == 0);
    if (s.family[g] == 0 && s.thr[2 * g] == T32) EXPECT(entries == n * (n - 1));
  }
}

}  // namespace

int main() {
  Spec s;
  for (int n : {1, 2, 3, 10, 32, 33, 64, 65, 130}) {
    const int64_t top = (int64_t)n * (n - 1) / 2;
    for (int64_t e : {(int64_t)n - 1, (int64_t)2 * n, (int64_t)n * n / 4, top}) {
      e = std::max<int64_t>(std::min(e, top), n - 1);
      const int64_t m = std::max<int64_t>(1, std::min<int64_t>(n - 1, n ? e / n : 0));
      s.add(0, n, 0, 0, top ? std::min<uint64_t>(T32, (uint64_t)((double)e / (double)top * 4294967296.0)) : 0, 0);
      s.add(1, n, std::min<int64_t>(2 * e / n, n - 1), e, T32 / 10, 0);
      s.add(2, n, e, 0, 0, 0);
      s.add(3, n, n > 1 ? m : 0, 0, 0, 0);
      s.add(4, n, n > 1 ? m : 0, 0, T32 / 2, T32 / 10 * 9);
      s.add(5, n, n > 1 ? std::max<int64_t>(1, std::min<int64_t>(m, n / 2)) : 0, 0, T32 / 2, 0);
    }
  }
  for (int n : {12, 20, 30}) s.add(1, n, 2, n, T32, 0), s.add(1, n, 1, n + 3, T32, 0), s.add(5, n, 3, 0, T32, 0);
  s.add(0, 200, 0, 0, T32 / 199, 0);
  const Out one = run(s, 0, s.size(), 0, 1), eight = run(s, 0, s.size(), 0, 8);
  EXPECT(one.rc == 0 && eight.rc == 0);
  EXPECT(one.col == eight.col && one.deg == eight.deg && one.status == eight.status && one.bits == eight.bits);
  check_graphs(s, one);
  const int64_t cut = 50;
  const Out tail = run(s, cut, s.size() - cut, cut, 3);
  EXPECT(tail.rc == 0);
  EXPECT(std::equal(tail.deg.begin(), tail.deg.end() - 1, one.deg.begin() + one.graph_ptr[cut]));
  EXPECT(std::equal(tail.status.begin(), tail.status.end() - 1, one.status.begin() + cut));
  EXPECT(std::equal(tail.bits.begin(), tail.bits.end() - 1, one.bits.begin() + one.bit_ptr[cut]));

  // bad input: refused by name, nothing written
  auto refused = [&](Spec b, const char* what) {
    const Out o = run(b, 0, b.size(), 0, 2);
    EXPECT(o.rc == DESCO_EINVAL);
    EXPECT(desco::last_error_ref().rfind("desco_graph_gen:", 0) == 0);
    EXPECT(desco::last_error_ref().find(what) != std::string::npos);
    EXPECT(std::all_of(o.bits.begin(), o.bits.end(), [](uint32_t w) { return w == 0; }));
    EXPECT(std::all_of(o.deg.begin(), o.deg.end(), [](int32_t w) { return w == 0; }));
  };
  Spec b;
  b.add(6, 5, 1, 0, 0, 0), refused(b, "unknown family");
  b = Spec(), b.add(3, 5, 5, 0, 0, 0), refused(b, "outside the family's range");
  b = Spec(), b.add(5, 5, 6, 0, 0, 0), refused(b, "outside the family's range");
  b = Spec(), b.add(0, 5, 0, 0, T32 + 1, 0), refused(b, "threshold above 2^32");
  b = Spec(), b.add(4, 5, 2, 0, 7, 3), refused(b, "threshold 0 <= threshold 1");
  EXPECT(desco_graph_gen(nullptr, nullptr, nullptr, nullptr, -1, 0, 0, 1, 0, nullptr, nullptr, nullptr, nullptr,
                         nullptr) == DESCO_EINVAL);
  EXPECT(desco_graph_gen(nullptr, nullptr, nullptr, nullptr, 2, 0, 0, 1, 0, nullptr, nullptr, nullptr, nullptr,
                         nullptr) == DESCO_EINVAL);
  int64_t out[2] = {0, 0};
  EXPECT(desco_graph_gen_draw(1, 2, 3, 4, 1000, out) == 0 && out[1] == ((out[0] * 1000) >> 32));
  EXPECT(desco_graph_gen_draw(1, -2, 3, 4, 1000, out) == DESCO_EINVAL);
  if (failures) {
    std::printf("%d expectation(s) failed\n", failures);
    return 1;
  }
  std::printf("ok: %lld graphs of six families\n", (long long)s.size());
  return 0;
}
