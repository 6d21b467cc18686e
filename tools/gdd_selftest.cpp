// Stand-alone check of the host twin of the graphlet degree distributions (desco_amd/csrc/graphlet_distribution.cpp);
// meant to be built with the host sanitizers -- it links no HIP and loads nothing into Python:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/gdd_selftest.cpp desco_amd/csrc/graphlet_distribution.cpp -o gdd_selftest
//   ./gdd_selftest          (exit code 0 and "ok" when every expectation holds)
//
// Expectations: on a built-in table (zeros, a constant, ties, distinct and huge values, segments of 0, 1, 2, 5, 64 and
// 130 rows, a permuted column list) every list equals the one found by counting value by value -- not the twin's sort
// --, the unused slots are zero, the result is the same on 1, 3 and 16 threads; the agreements are the chain of the
// definition over a std::map union, symmetric, exactly 1 on the diagonal, also into a strided view whose surroundings
// stay untouched, with and without the per-orbit output; bad input is refused by name before anything is written.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
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

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_word() {                                  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

using List = std::map<int64_t, double>;

// the list of one (segment, column) by counting: std::map keeps the keys ascending
List brute(const int64_t* counts, int64_t ld, int64_t r0, int64_t n, int col) {
  std::map<int64_t, int64_t> mult;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t v = counts[(r0 + i) * ld + col];
    if (v >= 1) ++mult[v];
  }
  List out;
  double T = 0.0;
  for (auto& [k, d] : mult) T = T + (out[k] = (double)d / (double)k);
  for (auto& [k, s] : out) s = s / T;
  return out;
}

double column_agreement(const List& x, const List& y) {
  List keys = x;
  keys.insert(y.begin(), y.end());
  double acc = 0.0;
  for (auto& [k, unused] : keys) {
    (void)unused;
    const double a = x.count(k) ? x.at(k) : 0.0, b = y.count(k) ? y.at(k) : 0.0, t = a - b;
    acc = std::fma(t, t, acc);
  }
  const double D = std::sqrt(0.5 * acc);
  return D > 1.0 ? 0.0 : 1.0 - D;
}

bool refused(int rc, const char* name) {
  return rc == DESCO_EINVAL && desco::last_error_ref().rfind(std::string(name) + ":", 0) == 0;
}

}  // namespace

int main() {
  const int64_t N = 202, ld = 8;
  std::vector<int64_t> counts((size_t)N * ld);
  for (int64_t i = 0; i < N; ++i) {
    int64_t* row = counts.data() + i * ld;
    row[0] = 0;                                          // nobody touches the orbit: an empty list
    row[1] = 7;                                          // one entry
    row[2] = (int64_t)(next_word() % 4);                 // heavy ties, zeros among them
    row[3] = i * 7 + 3;                                  // all distinct
    row[4] = (int64_t)(next_word() % 40);                // values shared between the segments
    row[5] = ((int64_t)1 << 53) + 1 + 2 * (int64_t)(next_word() % 3);     // the conversion to double rounds
    row[6] = ((int64_t)1 << 62) - 1 - (int64_t)(next_word() % 3);
    row[7] = (int64_t)(next_word() % 5) - 2;             // negative values are left out like zeros
  }
  const int64_t seg[] = {0, 0, 1, 3, 8, 72, 202};
  const int64_t S = 6;
  const int32_t cols[] = {7, 0, 3, 4, 1, 2, 6, 5};       // a permuted list
  for (int C : {8, 3, 1}) {
    std::vector<int32_t> len((size_t)S * C, -7), len3 = len, len16 = len;
    std::vector<int64_t> key((size_t)N * C, -7), key3 = key, key16 = key;
    std::vector<double> val((size_t)N * C, -7.0), val3 = val, val16 = val;
    EXPECT(desco_gdd_build(seg, S, counts.data(), ld, cols, C, len.data(), key.data(), val.data(), 1) == 0);
    EXPECT(desco_gdd_build(seg, S, counts.data(), ld, cols, C, len3.data(), key3.data(), val3.data(), 3) == 0);
    EXPECT(desco_gdd_build(seg, S, counts.data(), ld, cols, C, len16.data(), key16.data(), val16.data(), 16) == 0);
    EXPECT(len == len3 && len == len16 && key == key3 && key == key16);
    EXPECT(std::memcmp(val.data(), val3.data(), val.size() * 8) == 0);
    EXPECT(std::memcmp(val.data(), val16.data(), val.size() * 8) == 0);
    std::vector<std::vector<List>> lists((size_t)S);
    for (int64_t s = 0; s < S; ++s) {
      const int64_t n = seg[s + 1] - seg[s];
      for (int c = 0; c < C; ++c) {
        const List want = brute(counts.data(), ld, seg[s], n, cols[c]);
        lists[(size_t)s].push_back(want);
        const int64_t at = seg[s] * C + (int64_t)c * n;
        EXPECT(len[(size_t)(s * C + c)] == (int32_t)want.size());
        int64_t i = 0;
        for (auto& [k, v] : want) {
          EXPECT(key[(size_t)(at + i)] == k && val[(size_t)(at + i)] == v);
          ++i;
        }
        for (; i < n; ++i) EXPECT(key[(size_t)(at + i)] == 0 && val[(size_t)(at + i)] == 0.0);
      }
    }
    // ---- agreements: all pairs into a strided view, with and without the per-orbit output ------------------------------
    const int64_t ldo = S + 3;
    std::vector<double> out((size_t)(S + 2) * ldo, -3.0), out16 = out, per((size_t)S * S * C, -3.0);
    EXPECT(desco_gdd_agreement(seg, len.data(), key.data(), val.data(), S, seg, len.data(), key.data(), val.data(), S, C,
                               out.data() + ldo + 2, ldo, per.data(), 1) == 0);
    EXPECT(desco_gdd_agreement(seg, len.data(), key.data(), val.data(), S, seg, len.data(), key.data(), val.data(), S, C,
                               out16.data() + ldo + 2, ldo, nullptr, 16) == 0);
    EXPECT(std::memcmp(out.data(), out16.data(), out.size() * 8) == 0);
    for (int64_t i = 0; i < S + 2; ++i)
      for (int64_t j = 0; j < ldo; ++j) {
        const double got = out[(size_t)(i * ldo + j)];
        if (i >= 1 && i <= S && j >= 2 && j < 2 + S) {
          const int64_t a = i - 1, b = j - 2;
          double sum = 0.0;
          for (int c = 0; c < C; ++c) {
            const double A = column_agreement(lists[(size_t)a][(size_t)c], lists[(size_t)b][(size_t)c]);
            EXPECT(per[(size_t)((a * S + b) * C + c)] == A);
            sum = sum + A;
          }
          EXPECT(got == sum / (double)C);
          EXPECT(got == out[(size_t)((b + 1) * ldo + a + 2)]);           // symmetric, bit for bit
          if (a == b) EXPECT(got == 1.0);
        } else {
          EXPECT(got == -3.0);                            // outside the view: untouched
        }
      }
  }

  // ---- refusals ----------------------------------------------------------------------------------------------------
  std::vector<int32_t> len((size_t)S * 8, -7);
  std::vector<int64_t> key((size_t)N * 8, -7);
  std::vector<double> val((size_t)N * 8, -7.0);
  const char* b = "desco_gdd_build";
  const int64_t backwards[] = {0, 5, 4}, negative[] = {-1, 4};
  const int32_t outside[] = {0, 8};
  EXPECT(refused(desco_gdd_build(seg, -1, counts.data(), ld, cols, 8, len.data(), key.data(), val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(seg, S, counts.data(), -1, cols, 8, len.data(), key.data(), val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(seg, S, counts.data(), ld, cols, 0, len.data(), key.data(), val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(seg, S, counts.data(), ld, cols, 129, len.data(), key.data(), val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(nullptr, S, counts.data(), ld, cols, 8, len.data(), key.data(), val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(seg, S, nullptr, ld, cols, 8, len.data(), key.data(), val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(seg, S, counts.data(), ld, nullptr, 8, len.data(), key.data(), val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(seg, S, counts.data(), ld, cols, 8, nullptr, key.data(), val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(seg, S, counts.data(), ld, cols, 8, len.data(), nullptr, val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(seg, S, counts.data(), ld, cols, 8, len.data(), key.data(), nullptr, 1), b));
  EXPECT(refused(desco_gdd_build(seg, S, counts.data(), ld, outside, 2, len.data(), key.data(), val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(backwards, 2, counts.data(), ld, cols, 8, len.data(), key.data(), val.data(), 1), b));
  EXPECT(refused(desco_gdd_build(negative, 1, counts.data(), ld, cols, 8, len.data(), key.data(), val.data(), 1), b));
  for (int32_t v : len) EXPECT(v == -7);                 // refused before any write
  for (int64_t v : key) EXPECT(v == -7);
  EXPECT(desco_gdd_build(seg, 0, nullptr, ld, nullptr, 8, nullptr, nullptr, nullptr, 1) == 0);

  EXPECT(desco_gdd_build(seg, S, counts.data(), ld, cols, 8, len.data(), key.data(), val.data(), 2) == 0);
  std::vector<double> out((size_t)S * S, -3.0);
  const char* a = "desco_gdd_agreement";
  auto agree = [&](const int64_t* xs, const int32_t* xl, const int64_t* xk, const double* xv, int64_t Gx, int64_t Gy,
                   int C, double* o, int64_t ldo) {
    return desco_gdd_agreement(xs, xl, xk, xv, Gx, seg, len.data(), key.data(), val.data(), Gy, C, o, ldo, nullptr, 1);
  };
  EXPECT(agree(seg, len.data(), key.data(), val.data(), S, S, 8, out.data(), S) == 0 && out[0] == 1.0);
  std::fill(out.begin(), out.end(), -3.0);
  std::vector<int32_t> long_len = len;
  long_len[8 + 2] = 2;                                   // segment 1 has one row
  EXPECT(refused(agree(seg, len.data(), key.data(), val.data(), -1, S, 8, out.data(), S), a));
  EXPECT(refused(agree(seg, len.data(), key.data(), val.data(), S, -1, 8, out.data(), S), a));
  EXPECT(refused(agree(seg, len.data(), key.data(), val.data(), S, S, 0, out.data(), S), a));
  EXPECT(refused(agree(seg, len.data(), key.data(), val.data(), S, S, 129, out.data(), S), a));
  EXPECT(refused(agree(seg, len.data(), key.data(), val.data(), S, S, 8, out.data(), S - 1), a));
  EXPECT(refused(agree(seg, len.data(), key.data(), val.data(), S, S, 8, nullptr, S), a));
  EXPECT(refused(agree(nullptr, len.data(), key.data(), val.data(), S, S, 8, out.data(), S), a));
  EXPECT(refused(agree(seg, nullptr, key.data(), val.data(), S, S, 8, out.data(), S), a));
  EXPECT(refused(agree(seg, len.data(), nullptr, val.data(), S, S, 8, out.data(), S), a));
  EXPECT(refused(agree(seg, len.data(), key.data(), nullptr, S, S, 8, out.data(), S), a));
  EXPECT(refused(agree(backwards, len.data(), key.data(), val.data(), 2, S, 8, out.data(), S), a));
  EXPECT(refused(agree(negative, len.data(), key.data(), val.data(), 1, S, 8, out.data(), S), a));
  EXPECT(refused(agree(seg, long_len.data(), key.data(), val.data(), S, S, 8, out.data(), S), a));
  for (double v : out) EXPECT(v == -3.0);                // refused before any write
  EXPECT(agree(nullptr, nullptr, nullptr, nullptr, 0, S, 8, nullptr, S) == 0);

  if (failures) {
    std::printf("%d expectation(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
