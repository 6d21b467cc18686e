// Stand-alone check of the host twin of the graphlet correlation (desco_amd/csrc/graphlet_correlation.cpp); meant to be
// built with the host sanitizers -- it links no HIP and loads nothing into Python:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/graph_comparison_selftest.cpp desco_amd/csrc/graphlet_correlation.cpp -o graph_comparison_selftest
//   ./graph_comparison_selftest          (exit code 0 and "ok" when every expectation holds)
//
// Expectations: on built-in tables (ties, constant columns, segments of 0, 1 and 2 rows, a strided column list) S equals
// the product of the ranks counted pair by pair -- the kernel's way, not the twin's sort --, rho is its definition, the
// result is the same on 1 and on 8 threads and with either output left out; the distances are the fma chain, also into a
// strided view whose surroundings stay untouched; bad input is refused by name.
#include <cmath>
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

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_word() {                                  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// S and rho of one segment by all-pairs counting
void brute(const int64_t* counts, int64_t ld, int64_t r0, int64_t n, const int32_t* cols, int C, int dummy,
           std::vector<int64_t>& S, std::vector<double>& rho) {
  const int64_t np = n + dummy;
  std::vector<int64_t> D((size_t)np * C);
  auto value = [&](int64_t i, int c) { return i < n ? counts[(r0 + i) * ld + cols[c]] : (int64_t)1; };
  for (int c = 0; c < C; ++c)
    for (int64_t i = 0; i < np; ++i) {
      int64_t less = 0, equal = 0;
      for (int64_t j = 0; j < np; ++j) less += value(j, c) < value(i, c), equal += value(j, c) == value(i, c);
      D[(size_t)i * C + c] = 2 * less + equal - np;
    }
  S.assign((size_t)C * C, 0);
  rho.assign((size_t)C * C, 0.0);
  for (int a = 0; a < C; ++a)
    for (int b = 0; b < C; ++b)
      for (int64_t i = 0; i < np; ++i) S[(size_t)a * C + b] += D[(size_t)i * C + a] * D[(size_t)i * C + b];
  for (int a = 0; a < C; ++a)
    for (int b = 0; b < C; ++b) {
      const int64_t saa = S[(size_t)a * C + a], sbb = S[(size_t)b * C + b];
      rho[(size_t)a * C + b] =
          a == b ? 1.0 : saa == 0 || sbb == 0 ? 0.0 : (double)S[(size_t)a * C + b] / std::sqrt((double)saa * (double)sbb);
    }
}

bool refused(int rc, const char* name) {
  return rc == DESCO_EINVAL && desco::last_error_ref().rfind(std::string(name) + ":", 0) == 0;
}

}  // namespace

int main() {
  // ---- a table with every kind of column, cut into segments of 0, 1, 2, 5, 64 and 130 rows ---------------------------
  const int64_t N = 202, ld = 9;
  std::vector<int64_t> counts((size_t)N * ld);
  for (int64_t i = 0; i < N; ++i) {
    int64_t* row = counts.data() + i * ld;
    row[0] = 0;                                          // zeros: varies only through the dummy row
    row[1] = 1;                                          // ones: constant even with it
    row[2] = (int64_t)(next_word() % 3);                 // heavy ties
    row[3] = i * 7 + 3;                                  // ascending, all distinct
    row[4] = -row[3];                                    // descending: rho = -1 against column 3
    row[5] = (int64_t)(next_word() >> 20);               // large values
    row[6] = (int64_t)(next_word() % 11) - 5;            // negative values
    row[7] = i / 4;                                      // runs of four
    row[8] = (int64_t)(next_word() % 2) << 62;           // two values far apart
  }
  const int64_t seg[] = {0, 0, 1, 3, 8, 72, 202};
  const int64_t num_segs = 6;
  const int32_t cols[] = {8, 0, 3, 4, 1, 2, 7, 5, 6};     // a permuted list
  for (int C : {9, 4, 1})
    for (int dummy : {1, 0}) {
      std::vector<int64_t> S((size_t)num_segs * C * C, -7), S8 = S, Sonly = S;
      std::vector<double> rho((size_t)num_segs * C * C, -7.0), rho8 = rho, rhoonly = rho;
      EXPECT(desco_graphlet_correlation(seg, num_segs, counts.data(), ld, cols, C, dummy, S.data(), rho.data(), 1) == 0);
      EXPECT(desco_graphlet_correlation(seg, num_segs, counts.data(), ld, cols, C, dummy, S8.data(), rho8.data(), 8) == 0);
      EXPECT(desco_graphlet_correlation(seg, num_segs, counts.data(), ld, cols, C, dummy, Sonly.data(), nullptr, 3) == 0);
      EXPECT(desco_graphlet_correlation(seg, num_segs, counts.data(), ld, cols, C, dummy, nullptr, rhoonly.data(), 3) == 0);
      EXPECT(S == S8 && S == Sonly);
      EXPECT(std::memcmp(rho.data(), rho8.data(), rho.size() * 8) == 0);
      EXPECT(std::memcmp(rho.data(), rhoonly.data(), rho.size() * 8) == 0);
      std::vector<int64_t> Sb;
      std::vector<double> rb;
      for (int64_t s = 0; s < num_segs; ++s) {
        brute(counts.data(), ld, seg[s], seg[s + 1] - seg[s], cols, C, dummy, Sb, rb);
        EXPECT(std::memcmp(Sb.data(), S.data() + s * C * C, Sb.size() * 8) == 0);
        EXPECT(std::memcmp(rb.data(), rho.data() + s * C * C, rb.size() * 8) == 0);
      }
      if (C == 9) {
        const double* last = rho.data() + 5 * C * C;       // the 130-row segment
        EXPECT(last[2 * C + 3] == -1.0 && last[3 * C + 2] == -1.0);      // ascending against descending
        EXPECT(last[4 * C + 2] == 0.0 && last[4 * C + 4] == 1.0);        // the column of ones is constant
        EXPECT((last[1 * C + 2] != 0.0) == (dummy == 1));                // the zeros vary only with the dummy row
      }
    }

  // ---- distances -------------------------------------------------------------------------------------------------
  const int64_t Gx = 5, Gy = 3, P = 55, ldo = 7;
  std::vector<double> x((size_t)Gx * P), y((size_t)Gy * P), out((size_t)(Gx + 2) * ldo, -3.0), out8;
  for (double& v : x) v = (double)(int64_t)(next_word() >> 11) / 9007199254740992.0 * 2.0 - 1.0;
  for (double& v : y) v = (double)(int64_t)(next_word() >> 11) / 9007199254740992.0 * 2.0 - 1.0;
  out8 = out;
  EXPECT(desco_gcd_matrix(x.data(), Gx, y.data(), Gy, P, out.data() + ldo + 2, ldo, 1) == 0);
  EXPECT(desco_gcd_matrix(x.data(), Gx, y.data(), Gy, P, out8.data() + ldo + 2, ldo, 8) == 0);
  EXPECT(std::memcmp(out.data(), out8.data(), out.size() * 8) == 0);
  for (int64_t i = 0; i < Gx + 2; ++i)
    for (int64_t j = 0; j < ldo; ++j) {
      const double got = out[(size_t)(i * ldo + j)];
      if (i >= 1 && i <= Gx && j >= 2 && j < 2 + Gy) {
        double acc = 0.0;
        for (int64_t p = 0; p < P; ++p) {
          const double t = x[(size_t)((i - 1) * P + p)] - y[(size_t)((j - 2) * P + p)];
          acc = std::fma(t, t, acc);
        }
        EXPECT(got == std::sqrt(acc) && got > 0.0);
      } else {
        EXPECT(got == -3.0);                              // outside the view: untouched
      }
    }
  std::vector<double> self((size_t)Gx * Gx);
  EXPECT(desco_gcd_matrix(x.data(), Gx, x.data(), Gx, P, self.data(), Gx, 2) == 0);
  for (int64_t i = 0; i < Gx; ++i)
    for (int64_t j = 0; j < Gx; ++j) EXPECT(self[(size_t)(i * Gx + j)] == self[(size_t)(j * Gx + i)] && (i != j || self[(size_t)(i * Gx + j)] == 0.0));

  // ---- refusals --------------------------------------------------------------------------------------------------
  std::vector<int64_t> S(81);
  const char* g = "desco_graphlet_correlation";
  EXPECT(refused(desco_graphlet_correlation(seg, -1, counts.data(), ld, cols, 9, 1, S.data(), nullptr, 1), g));
  EXPECT(refused(desco_graphlet_correlation(seg, 1, counts.data(), ld, cols, 129, 1, S.data(), nullptr, 1), g));
  EXPECT(refused(desco_graphlet_correlation(seg, 1, counts.data(), ld, cols, 9, 2, S.data(), nullptr, 1), g));
  EXPECT(refused(desco_graphlet_correlation(nullptr, 1, counts.data(), ld, cols, 9, 1, S.data(), nullptr, 1), g));
  EXPECT(refused(desco_graphlet_correlation(seg, 1, counts.data(), ld, nullptr, 9, 1, S.data(), nullptr, 1), g));
  EXPECT(refused(desco_graphlet_correlation(seg, 6, nullptr, ld, cols, 9, 1, S.data(), nullptr, 1), g));
  EXPECT(refused(desco_graphlet_correlation(seg, 1, counts.data(), 8, cols, 9, 1, S.data(), nullptr, 1), g));
  const int64_t backwards[] = {0, 5, 4}, huge[] = {0, 2097152};
  EXPECT(refused(desco_graphlet_correlation(backwards, 2, counts.data(), ld, cols, 9, 1, S.data(), nullptr, 1), g));
  EXPECT(refused(desco_graphlet_correlation(huge, 1, counts.data(), ld, cols, 9, 0, S.data(), nullptr, 1), g));
  EXPECT(desco_graphlet_correlation(seg, 0, nullptr, ld, nullptr, 9, 1, nullptr, nullptr, 1) == 0);
  const char* d = "desco_gcd_matrix";
  EXPECT(refused(desco_gcd_matrix(x.data(), Gx, y.data(), Gy, -1, out.data(), ldo, 1), d));
  EXPECT(refused(desco_gcd_matrix(x.data(), Gx, y.data(), Gy, P, out.data(), Gy - 1, 1), d));
  EXPECT(refused(desco_gcd_matrix(x.data(), Gx, y.data(), Gy, P, nullptr, ldo, 1), d));
  EXPECT(refused(desco_gcd_matrix(nullptr, Gx, y.data(), Gy, P, out.data(), ldo, 1), d));

  if (failures) {
    std::printf("%d expectation(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
