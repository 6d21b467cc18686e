// Stand-alone check of the host colour refinement (desco_amd/csrc/wl_refine.cpp) on hand-made and seeded random blocks,
// against a naive restatement of the definition inside this program; meant to be built with the host sanitizers -- it
// links no HIP and loads nothing into Python:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/expressiveness_selftest.cpp desco_amd/csrc/wl_refine.cpp -o expressiveness_selftest
//   ./expressiveness_selftest            (exit code 0 and "ok" when every expectation holds)
//
// Expectations: signatures, final colours and status equal to the restatement for rounds 0, 1, 3 and 64, every view, with
// and without anchors, with and without init, an empty slot, a segment without count rows, an empty block; 1 thread
// equal to 8 threads; colours = NULL leaves the signatures alone; a range of segments through shifted pointers equals the
// whole call; an entry outside its segment gives status -1 for that segment only and nothing else of it written; bad
// arguments refused by name with nothing written.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
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
#define EXPECT(cond, what)                                        \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, what); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

constexpr uint64_t G = 0x9E3779B97F4A7C15ull;
constexpr int64_t kUntouched = 0x7777777777777777ll;

uint64_t mix(uint64_t x) {
  x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27, x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct Block {
  int slots = 4;
  int64_t num_rows = 0, anchor_base = -1;
  std::vector<int32_t> vrowptr{0}, vcol, seg_ptr{0};
  int64_t segs() const { return (int64_t)seg_ptr.size() - 1; }
};

// segments of sizes[i] rows (anchor included when anchored), random entries inside each, a random slot per entry
Block random_block(const std::vector<int>& sizes, bool anchored, int slots, unsigned seed, double degree = 3.0) {
  std::mt19937 rng(seed);
  Block b;
  b.slots = slots;
  for (int s : sizes) b.seg_ptr.push_back(b.seg_ptr.back() + (anchored ? s - 1 : s));
  const int64_t nc = b.seg_ptr.back();
  b.num_rows = nc + (anchored ? (int64_t)sizes.size() : 0);
  b.anchor_base = anchored ? nc : -1;
  std::vector<std::vector<int32_t>> rows((size_t)(b.num_rows * slots));
  for (size_t i = 0; i < sizes.size(); ++i) {
    std::vector<int32_t> ids;
    for (int32_t r = b.seg_ptr[i]; r < b.seg_ptr[i + 1]; ++r) ids.push_back(r);
    if (anchored) ids.push_back((int32_t)(nc + (int64_t)i));
    const int s = sizes[i];
    for (int k = 0; s > 1 && k < (int)(degree * s / 2); ++k) {
      const int a = (int)(rng() % s), c = (int)(rng() % s);
      if (a == c) continue;
      rows[(size_t)ids[a] * slots + rng() % slots].push_back(ids[c]);
      rows[(size_t)ids[c] * slots + rng() % slots].push_back(ids[a]);
    }
  }
  for (auto& r : rows) {
    b.vcol.insert(b.vcol.end(), r.begin(), r.end());
    b.vrowptr.push_back((int32_t)b.vcol.size());
  }
  return b;
}

struct Result {
  std::vector<int64_t> sig, colours;
  std::vector<int32_t> status;
  bool operator==(const Result& o) const { return sig == o.sig && colours == o.colours && status == o.status; }
};

// the definition, row by row, with nothing shared with wl_refine.cpp; untouched words keep kUntouched
Result naive(const Block& b, const int* group, int rounds, const int64_t* init) {
  Result out;
  out.sig.assign((size_t)b.segs(), kUntouched), out.colours.assign((size_t)b.num_rows, kUntouched);
  out.status.assign((size_t)b.segs(), 0);
  for (int64_t i = 0; i < b.segs(); ++i) {
    std::vector<int64_t> mine;
    for (int64_t r = b.seg_ptr[i]; r < b.seg_ptr[i + 1]; ++r) mine.push_back(r);
    const int64_t a = b.anchor_base >= 0 ? b.anchor_base + i : -1;
    if (a >= 0) mine.push_back(a);
    auto inside = [&](int64_t c) { return (c >= b.seg_ptr[i] && c < b.seg_ptr[i + 1]) || c == a; };
    bool ok = true;
    for (int64_t r : mine)
      for (int32_t e = b.vrowptr[r * b.slots]; e < b.vrowptr[(r + 1) * b.slots]; ++e) ok = ok && inside(b.vcol[e]);
    if (!ok) {
      out.status[i] = -1;
      continue;
    }
    std::vector<uint64_t> c((size_t)b.num_rows, 0), next((size_t)b.num_rows, 0);
    for (int64_t r : mine) c[r] = init ? (uint64_t)init[r] : (uint64_t)(r == a);
    for (int t = 0; t < rounds; ++t) {
      for (int64_t r : mine) {
        uint64_t m[4] = {0, 0, 0, 0};
        for (int s = 0; s < b.slots; ++s)
          for (int32_t e = b.vrowptr[r * b.slots + s]; e < b.vrowptr[r * b.slots + s + 1]; ++e)
            m[group[s]] += mix(c[b.vcol[e]] + G);
        uint64_t h = mix(c[r] + G);
        for (int g = 0; g < b.slots; ++g) h = mix(h ^ (m[g] + (uint64_t)(g + 1) * G));
        next[r] = h;
      }
      c.swap(next);
    }
    uint64_t p = 0;
    for (int64_t r : mine)
      if (r != a) p += mix(c[r] + G);
    out.sig[i] = (int64_t)(a >= 0 ? mix(mix(c[a] + G) ^ (p + G)) : mix(p + G));
    for (int64_t r : mine) out.colours[r] = (int64_t)c[r];
  }
  return out;
}

Result twin(const Block& b, const int* group, int rounds, const int64_t* init, int threads, bool colours = true,
            int* rc_out = nullptr) {
  Result out;
  out.sig.assign((size_t)b.segs(), kUntouched), out.colours.assign((size_t)b.num_rows, kUntouched);
  out.status.assign((size_t)b.segs(), 0);
  const int32_t grp[4] = {group[0], group[1], group[2], group[3]};
  const int rc = desco_wl_refine(b.vrowptr.data(), b.vcol.data(), b.num_rows, b.slots, grp, b.seg_ptr.data(), b.segs(),
                                 b.anchor_base, init, rounds, threads, out.sig.data(),
                                 colours ? out.colours.data() : nullptr, out.status.data());
  if (rc_out) *rc_out = rc;
  else EXPECT(rc == 0, desco::last_error_ref().c_str());
  return out;
}

const int kViews4[4][4] = {{0, 1, 2, 3}, {0, 0, 1, 1}, {0, 0, 0, 0}, {1, 0, 0, 3}};
const int kViews2[2][4] = {{0, 1, 0, 0}, {0, 0, 0, 0}};

void check_block(const Block& b, const char* name) {
  std::mt19937_64 rng(99);
  std::vector<int64_t> init((size_t)b.num_rows);
  for (auto& x : init) x = (int64_t)rng();
  const int views = b.slots == 4 ? 4 : 2;
  for (int v = 0; v < views; ++v) {
    const int* group = b.slots == 4 ? kViews4[v] : kViews2[v];
    for (int rounds : {0, 1, 3, 64})
      for (const int64_t* in : {(const int64_t*)nullptr, (const int64_t*)init.data()}) {
        const Result want = naive(b, group, rounds, in);
        const Result one = twin(b, group, rounds, in, 1), many = twin(b, group, rounds, in, 8);
        EXPECT(one == want, name);
        EXPECT(many == want, name);
        const Result bare = twin(b, group, rounds, in, 3, false);
        EXPECT(bare.sig == want.sig && bare.status == want.status, name);
        for (int64_t c : bare.colours) EXPECT(c == kUntouched, "colours = NULL wrote a colour");
      }
  }
}

void check_range(const Block& b) {
  const int group[4] = {0, 1, 2, 3};
  const int32_t grp[4] = {0, 1, 2, 3};
  const Result whole = twin(b, group, 5, nullptr, 4);
  const int64_t i0 = 2, i1 = b.segs() - 1;
  std::vector<int64_t> sig((size_t)b.segs(), kUntouched), colours((size_t)b.num_rows, kUntouched);
  std::vector<int32_t> status((size_t)b.segs(), 9);
  EXPECT(desco_wl_refine(b.vrowptr.data(), b.vcol.data(), b.num_rows, b.slots, grp, b.seg_ptr.data() + i0, i1 - i0,
                         b.anchor_base + i0, nullptr, 5, 2, sig.data() + i0, colours.data(), status.data() + i0) == 0,
         "a range of segments");
  for (int64_t i = 0; i < b.segs(); ++i) {
    const bool in = i >= i0 && i < i1;
    EXPECT(sig[i] == (in ? whole.sig[i] : kUntouched) && status[i] == (in ? 0 : 9), "a range writes its segments only");
  }
}

void check_guard() {
  Block b = random_block({12, 30, 7, 64, 5}, true, 4, 31);
  const int group[4] = {0, 1, 2, 3};
  const Result want = twin(b, group, 4, nullptr, 2);
  for (int32_t bad : {(int32_t)0, (int32_t)(b.num_rows - 1), (int32_t)-3, (int32_t)INT32_MAX}) {
    Block x = b;
    const int64_t where = 1;
    x.vcol[(size_t)x.vrowptr[(size_t)(x.seg_ptr[where] + 1) * 4]] = bad;      // an entry of segment 1 (its rows have some)
    const Result got = twin(x, group, 4, nullptr, 2), ref = naive(x, group, 4, nullptr);
    EXPECT(got == ref, "guard: twin and restatement");
    EXPECT(got.status[where] == -1 && got.sig[where] == kUntouched, "guard: status -1, nothing written");
    for (int64_t i = 0; i < b.segs(); ++i)
      if (i != where) EXPECT(got.status[i] == 0 && got.sig[i] == want.sig[i], "guard: the neighbours are intact");
  }
}

void check_refusals() {
  Block b = random_block({4, 1, 3}, true, 4, 5);
  const int32_t grp[4] = {0, 1, 2, 3}, bad_grp[4] = {0, 1, 4, 0};
  std::vector<int64_t> sig(3, kUntouched);
  std::vector<int32_t> status(3, 9);
  auto refused = [&](int rc, const char* word) {
    EXPECT(rc == DESCO_EINVAL, word);
    EXPECT(desco::last_error_ref().find("desco_wl_refine") != std::string::npos, "the entry point is named");
    EXPECT(desco::last_error_ref().find(word) != std::string::npos, word);
    for (int i = 0; i < 3; ++i) EXPECT(sig[i] == kUntouched && status[i] == 9, "a refusal wrote something");
    desco::last_error_ref().clear();
  };
  auto call = [&](const int32_t* vr, int slots, const int32_t* g, const int32_t* sp, int64_t segs, int rounds,
                  int64_t* s, int32_t* st) {
    return desco_wl_refine(vr, b.vcol.data(), b.num_rows, slots, g, sp, segs, b.anchor_base, nullptr, rounds, 1, s, nullptr,
                           st);
  };
  const int32_t *vr = b.vrowptr.data(), *sp = b.seg_ptr.data();
  refused(call(vr, 0, grp, sp, 3, 8, sig.data(), status.data()), "slots");
  refused(call(vr, 5, grp, sp, 3, 8, sig.data(), status.data()), "slots");
  refused(call(vr, 4, grp, sp, 3, 65, sig.data(), status.data()), "rounds");
  refused(call(vr, 4, grp, sp, 3, -1, sig.data(), status.data()), "rounds");
  refused(call(vr, 4, bad_grp, sp, 3, 8, sig.data(), status.data()), "group entry");
  refused(call(vr, 4, nullptr, sp, 3, 8, sig.data(), status.data()), "group is null");
  refused(call(nullptr, 4, grp, sp, 3, 8, sig.data(), status.data()), "vrowptr is null");
  refused(call(vr, 4, grp, nullptr, 3, 8, sig.data(), status.data()), "seg_ptr is null");
  refused(call(vr, 4, grp, sp, 3, 8, nullptr, status.data()), "sig is null");
  refused(call(vr, 4, grp, sp, 3, 8, sig.data(), nullptr), "status is null");
  refused(call(vr, 4, grp, sp, -1, 8, sig.data(), status.data()), "negative");
  std::vector<int32_t> broken = b.vrowptr;
  broken[5] = broken[4] - 1 < 0 ? 7 : broken[4] - 1;
  if (broken[5] >= broken[4]) broken[6] = broken[5] - 1;
  refused(call(broken.data(), 4, grp, sp, 3, 8, sig.data(), status.data()), "monotone");
  EXPECT(call(vr, 4, grp, sp, 0, 8, nullptr, nullptr) == 0, "an empty call is fine");
  // a segment whose rows or anchor lie outside the block is guarded, not read
  std::vector<int32_t> far = b.seg_ptr;
  far[3] = (int32_t)b.num_rows + 5;
  EXPECT(call(vr, 4, grp, far.data(), 3, 8, sig.data(), status.data()) == 0 && status[2] == -1 && status[0] == 0,
         "a segment past the block");
}

}  // namespace

int main() {
  check_block(random_block({4, 1, 3, 2, 9}, true, 4, 1), "small anchored");
  check_block(random_block({1, 1, 1}, true, 4, 2), "no count rows at all");
  check_block(random_block({5, 1, 8, 33}, false, 4, 3), "unanchored, 4 slots");
  check_block(random_block({6, 10, 3, 1, 17}, false, 2, 4), "whole graphs, 2 slots");
  check_block(random_block({63, 64, 65, 129, 200}, true, 4, 5, 6.0), "larger and denser");
  check_block(random_block({40, 12}, true, 4, 6, 0.2), "sparse: most slots empty");
  check_block(random_block({}, true, 4, 7), "an empty block");
  check_range(random_block({4, 1, 3, 2, 9, 30, 2}, true, 4, 8));
  check_guard();
  check_refusals();
  if (failures) {
    std::printf("%d expectations failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
