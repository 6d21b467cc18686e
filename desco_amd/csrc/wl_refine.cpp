// Host twin of wl_refine_dev.hip (C ABI: desco_wl_refine), see include/desco_hip.h, "COLOUR REFINEMENT".
//
// 1-WL colour refinement of every segment of a typed CSR block, OpenMP over segments.  A segment keeps two colour
// vectors (its rows, then its anchor) and ping-pongs between them; the hash chain (wl_refine.hpp) adds modulo 2^64, so
// this sequential walk and the kernel's lanes return the same integers.
#include <cstdint>
#include <new>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/desco_hip.h"
#include "common_host.hpp"
#include "wl_refine.hpp"

namespace {

using desco::wl::message;

struct Block {
  const int32_t* vrowptr;
  const int32_t* vcol;
  int64_t num_rows;
  int slots;
  int group[desco::wl::kMaxSlots];
  const int32_t* seg_ptr;
  int64_t anchor_base;
  const int64_t* init;
  int rounds;
};

// one segment; false = it breaks the guard (nothing may be written for it)
bool refine_segment(const Block& b, int64_t i, std::vector<uint64_t>& cur, std::vector<uint64_t>& next, int64_t* sig,
                    int64_t* colours) {
  const int64_t s0 = b.seg_ptr[i], s1 = b.seg_ptr[i + 1], n = s1 - s0;
  const int64_t a = b.anchor_base >= 0 ? b.anchor_base + i : -1;
  if (s0 < 0 || n < 0 || s1 > b.num_rows) return false;
  if (a >= 0 && (a >= b.num_rows || (a >= s0 && a < s1))) return false;
  const int64_t nloc = n + (a >= 0);
  auto row_of = [&](int64_t l) { return l < n ? s0 + l : a; };
  for (int64_t l = 0; l < nloc; ++l) {                    // the guard: every entry stays inside the segment
    const int64_t r = row_of(l);
    for (int64_t e = b.vrowptr[r * b.slots]; e < b.vrowptr[(r + 1) * b.slots]; ++e) {
      const int64_t c = b.vcol[e];
      if (!((c >= s0 && c < s1) || c == a)) return false;
    }
  }
  cur.resize((size_t)nloc), next.resize((size_t)nloc);
  for (int64_t l = 0; l < nloc; ++l) {
    const int64_t r = row_of(l);
    cur[l] = b.init ? (uint64_t)b.init[r] : (uint64_t)(r == a);
  }
  for (int t = 0; t < b.rounds; ++t) {
    for (int64_t l = 0; l < nloc; ++l) {
      const int64_t r = row_of(l);
      uint64_t ms[desco::wl::kMaxSlots] = {0, 0, 0, 0};
      for (int s = 0; s < b.slots; ++s)
        for (int64_t e = b.vrowptr[r * b.slots + s]; e < b.vrowptr[r * b.slots + s + 1]; ++e) {
          const int64_t c = b.vcol[e];
          ms[s] += message(cur[c == a ? n : c - s0]);
        }
      next[l] = desco::wl::update(cur[l], ms, b.group, b.slots);
    }
    cur.swap(next);
  }
  uint64_t pool = 0;
  for (int64_t l = 0; l < n; ++l) pool += message(cur[l]);
  sig[i] = (int64_t)desco::wl::signature(a >= 0, a >= 0 ? cur[n] : 0, pool);
  if (colours)
    for (int64_t l = 0; l < nloc; ++l) colours[row_of(l)] = (int64_t)cur[l];
  return true;
}

}  // namespace

extern "C" int desco_wl_refine(const int32_t* vrowptr, const int32_t* vcol, int64_t num_rows, int slots,
                               const int32_t* group, const int32_t* seg_ptr, int64_t num_segs, int64_t anchor_base,
                               const int64_t* init, int rounds, int num_threads, int64_t* sig, int64_t* colours,
                               int32_t* status) {
  if (slots < 1 || slots > desco::wl::kMaxSlots)
    return desco::fail(DESCO_EINVAL, "desco_wl_refine: slots is outside 1..4");
  if (rounds < 0 || rounds > DESCO_WL_MAX_ROUNDS)
    return desco::fail(DESCO_EINVAL, "desco_wl_refine: rounds is outside 0..64 (DESCO_WL_MAX_ROUNDS)");
  if (num_rows < 0 || num_segs < 0) return desco::fail(DESCO_EINVAL, "desco_wl_refine: negative num_rows or num_segs");
  if (!group) return desco::fail(DESCO_EINVAL, "desco_wl_refine: group is null");
  for (int s = 0; s < slots; ++s)
    if (group[s] < 0 || group[s] >= slots)
      return desco::fail(DESCO_EINVAL, "desco_wl_refine: a group entry is outside 0..slots-1");
  if (num_segs == 0) return 0;
  if (!vrowptr) return desco::fail(DESCO_EINVAL, "desco_wl_refine: vrowptr is null");
  if (!seg_ptr) return desco::fail(DESCO_EINVAL, "desco_wl_refine: seg_ptr is null");
  if (!sig) return desco::fail(DESCO_EINVAL, "desco_wl_refine: sig is null");
  if (!status) return desco::fail(DESCO_EINVAL, "desco_wl_refine: status is null");
  if (num_rows * slots + 1 > INT32_MAX) return desco::fail(DESCO_EINVAL, "desco_wl_refine: more than 2^31 - 1 virtual rows");
  if (vrowptr[0] != 0) return desco::fail(DESCO_EINVAL, "desco_wl_refine: vrowptr does not start at 0");
  for (int64_t v = 0; v < num_rows * slots; ++v)     // (before any row is read: monotone offsets end within vcol's E)
    if (vrowptr[v + 1] < vrowptr[v]) return desco::fail(DESCO_EINVAL, "desco_wl_refine: vrowptr is not monotone");
  if (vrowptr[num_rows * slots] > 0 && !vcol) return desco::fail(DESCO_EINVAL, "desco_wl_refine: vcol is null");

  Block b;
  b.vrowptr = vrowptr, b.vcol = vcol, b.num_rows = num_rows, b.slots = slots, b.seg_ptr = seg_ptr;
  b.anchor_base = anchor_base < 0 ? -1 : anchor_base, b.init = init, b.rounds = rounds;
  for (int s = 0; s < desco::wl::kMaxSlots; ++s) b.group[s] = s < slots ? group[s] : 0;
  int nt = 1;
#ifdef _OPENMP
  nt = num_threads > 0 ? num_threads : omp_get_max_threads();
#endif
  (void)num_threads;
  bool no_memory = false;
#ifdef _OPENMP
#pragma omp parallel num_threads(nt)
#endif
  {
    std::vector<uint64_t> cur, next;
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 64)
#endif
    for (int64_t i = 0; i < num_segs; ++i) {
      try {
        status[i] = refine_segment(b, i, cur, next, sig, colours) ? 0 : -1;
      } catch (const std::bad_alloc&) {
#ifdef _OPENMP
#pragma omp atomic write
#endif
        no_memory = true;
      }
    }
  }
  if (no_memory) return desco::fail(DESCO_ENOMEM, "desco_wl_refine: out of memory for a segment's colours");
  return 0;
}
