// Device side of the colour refinement (C ABI: desco_wl_refine_dev), see include/desco_hip.h, "COLOUR REFINEMENT".
// Equal to the host twin (wl_refine.cpp) bit for bit: every sum of the hash chain (wl_refine.hpp) is an addition
// modulo 2^64, so the order in which lanes and waves add does not matter.
//
// Segments never reference each other, so ALL rounds and the signature of a segment run in one launch with no
// grid-wide step: one wave per segment (THREADS = 64) where the launch's bound is at most DESCO_WL_WAVE_ROWS rows, one
// workgroup of four waves above it.  The owner keeps both colour buffers of its segment in LDS,
//
//   bytes 0 .. 63        four wave partials of the signature's pool, the guard flag
//   buf0 [rows]          uint64 colours; local row l = segment row s0 + l, the anchor last
//   buf1 [rows]          (from the next 16-byte boundary)
//
// and ping-pongs between them; a barrier of the owner separates the rounds.  Global traffic is the segment's CSR -- once
// for the guard and once per round, the rounds' reads coming out of L2 -- and 8 bytes of signature out.
//
//   guard   every thread strides over the segment's two flat entry ranges (its rows' and its anchor's): an entry may
//           name only a row of the segment or its anchor.  A bad segment gets status -1 and nothing else; nothing has
//           indexed LDS with an entry by then.  The row pointers are checked first (monotone, inside [0, E]).
//   round   lane per row: the row's entries slot by slot, each message mix(c[src] + G) read from LDS.  A row of more
//           than kLongRow entries (the anchor of a dense neighborhood, the centre of a star) is left out of that walk
//           and then taken by the whole wave, 64 entries a step, with a shuffle reduction per slot.
//   pool    lane partials, a shuffle reduction per wave, the wave partials through LDS.
//
// Every LDS index is below the segment's rows by construction: the guard has seen every entry the rounds read.
#include "common_device.hpp"
#include "wl_refine.hpp"

namespace desco {

struct WlArgs {
  const int32_t* vrowptr;     // [slots * num_rows + 1]
  const int32_t* vcol;        // [E]
  const int32_t* seg_ptr;     // [num_segs + 1]
  const int64_t* init;        // [num_rows] or null
  const int64_t* seg_ids;     // [num_ids] the segments of this launch, or null: all of them
  int64_t num_rows, num_segs, anchor_base;
  int64_t max_rows;           // the launch's bound on a segment's rows, anchor included
  int64_t ws_rows;            // rows per colour buffer of the launch: max_rows rounded up to even
  int slots, rounds;
  int group[wl::kMaxSlots];
  int64_t* sig;               // [num_segs]
  int64_t* colours;           // [num_rows] or null
  int32_t* status;            // [num_segs]
};

constexpr int kLongRow = 64;   // entries above which a row is walked by its whole wave

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, kWave);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, kWave);
    v += (uint64_t)hi << 32 | lo;
  }
  return v;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void wl_refine_kernel(WlArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint64_t wl_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t i = p.seg_ids ? p.seg_ids[blockIdx.x] : (int64_t)blockIdx.x;
  if (i < 0 || i >= p.num_segs) return;                          // (uniform) a bad id: nothing to write to
  int32_t* __restrict__ status = p.status + i;
  const int slots = p.slots;
  const int64_t s0 = p.seg_ptr[i], s1 = p.seg_ptr[i + 1], n64 = s1 - s0;
  const int64_t a = p.anchor_base >= 0 ? p.anchor_base + i : -1;
  const int64_t nloc64 = n64 + (a >= 0);
  if (s0 < 0 || n64 < 0 || s1 > p.num_rows || (a >= 0 && (a >= p.num_rows || (a >= s0 && a < s1))) ||
      nloc64 > p.max_rows) {
    if (tid == 0) *status = -1;                                  // (uniform) not this launch's: no LDS is touched
    return;
  }
  const int n = (int)n64, nloc = (int)nloc64;
  uint64_t* part = wl_lds;                                       // [4]
  int& sh_bad = reinterpret_cast<int*>(wl_lds + 4)[0];
  uint64_t* cur = wl_lds + 8;
  uint64_t* next = cur + ((nloc + 1) & ~1);
  const int32_t* __restrict__ vrowptr = p.vrowptr;
  const int32_t* __restrict__ vcol = p.vcol;
  const int64_t E = vrowptr[(int64_t)slots * p.num_rows];

  // ---- guard, initial colours ----------------------------------------------------------------------------------------
  if (tid == 0) sh_bad = 0;
  int bad = E > 0 && !vcol;
  for (int l = tid; l < nloc; l += THREADS) {                    // row pointers: monotone inside [0, E]
    const int64_t r = l < n ? s0 + l : a;
    int64_t o = vrowptr[r * slots];
    bad |= o < 0;
    for (int s = 1; s <= slots; ++s) {
      const int64_t o1 = vrowptr[r * slots + s];
      bad |= o1 < o;
      o = o1;
    }
    bad |= o > E;
    cur[l] = p.init ? (uint64_t)p.init[r] : (uint64_t)(r == a);
  }
  __syncthreads();
  if (bad) sh_bad = 1;
  __syncthreads();
  if (sh_bad) {                                                  // (uniform: an LDS word read behind a barrier)
    if (tid == 0) *status = -1;
    return;
  }
  {
    // the rows' pointers are monotone inside [0, E] by now, so both flat ranges lie inside vcol
    const int64_t c0 = vrowptr[s0 * slots], c1 = vrowptr[s1 * slots];
    for (int64_t e = c0 + tid; e < c1; e += THREADS) {
      const int64_t c = vcol[e];
      bad |= !((c >= s0 && c < s1) || c == a);
    }
    if (a >= 0) {
      const int64_t a0 = vrowptr[a * slots], a1 = vrowptr[(a + 1) * slots];
      for (int64_t e = a0 + tid; e < a1; e += THREADS) {
        const int64_t c = vcol[e];
        bad |= !((c >= s0 && c < s1) || c == a);
      }
    }
  }
  if (bad) sh_bad = 1;
  __syncthreads();
  if (sh_bad) {
    if (tid == 0) *status = -1;
    return;
  }

  // ---- rounds ------------------------------------------------------------------------------------------------------
  const int32_t as0 = (int32_t)s0, aa = (int32_t)a;             // (rows are below 2^31: vrowptr is indexed by int32)
  auto local = [&](int32_t c) { return c == aa ? n : c - as0; };
  for (int t = 0; t < p.rounds; ++t) {
    for (int base = 0; base < nloc; base += THREADS) {           // (uniform trip count: the wave steps stay converged)
      const int l = base + tid;
      const bool active = l < nloc;
      const int64_t r = !active ? 0 : l < n ? s0 + l : a;
      int32_t o[wl::kMaxSlots + 1] = {0, 0, 0, 0, 0};
      int32_t end = 0;
      if (active) {
#pragma unroll
        for (int s = 0; s <= wl::kMaxSlots; ++s)
          if (s <= slots) end = o[s] = vrowptr[r * slots + s];
      }
      const bool is_long = active && end - o[0] > kLongRow;
      uint64_t ms[wl::kMaxSlots] = {0, 0, 0, 0};
      if (active && !is_long) {
#pragma unroll
        for (int s = 0; s < wl::kMaxSlots; ++s)
          if (s < slots)
            for (int32_t e = o[s]; e < o[s + 1]; ++e) ms[s] += wl::message(cur[local(vcol[e])]);
      }
      unsigned long long todo = __ballot(is_long);
      while (todo) {                                             // (wave-uniform)
        const int j = __ffsll(todo) - 1;
        todo &= todo - 1;
#pragma unroll
        for (int s = 0; s < wl::kMaxSlots; ++s) {
          if (s >= slots) break;
          const int32_t e0 = __shfl(o[s], j, kWave), e1 = __shfl(o[s + 1], j, kWave);
          uint64_t m = 0;
          for (int32_t e = e0 + lane; e < e1; e += kWave) m += wl::message(cur[local(vcol[e])]);
          m = wave_sum_u64(m);
          if (lane == j) ms[s] = m;
        }
      }
      if (active) next[l] = wl::update(cur[l], ms, p.group, slots);
    }
    __syncthreads();
    uint64_t* x = cur;
    cur = next, next = x;
  }

  // ---- colours and signature ---------------------------------------------------------------------------------------
  uint64_t pool = 0;
  for (int l = tid; l < nloc; l += THREADS) {
    const uint64_t c = cur[l];
    if (l < n) pool += wl::message(c);
    if (p.colours) p.colours[l < n ? s0 + l : a] = (int64_t)c;
  }
  pool = wave_sum_u64(pool);
  if (lane == 0) part[wave] = pool;
  __syncthreads();
  if (tid == 0) {
    pool = 0;
    for (int w = 0; w < THREADS / kWave; ++w) pool += part[w];
    p.sig[i] = (int64_t)wl::signature(a >= 0, a >= 0 ? cur[n] : 0, pool);
    *status = 0;
  }
}

template <int THREADS>
int launch(const WlArgs& a, int64_t num_ids, hipStream_t stream) {
  const hipError_t e = size_dynamic_lds<wl_refine_kernel<THREADS>>(64 + 16 * DESCO_WL_DEV_MAX_ROWS);
  if (e != hipSuccess) return fail((int)e, "desco_wl_refine_dev: cannot size LDS");
  hipLaunchKernelGGL(wl_refine_kernel<THREADS>, dim3((unsigned)num_ids), dim3(THREADS), (size_t)(64 + 16 * a.ws_rows),
                     stream, a);
  return launch_status("desco_wl_refine_dev");
}

}  // namespace desco

using namespace desco;

extern "C" int desco_wl_refine_dev(const int32_t* vrowptr, const int32_t* vcol, int64_t num_rows, int slots,
                                   const int32_t* group, const int32_t* seg_ptr, int64_t num_segs, int64_t anchor_base,
                                   const int64_t* init, int rounds, const int64_t* seg_ids, int64_t num_ids,
                                   int64_t max_rows, int64_t* sig, int64_t* colours, int32_t* status,
                                   desco_stream_t stream) {
  if (slots < 1 || slots > wl::kMaxSlots) return fail(DESCO_EINVAL, "desco_wl_refine_dev: slots is outside 1..4");
  if (rounds < 0 || rounds > DESCO_WL_MAX_ROUNDS)
    return fail(DESCO_EINVAL, "desco_wl_refine_dev: rounds is outside 0..64 (DESCO_WL_MAX_ROUNDS)");
  if (num_rows < 0 || num_segs < 0 || num_ids < 0)
    return fail(DESCO_EINVAL, "desco_wl_refine_dev: negative num_rows, num_segs or num_ids");
  if (max_rows < 0) return fail(DESCO_EINVAL, "desco_wl_refine_dev: negative max_rows");
  if (!group) return fail(DESCO_EINVAL, "desco_wl_refine_dev: group is null");
  for (int s = 0; s < slots; ++s)
    if (group[s] < 0 || group[s] >= slots)
      return fail(DESCO_EINVAL, "desco_wl_refine_dev: a group entry is outside 0..slots-1");
  if (!seg_ids) num_ids = num_segs;
  if (num_ids == 0) return 0;
  if (max_rows > DESCO_WL_DEV_MAX_ROWS)
    return fail(DESCO_EINVAL,
                "desco_wl_refine_dev: a segment's rows, anchor included, exceed DESCO_WL_DEV_MAX_ROWS (10236); use "
                "desco_wl_refine for it");
  if (num_ids > INT32_MAX) return fail(DESCO_EINVAL, "desco_wl_refine_dev: num_ids is above 2^31 - 1");
  if (num_rows * slots + 1 > INT32_MAX)
    return fail(DESCO_EINVAL, "desco_wl_refine_dev: more than 2^31 - 1 virtual rows");
  if (!vrowptr) return fail(DESCO_EINVAL, "desco_wl_refine_dev: vrowptr is null");
  if (!seg_ptr) return fail(DESCO_EINVAL, "desco_wl_refine_dev: seg_ptr is null");
  if (!sig) return fail(DESCO_EINVAL, "desco_wl_refine_dev: sig is null");
  if (!status) return fail(DESCO_EINVAL, "desco_wl_refine_dev: status is null");
  if (mis8(init) || mis8(seg_ids) || mis8(sig) || mis8(colours))
    return fail(DESCO_EINVAL, "desco_wl_refine_dev: a 64-bit array is not 8-byte aligned");
  WlArgs a;
  a.vrowptr = vrowptr, a.vcol = vcol, a.seg_ptr = seg_ptr, a.init = init, a.seg_ids = seg_ids;
  a.num_rows = num_rows, a.num_segs = num_segs, a.anchor_base = anchor_base < 0 ? -1 : anchor_base;
  a.max_rows = max_rows, a.ws_rows = (max_rows + 1) & ~(int64_t)1;
  a.slots = slots, a.rounds = rounds;
  for (int s = 0; s < wl::kMaxSlots; ++s) a.group[s] = s < slots ? group[s] : 0;
  a.sig = sig, a.colours = colours, a.status = status;
  // one wave per segment where the launch's segments are small (DESCO_WL_WAVE_ROWS), four above
  return max_rows <= DESCO_WL_WAVE_ROWS ? launch<64>(a, num_ids, (hipStream_t)stream)
                                        : launch<256>(a, num_ids, (hipStream_t)stream);
}
