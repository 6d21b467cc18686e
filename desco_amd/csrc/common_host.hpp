// Shared error plumbing of libdesco_hip.so (host side).
#pragma once
#include <string>

namespace desco {
std::string& last_error_ref();
int fail(int code, const char* msg);
}  // namespace desco

#if defined(__HIPCC__)
#include <atomic>
#include <cstdint>
#include <hip/hip_runtime.h>
namespace desco {
// "Done once PER DEVICE" flag of size_dynamic_lds below: function attributes belong to the device's code object, and
// one process may drive several devices.
struct DeviceOnce {
  std::atomic<uint64_t> mask{0};
  static int device() {
    int d = 0;
    return hipGetDevice(&d) == hipSuccess && d >= 0 && d < 64 ? d : 0;
  }
  bool done() const { return (mask.load(std::memory_order_relaxed) >> device()) & 1u; }
  void mark() { mask.fetch_or(uint64_t(1) << device(), std::memory_order_relaxed); }
};

// Raise Kernel's dynamic LDS limit to `bytes`, once per device (one flag per kernel: Kernel is a template argument).
// The caller reports a failure as fail((int)e, "<entry point>: cannot size LDS").
template <auto Kernel>
hipError_t size_dynamic_lds(int bytes) {
  static DeviceOnce once;
  if (once.done()) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) once.mark();
  return e;
}

// Compute units of the current device (asked on every call), 256 when the runtime does not say
inline int cu_count() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
    return v;
  return 256;
}
// Grid of a persistent kernel: one block per CU, fewer when there is less work
inline unsigned persistent_grid(int64_t work_items) {
  const int cus = cu_count();
  return (unsigned)(work_items < cus ? work_items : cus);
}

// pointer not aligned for 16-byte (float4) / 8-byte accesses
inline bool mis16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline bool mis8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; }
}  // namespace desco
#endif
