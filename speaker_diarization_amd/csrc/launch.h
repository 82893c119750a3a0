// Host-side launch setup shared by the kernel launchers: the current device's CU count and the opt-in to more
// than 64 KiB of dynamic LDS.  Both are cached per device id and safe under concurrent first calls.
#pragma once
#include <atomic>

#include "common.h"

namespace sd {

constexpr int kMaxDevices = 64;   // one bit per device in a kernel's opt-in mask

inline int current_device() {
  int dev = 0;
  SD_HIP(hipGetDevice(&dev));
  SD_CHECK(dev >= 0 && dev < kMaxDevices, kErrHip, "device id out of range");
  return dev;
}

// Compute units of the current device.
inline int device_cus() {
  static std::atomic<int> cus[kMaxDevices];   // 0: not read yet
  const int dev = current_device();
  int n = cus[dev].load(std::memory_order_relaxed);
  if (!n) {
    SD_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

inline void set_dynamic_lds(const void* kernel, int bytes) {
  SD_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
}

// allow_dynamic_lds<&kernel, ...>(bytes): lets the kernels be launched with up to `bytes` of dynamic LDS on the
// current device.  hipFuncSetAttribute runs once per (kernel, device); a thread returns only after the attribute
// is set (by it or by another thread), so the launch that follows is always covered.  Kernels named together are
// opted in together, on the first call.
template <auto*... Kernels>
inline void allow_dynamic_lds(int bytes) {
  static std::atomic<uint64_t> opted{0};   // devices done, per instantiation
  const uint64_t bit = 1ull << current_device();
  if (opted.load(std::memory_order_acquire) & bit) return;
  (set_dynamic_lds(reinterpret_cast<const void*>(Kernels), bytes), ...);
  opted.fetch_or(bit, std::memory_order_release);
}

}  // namespace sd
