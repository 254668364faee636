// drag_launch.h — the two facts about the device that the host side of a launch needs, each stated once: how many CUs the current device
// has, and the permission a kernel needs before it may take more dynamic LDS than the default limit.  Host-only; any .hip that needs one
// of them includes this header (the function-local statics of inline functions and templates are one object per library, not per source).
#pragma once
#include "drag_common.h"

// multiprocessors of the CURRENT device (256 when the runtime cannot tell), cached per device.  Callers round as they need: a multiple
// of the 8 XCDs for persistent grids, an eighth of it for per-XCD slots.
inline int drag_cu_count() {
  static int cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

template <class Args>
Args drag_kernel_args(void (*)(Args));      // (declaration only: the argument struct of a one-argument kernel)

// Launch Kernel(p).  More dynamic LDS than the default limit of 64 KiB has to be allowed once per device and kernel: the attribute belongs
// to the device's copy of the kernel, so what has been allowed is kept per device (the bytes, not a flag: a kernel whose LDS grows with
// its problem — the top-k scan with the embedding width — asks again when a launch needs more than the last permission covered).
// Launches at or under the limit make no attribute call.  Returns 0, or non-zero with the library error set.
template <auto Kernel>
int drag_launch(dim3 grid, int block, int lds_bytes, hipStream_t st, const decltype(drag_kernel_args(Kernel))& p) {
  if (lds_bytes > 64 * 1024) {
    static int allowed[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (lds_bytes > allowed[dev & 63]) {
      DRAG_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) == hipSuccess,
                 "drag_launch: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: the kernel's dynamic LDS was not allowed");
      allowed[dev & 63] = lds_bytes;
    }
  }
  hipLaunchKernelGGL(Kernel, grid, dim3(block), lds_bytes, st, p);
  DRAG_LAUNCH_CHECK();
  return 0;
}
