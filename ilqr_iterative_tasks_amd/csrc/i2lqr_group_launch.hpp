// Host-side helpers shared by the translation units that launch the eight- / sixteen-lane kernels
// (i2lqr_group.hip, i2lqr_group_fixed.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "i2lqr_geometry.hpp"
#include "i2lqr_group.hpp"

namespace i2lqr {

template <class T, class Sys, int G = kGroup> size_t group_lds_bytes(int N) {
  return (size_t)GLayout<Sys, G>(N).wave_words() * sizeof(T);
}

// Launches with more than 64 KiB of dynamic LDS need the kernel's attribute raised — per kernel
// AND per device (a second GPU used from the same thread has its own copy of the attribute):
// once per (kernel, device, size).
template <auto Kernel> hipError_t raise_lds_limit(size_t lds) {
  if (lds <= device_geometry().default_dyn_lds) return hipSuccess;
  constexpr int kMaxDev = 64;
  static thread_local int raised_for[kMaxDev] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= kMaxDev || raised_for[dev] < (int)lds) {
    e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < kMaxDev) raised_for[dev] = (int)lds;
  }
  return hipSuccess;
}

}  // namespace i2lqr
