// The several-obstacles form of the one-problem-per-wavefront kernel (k_iterate_obs), compiled in
// its own translation unit (i2lqr_wave_obs.hip): its declaration, the list of its instantiations
// and its launcher.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/i2lqr.h"
#include "i2lqr_devcfg.hpp"
#include "i2lqr_wave.hpp"

namespace i2lqr {

// a.obs is obs[B][n_obs][6]; every iteration tries `steps` step sizes as k_iterate_ls does (1: the
// full step only).
template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_iterate_obs(const DevCfg<T, Sys::n, Sys::m> c,
                                                    const IterArgs<T> a, const int steps,
                                                    const int n_obs);

// The twelve instantiations: three plants x two precisions x with (QR) / without stage weights.
// Expanded here as `extern template`, in i2lqr_wave_obs.hip as the instantiations: a unit that
// launches one of them does not compile it again, and one missing from that unit fails the link.
#define I2LQR_WAVE_OBS_KERNELS_(DECL, REAL, SYS, N_, M_)                                           \
  DECL void k_iterate_obs<REAL, SYS<REAL>, false>(const DevCfg<REAL, N_, M_>,                      \
                                                  const IterArgs<REAL>, const int, const int);     \
  DECL void k_iterate_obs<REAL, SYS<REAL>, true>(const DevCfg<REAL, N_, M_>, const IterArgs<REAL>, \
                                                 const int, const int);
#define I2LQR_WAVE_OBS_KERNELS(DECL, REAL)                                                         \
  I2LQR_WAVE_OBS_KERNELS_(DECL, REAL, Bicycle4, 4, 2)                                              \
  I2LQR_WAVE_OBS_KERNELS_(DECL, REAL, Bicycle6, 6, 2)                                              \
  I2LQR_WAVE_OBS_KERNELS_(DECL, REAL, Quad12, 12, 4)

I2LQR_WAVE_OBS_KERNELS(extern template __global__, double)
I2LQR_WAVE_OBS_KERNELS(extern template __global__, float)

// LDS the records of one problem take behind its slice
inline size_t wave_obs_lds_bytes(int n_obs, size_t word) { return (size_t)n_obs * 6 * word; }

// Enqueue k_iterate_obs for a.B problems (problem-major layout; the three plants, both precisions,
// with or without stage weights).  n_obs: 2 ... I2LQR_MAX_OBSTACLES records per problem, a.obs
// holding a.B * n_obs * 6 words (or NULL: no obstacle).  steps: 1, or the line search's 2, 4 or 8.
// lds: the handle's LDS bytes per wavefront (Layout<Sys>(N).total words); the launch takes
// wave_obs_lds_bytes(n_obs, sizeof(T)) more for the records, and the caller has checked that the sum
// fits the device.
// Returns hipSuccess or the HIP error of the attribute call / launch.
template <class T> hipError_t wave_obs_iterate(const i2lqr_config& cfg, const IterArgs<T>& a,
                                               int steps, int n_obs, size_t lds, hipStream_t stream);

}  // namespace i2lqr
