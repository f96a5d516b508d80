// The state-box form of the one-problem-per-wavefront kernel (k_iterate_box), compiled in its own
// translation unit (i2lqr_wave_box.hip): its declaration, the list of its instantiations and its
// launcher.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/i2lqr.h"
#include "i2lqr_devcfg.hpp"
#include "i2lqr_wave.hpp"

namespace i2lqr {

// The box as the kernel takes it, by value: bounds (0 where the side is unbounded: no arithmetic
// is done on infinities, the masks say which sides count), q1 q2, q1 q2^2, q2 and the two n-bit
// masks of the finite sides.
template <class T, int n> struct BoxCfg {
  T lo[n], hi[n];
  T q12, q122, q2;
  unsigned m_lo, m_hi;
};

// The box as the handle keeps it (i2lqr_set_state_box): doubles, converted by the launcher.
struct StateBox {
  double lo[I2LQR_MAX_N] = {}, hi[I2LQR_MAX_N] = {};  // 0 where the side is unbounded
  double q1 = 1.0, q2 = 1.0;
  unsigned m_lo = 0, m_hi = 0;  // bit i: lo[i] / hi[i] is finite
  bool on() const { return (m_lo | m_hi) != 0; }
};

// k_iterate_obs (a.obs is obs[B][n_obs][6], `steps` step sizes per iteration) with the exponential
// barrier of the box on every state x_t, t = 0 ... N, in the backward pass's derivatives.
template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_iterate_box(const DevCfg<T, Sys::n, Sys::m> c,
                                                    const IterArgs<T> a, const int steps,
                                                    const int n_obs, const BoxCfg<T, Sys::n> box);

// The twelve instantiations: three plants x two precisions x with (QR) / without stage weights.
// Expanded here as `extern template`, in i2lqr_wave_box.hip as the instantiations: a unit that
// launches one of them does not compile it again, and one missing from that unit fails the link.
#define I2LQR_WAVE_BOX_KERNELS_(DECL, REAL, SYS, N_, M_)                                           \
  DECL void k_iterate_box<REAL, SYS<REAL>, false>(const DevCfg<REAL, N_, M_>,                      \
                                                  const IterArgs<REAL>, const int, const int,      \
                                                  const BoxCfg<REAL, N_>);                         \
  DECL void k_iterate_box<REAL, SYS<REAL>, true>(const DevCfg<REAL, N_, M_>, const IterArgs<REAL>, \
                                                 const int, const int, const BoxCfg<REAL, N_>);
#define I2LQR_WAVE_BOX_KERNELS(DECL, REAL)                                                         \
  I2LQR_WAVE_BOX_KERNELS_(DECL, REAL, Bicycle4, 4, 2)                                              \
  I2LQR_WAVE_BOX_KERNELS_(DECL, REAL, Bicycle6, 6, 2)                                              \
  I2LQR_WAVE_BOX_KERNELS_(DECL, REAL, Quad12, 12, 4)

I2LQR_WAVE_BOX_KERNELS(extern template __global__, double)
I2LQR_WAVE_BOX_KERNELS(extern template __global__, float)

// LDS one problem takes behind its slice: the obstacle records (wave_obs_lds_bytes) and, behind
// them, d1[N+1][n], d2[N+1][n] and the bounds lo[n], hi[n]
inline size_t wave_box_lds_bytes(int n_obs, int n, int N, size_t word) {
  return ((size_t)n_obs * 6 + (size_t)2 * n * (N + 1) + (size_t)2 * n) * word;
}

// Enqueue k_iterate_box for a.B problems (problem-major layout; the three plants, both precisions,
// with or without stage weights).  n_obs: 1 ... I2LQR_MAX_OBSTACLES records per problem, a.obs
// holding a.B * n_obs * 6 words (or NULL: no obstacle).  steps: 1, or the line search's 2, 4 or 8.
// lds: the handle's LDS bytes per wavefront (Layout<Sys>(N).total words); the launch takes
// wave_box_lds_bytes(n_obs, n, N, sizeof(T)) more, and the caller has checked that the sum fits the
// device.
// Returns hipSuccess or the HIP error of the attribute call / launch.
template <class T> hipError_t wave_box_iterate(const i2lqr_config& cfg, const IterArgs<T>& a,
                                               int steps, int n_obs, const StateBox& box, size_t lds,
                                               hipStream_t stream);

}  // namespace i2lqr
