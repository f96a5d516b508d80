// The opt-in forms of the one-problem-per-wavefront kernel - k_iterate_ls, k_iterate_obs,
// k_iterate_box, k_iterate_merit and the chained k_chain_box, each compiled in a translation unit of
// its own (i2lqr_wave_ls.hip, i2lqr_wave_obs.hip, i2lqr_wave_box.hip, i2lqr_wave_merit.hip,
// i2lqr_wave_chain.hip): their
// declarations, the one list of their instantiations and their one launcher (i2lqr_wave_opt.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/i2lqr.h"
#include "i2lqr_wave.hpp"
#include "i2lqr_wave_model.hpp"

namespace i2lqr {

// The box as the kernel takes it, by value: bounds (0 where the side is unbounded: no arithmetic
// is done on infinities, the masks say which sides count), q1 q2, q1 q2^2, q2 and the two n-bit
// masks of the finite sides.
template <class T, int n> struct BoxCfg {
  T lo[n], hi[n];
  T q12, q122, q2;
  unsigned m_lo, m_hi;
};

// The handle's box in the kernel's precision: the one place q12, q122 and the masks are formed.
template <class T, int n> inline BoxCfg<T, n> make_box_cfg(const StateBox& box) {
  BoxCfg<T, n> b;
  for (int i = 0; i < n; i++) {
    b.lo[i] = (T)box.lo[i];
    b.hi[i] = (T)box.hi[i];
  }
  const T q1 = (T)box.q1;
  b.q2 = (T)box.q2;
  b.q12 = q1 * b.q2;  // (as make_dev_cfg forms ctrl_q12 / ctrl_q122)
  b.q122 = q1 * (b.q2 * b.q2);
  b.m_lo = box.m_lo & ((1u << n) - 1);
  b.m_hi = box.m_hi & ((1u << n) - 1);
  return b;
}

// k_iterate with a parallel line search: every iteration tries the `steps` step sizes 2^-j,
// j = 0 ... steps - 1 (2, 4 or 8), on lane groups of the wavefront and continues with the cheapest.
template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_iterate_ls(const DevCfg<T, Sys::n, Sys::m> c,
                                                   const IterArgs<T> a, const int steps);

// a.obs is obs[B][n_obs][6] (n_obs: 1 ... I2LQR_MAX_OBSTACLES; a.obs NULL: no obstacle); every
// iteration tries `steps` step sizes as k_iterate_ls does (1: the full step only).
template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_iterate_obs(const DevCfg<T, Sys::n, Sys::m> c,
                                                    const IterArgs<T> a, const int steps,
                                                    const int n_obs);

// k_iterate_obs with the exponential barrier of the box on every state x_t, t = 0 ... N, in the
// backward pass's derivatives.
template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_iterate_box(const DevCfg<T, Sys::n, Sys::m> c,
                                                    const IterArgs<T> a, const int steps,
                                                    const int n_obs, const BoxCfg<T, Sys::n> box);

// k_iterate_box whose line search, accept / reject and convergence test see the merit J = c + P: the
// barrier-free cost plus the barriers of the inputs, the records and the box ("barrier_cost",
// include/i2lqr.h); box_q1: the box's q1 (BoxCfg carries its products only).  a.cost returns J.
template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_iterate_merit(const DevCfg<T, Sys::n, Sys::m> c,
                                                      const IterArgs<T> a, const int steps,
                                                      const int n_obs, const BoxCfg<T, Sys::n> box,
                                                      const T box_q1);

// a.B chains of a.chain_len problems each, stored chain after chain; one wavefront solves the
// problems of its chain one after the other as k_iterate_box solves one (to termination:
// a.early_exit = 1, a.n_iters = max_iter).  lamb is read from a.lamb[] for the first problem of a
// chain only, carried in a register to the next one, and written to a.lamb[] for every problem.
// A box that is off, n_obs = 1 and steps = 1 give k_iterate's numbers.
template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_chain_box(const DevCfg<T, Sys::n, Sys::m> c,
                                                  const IterArgs<T> a, const int steps,
                                                  const int n_obs, const BoxCfg<T, Sys::n> box);

// The twelve instantiations of KERNEL: three plants x two precisions x with (true) / without stage
// weights; TAIL(REAL, N_) spells the parameter types that follow DevCfg and IterArgs.  Expanded
// here as `extern template`, in the kernel's unit as the instantiations: a unit that launches one
// of them does not compile it again, and one missing from its unit fails the link.
#define I2LQR_WAVE_TAIL_LS(REAL, N_) const int
#define I2LQR_WAVE_TAIL_OBS(REAL, N_) const int, const int
#define I2LQR_WAVE_TAIL_BOX(REAL, N_) const int, const int, const BoxCfg<REAL, N_>
#define I2LQR_WAVE_TAIL_MERIT(REAL, N_) const int, const int, const BoxCfg<REAL, N_>, const REAL
#define I2LQR_WAVE_OPT_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_)                             \
  DECL void KERNEL<REAL, SYS<REAL>, false>(const DevCfg<REAL, N_, M_>, const IterArgs<REAL>,       \
                                           TAIL(REAL, N_));                                        \
  DECL void KERNEL<REAL, SYS<REAL>, true>(const DevCfg<REAL, N_, M_>, const IterArgs<REAL>,        \
                                          TAIL(REAL, N_));
#define I2LQR_WAVE_OPT_KERNELS(DECL, KERNEL, TAIL)                                                 \
  I2LQR_WAVE_OPT_KERNELS_(DECL, KERNEL, TAIL, double, Bicycle4, 4, 2)                              \
  I2LQR_WAVE_OPT_KERNELS_(DECL, KERNEL, TAIL, double, Bicycle6, 6, 2)                              \
  I2LQR_WAVE_OPT_KERNELS_(DECL, KERNEL, TAIL, double, Quad12, 12, 4)                               \
  I2LQR_WAVE_OPT_KERNELS_(DECL, KERNEL, TAIL, float, Bicycle4, 4, 2)                               \
  I2LQR_WAVE_OPT_KERNELS_(DECL, KERNEL, TAIL, float, Bicycle6, 6, 2)                               \
  I2LQR_WAVE_OPT_KERNELS_(DECL, KERNEL, TAIL, float, Quad12, 12, 4)

I2LQR_WAVE_OPT_KERNELS(extern template __global__, k_iterate_ls, I2LQR_WAVE_TAIL_LS)
I2LQR_WAVE_OPT_KERNELS(extern template __global__, k_iterate_obs, I2LQR_WAVE_TAIL_OBS)
I2LQR_WAVE_OPT_KERNELS(extern template __global__, k_iterate_box, I2LQR_WAVE_TAIL_BOX)
I2LQR_WAVE_OPT_KERNELS(extern template __global__, k_iterate_merit, I2LQR_WAVE_TAIL_MERIT)
I2LQR_WAVE_OPT_KERNELS(extern template __global__, k_chain_box, I2LQR_WAVE_TAIL_BOX)

// Enqueue the form model.form(chained) for a.B problems - chained: a.B chains of a.chain_len
// problems, a's arrays holding a.B * a.chain_len of them - in the problem-major layout (the three
// plants, both precisions, with or without stage weights).  The kernel is given model.steps() step
// sizes, model.records() records per problem (a.obs holding that many times six words per problem,
// or NULL: no obstacle) and model.box.  lds: the handle's LDS bytes per wavefront
// (Layout<Sys>(N).total words); the launch takes model.extra_lds_bytes(form, n, N, sizeof(T)) more,
// and the caller has checked that the sum fits the device.
// Returns hipSuccess or the HIP error of the attribute call / launch; hipErrorInvalidValue for a
// model that is off (k_iterate's launch is the caller's).
template <class T> hipError_t wave_opt_launch(const i2lqr_config& cfg, const IterArgs<T>& a,
                                              const WaveModel& model, bool chained, size_t lds,
                                              hipStream_t stream);

}  // namespace i2lqr
