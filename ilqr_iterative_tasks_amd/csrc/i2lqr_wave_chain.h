// The chained form of the one-problem-per-wavefront kernel with a state box (k_chain_box), compiled
// in its own translation unit (i2lqr_wave_chain.hip): its declaration, the list of its
// instantiations and its launcher.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/i2lqr.h"
#include "i2lqr_devcfg.hpp"
#include "i2lqr_wave.hpp"
#include "i2lqr_wave_box.h"  // BoxCfg, StateBox, wave_box_lds_bytes

namespace i2lqr {

// a.B chains of a.chain_len problems each, stored chain after chain; one wavefront solves the
// problems of its chain one after the other as k_iterate_box solves one (to termination:
// a.early_exit = 1, a.n_iters = max_iter).  lamb is read from a.lamb[] for the first problem of a
// chain only, carried in a register to the next one, and written to a.lamb[] for every problem.
template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_chain_box(const DevCfg<T, Sys::n, Sys::m> c,
                                                  const IterArgs<T> a, const int steps,
                                                  const int n_obs, const BoxCfg<T, Sys::n> box);

// The twelve instantiations: three plants x two precisions x with (QR) / without stage weights.
// Expanded here as `extern template`, in i2lqr_wave_chain.hip as the instantiations (as
// I2LQR_WAVE_BOX_KERNELS).
#define I2LQR_WAVE_CHAIN_KERNELS_(DECL, REAL, SYS, N_, M_)                                         \
  DECL void k_chain_box<REAL, SYS<REAL>, false>(const DevCfg<REAL, N_, M_>, const IterArgs<REAL>,  \
                                                const int, const int, const BoxCfg<REAL, N_>);     \
  DECL void k_chain_box<REAL, SYS<REAL>, true>(const DevCfg<REAL, N_, M_>, const IterArgs<REAL>,   \
                                               const int, const int, const BoxCfg<REAL, N_>);
#define I2LQR_WAVE_CHAIN_KERNELS(DECL, REAL)                                                       \
  I2LQR_WAVE_CHAIN_KERNELS_(DECL, REAL, Bicycle4, 4, 2)                                            \
  I2LQR_WAVE_CHAIN_KERNELS_(DECL, REAL, Bicycle6, 6, 2)                                            \
  I2LQR_WAVE_CHAIN_KERNELS_(DECL, REAL, Quad12, 12, 4)

I2LQR_WAVE_CHAIN_KERNELS(extern template __global__, double)
I2LQR_WAVE_CHAIN_KERNELS(extern template __global__, float)

// Enqueue k_chain_box for a.B chains of a.chain_len problems (problem-major layout; the three
// plants, both precisions, with or without stage weights); a's arrays hold a.B * a.chain_len
// problems.  n_obs, steps, box, lds: as wave_box_iterate takes them (a box that is off, n_obs = 1
// and steps = 1 give k_iterate's numbers); the launch takes
// lds + wave_box_lds_bytes(n_obs, n, N, sizeof(T)) bytes of LDS, and the caller has checked that
// the sum fits the device.
// Returns hipSuccess or the HIP error of the attribute call / launch.
template <class T> hipError_t wave_chain_solve(const i2lqr_config& cfg, const IterArgs<T>& a,
                                               int steps, int n_obs, const StateBox& box, size_t lds,
                                               hipStream_t stream);

}  // namespace i2lqr
