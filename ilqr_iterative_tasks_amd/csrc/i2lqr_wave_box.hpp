// BoxWorker: ObsWorker (i2lqr_wave_obs.hpp) with the state box's prep.  Shared by the two units that
// build on it: i2lqr_wave_box.hip (k_iterate_box: one problem per wavefront) and
// i2lqr_wave_chain.hip (k_chain_box: a chain of problems per wavefront).
#pragma once
#include "i2lqr_wave_opt.h"  // BoxCfg
#include "i2lqr_wave_obs.hpp"  // ObsWorker: LsWorker with the records' prep

namespace i2lqr {

template <class T, class Sys, bool HASQR> struct BoxWorker : ObsWorker<T, Sys, HASQR> {
  using Obs = ObsWorker<T, Sys, HASQR>;
  using Base = typename Obs::Base;
  static constexpr int n = Sys::n, m = Sys::m;
  using Base::N;
  using Base::S;
  using Base::sl;

  __device__ BoxWorker(const typename Base::Cfg& c_, T* smem, int lane) : Obs(c_, smem, lane) {}

  // once per kernel: the bounds into LDS behind d1, d2 (lo[n], hi[n]).  A lane-dependent index
  // into the by-value argument compiles to a vector load from the kernel-argument segment - host
  // memory, several microseconds - in every prep_box; here every lane stores the uniform values.
  __device__ __forceinline__ void stage_box(const BoxCfg<T, n>& b, T* bx) const {
    T* bl = bx + 2 * (N + 1) * n;
#pragma unroll
    for (int i = 0; i < n; i++) {
      bl[i] = b.lo[i];
      bl[n + i] = b.hi[i];
    }
  }

  // d1, d2 of every (t, i), t = 0 ... N (index N is the terminal term): pair p = t n + i is word p
  // of the trajectory and of each of the two arrays behind bx.  An unbounded side is masked out (its
  // bound is stored as 0: the exponential of a finite number, dropped by the select).  No
  // wave_sync: the caller's prep_obs ends with one.
  __device__ __forceinline__ void prep_box(int Xo, const BoxCfg<T, n>& b, T* bx) const {
    const int P = (N + 1) * n;
    const T* bl = bx + 2 * P;
    for (int p = sl; p < P; p += 64) {
      const int i = p % n;
      const T x = S[Xo + p];
      const T e_hi = t_exp(b.q2 * (x - bl[n + i]));
      const T e_lo = t_exp(b.q2 * (bl[i] - x));
      const T eh = ((b.m_hi >> i) & 1u) ? e_hi : T(0);
      const T el = ((b.m_lo >> i) & 1u) ? e_lo : T(0);
      bx[p] = b.q12 * (eh - el);
      bx[P + p] = b.q122 * (eh + el);
    }
  }
};

}  // namespace i2lqr
