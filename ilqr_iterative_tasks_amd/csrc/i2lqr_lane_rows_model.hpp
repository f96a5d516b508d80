// k_lane_iterate_rows_model: the row-block plants' one-problem-per-lane kernel (quad12,
// k_lane_iterate_rows) with the opt-in models that enter the backward pass's derivatives only —
// several obstacle records per problem and the state box ("lane_rows_models" 1 on top of
// "lane_models" 1, include/i2lqr.h).  It is k_lane_iterate_rows's iteration loop without the chunk
// protocol (a model solve is one launch with early exit) around LaneWorker::backward_blocked with the
// MODEL hook below.  Compiled in units of its own (i2lqr_lane_rows_model_f64.hip, _f32.hip): the
// kernels of the existing quad12 units do not see it.
//
// obs has the bicycles' model layouts, record r's word q in row q K + r:
//     batch-minor  obs[6][K][B]        batch-tiled  obs[B/64][6][K][64]
// Record 0 lives where k_lane_iterate_rows keeps its one record.  Records 1 ... K - 1 are NOT staged:
// the kernel lives on four workgroups per CU and its 40 KB of LDS per wavefront leave no room for 6
// (K - 1) words per lane, so every step reads them from the obs rows where it uses them (coalesced,
// L2-resident after the first step; 6 (K - 1) words against the 52 gain words the step stores) and
// forms the two reciprocals there.  The box is a by-value kernel argument, wave-uniform.  The kernel
// takes no LDS beyond k_lane_iterate_rows's own (lane_rows_model_plan, i2lqr_lane_plan.hpp).
//
// Where the terms enter the step decides whether the step still fits its registers.  The records join
// record 0's five words where the step forms them, so they are parked and added with them; the box
// goes on [Vxx | Vx] at the TOP of the step whose evaluation state x_{t+1} it is evaluated at (one
// site for every step and the terminal block).  Both at the end of the step, where the parked terms
// are added, sent all of [Vxx | Vx] to scratch (+816 bytes per lane in fp64, whichever of the two was
// compiled in); placed as they are the kernels compile with less scratch than k_lane_iterate_rows
// itself (fp64 1380 / 1356 against 1420 / 1428 bytes per lane, fp32 424 / 468 against 616 / 836).
#pragma once
#include <hip/hip_runtime.h>

#include "i2lqr_lane.hpp"
#include "i2lqr_wave_opt.h"  // BoxCfg

namespace i2lqr {

template <class T, int n> struct LaneRowsModelHook {
  static constexpr bool kOn = true;
  const T* gob;  // the wavefront's re-based obs rows; null: no record
  int K;         // records per problem, 1 ... I2LQR_MAX_OBSTACLES (1 with a null obs)
  const BoxCfg<T, n>& box;

  __device__ __forceinline__ bool box_on() const { return (box.m_lo | box.m_hi) != 0; }
  // t_exp with, in fp64, its literals in scalar registers at their point of use (t_exp_d's SLIT form:
  // bit for bit t_exp's values).  Materialised in vector registers they are hoisted out of the horizon
  // loop as invariants and spilled, which is why the row-block pass's own exponentials take this form.
  static __device__ __forceinline__ T exp_at(T x) {
    if constexpr (sizeof(T) == 8) {
      const double xa[1] = {x};
      double ea[1];
      t_exp_d<true, 1, 0>(xa, ea);
      return ea[0];
    } else {
      return t_exp(x);
    }
  }
  // Records 1 ... K - 1 join o[] (record 0's five words; any: record 0 is enabled) in record order,
  // each with LaneWorker::obstacle()'s arithmetic - computed for every lane and selected, as the hot
  // form of record 0: the same values in the hot and the general pass.  A record with moving_option
  // < 0 adds nothing, and the first enabled record's words are taken as they are, not added to zeros
  // (LaneModelHook::more_obstacles, with the records read from the obs rows).  Reads only: the pass
  // stays repeatable.
  template <class W>
  __device__ __forceinline__ void more_obstacles(const W& w, bool any, T px, T py, int t,
                                                 T (&o)[5]) const {
    for (int r = 1; r < K; r++) {
      T rec[6];
#pragma unroll
      for (int q = 0; q < 6; q++) rec[q] = w.at(gob, q * K + r);
      const T pa = T(1) / (rec[2] * rec[2]), pb = T(1) / (rec[3] * rec[3]);
      const bool en = rec[5] >= T(0);
      const int opt = en ? (int)rec[5] : 0;
      const T dy = opt == 1 ? py - (rec[1] + T(t) * rec[4]) : py - rec[1];
      const T dz = opt == 2 ? px - (rec[0] - T(t) * rec[4]) : px - rec[0];
      const T h = T(1) + w.c.safety_margin - (dz * pa * dz + dy * pb * dy);
      const T hd0 = T(-2) * pa * dz, hd1 = T(-2) * pb * dy;
      const T e = exp_at(w.c.obs_q2 * h);
      const T c1 = w.c.obs_q12 * e, c2 = w.c.obs_q122 * e;
      const T oo[5] = {c1 * hd0, c1 * hd1, c2 * (hd0 * hd0), c2 * (hd0 * hd1), c2 * (hd1 * hd1)};
#pragma unroll
      for (int q = 0; q < 5; q++) o[q] = en ? (any ? o[q] + oo[q] : oo[q]) : o[q];
      any = any || en;
    }
  }
  // d1 = q1 q2 (e_hi - e_lo) of the state x on Vx and d2 = q1 q2^2 (e_hi + e_lo) on the diagonal of Vxx,
  // e_hi = exp(q2 (x - hi)), e_lo = exp(q2 (lo - x)); an unbounded side is not computed (wave-uniform
  // masks), a box that is off adds nothing
  __device__ __forceinline__ void box_add(const T (&x)[n], T (&V)[n][n], T (&vx)[n]) const {
    if (box_on()) {
#pragma unroll
      for (int i = 0; i < n; i++) {
        T eh = T(0), el = T(0);
        if ((box.m_hi >> i) & 1u) eh = exp_at(box.q2 * (x[i] - box.hi[i]));
        if ((box.m_lo >> i) & 1u) el = exp_at(box.q2 * (box.lo[i] - x[i]));
        vx[i] += box.q12 * (eh - el);
        V[i][i] += box.q122 * (eh + el);
      }
    }
  }
};

// LaneArgs as k_lane_iterate_rows takes them; count / resume / max_total / cp are not read (the
// launcher leaves them neutral).  Static LDS only: the gain slice and the warm-up sink of
// k_lane_iterate_rows.
// (a copy of k_lane_iterate_rows's loop on purpose: that kernel is the text it was)
template <class T, class Sys, bool HASQR, bool TILED>
__global__ __launch_bounds__(64, 1) void k_lane_iterate_rows_model(const DevCfg<T, Sys::n, Sys::m> c,
                                                                   const LaneArgs<T> a, const int K,
                                                                   const BoxCfg<T, Sys::n> box) {
  constexpr int n = Sys::n, m = Sys::m;
  static_assert(Sys::NBLK > 0, "built for the plants with a row-block form");
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const LaneView<TILED> v(a.B);
  LaneWorker<T, Sys, HASQR, TILED> w(c, v.Bs, v.bl);
  const T* gxt = v.rebase(a.x_term, n);
  const T* gob = v.rebase(a.obs, 6 * K);
  T xT[n], ob[6];
#pragma unroll
  for (int i = 0; i < n; i++) xT[i] = gxt[(int64_t)i * v.Bs + v.bl];
  // a NULL obs disables every record (finite placeholders for record 0, as k_lane_iterate_rows's)
#pragma unroll
  for (int q = 0; q < 6; q++)
    ob[q] = gob ? gob[(int64_t)(q * K) * v.Bs + v.bl] : T(q == 5 ? -1 : 1);
  using Hook = LaneRowsModelHook<T, n>;
  const Hook mdl{gob, gob ? K : 1, box};
  T lamb = a.lamb[b];
  T* gK = v.rebase(a.K ? a.K : a.wsK, m * n * c.N);
  T* gk = v.rebase(a.K ? a.k : a.wsk, m * c.N);
  T* const X = v.rebase(a.X, n * (c.N + 1));
  T* const U0 = v.rebase(a.U, m * c.N);
  T *Uc = U0, *Un = v.rebase(a.wsU, m * c.N);
  __shared__ T lds_gains[LaneWorker<T, Sys, HASQR, TILED>::kGainWords];
  __shared__ unsigned lds_sink[64];  // LaneWorker::warm_rows
  w.sink = lds_sink;
  if (a.stagger > 0 && ((blockIdx.x >> 9) & 1)) {  // see k_lane_iterate_rows
    for (int q = 0; q < a.stagger; q++) __builtin_amdgcn_s_sleep(127);
  }
  T cost = w.rollout(X, Uc, xT);
  int it = 0, status = a.early_exit ? 2 : 0;
  T cost_ret = cost;
  const bool general = !(sizeof(T) == 8 && c.fast_barrier);  // configurations outside the hot form
  while (it < a.n_iters) {
    // hot, branch-free passes first; the general forms only if a lane asked for them
    if (__builtin_expect(__any(general || w.template backward_blocked<true, false, Hook>(X, Uc, xT, ob, lamb, gK, gk, lds_gains, mdl)), 0))
      w.template backward_blocked<true, true, Hook>(X, Uc, xT, ob, lamb, gK, gk, lds_gains, mdl);
    bool big = false;
    T cost_new = w.template forward_rows<false>(X, Uc, gK, gk, Un, xT, &big);
    if (__builtin_expect(__any(big), 0))
      cost_new = w.template forward_rows<true>(X, Uc, gK, gk, Un, xT, &big);
    it++;
    const bool accepted = cost_new < cost;
    if (__all(accepted)) {  // the two input buffers change roles for the whole wavefront
      T* tp = Uc; Uc = Un; Un = tp;
      if (__builtin_expect(__any(w.template restore_rows<false, false>(X, Uc)), 0))
        w.template restore_rows<false, true>(X, Uc);
    } else if (__any(accepted)) {
      if (__builtin_expect(__any(w.template restore_rows<true, false>(X, Uc, Un, accepted)), 0))
        w.template restore_rows<true, true>(X, Uc, Un, accepted);
    }
    if (accepted) {  // control/iterative_ilqr.py:74-80
      lamb /= c.lamb_factor;
      const bool conv = t_abs((cost_new - cost) / cost) < c.eps;
      cost_ret = cost_new;
      // next iteration's nominal cost: stage terms are measured to xtarget, not x_terminal
      cost = HASQR ? w.nominal_cost(X, Uc, xT) : cost_new;
      if (conv) {
        if (a.early_exit) { status = 1; break; }
        if (status == 0) status = 1;
      }
    } else {  // control/iterative_ilqr.py:81-84
      lamb *= c.lamb_factor;
      cost_ret = cost;
      if (lamb > c.max_lamb) {
        if (a.early_exit) { status = 3; break; }
        if (status == 0) status = 3;
      }
    }
  }
  if (!t_isfinite(cost_ret)) status = 4;
  if (Uc != U0) {  // the accepted inputs sit in the workspace: copy them out
    for (int e = 0; e < m * c.N; e++) U0[(int64_t)e * v.Bs + v.bl] = Uc[(int64_t)e * v.Bs + v.bl];
  }
  a.lamb[b] = lamb;
  a.cost[b] = cost_ret;
  if (a.iters) a.iters[b] = it;
  if (a.status) a.status[b] = status;
}

// The instantiations (quad12 x lane layout), one unit per word size, Q = R = 0.  Expanded as `extern
// template` for the launcher, in the kernel's units as the instantiations.  The fp64 stage-weight form
// (HASQR) is not built: it compiles with more scratch than k_lane_iterate_rows<HASQR> itself (3660 /
// 3684 against 3496 / 3516 bytes per lane), so LaneLaunch::iterate_model refuses Q, R != 0 (DESIGN.md
// 3.7).
#define I2LQR_LANE_ROWS_MODEL_KERNELS_(DECL, REAL, QR)                                             \
  DECL void k_lane_iterate_rows_model<REAL, Quad12<REAL>, QR, false>(                              \
      const DevCfg<REAL, 12, 4>, const LaneArgs<REAL>, const int, const BoxCfg<REAL, 12>);         \
  DECL void k_lane_iterate_rows_model<REAL, Quad12<REAL>, QR, true>(                               \
      const DevCfg<REAL, 12, 4>, const LaneArgs<REAL>, const int, const BoxCfg<REAL, 12>);
#define I2LQR_LANE_ROWS_MODEL_F64_KERNELS(DECL) I2LQR_LANE_ROWS_MODEL_KERNELS_(DECL, double, false)
#define I2LQR_LANE_ROWS_MODEL_F32_KERNELS(DECL) I2LQR_LANE_ROWS_MODEL_KERNELS_(DECL, float, false)
#ifndef I2LQR_LANE_ROWS_MODEL_F64_DEFINE
I2LQR_LANE_ROWS_MODEL_F64_KERNELS(extern template __global__)
#endif
#ifndef I2LQR_LANE_ROWS_MODEL_F32_DEFINE
I2LQR_LANE_ROWS_MODEL_F32_KERNELS(extern template __global__)
#endif

}  // namespace i2lqr
