// k_lane_iterate_merit: k_lane_iterate_model (i2lqr_lane_model.hpp) whose accept / reject step sees
// the barriers ("lane_barrier_cost" 1, include/i2lqr.h).  NOT the reference's model: there the
// exponential barriers enter the backward pass's derivatives only
// (control/iterative_ilqr.py:43-48), and so they do in every other lane kernel.  Opt-in.
//
// With c(X, U) the barrier-free cost of the other forms and P(X, U) the penalty of "barrier_cost",
// the merit is J = c + P, with one step size (no argmin) and k_iterate_merit's accept block
// (i2lqr_wave_merit.hip):
//   accept        iff J_new is finite and J_new < J; the lamb schedule is unchanged
//   convergence   accepted and |(J_new - J) / c| < eps, c the barrier-free cost of the nominal
//                 being replaced
//   next nominal  c = c_new (nominal_cost() with stage weights), P = P_new: carried separately
//   cost[]        J of the returned trajectory
// A box that is off and one record are valid.
//
// P of a candidate is summed inside LaneWorker::forward (its MERIT parameter) from the x_t and the
// clipped u_t every form of the pass holds in registers, so "defer_states", "reroll_nominal",
// "merge_inputs", the LDS-resident gain steps and "stagger" keep the bits.  The terms of horizon
// index t, in this order, into one step sum that is then added to the pass's accumulator:
//   a = 0 ... m - 1 (t < N)  ctrl_q1 (e^{ctrl_q2 (u[a] - u_max[a])} + e^{ctrl_q2 (-u_max[a] - u[a])})
//   r = 0 ... K - 1          obs_q1 e^{obs_q2 h_r(x_t, t)}, h as LaneWorker::obstacle() forms it; a
//                            disabled record is skipped
//   i = 0 ... n - 1          box q1 (e_hi + e_lo); a side without bound is not computed
// P of the nominal is computed once per launch, after rollout(), by a read pass over the stored
// clipped trajectory with the same device functions (nominal_penalty), and carried from then on.
// Records and LDS are k_lane_iterate_model's: the penalty takes no LDS.
#pragma once
#include "i2lqr_lane_model.hpp"

namespace i2lqr {

template <class T, int n, int m> struct LaneMeritHook {
  static constexpr bool kOn = true;
  typedef __attribute__((address_space(3))) T lds_t;
  const LaneModelHook<T, n>& mdl;  // the staged records 1 ... K - 1, K and the box
  const T (&ob)[6];                // record 0
  T pa, pb;                        // 1 / ob[2]^2, 1 / ob[3]^2, as LaneWorker::backward forms them
  T box_q1;                        // (BoxCfg carries the products q1 q2 and q1 q2^2 only)

  // obs_q1 e^{obs_q2 h} of one record at (px, py), horizon index t: LaneWorker::obstacle()'s h
  template <class W>
  __device__ __forceinline__ T record_term(const W& w, const T (&rec)[6], T ra, T rb, T px, T py,
                                           int t) const {
    const int opt = (int)rec[5];
    T dz = px - rec[0], dy = py - rec[1];
    if (opt == 1) dy = py - (rec[1] + T(t) * rec[4]);
    if (opt == 2) dz = px - (rec[0] - T(t) * rec[4]);
    const T h = T(1) + w.c.safety_margin - (dz * ra * dz + dy * rb * dy);
    return w.c.obs_q1 * t_exp(w.c.obs_q2 * h);
  }
  // the record and box terms of x_t (t <= N)
  template <class W> __device__ __forceinline__ T state_terms(const W& w, const T (&x)[n], int t) const {
    T s = T(0);
    {
      const T e = record_term(w, ob, pa, pb, x[0], x[1], t);
      s = ob[5] >= T(0) ? s + e : s;
    }
    const lds_t* p = mdl.recs + (threadIdx.x & 63);
    for (int r = 1; r < mdl.K; r++, p += 6 * 64) {
      T rec[6];
#pragma unroll
      for (int q = 0; q < 6; q++) rec[q] = p[q * 64];
      const T e = record_term(w, rec, rec[2], rec[3], x[0], x[1], t);
      s = rec[5] >= T(0) ? s + e : s;
    }
    const auto& box = mdl.box;
#pragma unroll
    for (int i = 0; i < n; i++) {
      if (((box.m_hi | box.m_lo) >> i) & 1u) {
        T eh = T(0), el = T(0);
        if ((box.m_hi >> i) & 1u) eh = t_exp(box.q2 * (x[i] - box.hi[i]));
        if ((box.m_lo >> i) & 1u) el = t_exp(box.q2 * (box.lo[i] - x[i]));
        s += box_q1 * (eh + el);
      }
    }
    return s;
  }
  // the terms of step t < N: the input barriers of the clipped u_t, then x_t's
  template <class W>
  __device__ __forceinline__ T step_terms(const W& w, const T (&x)[n], const T (&u)[m], int t) const {
    T s = T(0);
#pragma unroll
    for (int a = 0; a < m; a++) {
      const T eh = t_exp(w.c.ctrl_q2 * (u[a] - w.c.u_max[a]));
      const T el = t_exp(w.c.ctrl_q2 * (-w.c.u_max[a] - u[a]));
      s += w.c.ctrl_q1 * (eh + el);
    }
    return s + state_terms(w, x, t);
  }
  // P of the stored trajectory (the nominal at entry; U holds the clipped inputs): one read pass
  template <class W> __device__ __forceinline__ T nominal_penalty(const W& w, const T* X, const T* U) const {
    T x[n], u[m];
    T p = T(0);
    for (int t = 0; t < w.N; t++) {
#pragma unroll
      for (int i = 0; i < n; i++) x[i] = w.at(X, w.rx(i, t));
#pragma unroll
      for (int a = 0; a < m; a++) u[a] = w.at(U, w.ru(a, t));
      p += step_terms(w, x, u, t);
    }
#pragma unroll
    for (int i = 0; i < n; i++) x[i] = w.at(X, w.rx(i, w.N));
    return p + state_terms(w, x, w.N);
  }
};

// LaneArgs, K, the box and the dynamic LDS as k_lane_iterate_model takes them; box_q1: the box's q1.
// a.cost returns J.
// (k_lane_chunk_merit below is a copy of this loop with the chunk protocol: it must follow every change)
template <class T, class Sys, bool HASQR, bool TILED>
__global__ __launch_bounds__(64, (sizeof(T) == 4 ? I2LQR_F32_WAVES : I2LQR_F64_WAVES)) void
k_lane_iterate_merit(const DevCfg<T, Sys::n, Sys::m> c, const LaneArgs<T> a, const int K,
                     const BoxCfg<T, Sys::n> box, const T box_q1) {
  constexpr int n = Sys::n, m = Sys::m;
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int N = c.N;
  const LaneView<TILED> v(a.B);
  LaneWorker<T, Sys, HASQR, TILED> w(c, v.Bs, v.bl);
  extern __shared__ __align__(16) unsigned char lane_smem[];
  typedef __attribute__((address_space(3))) T lds_t;
  w.lds = (lds_t*)lane_smem;
  w.has_lds = true;
  w.lds_steps = a.lds_steps;
  using Hook = LaneModelHook<T, n>;
  using Merit = LaneMeritHook<T, n, m>;
  const Hook mdl{(lds_t*)lane_smem + (size_t)a.lds_steps * 64 * m * (n + 1) + 64 * m, K, box};
  const T* gxt = v.rebase(a.x_term, n);
  const T* gob = v.rebase(a.obs, 6 * K);
  T xT[n], ob[6];
#pragma unroll
  for (int i = 0; i < n; i++) xT[i] = gxt[(int64_t)i * v.Bs + v.bl];
  // a NULL obs disables every record (finite placeholders, as k_lane_iterate's)
#pragma unroll
  for (int q = 0; q < 6; q++)
    ob[q] = gob ? gob[(int64_t)(q * K) * v.Bs + v.bl] : T(q == 5 ? -1 : 1);
  for (int r = 1; r < K; r++) {
    T rec[6];
#pragma unroll
    for (int q = 0; q < 6; q++)
      rec[q] = gob ? gob[(int64_t)(q * K + r) * v.Bs + v.bl] : T(q == 5 ? -1 : 1);
    rec[2] = T(1) / (rec[2] * rec[2]);
    rec[3] = T(1) / (rec[3] * rec[3]);
#pragma unroll
    for (int q = 0; q < 6; q++) mdl.stage(r, q, rec[q]);
  }
  const Merit mh{mdl, ob, T(1) / (ob[2] * ob[2]), T(1) / (ob[3] * ob[3]), box_q1};
  T lamb = a.lamb[b];
  T* gK = v.rebase(a.K ? a.K : a.wsK, m * n * N);
  T* gk = v.rebase(a.K ? a.k : a.wsk, m * N);
  // (states in ONE buffer, inputs double-buffered per lane: see k_lane_iterate)
  T* const X = v.rebase(a.X, n * (N + 1));
  T* const U0 = v.rebase(a.U, m * N);
  T *Uc = U0, *Un = v.rebase(a.wsU, m * N);
  if (a.stagger > 0 && ((blockIdx.x >> 9) & 1)) {  // see k_lane_iterate_rows
    for (int q = 0; q < a.stagger; q++) __builtin_amdgcn_s_sleep(127);
  }
  T cost = w.rollout(X, Uc, xT);  // c of the nominal: barrier-free
  T pen = mh.nominal_penalty(w, X, Uc);
  T J = cost + pen;
  int it = 0, status = a.early_exit ? 2 : 0;
  T J_ret = J;
  while (it < a.n_iters) {
    // K_0 goes to HBM from the passes that can be this launch's last one for the problem
    const bool k0_out = a.early_exit || it + 1 >= a.n_iters;
    w.template backward<true, false, 0, Hook>(X, Uc, xT, ob, lamb, gK, gk, k0_out, nullptr, mdl);
    constexpr int D = LaneWorker<T, Sys, HASQR, TILED>::DEEP ? 2 : 1;  // (forward's own default)
    T cost_new, pen_new;
    if (a.defer) {
      cost_new = a.reroll
          ? w.template forward<true, false, D, Merit>(X, Uc, gK, gk, X, Un, xT, mh, &pen_new)
          : w.template forward<false, false, D, Merit>(X, Uc, gK, gk, X, Un, xT, mh, &pen_new);
    } else {
      cost_new = a.reroll
          ? w.template forward<true, true, D, Merit>(X, Uc, gK, gk, X, Un, xT, mh, &pen_new)
          : w.template forward<false, true, D, Merit>(X, Uc, gK, gk, X, Un, xT, mh, &pen_new);
    }
    it++;
    // accept / reject on the merit, with the lamb schedule of control/iterative_ilqr.py:74-84
    const T J_new = cost_new + pen_new;
    const bool accepted = t_isfinite(J_new) && J_new < J;
    // X must hold the states of each lane's CURRENT inputs (see k_lane_iterate)
    if (a.defer && a.merge) {
      if (__all(accepted)) {
        T* tp = Uc; Uc = Un; Un = tp;
        w.restore_states(X, Uc);
      } else if (__any(accepted)) {
        w.merge_and_restore(X, Uc, Un, accepted);
      }
    } else {
      if (accepted) {
        T* tp = Uc; Uc = Un; Un = tp;
      }
      if (__any(a.defer ? accepted : !accepted)) w.restore_states(X, Uc);
    }
    if (accepted) {
      lamb /= c.lamb_factor;
      const bool conv = t_abs((J_new - J) / cost) < c.eps;
      J_ret = J_new;
      // next nominal: stage terms are measured to xtarget, not x_terminal, when Q != 0
      cost = HASQR ? w.nominal_cost(X, Uc, xT) : cost_new;
      pen = pen_new;
      J = cost + pen;
      if (conv) {
        if (a.early_exit) { status = 1; break; }
        if (status == 0) status = 1;
      }
    } else {
      lamb *= c.lamb_factor;
      J_ret = J;
      if (lamb > c.max_lamb) {
        if (a.early_exit) { status = 3; break; }
        if (status == 0) status = 3;
      }
    }
  }
  if (!t_isfinite(J_ret)) status = 4;
  w.flush_gains(gK, gk);
  if (Uc != U0) {  // the accepted inputs sit in the workspace: copy them out
    for (int e = 0; e < m * N; e++) U0[(int64_t)e * v.Bs + v.bl] = Uc[(int64_t)e * v.Bs + v.bl];
  }
  a.lamb[b] = lamb;
  a.cost[b] = J_ret;
  if (a.iters) a.iters[b] = it;
  if (a.status) a.status[b] = status;
}

// k_lane_chunk_merit: k_lane_iterate_merit as a chunk of the chunked, compacting solve, with the chunk
// protocol of k_lane_chunk_model (i2lqr_lane_model.hpp; a copy of the kernel above for the same reason,
// units i2lqr_lane_merit_chunk_f64.hip, _f32.hip).  c and P of a survivor's nominal go through the work
// set's cost and penalty rows (ck.pen): the convergence test divides by c alone, and P inside the loop is
// the forward pass's running sum, not nominal_penalty()'s.
template <class T, class Sys, bool HASQR, bool TILED>
__global__ __launch_bounds__(64, (sizeof(T) == 4 ? I2LQR_F32_WAVES : I2LQR_F64_WAVES)) void
k_lane_chunk_merit(const DevCfg<T, Sys::n, Sys::m> c, const LaneArgs<T> a, const int K,
                   const BoxCfg<T, Sys::n> box, const T box_q1, const LaneChunk<T> ck) {
  constexpr int n = Sys::n, m = Sys::m;
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t live = ck.count ? (int64_t)*ck.count : a.B;
  if (b >= live) return;
  const int N = c.N;
  const LaneView<TILED> v(a.B);
  LaneWorker<T, Sys, HASQR, TILED> w(c, v.Bs, v.bl);
  extern __shared__ __align__(16) unsigned char lane_smem[];
  typedef __attribute__((address_space(3))) T lds_t;
  w.lds = (lds_t*)lane_smem;
  w.has_lds = true;
  w.lds_steps = a.lds_steps;
  using Hook = LaneModelHook<T, n>;
  using Merit = LaneMeritHook<T, n, m>;
  const Hook mdl{(lds_t*)lane_smem + (size_t)a.lds_steps * 64 * m * (n + 1) + 64 * m, K, box};
  const T* gxt = v.rebase(a.x_term, n);
  const T* gob = v.rebase(a.obs, 6 * K);
  T xT[n], ob[6];
#pragma unroll
  for (int i = 0; i < n; i++) xT[i] = gxt[(int64_t)i * v.Bs + v.bl];
  // a NULL obs disables every record (finite placeholders, as k_lane_iterate's)
#pragma unroll
  for (int q = 0; q < 6; q++)
    ob[q] = gob ? gob[(int64_t)(q * K) * v.Bs + v.bl] : T(q == 5 ? -1 : 1);
  for (int r = 1; r < K; r++) {
    T rec[6];
#pragma unroll
    for (int q = 0; q < 6; q++)
      rec[q] = gob ? gob[(int64_t)(q * K + r) * v.Bs + v.bl] : T(q == 5 ? -1 : 1);
    rec[2] = T(1) / (rec[2] * rec[2]);
    rec[3] = T(1) / (rec[3] * rec[3]);
#pragma unroll
    for (int q = 0; q < 6; q++) mdl.stage(r, q, rec[q]);
  }
  const Merit mh{mdl, ob, T(1) / (ob[2] * ob[2]), T(1) / (ob[3] * ob[3]), box_q1};
  T lamb = a.lamb[b];
  T* gK = v.rebase(a.K ? a.K : a.wsK, m * n * N);
  T* gk = v.rebase(a.K ? a.k : a.wsk, m * N);
  // (states in ONE buffer, inputs double-buffered per lane: see k_lane_iterate)
  T* const X = v.rebase(a.X, n * (N + 1));
  T* const U0 = v.rebase(a.U, m * N);
  T *Uc = U0, *Un = v.rebase(a.wsU, m * N);
  if (a.stagger > 0 && ((blockIdx.x >> 9) & 1)) {  // see k_lane_iterate_rows
    for (int q = 0; q < a.stagger; q++) __builtin_amdgcn_s_sleep(127);
  }
  T cost = w.rollout(X, Uc, xT);  // c of the nominal: barrier-free
  T pen;
  // iterations of earlier chunks: the same for every problem of a chunk (no tail kernel between model
  // chunks, and a survivor has used every iteration of every earlier chunk), so a scalar
  const int it0 = ck.resume ? __builtin_amdgcn_readfirstlane(a.iters[b]) : 0;
  if (ck.resume) {  // ... and c, P of the nominal they left
    cost = a.cost[b];
    pen = ck.pen.in[b];
  } else {
    pen = mh.nominal_penalty(w, X, Uc);
  }
  T J = cost + pen;
  int it = 0, status = a.early_exit ? 2 : 0;
  T J_ret = J;
  // it < a.n_iters && it0 + it < max_total, as one wave-uniform bound
  const int n_run = a.n_iters < ck.max_total - it0 ? a.n_iters : ck.max_total - it0;
  while (it < n_run) {
    // K_0 goes to HBM from the passes that can be this launch's last one for the problem
    const bool k0_out = a.early_exit || it + 1 >= n_run;
    w.template backward<true, false, 0, Hook>(X, Uc, xT, ob, lamb, gK, gk, k0_out, nullptr, mdl);
    constexpr int D = LaneWorker<T, Sys, HASQR, TILED>::DEEP ? 2 : 1;  // (forward's own default)
    T cost_new, pen_new;
    if (a.defer) {
      cost_new = a.reroll
          ? w.template forward<true, false, D, Merit>(X, Uc, gK, gk, X, Un, xT, mh, &pen_new)
          : w.template forward<false, false, D, Merit>(X, Uc, gK, gk, X, Un, xT, mh, &pen_new);
    } else {
      cost_new = a.reroll
          ? w.template forward<true, true, D, Merit>(X, Uc, gK, gk, X, Un, xT, mh, &pen_new)
          : w.template forward<false, true, D, Merit>(X, Uc, gK, gk, X, Un, xT, mh, &pen_new);
    }
    it++;
    // accept / reject on the merit, with the lamb schedule of control/iterative_ilqr.py:74-84
    const T J_new = cost_new + pen_new;
    const bool accepted = t_isfinite(J_new) && J_new < J;
    // X must hold the states of each lane's CURRENT inputs (see k_lane_iterate)
    if (a.defer && a.merge) {
      if (__all(accepted)) {
        T* tp = Uc; Uc = Un; Un = tp;
        w.restore_states(X, Uc);
      } else if (__any(accepted)) {
        w.merge_and_restore(X, Uc, Un, accepted);
      }
    } else {
      if (accepted) {
        T* tp = Uc; Uc = Un; Un = tp;
      }
      if (__any(a.defer ? accepted : !accepted)) w.restore_states(X, Uc);
    }
    if (accepted) {
      lamb /= c.lamb_factor;
      const bool conv = t_abs((J_new - J) / cost) < c.eps;
      J_ret = J_new;
      // next nominal: stage terms are measured to xtarget, not x_terminal, when Q != 0
      cost = HASQR ? w.nominal_cost(X, Uc, xT) : cost_new;
      pen = pen_new;
      J = cost + pen;
      if (conv) {
        if (a.early_exit) { status = 1; break; }
        if (status == 0) status = 1;
      }
    } else {
      lamb *= c.lamb_factor;
      J_ret = J;
      if (lamb > c.max_lamb) {
        if (a.early_exit) { status = 3; break; }
        if (status == 0) status = 3;
      }
    }
  }
  // a chunk that ran out before the problem terminated: RUNNING unless the iteration cap is hit
  if (a.early_exit && status == 2 && it0 + it < ck.max_total) status = 0;
  if (!t_isfinite(J_ret) && (status != 0 || !a.early_exit)) status = 4;
  w.flush_gains(gK, gk);
  if (Uc != U0) {  // the accepted inputs sit in the workspace: copy them out
    for (int e = 0; e < m * N; e++) U0[(int64_t)e * v.Bs + v.bl] = Uc[(int64_t)e * v.Bs + v.bl];
  }
  a.lamb[b] = lamb;
  a.cost[b] = J_ret;
  if (a.iters) a.iters[b] = it0 + it;
  if (a.status) a.status[b] = status;
  if (a.cp.on) {
    const int64_t j = lane_exit_compact(a.cp, n, m, N, b, v.Bs, v.bl, X, U0, gxt, gob, gK, gk, lamb,
                                        J_ret, it0 + it, status, c.trap, 6 * K);
    if (j >= 0) {
      a.cp.dst.cost[j] = cost;
      ck.pen.out[j] = pen;
    }
  }
}

// The sixteen instantiations (I2LQR_LANE_OPT_KERNELS, i2lqr_lane_model.hpp): `extern template` for
// the launcher, the instantiations in the two units
I2LQR_LANE_OPT_KERNELS(extern template __global__, k_lane_iterate_merit, I2LQR_LANE_TAIL_MERIT, double)
I2LQR_LANE_OPT_KERNELS(extern template __global__, k_lane_iterate_merit, I2LQR_LANE_TAIL_MERIT, float)
I2LQR_LANE_OPT_KERNELS(extern template __global__, k_lane_chunk_merit, I2LQR_LANE_TAIL_CHUNK_MERIT, double)
I2LQR_LANE_OPT_KERNELS(extern template __global__, k_lane_chunk_merit, I2LQR_LANE_TAIL_CHUNK_MERIT, float)

}  // namespace i2lqr
