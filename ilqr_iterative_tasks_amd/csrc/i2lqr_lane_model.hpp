// k_lane_iterate_model: the one-problem-per-lane kernel with the opt-in models that enter the
// backward pass's derivatives only — several obstacle records per problem and the state box
// ("lane_models" 1, include/i2lqr.h).  It is k_lane_iterate's iteration loop in the one-wavefront
// form (deferred states, re-rolling forward pass, merged inputs, LDS-resident gain steps; no
// helper wavefront, no state checkpoints, no chunk entry / exit) around LaneWorker::backward with
// the MODEL hook below.  Compiled in units of its own (i2lqr_lane_model_f64.hip, _f32.hip): the
// kernels of the existing lane units do not see it.
//
// obs holds K records of six words per problem, record r's word q in row q K + r:
//     batch-minor  obs[6][K][B]        batch-tiled  obs[B/64][6][K][64]
// (K = 1: the layouts of i2lqr_lane.hpp).  Record 0 lives in registers as in k_lane_iterate;
// records 1 ... K - 1 are staged once per launch in LDS behind the gain steps and k_0, as
// [x, y, 1 / width^2, 1 / height^2, speed, option] (the two reciprocals are what
// LaneWorker::backward forms of record 0): word (r - 1) 6 + q of lane l at recs[((r - 1) 6 + q) 64
// + l].  Every lane reads the words it wrote itself: no barrier.  The box is a by-value kernel
// argument, wave-uniform: its bounds and masks sit in scalar registers and take no LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "i2lqr_lane.hpp"
#include "i2lqr_wave_opt.h"  // BoxCfg

namespace i2lqr {

template <class T, int n> struct LaneModelHook {
  static constexpr bool kOn = true;
  typedef __attribute__((address_space(3))) T lds_t;
  lds_t* recs;  // staged records 1 ... K - 1 of this wavefront
  int K;        // records per problem, 1 ... I2LQR_MAX_OBSTACLES
  const BoxCfg<T, n>& box;

  __device__ __forceinline__ void stage(int r, int q, T v) const {
    recs[((r - 1) * 6 + q) * 64 + (threadIdx.x & 63)] = v;
  }
  // Records 1 ... K - 1 join o[] (record 0's five words; any: record 0 is enabled) in record
  // order, each with LaneWorker::obstacle()'s own arithmetic.  A disabled record adds nothing, and
  // the first enabled record's words are taken as they are, not added to zeros.
  template <class W>
  __device__ __forceinline__ void more_obstacles(const W& w, bool any, T px, T py, int t,
                                                 T (&o)[5]) const {
    const lds_t* p = recs + (threadIdx.x & 63);
    for (int r = 1; r < K; r++, p += 6 * 64) {
      T rec[6], oo[5];
#pragma unroll
      for (int q = 0; q < 6; q++) rec[q] = p[q * 64];
      w.obstacle(rec, rec[2], rec[3], px, py, t, oo);
      const bool en = rec[5] >= T(0);
#pragma unroll
      for (int q = 0; q < 5; q++) o[q] = en ? (any ? o[q] + oo[q] : oo[q]) : o[q];
      any = any || en;
    }
  }
  __device__ __forceinline__ bool box_on() const { return (box.m_lo | box.m_hi) != 0; }
  // d1 = q1 q2 (e_hi - e_lo), d2 = q1 q2^2 (e_hi + e_lo) of a state, e_hi = exp(q2 (x - hi)),
  // e_lo = exp(q2 (lo - x)); an unbounded side is not computed (wave-uniform masks)
  __device__ __forceinline__ void box_terms(const T (&x)[n], T (&d1)[n], T (&d2)[n]) const {
#pragma unroll
    for (int i = 0; i < n; i++) {
      T eh = T(0), el = T(0);
      if ((box.m_hi >> i) & 1u) eh = t_exp(box.q2 * (x[i] - box.hi[i]));
      if ((box.m_lo >> i) & 1u) el = t_exp(box.q2 * (box.lo[i] - x[i]));
      d1[i] = box.q12 * (eh - el);
      d2[i] = box.q122 * (eh + el);
    }
  }
};

// LaneArgs as k_lane_iterate takes them; count / resume / ckpt / cp / wsX are not read (the
// launcher leaves them neutral).  Dynamic LDS: a.lds_steps gain steps, k_0, then 6 (K - 1) words per
// lane (lane_model_bytes, i2lqr_lane_plan.hpp).
// (k_lane_chunk_model below is a copy of this loop with the chunk protocol: it must follow every change)
template <class T, class Sys, bool HASQR, bool TILED>
__global__ __launch_bounds__(64, (sizeof(T) == 4 ? I2LQR_F32_WAVES : I2LQR_F64_WAVES)) void
k_lane_iterate_model(const DevCfg<T, Sys::n, Sys::m> c, const LaneArgs<T> a, const int K,
                     const BoxCfg<T, Sys::n> box) {
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
  T cost = w.rollout(X, Uc, xT);
  int it = 0, status = a.early_exit ? 2 : 0;
  T cost_ret = cost;
  while (it < a.n_iters) {
    // K_0 goes to HBM from the passes that can be this launch's last one for the problem
    const bool k0_out = a.early_exit || it + 1 >= a.n_iters;
    w.template backward<true, false, 0, Hook>(X, Uc, xT, ob, lamb, gK, gk, k0_out, nullptr, mdl);
    T cost_new;
    if (a.defer) {
      cost_new = a.reroll ? w.template forward<true, false>(X, Uc, gK, gk, X, Un, xT)
                          : w.template forward<false, false>(X, Uc, gK, gk, X, Un, xT);
    } else {
      cost_new = a.reroll ? w.template forward<true>(X, Uc, gK, gk, X, Un, xT)
                          : w.template forward<false>(X, Uc, gK, gk, X, Un, xT);
    }
    it++;
    const bool accepted = cost_new < cost;
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
  w.flush_gains(gK, gk);
  if (Uc != U0) {  // the accepted inputs sit in the workspace: copy them out
    for (int e = 0; e < m * N; e++) U0[(int64_t)e * v.Bs + v.bl] = Uc[(int64_t)e * v.Bs + v.bl];
  }
  a.lamb[b] = lamb;
  a.cost[b] = cost_ret;
  if (a.iters) a.iters[b] = it;
  if (a.status) a.status[b] = status;
}

// The penalty row of the chunked solve's work sets (k_lane_chunk_merit, k_lane_chunk_ls with the
// barrier cost): P of a survivor's nominal travels beside its cost.  in: the row of the set the chunk
// runs on (read with resume); out: the row of the set its exit packs into.
template <class T> struct LanePen {
  const T* in;
  T* out;
};

// What a chunk kernel takes beside the arguments of its single-launch form: LaneArgs' count, resume
// and max_total under the same names (the launcher copies them; the kernels do not read LaneArgs'), and
// the penalty rows (null without the barrier cost)
template <class T> struct LaneChunk {
  const int32_t* count;
  int resume, max_total;
  LanePen<T> pen;
};

// k_lane_chunk_model: k_lane_iterate_model as a chunk of the chunked, compacting solve
// ("lane_model_chunks" 1; LaneLaunch::solve_compacting).  A copy of the kernel above on purpose, in
// units of its own (i2lqr_lane_model_chunk_f64.hip, _f32.hip): the compiler's output for these kernels
// moves with the shape of their source (profiles/iterate_refactor.md; a body shared through an inlined
// function cost k_lane_iterate_model up to 6 % with the option off), so the kernel above is the text it
// was and the chunk protocol lives here alone.
//
// The chunk protocol is k_lane_iterate's, its fields in a kernel argument of their own (LaneChunk: read
// from LaneArgs they widen the scalar load of the option fields beside them, which then stays live
// through the loop and is spilled): the live batch from *ck.count, the iteration counter
// continued from a.iters[b] (ck.resume), the cap ck.max_total, status RUNNING for a problem the chunk
// leaves unfinished, and lane_exit_compact at the exit (a.cp.on) with the 6 K rows of the records.  No
// tail kernel runs between model chunks, so a problem of a work set is always RUNNING at entry.  A
// resumed chunk re-rolls the states from x_0 and the inputs as k_lane_iterate does; the cost of the
// nominal is NOT formed again but carried: the exit stores it in the next work set's cost row at the
// survivor's slot and the resumed chunk reads a.cost[b], so what the loop carries across the chunk
// boundary has the single launch's bits by construction (with stage weights, the barrier cost or a
// short step it comes from another pass than the entry rollout's).
template <class T, class Sys, bool HASQR, bool TILED>
__global__ __launch_bounds__(64, (sizeof(T) == 4 ? I2LQR_F32_WAVES : I2LQR_F64_WAVES)) void
k_lane_chunk_model(const DevCfg<T, Sys::n, Sys::m> c, const LaneArgs<T> a, const int K,
                   const BoxCfg<T, Sys::n> box, const LaneChunk<T> ck) {
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
  T cost = w.rollout(X, Uc, xT);
  // iterations of earlier chunks: the same for every problem of a chunk (no tail kernel between model
  // chunks, and a survivor has used every iteration of every earlier chunk), so a scalar
  const int it0 = ck.resume ? __builtin_amdgcn_readfirstlane(a.iters[b]) : 0;
  if (ck.resume) cost = a.cost[b];             // ... and the nominal cost they left
  int it = 0, status = a.early_exit ? 2 : 0;
  T cost_ret = cost;
  // it < a.n_iters && it0 + it < max_total, as one wave-uniform bound
  const int n_run = a.n_iters < ck.max_total - it0 ? a.n_iters : ck.max_total - it0;
  while (it < n_run) {
    // K_0 goes to HBM from the passes that can be this launch's last one for the problem
    const bool k0_out = a.early_exit || it + 1 >= n_run;
    w.template backward<true, false, 0, Hook>(X, Uc, xT, ob, lamb, gK, gk, k0_out, nullptr, mdl);
    T cost_new;
    if (a.defer) {
      cost_new = a.reroll ? w.template forward<true, false>(X, Uc, gK, gk, X, Un, xT)
                          : w.template forward<false, false>(X, Uc, gK, gk, X, Un, xT);
    } else {
      cost_new = a.reroll ? w.template forward<true>(X, Uc, gK, gk, X, Un, xT)
                          : w.template forward<false>(X, Uc, gK, gk, X, Un, xT);
    }
    it++;
    const bool accepted = cost_new < cost;
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
  // a chunk that ran out before the problem terminated: RUNNING unless the iteration cap is hit
  if (a.early_exit && status == 2 && it0 + it < ck.max_total) status = 0;
  if (!t_isfinite(cost_ret) && (status != 0 || !a.early_exit)) status = 4;
  w.flush_gains(gK, gk);
  if (Uc != U0) {  // the accepted inputs sit in the workspace: copy them out
    for (int e = 0; e < m * N; e++) U0[(int64_t)e * v.Bs + v.bl] = Uc[(int64_t)e * v.Bs + v.bl];
  }
  a.lamb[b] = lamb;
  a.cost[b] = cost_ret;
  if (a.iters) a.iters[b] = it0 + it;
  if (a.status) a.status[b] = status;
  if (a.cp.on) {
    const int64_t j = lane_exit_compact(a.cp, n, m, N, b, v.Bs, v.bl, X, U0, gxt, gob, gK, gk, lamb,
                                        cost_ret, it0 + it, status, c.trap, 6 * K);
    if (j >= 0) a.cp.dst.cost[j] = cost;
  }
}

// The sixteen instantiations of KERNEL (two bicycles x two precisions x stage weights x lane layout);
// TAIL(REAL) spells the parameter types that follow DevCfg, LaneArgs, the record count and the box.
// Expanded as `extern template` for the launcher, in the kernel's two units as the instantiations.
#define I2LQR_LANE_TAIL_MODEL(REAL)
#define I2LQR_LANE_TAIL_MERIT(REAL) , const REAL
#define I2LQR_LANE_TAIL_CHUNK_MODEL(REAL) , const LaneChunk<REAL>
#define I2LQR_LANE_TAIL_CHUNK_MERIT(REAL) , const REAL, const LaneChunk<REAL>
#define I2LQR_LANE_OPT_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, QR, TL)                     \
  DECL void KERNEL<REAL, SYS<REAL>, QR, TL>(const DevCfg<REAL, N_, M_>, const LaneArgs<REAL>,      \
                                            const int, const BoxCfg<REAL, N_> TAIL(REAL));
#define I2LQR_LANE_OPT_BICYCLE_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_)                             \
  I2LQR_LANE_OPT_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, false, false)                     \
  I2LQR_LANE_OPT_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, false, true)                      \
  I2LQR_LANE_OPT_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, true, false)                      \
  I2LQR_LANE_OPT_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, true, true)
#define I2LQR_LANE_OPT_KERNELS(DECL, KERNEL, TAIL, REAL)                                           \
  I2LQR_LANE_OPT_BICYCLE_(DECL, KERNEL, TAIL, REAL, Bicycle4, 4, 2)                                \
  I2LQR_LANE_OPT_BICYCLE_(DECL, KERNEL, TAIL, REAL, Bicycle6, 6, 2)

I2LQR_LANE_OPT_KERNELS(extern template __global__, k_lane_iterate_model, I2LQR_LANE_TAIL_MODEL, double)
I2LQR_LANE_OPT_KERNELS(extern template __global__, k_lane_iterate_model, I2LQR_LANE_TAIL_MODEL, float)
I2LQR_LANE_OPT_KERNELS(extern template __global__, k_lane_chunk_model, I2LQR_LANE_TAIL_CHUNK_MODEL, double)
I2LQR_LANE_OPT_KERNELS(extern template __global__, k_lane_chunk_model, I2LQR_LANE_TAIL_CHUNK_MODEL, float)

}  // namespace i2lqr
