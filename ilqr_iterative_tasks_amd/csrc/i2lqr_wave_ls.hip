// k_iterate_ls: the one-problem-per-wavefront kernel (k_iterate, i2lqr_wave.hpp) with a parallel
// line search in the forward pass.  NOT the reference's algorithm: control/iterative_ilqr.py takes
// one full step per iteration and leaves everything else to the lamb schedule (:74-84).
//
// One iteration with A step sizes (A = 2, 4, 8; alpha_j = 2^-j, j = 0 ... A - 1):
//   1. backward pass as in k_iterate: K_t, k_t;
//   2. A candidate rollouts u'_t = clip((u_t + alpha_j k_t) + K_t (x'_t - x_t)), x'_{t+1} =
//      f(x'_t, u'_t) with the forward pass's cost (stage terms to x_terminal, :151);
//   3. j* = argmin_j cost_j — a NaN cost never wins, ties go to the smallest j, j* = 0 if no
//      candidate has a cost below +inf;
//   4. the reference's accept / reject with cost_new = cost_{j*}, unchanged.
// The gains a call returns are the backward pass's, NOT scaled by the step that was taken.
//
// Worker::forward is executed redundantly by all 64 lanes; here lane l runs candidate l mod A, so
// the candidates cost no more than the one rollout they replace.  Lane 0 runs j = 0 and publishes
// its trajectory as Worker::forward does; only an ACCEPTED iteration whose winner is a shorter step
// repeats the rollout with that step on every lane (same code, same inputs: the same bits the
// winning lanes computed).  No extra LDS.
#include "i2lqr_wave_opt.h"

#include "i2lqr_wave_ls.hpp"  // LsWorker: Worker with the line search's forward pass

namespace i2lqr {

template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_iterate_ls(const DevCfg<T, Sys::n, Sys::m> c,
                                                   const IterArgs<T> a, const int steps) {
  constexpr int n = Sys::n, m = Sys::m;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int64_t prob = blockIdx.x;
  if (prob >= a.B) return;
  LsWorker<T, Sys, HASQR> w(c, reinterpret_cast<T*>(smem_raw), lane);
  const int N = c.N;
  const auto& L = w.L;
  const auto S = w.S;

  // entry: x0, U, x_term, lamb, obs  (HBM -> LDS/registers), as k_iterate
  T xT[n], ob[6];
  const T* gX = a.X + prob * (int64_t)(n * (N + 1));
  if (w.sl < n) S[L.X0 + w.sl] = gX[w.sl * (N + 1)];
  w.load_rec(a.U + prob * (int64_t)(m * N), L.U0, m, N);
#pragma unroll
  for (int i = 0; i < n; i++) xT[i] = a.x_term[prob * n + i];
#pragma unroll
  for (int q = 0; q < 6; q++) ob[q] = a.obs ? a.obs[prob * 6 + q] : T(q == 5 ? -1 : 1);
  w.stage_consts();
  T lamb = a.lamb[prob];
  // this lane's candidate: j = lane mod steps, alpha = 2^-j
  const int A = steps < 1 ? 1 : (steps > kLsMaxSteps ? kLsMaxSteps : steps);
  const T alpha_lane = T(1) / T(1 << (lane % A));
  wave_sync();

  int cur = 0;  // which of the two trajectory buffers holds the nominal
  T cost = w.rollout(L.X0, L.U0, xT);
  int it = 0, status = a.early_exit ? 2 /*MAX_ITER*/ : 0 /*RUNNING*/;
  T cost_ret = cost;
  bool fresh = true;  // the nominal trajectory changed since the last prep()
  while (it < a.n_iters) {
    const int Xo = cur ? L.X1 : L.X0, Uo = cur ? L.U1 : L.U0;
    const int Xn = cur ? L.X0 : L.X1, Un = cur ? L.U0 : L.U1;
    if (fresh) w.prep(Xo, Uo, ob);
    if (__builtin_expect(__any(w.template backward<false>(Xo, Uo, xT, lamb)), 0))
      w.template backward<true>(Xo, Uo, xT, lamb);
    // the candidates: optimistic sincos first, the general form for ALL of them if one candidate
    // left the short kernel's range (lane by lane the two forms agree bit for bit inside it)
    bool big = false;
    T cost_lane = w.template forward_ls<false>(Xo, Uo, Xn, Un, xT, alpha_lane, &big);
    const bool general = __any(big);
    if (__builtin_expect(general, 0))
      cost_lane = w.template forward_ls<true>(Xo, Uo, Xn, Un, xT, alpha_lane, &big);
    // j* = argmin_j cost_j: lane j holds candidate j; NaN never wins, ties go to the smallest j
    int js = 0;
    T best = (T)INFINITY;
#pragma unroll
    for (int j = 0; j < kLsMaxSteps; j++) {
      const T cj = __shfl(cost_lane, j);
      if (j < A && cj < best) {
        best = cj;
        js = j;
      }
    }
    const T cost_new = __shfl(cost_lane, js);
    it++;
    // accept / reject with the lamb schedule: control/iterative_ilqr.py:74-84
    fresh = cost_new < cost;
    if (fresh) {
      if (js != 0) {  // (Xn, Un) hold the full step's trajectory: roll the winner out on every lane
        const T alpha = T(1) / T(1 << js);
        if (general) w.template forward_ls<true>(Xo, Uo, Xn, Un, xT, alpha, &big);
        else w.template forward_ls<false>(Xo, Uo, Xn, Un, xT, alpha, &big);
      }
      cur ^= 1;
      lamb /= c.lamb_factor;
      const bool conv = t_abs((cost_new - cost) / cost) < c.eps;
      cost_ret = cost_new;
      // next nominal cost: stage terms are measured to xtarget, not x_terminal, when Q != 0
      cost = HASQR ? w.nominal_cost(Xn, Un, xT) : cost_new;
      if (conv) {
        if (a.early_exit) { status = 1; break; }
        if (status == 0) status = 1;
      }
    } else {
      lamb *= c.lamb_factor;
      cost_ret = cost;
      if (lamb > c.max_lamb) {
        if (a.early_exit) { status = 3; break; }
        if (status == 0) status = 3;
      }
    }
  }
  if (!t_isfinite(cost_ret)) status = 4;

  // exit: X, U, gains (the backward pass's, unscaled), scalars (LDS -> HBM)
  const int Xo = cur ? L.X1 : L.X0, Uo = cur ? L.U1 : L.U0;
  w.store_rec(a.X + prob * (int64_t)(n * (N + 1)), Xo, n, N + 1);
  w.store_rec(a.U + prob * (int64_t)(m * N), Uo, m, N);
  if (a.K) w.store_gains(a.K + prob * (int64_t)(m * n * N), a.k + prob * (int64_t)(m * N));
  if (w.sl == 0) {
    a.lamb[prob] = lamb;
    a.cost[prob] = cost_ret;
    if (a.iters) a.iters[prob] = it;
    if (a.status) a.status[prob] = status;
  }
}

I2LQR_WAVE_OPT_KERNELS(template __global__, k_iterate_ls, I2LQR_WAVE_TAIL_LS)

}  // namespace i2lqr
