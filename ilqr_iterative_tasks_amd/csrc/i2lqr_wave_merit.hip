// k_iterate_merit: k_iterate_box (i2lqr_wave_box.hip) whose accept / reject step sees the barriers
// ("barrier_cost", include/i2lqr.h).  NOT the reference's model: there the exponential barriers
// enter the backward pass's derivatives only (control/iterative_ilqr.py:43-48), and so they do in
// every other form of this kernel.  Opt-in.
//
// With c(X, U) the barrier-free cost of the other forms and P(X, U) the penalty of
// i2lqr_wave_merit.hpp, the merit is J = c + P:
//   line search   the winner is argmin_j J_j (NaN never wins, ties go to the smallest j)
//   accept        iff J_new is finite and J_new < J; the lamb schedule is unchanged
//   convergence   accepted and |(J_new - J) / c| < eps, c the barrier-free cost of the nominal
//                 being replaced: the input barriers alone put a near-constant floor under J, which
//                 a test relative to J would mistake for convergence
//   next nominal  c = c_new (nominal_cost() with stage weights), P = P_new: carried separately
//   cost[]        J of the returned trajectory
// Records, step sizes and the box are k_iterate_box's; a box that is off and one record are valid.
#include "i2lqr_wave_opt.h"

#include "i2lqr_wave_merit.hpp"  // MeritWorker: BoxWorker with the penalty

namespace i2lqr {

template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_iterate_merit(const DevCfg<T, Sys::n, Sys::m> c,
                                                      const IterArgs<T> a, const int steps,
                                                      const int n_obs, const BoxCfg<T, Sys::n> box,
                                                      const T box_q1) {
  constexpr int n = Sys::n, m = Sys::m;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int64_t prob = blockIdx.x;
  if (prob >= a.B) return;
  MeritWorker<T, Sys, HASQR> w(c, reinterpret_cast<T*>(smem_raw), lane);
  const int N = c.N;
  const auto& L = w.L;
  const auto S = w.S;
  const int K = n_obs < 1 ? 1 : (n_obs > I2LQR_MAX_OBSTACLES ? I2LQR_MAX_OBSTACLES : n_obs);

  // entry: x0, U, x_term, lamb, the records and the box  (HBM -> LDS/registers), as k_iterate_box
  T xT[n], ob[6];
  const T* gX = a.X + prob * (int64_t)(n * (N + 1));
  if (w.sl < n) S[L.X0 + w.sl] = gX[w.sl * (N + 1)];
  w.load_rec(a.U + prob * (int64_t)(m * N), L.U0, m, N);
#pragma unroll
  for (int i = 0; i < n; i++) xT[i] = a.x_term[prob * n + i];
  const T* gob = a.obs ? a.obs + prob * (int64_t)(K * 6) : nullptr;  // this problem's obs[K][6]
#pragma unroll
  for (int q = 0; q < 6; q++) ob[q] = gob ? gob[q] : T(q == 5 ? -1 : 1);
  static_assert(I2LQR_MAX_OBSTACLES * 6 <= 64, "one record word per lane");
  T* recs = reinterpret_cast<T*>(smem_raw) + L.total;
  if (gob && lane < K * 6) recs[lane] = gob[lane];
  T* bx = recs + K * 6;  // d1[N+1][n], d2[N+1][n], lo[n], hi[n] behind the records (extra_lds_bytes)
  const T* bl = bx + 2 * (N + 1) * n;
  const T* g = gob ? recs : nullptr;
  w.stage_box(box, bx);
  w.stage_consts();
  T lamb = a.lamb[prob];
  // this lane's candidate: j = lane mod steps, alpha = 2^-j
  const int A = steps < 1 ? 1 : (steps > kLsMaxSteps ? kLsMaxSteps : steps);
  const T alpha_lane = T(1) / T(1 << (lane % A));
  wave_sync();

  int cur = 0;  // which of the two trajectory buffers holds the nominal
  T cost = w.rollout(L.X0, L.U0, xT);  // c of the nominal: barrier-free
  T pen = w.nominal_penalty(L.X0, L.U0, g, K, box, box_q1, bl);
  T J = cost + pen;
  int it = 0, status = a.early_exit ? 2 /*MAX_ITER*/ : 0 /*RUNNING*/;
  T J_ret = J;
  bool fresh = true;  // the nominal trajectory changed since the last prep
  while (it < a.n_iters) {
    const int Xo = cur ? L.X1 : L.X0, Uo = cur ? L.U1 : L.U0;
    const int Xn = cur ? L.X0 : L.X1, Un = cur ? L.U0 : L.U1;
    if (fresh) {
      w.prep_box(Xo, box, bx);  // (made visible by the wave_sync that ends prep_obs)
      w.prep_obs(Xo, Uo, ob, g, K);
    }
    if (__builtin_expect(__any(w.template backward<false, true>(Xo, Uo, xT, lamb, bx)), 0))
      w.template backward<true, true>(Xo, Uo, xT, lamb, bx);
    // the candidates, as in k_iterate_box: optimistic sincos first, the general form for all of them
    // if one candidate left the short kernel's range
    bool big = false;
    T pen_lane;
    T cost_lane = w.template forward_merit<false>(Xo, Uo, Xn, Un, xT, alpha_lane, &big, A, g, K, box,
                                                  box_q1, bl, &pen_lane);
    const bool general = __any(big);
    if (__builtin_expect(general, 0))
      cost_lane = w.template forward_merit<true>(Xo, Uo, Xn, Un, xT, alpha_lane, &big, A, g, K, box,
                                                 box_q1, bl, &pen_lane);
    // j* = argmin_j J_j: lane j holds candidate j; NaN never wins, ties go to the smallest j
    const T J_lane = cost_lane + pen_lane;
    int js = 0;
    T best = (T)INFINITY;
#pragma unroll
    for (int j = 0; j < kLsMaxSteps; j++) {
      const T Jj = __shfl(J_lane, j);
      if (j < A && Jj < best) {
        best = Jj;
        js = j;
      }
    }
    const T J_new = __shfl(J_lane, js);
    const T cost_new = __shfl(cost_lane, js), pen_new = __shfl(pen_lane, js);
    it++;
    // accept / reject on the merit, with the lamb schedule of control/iterative_ilqr.py:74-84
    fresh = t_isfinite(J_new) && J_new < J;
    if (fresh) {
      if (js != 0) {  // (Xn, Un) hold the full step's trajectory: roll the winner out on every lane
        const T alpha = T(1) / T(1 << js);
        if (general) w.template forward_ls<true>(Xo, Uo, Xn, Un, xT, alpha, &big);
        else w.template forward_ls<false>(Xo, Uo, Xn, Un, xT, alpha, &big);
      }
      cur ^= 1;
      lamb /= c.lamb_factor;
      const bool conv = t_abs((J_new - J) / cost) < c.eps;
      J_ret = J_new;
      // next nominal: stage terms are measured to xtarget, not x_terminal, when Q != 0
      cost = HASQR ? w.nominal_cost(Xn, Un, xT) : cost_new;
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

  // exit: X, U, gains (the backward pass's, unscaled), scalars (LDS -> HBM)
  const int Xo = cur ? L.X1 : L.X0, Uo = cur ? L.U1 : L.U0;
  w.store_rec(a.X + prob * (int64_t)(n * (N + 1)), Xo, n, N + 1);
  w.store_rec(a.U + prob * (int64_t)(m * N), Uo, m, N);
  if (a.K) w.store_gains(a.K + prob * (int64_t)(m * n * N), a.k + prob * (int64_t)(m * N));
  if (w.sl == 0) {
    a.lamb[prob] = lamb;
    a.cost[prob] = J_ret;
    if (a.iters) a.iters[prob] = it;
    if (a.status) a.status[prob] = status;
  }
}

I2LQR_WAVE_OPT_KERNELS(template __global__, k_iterate_merit, I2LQR_WAVE_TAIL_MERIT)

}  // namespace i2lqr
