// k_iterate_box: the one-problem-per-wavefront kernel with a box on the states (speed limits and
// the like).  NOT the reference's model: its v_min / v_max and tuning_state_q1 / q2
// (utils/base.py:15-20, 242-302) are read by nothing there.  Opt-in (i2lqr_set_state_box,
// include/i2lqr.h).
//
// For every horizon index t = 0 ... N and every state component i with a finite bound the
// exponential barrier of add_control_constraint (control/ilqr_helper.py:59-64, 83-103) is applied
// to x_t[i]:
//   e_hi = exp(q2 (x - hi)), e_lo = exp(q2 (lo - x))     (0 on a side without bound)
//   d1 = q1 q2 (e_hi - e_lo) -> l_x[i] (t < N) / V_x[i] (t = N)
//   d2 = q1 q2^2 (e_hi + e_lo) -> l_xx[i][i] / V_xx[i][i]
// The barrier enters the derivatives only; the accept / reject cost is the reference's.
//
// The (t, i) pairs are independent - each writes its own two words, nothing is summed - so prep_box
// spreads them over all 64 lanes, not over the lanes that own t as the obstacle records are
// (DESIGN.md 3.1).  The 2 n (N + 1) words sit in LDS behind the obstacle records, the 2 n bounds
// behind them.  The backward pass
// is Worker::backward with BOX = true: three more reads (terminal block, the diagonal of l_xx, l_x),
// issued with the phase's other reads.  Everything else - records, line search, accept / reject,
// exit and stores - is k_iterate_obs's (i2lqr_wave_obs.hip), so the box composes with "obstacles"
// and "line_search".
#include "i2lqr_wave_opt.h"

#include "i2lqr_wave_box.hpp"  // BoxWorker: ObsWorker with the box's prep

namespace i2lqr {

// k_iterate_obs (i2lqr_wave_obs.hip) with prep_box in front of prep_obs and the BOX backward pass.
template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_iterate_box(const DevCfg<T, Sys::n, Sys::m> c,
                                                    const IterArgs<T> a, const int steps,
                                                    const int n_obs, const BoxCfg<T, Sys::n> box) {
  constexpr int n = Sys::n, m = Sys::m;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int64_t prob = blockIdx.x;
  if (prob >= a.B) return;
  BoxWorker<T, Sys, HASQR> w(c, reinterpret_cast<T*>(smem_raw), lane);
  const int N = c.N;
  const auto& L = w.L;
  const auto S = w.S;
  const int K = n_obs < 1 ? 1 : (n_obs > I2LQR_MAX_OBSTACLES ? I2LQR_MAX_OBSTACLES : n_obs);

  // entry: x0, U, x_term, lamb, record 0  (HBM -> LDS/registers), as k_iterate
  T xT[n], ob[6];
  const T* gX = a.X + prob * (int64_t)(n * (N + 1));
  if (w.sl < n) S[L.X0 + w.sl] = gX[w.sl * (N + 1)];
  w.load_rec(a.U + prob * (int64_t)(m * N), L.U0, m, N);
#pragma unroll
  for (int i = 0; i < n; i++) xT[i] = a.x_term[prob * n + i];
  const T* gob = a.obs ? a.obs + prob * (int64_t)(K * 6) : nullptr;  // this problem's obs[K][6]
#pragma unroll
  for (int q = 0; q < 6; q++) ob[q] = gob ? gob[q] : T(q == 5 ? -1 : 1);
  // ... and all K records behind the slice (extra_lds_bytes; visible after the wave_sync below)
  static_assert(I2LQR_MAX_OBSTACLES * 6 <= 64, "one record word per lane");
  T* recs = reinterpret_cast<T*>(smem_raw) + L.total;
  if (gob && lane < K * 6) recs[lane] = gob[lane];
  T* bx = recs + K * 6;  // d1[N+1][n], d2[N+1][n], lo[n], hi[n] behind the records (extra_lds_bytes)
  w.stage_box(box, bx);
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
  bool fresh = true;  // the nominal trajectory changed since the last prep
  while (it < a.n_iters) {
    const int Xo = cur ? L.X1 : L.X0, Uo = cur ? L.U1 : L.U0;
    const int Xn = cur ? L.X0 : L.X1, Un = cur ? L.U0 : L.U1;
    if (fresh) {
      w.prep_box(Xo, box, bx);  // (made visible by the wave_sync that ends prep_obs)
      w.prep_obs(Xo, Uo, ob, gob ? recs : nullptr, K);
    }
    if (__builtin_expect(__any(w.template backward<false, true>(Xo, Uo, xT, lamb, bx)), 0))
      w.template backward<true, true>(Xo, Uo, xT, lamb, bx);
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

I2LQR_WAVE_OPT_KERNELS(template __global__, k_iterate_box, I2LQR_WAVE_TAIL_BOX)

}  // namespace i2lqr
