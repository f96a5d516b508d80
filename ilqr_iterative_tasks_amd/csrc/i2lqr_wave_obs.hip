// k_iterate_obs: the one-problem-per-wavefront kernel (k_iterate, i2lqr_wave.hpp) with several
// elliptical obstacles per problem.  NOT the reference's model: get_cost_derivation /
// get_cost_final (control/ilqr_helper.py) take ONE obstacle.  Opt-in ("obstacles" 2 ...
// I2LQR_MAX_OBSTACLES, include/i2lqr.h).
//
// The barrier is additive and an obstacle's whole contribution to an iteration is five words per
// horizon step (l_x[0:2] and the symmetric 2x2 block of l_xx; index N is the terminal term), written
// by Worker::prep in a phase that is parallel over t and outside the serial Riccati chain.  Here the
// lane that has written record 0's five words for its t adds records 1 ... K - 1 for that t, each
// with Worker::prep's arithmetic term for term, in record order.  A record whose moving_option is
// negative adds nothing; where record 0 is the disabled one the first enabled record's words are
// stored as they are (not added to zero), so a problem with one enabled record computes that
// obstacle's k_iterate numbers bit for bit, whichever slot it sits in.
//
// The records cannot live in registers (k_iterate_ls already sits at the register limit on bicycle6
// fp64; 6 K more words per lane would spill).  They sit in 6 K words of LDS behind the problem's
// slice, loaded once at entry, one word per lane; record 0 is also held in registers, as in
// k_iterate.  What a record costs is not its loads (reading them from global memory in prep
// measured the same) but its arithmetic: two divisions and an exponential in fp64, about 150
// dependent instructions on the one lane that owns the step, ~1 us on a lone wavefront
// (DESIGN.md 3.1).  Spreading the (step, record) pairs over the idle lanes is described there, not
// built.
// Backward pass, forward pass (the line search's: `steps` = 1 is its one-candidate path), accept /
// reject (whose cost has no barrier term), exit and stores are LsWorker's / Worker's, unchanged.
#include "i2lqr_wave_opt.h"

#include "i2lqr_wave_obs.hpp"  // ObsWorker: LsWorker with the records' prep

namespace i2lqr {

// k_iterate_ls (i2lqr_wave_ls.hip) with prep_obs in the place of prep.
template <class T, class Sys, bool HASQR>
__global__ __launch_bounds__(64) void k_iterate_obs(const DevCfg<T, Sys::n, Sys::m> c,
                                                    const IterArgs<T> a, const int steps,
                                                    const int n_obs) {
  constexpr int n = Sys::n, m = Sys::m;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int64_t prob = blockIdx.x;
  if (prob >= a.B) return;
  ObsWorker<T, Sys, HASQR> w(c, reinterpret_cast<T*>(smem_raw), lane);
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
  bool fresh = true;  // the nominal trajectory changed since the last prep_obs()
  while (it < a.n_iters) {
    const int Xo = cur ? L.X1 : L.X0, Uo = cur ? L.U1 : L.U0;
    const int Xn = cur ? L.X0 : L.X1, Un = cur ? L.U0 : L.U1;
    if (fresh) w.prep_obs(Xo, Uo, ob, gob ? recs : nullptr, K);
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

I2LQR_WAVE_OPT_KERNELS(template __global__, k_iterate_obs, I2LQR_WAVE_TAIL_OBS)

}  // namespace i2lqr
