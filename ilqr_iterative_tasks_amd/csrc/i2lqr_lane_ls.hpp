// k_lane_iterate_ls: k_lane_iterate_model / k_lane_iterate_merit (i2lqr_lane_model.hpp,
// i2lqr_lane_merit.hpp) with the parallel line search of "line_search" ("lane_line_search" 2 / 4 / 8,
// include/i2lqr.h).  NOT the reference's model: its forward pass takes the full step only
// (control/iterative_ilqr.py:133-160).  Opt-in.
//
// Per iteration ONE backward pass, unchanged.  Then the candidates j = 0 ... A - 1,
//   u_t = clip(U_t + 2^-j k_t + K_t (x_t^j - X_t))        (the product 2^-j k_t is exact),
// are rolled out and J_j = c_j (MERIT: c_j + P_j, LaneMeritHook's terms in its order) decides:
// j* = argmin_j J_j, a NaN counted as +inf, ties to the smallest j (all NaN: 0).  Candidate j* goes
// through the accept / reject block of k_lane_iterate_model (MERIT: k_lane_iterate_merit's, c and P
// carried separately) as its one candidate would: lamb schedule, status words and cost[] are theirs;
// K and k are returned unscaled.
//
// The lane kernel streams its trajectory, so the candidates do not multiply its traffic:
//   trial pass     lane_forward_ls<.., AC>: the nominal x_t, U_t, K_t, k_t of a step are loaded once
//                  (the D-deep prefetch and the LDS-resident gain steps of LaneWorker::forward) and
//                  AC candidate states advance from them in registers, their costs and penalties in
//                  accumulators of their own.  No candidate state is stored; candidate 0's inputs go
//                  to Un.  A = 2: one pass of two; A = 4: one pass of four; A = 8: two passes of four
//                  (eight fp64 states of bicycle6 with their successors do not fit beside the loads;
//                  bicycle6 in fp64 with stage weights: passes of two, kLaneLsGroup).
//                  The candidates are independent and the argmin order is fixed: same bits.
//   winner's pass  if any lane of the wavefront chose j* > 0, the pass runs once more with one
//                  candidate and each lane's own 2^-j*, and writes Un.  A lane with j* = 0 stores
//                  what it stored already: 1 k_t is k_t, and every other operation is the same.
// Candidate 0 is computed with LaneWorker::forward's arithmetic, operation for operation (with
// -ffp-contract=off, U_t + 1 k_t is U_t + k_t): a run in which no problem ever takes a short step
// returns the bits of the run with the option off.
//
// The states are never written by the passes ("defer_states" has no effect: an accepted step
// re-rolls them, as its deferred form does); "reroll_nominal", "merge_inputs", the LDS-resident gain
// steps and "stagger" keep their meaning and the bits.  Records, box and LDS are
// k_lane_iterate_model's: the step sizes take no LDS and no workspace.
#pragma once
#include "i2lqr_lane_merit.hpp"

namespace i2lqr {

// One forward pass of AC candidates with the step sizes s[j] from one stream of loads.  cost[j]: the
// barrier-free cost of candidate j; pen[j]: its penalty (MERIT::kOn).  store: candidate 0's clipped
// inputs go to Un.  LaneWorker::forward<REROLL, false, D, MERIT> candidate by candidate.
template <bool REROLL, int AC, class T, class Sys, bool HASQR, bool TILED, class MERIT>
__device__ __forceinline__ void lane_forward_ls(const LaneWorker<T, Sys, HASQR, TILED>& w, const T* X,
                                                const T* U, const T* gK, const T* gk, T* Un,
                                                const T (&xT)[Sys::n], const MERIT& mh,
                                                const T (&s)[AC], const bool store, T (&cost)[AC],
                                                T (&pen)[AC]) {
  constexpr int n = Sys::n, m = Sys::m, NT = Sys::NTRIG;
  // Prefetch distance in horizon steps: LaneWorker::forward's (two in fp32), but one for a pass of four
  // - its step computes as long as four of the one-candidate pass's, so one step hides the loads the
  // other took two for, and the second register set is what pushed three fp32 instantiations of
  // bicycle6 into scratch (20 ... 180 bytes).  The order of the loads is no arithmetic: same bits.
  constexpr int D = (LaneWorker<T, Sys, HASQR, TILED>::DEEP && AC < 4) ? 2 : 1;
  const int N = w.N;
  T x[AC][n], xo[n];
#pragma unroll
  for (int i = 0; i < n; i++) {
    xo[i] = w.at(X, w.rx(i, 0));
#pragma unroll
    for (int j = 0; j < AC; j++) x[j][i] = xo[i];
  }
#pragma unroll
  for (int j = 0; j < AC; j++) {
    cost[j] = T(0);
    pen[j] = T(0);
  }
  // (LaneWorker::forward's load_step)
  auto load_step = [&](int t, T (&xl)[n], T (&ul)[m], T (&kl)[m][n + 1])
      __attribute__((always_inline)) {
    if constexpr (!REROLL) {
#pragma unroll
      for (int i = 0; i < n; i++) xl[i] = w.at(X, w.rx(i, t));
    }
#pragma unroll
    for (int a = 0; a < m; a++) ul[a] = w.at(U, w.ru(a, t));
    if (t == 0 && w.has_lds) {  // x_0 is common to the nominal and the candidates: K_0 multiplies zeros
#pragma unroll
      for (int a = 0; a < m; a++) {
#pragma unroll
        for (int i = 0; i < n; i++) kl[a][i] = T(0);
        kl[a][n] = w.lds_k0(a);
      }
    } else if (t >= 1 && t <= w.lds_steps) {
#pragma unroll
      for (int a = 0; a < m; a++)
#pragma unroll
        for (int i = 0; i <= n; i++) kl[a][i] = w.lds_gain(t, a * (n + 1) + i);
    } else {
#pragma unroll
      for (int a = 0; a < m; a++) {
#pragma unroll
        for (int i = 0; i < n; i++) kl[a][i] = w.at(gK, w.rK(a, i, t));
        kl[a][n] = w.at(gk, w.ru(a, t));
      }
    }
  };
  auto body = [&](const int t, T (&xl)[n], T (&ul)[m], T (&kl)[m][n + 1])
      __attribute__((always_inline)) {
    T u[AC][m], uon[m];
#pragma unroll
    for (int j = 0; j < AC; j++) {
#pragma unroll
      for (int a = 0; a < m; a++) {
        T acc = T(0);
#pragma unroll
        for (int i = 0; i < n; i++)
          acc = t_fma(kl[a][i], x[j][i] - (REROLL ? xo[i] : xl[i]), acc);
        u[j][a] = clip(ul[a] + s[j] * kl[a][n] + acc, -w.c.u_max[a], w.c.u_max[a]);
      }
    }
#pragma unroll
    for (int a = 0; a < m; a++) uon[a] = ul[a];
    // the loads of step t + D right behind the last use of step t's, as in LaneWorker::forward
    if (t + D < N) load_step(t + D, xl, ul, kl);
    if (store) {
#pragma unroll
      for (int a = 0; a < m; a++) w.at(Un, w.ru(a, t)) = u[0][a];
    }
    T tr[NT], xn[n];
    if constexpr (REROLL) {  // nominal state of step t + 1
      Sys::trig(xo, tr);
      Sys::step_tr(w.c, xo, uon, tr, xn);
#pragma unroll
      for (int i = 0; i < n; i++) xo[i] = xn[i];
    }
#pragma unroll
    for (int j = 0; j < AC; j++) {
      Sys::trig(x[j], tr);
      Sys::step_tr(w.c, x[j], u[j], tr, xn);
      cost[j] = cost[j] + w.stage_cost(x[j], xT, u[j]);
      if constexpr (MERIT::kOn) pen[j] += mh.step_terms(w, x[j], u[j], t);
#pragma unroll
      for (int i = 0; i < n; i++) x[j][i] = xn[i];
    }
  };
  T xl[D][n], ul[D][m], kl[D][m][n + 1];
#pragma unroll
  for (int i = 0; i < n; i++) xl[0][i] = xo[i];
#pragma unroll
  for (int d = 0; d < D; d++)
    if (d < N) load_step(d, xl[d], ul[d], kl[d]);
  if constexpr (D > 1) {
    int t = 0;
    for (; t + D <= N; t += D) {
#pragma unroll
      for (int d = 0; d < D; d++) body(t + d, xl[d], ul[d], kl[d]);
    }
#pragma unroll
    for (int d = 0; d < D - 1; d++)
      if (t + d < N) body(t + d, xl[d], ul[d], kl[d]);
  } else {
    for (int t = 0; t < N; t++) body(t, xl[0], ul[0], kl[0]);
  }
#pragma unroll
  for (int j = 0; j < AC; j++) {
    cost[j] = cost[j] + w.terminal_cost(x[j], xT);
    if constexpr (MERIT::kOn) pen[j] = pen[j] + mh.state_terms(w, x[j], N);
  }
}

// Candidates of one trial pass.  Four; bicycle6 in fp64 with stage weights: two - four candidate
// states beside the weight matrices do not fit the 512 registers of a wavefront (four at once: 250 of
// 256 AGPRs in the soft batch-minor instantiation, 52 bytes of scratch with the barrier cost), so
// A = 4 runs there as two passes of two and A = 8 as four.
template <class T, class Sys, bool HASQR>
constexpr int kLaneLsGroup = (sizeof(T) == 8 && Sys::n > 4 && HASQR) ? 2 : 4;

// The running argmin of the line search over the candidates seen so far
template <class T> struct LaneLsPick {
  int j;     // j*
  T key;     // J_j* with a NaN counted as +inf
  T c, p;    // c_j*, P_j* as the pass summed them
  // candidates j0 ... j0 + AC - 1, in order: a strictly smaller key wins, so ties stay with the
  // smallest j and j* = 0 if every J is NaN
  template <bool MERIT, int AC>
  __device__ __forceinline__ void take(int j0, const T (&cost)[AC], const T (&pen)[AC]) {
#pragma unroll
    for (int q = 0; q < AC; q++) {
      const T J = MERIT ? cost[q] + pen[q] : cost[q];
      const T masked = J != J ? T(__builtin_huge_val()) : J;
      if ((j0 == 0 && q == 0) || masked < key) {
        j = j0 + q;
        key = masked;
        c = cost[q];
        p = pen[q];
      }
    }
  }
};

// LaneArgs, K, the box, the box's q1 and the dynamic LDS as k_lane_iterate_merit takes them (box_q1
// is read with MERIT only); A: 2, 4 or 8 step sizes.  a.cost returns c, with MERIT J.
// (k_lane_chunk_ls below is a copy of this loop with the chunk protocol: it must follow every change)
template <class T, class Sys, bool HASQR, bool TILED, bool MERIT>
__global__ __launch_bounds__(64, (sizeof(T) == 4 ? I2LQR_F32_WAVES : I2LQR_F64_WAVES)) void
k_lane_iterate_ls(const DevCfg<T, Sys::n, Sys::m> c, const LaneArgs<T> a, const int K,
                  const BoxCfg<T, Sys::n> box, const T box_q1, const int A) {
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
  // one pass of AC candidates over the current nominal, with or without the penalty
  auto pass = [&](auto ac_, const auto& s, bool store, auto& cj, auto& pj)
      __attribute__((always_inline)) {
    constexpr int AC = decltype(ac_)::value;
    if constexpr (MERIT) {
      if (a.reroll) lane_forward_ls<true, AC>(w, X, Uc, gK, gk, Un, xT, mh, s, store, cj, pj);
      else lane_forward_ls<false, AC>(w, X, Uc, gK, gk, Un, xT, mh, s, store, cj, pj);
    } else {
      if (a.reroll) lane_forward_ls<true, AC>(w, X, Uc, gK, gk, Un, xT, NoMerit(), s, store, cj, pj);
      else lane_forward_ls<false, AC>(w, X, Uc, gK, gk, Un, xT, NoMerit(), s, store, cj, pj);
    }
  };
  T cost = w.rollout(X, Uc, xT);  // c of the nominal: barrier-free
  [[maybe_unused]] T pen = T(0);
  if constexpr (MERIT) pen = mh.nominal_penalty(w, X, Uc);
  T J = MERIT ? cost + pen : cost;
  int it = 0, status = a.early_exit ? 2 : 0;
  T J_ret = J;
  while (it < a.n_iters) {
    // K_0 goes to HBM from the passes that can be this launch's last one for the problem
    const bool k0_out = a.early_exit || it + 1 >= a.n_iters;
    w.template backward<true, false, 0, Hook>(X, Uc, xT, ob, lamb, gK, gk, k0_out, nullptr, mdl);
    // trial pass(es): A is wave-uniform (a kernel argument)
    LaneLsPick<T> best{0, T(0), T(0), T(0)};
    constexpr int G = kLaneLsGroup<T, Sys, HASQR>;
    if (G > 2 && A == 2) {
      const T s[2] = {T(1), T(0.5)};
      T cj[2], pj[2];
      pass(std::integral_constant<int, 2>{}, s, true, cj, pj);
      best.template take<MERIT>(0, cj, pj);
    } else {
      T s0 = T(1);
      for (int j0 = 0; j0 < A; j0 += G, s0 *= T(1) / T(1 << G)) {
        T s[G], cj[G], pj[G];
#pragma unroll
        for (int q = 0; q < G; q++) s[q] = s0 * (T(1) / T(1 << q));
        pass(std::integral_constant<int, G>{}, s, j0 == 0, cj, pj);
        best.template take<MERIT>(j0, cj, pj);
      }
    }
    // winner's pass: Un holds candidate 0's inputs; a lane that chose a shorter step needs its own
    if (__any(best.j > 0)) {
      const T s[1] = {T(1) / T(1 << best.j)};
      T cj[1], pj[1];
      pass(std::integral_constant<int, 1>{}, s, true, cj, pj);
    }
    it++;
    const T cost_new = best.c;
    [[maybe_unused]] const T pen_new = best.p;
    const T J_new = MERIT ? cost_new + pen_new : cost_new;
    // accept / reject with the lamb schedule of control/iterative_ilqr.py:74-84: the soft test of
    // k_lane_iterate_model, with MERIT the test of k_lane_iterate_merit
    const bool accepted = MERIT ? (t_isfinite(J_new) && J_new < J) : (J_new < J);
    // X must hold the states of each lane's CURRENT inputs (see k_lane_iterate); no pass wrote them
    if (a.merge) {
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
      if (__any(accepted)) w.restore_states(X, Uc);
    }
    if (accepted) {
      lamb /= c.lamb_factor;
      const bool conv = t_abs((J_new - J) / cost) < c.eps;
      J_ret = J_new;
      // next nominal: stage terms are measured to xtarget, not x_terminal, when Q != 0
      cost = HASQR ? w.nominal_cost(X, Uc, xT) : cost_new;
      if constexpr (MERIT) pen = pen_new;
      J = MERIT ? cost + pen : cost;
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

// k_lane_chunk_ls: k_lane_iterate_ls as a chunk of the chunked, compacting solve, with the chunk
// protocol of k_lane_chunk_model (i2lqr_lane_model.hpp; a copy of the kernel above for the same reason,
// units i2lqr_lane_ls_chunk_f64.hip, _f32.hip).  The winner's cost is the trial pass's sum: a chunk
// carries it (and with MERIT P, through ck.pen) through the work set as k_lane_chunk_merit does.
template <class T, class Sys, bool HASQR, bool TILED, bool MERIT>
__global__ __launch_bounds__(64, (sizeof(T) == 4 ? I2LQR_F32_WAVES : I2LQR_F64_WAVES)) void
k_lane_chunk_ls(const DevCfg<T, Sys::n, Sys::m> c, const LaneArgs<T> a, const int K,
                const BoxCfg<T, Sys::n> box, const T box_q1, const int A, const LaneChunk<T> ck) {
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
  // one pass of AC candidates over the current nominal, with or without the penalty
  auto pass = [&](auto ac_, const auto& s, bool store, auto& cj, auto& pj)
      __attribute__((always_inline)) {
    constexpr int AC = decltype(ac_)::value;
    if constexpr (MERIT) {
      if (a.reroll) lane_forward_ls<true, AC>(w, X, Uc, gK, gk, Un, xT, mh, s, store, cj, pj);
      else lane_forward_ls<false, AC>(w, X, Uc, gK, gk, Un, xT, mh, s, store, cj, pj);
    } else {
      if (a.reroll) lane_forward_ls<true, AC>(w, X, Uc, gK, gk, Un, xT, NoMerit(), s, store, cj, pj);
      else lane_forward_ls<false, AC>(w, X, Uc, gK, gk, Un, xT, NoMerit(), s, store, cj, pj);
    }
  };
  T cost = w.rollout(X, Uc, xT);  // c of the nominal: barrier-free
  [[maybe_unused]] T pen = T(0);
  // iterations of earlier chunks: the same for every problem of a chunk (no tail kernel between model
  // chunks, and a survivor has used every iteration of every earlier chunk), so a scalar
  const int it0 = ck.resume ? __builtin_amdgcn_readfirstlane(a.iters[b]) : 0;
  if (ck.resume) {  // ... and c (P) of the nominal they left
    cost = a.cost[b];
    if constexpr (MERIT) pen = ck.pen.in[b];
  } else {
    if constexpr (MERIT) pen = mh.nominal_penalty(w, X, Uc);
  }
  T J = MERIT ? cost + pen : cost;
  int it = 0, status = a.early_exit ? 2 : 0;
  T J_ret = J;
  // it < a.n_iters && it0 + it < max_total, as one wave-uniform bound
  const int n_run = a.n_iters < ck.max_total - it0 ? a.n_iters : ck.max_total - it0;
  while (it < n_run) {
    // K_0 goes to HBM from the passes that can be this launch's last one for the problem
    const bool k0_out = a.early_exit || it + 1 >= n_run;
    w.template backward<true, false, 0, Hook>(X, Uc, xT, ob, lamb, gK, gk, k0_out, nullptr, mdl);
    // trial pass(es): A is wave-uniform (a kernel argument)
    LaneLsPick<T> best{0, T(0), T(0), T(0)};
    constexpr int G = kLaneLsGroup<T, Sys, HASQR>;
    if (G > 2 && A == 2) {
      const T s[2] = {T(1), T(0.5)};
      T cj[2], pj[2];
      pass(std::integral_constant<int, 2>{}, s, true, cj, pj);
      best.template take<MERIT>(0, cj, pj);
    } else {
      T s0 = T(1);
      for (int j0 = 0; j0 < A; j0 += G, s0 *= T(1) / T(1 << G)) {
        T s[G], cj[G], pj[G];
#pragma unroll
        for (int q = 0; q < G; q++) s[q] = s0 * (T(1) / T(1 << q));
        pass(std::integral_constant<int, G>{}, s, j0 == 0, cj, pj);
        best.template take<MERIT>(j0, cj, pj);
      }
    }
    // winner's pass: Un holds candidate 0's inputs; a lane that chose a shorter step needs its own
    if (__any(best.j > 0)) {
      const T s[1] = {T(1) / T(1 << best.j)};
      T cj[1], pj[1];
      pass(std::integral_constant<int, 1>{}, s, true, cj, pj);
    }
    it++;
    const T cost_new = best.c;
    [[maybe_unused]] const T pen_new = best.p;
    const T J_new = MERIT ? cost_new + pen_new : cost_new;
    // accept / reject with the lamb schedule of control/iterative_ilqr.py:74-84: the soft test of
    // k_lane_iterate_model, with MERIT the test of k_lane_iterate_merit
    const bool accepted = MERIT ? (t_isfinite(J_new) && J_new < J) : (J_new < J);
    // X must hold the states of each lane's CURRENT inputs (see k_lane_iterate); no pass wrote them
    if (a.merge) {
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
      if (__any(accepted)) w.restore_states(X, Uc);
    }
    if (accepted) {
      lamb /= c.lamb_factor;
      const bool conv = t_abs((J_new - J) / cost) < c.eps;
      J_ret = J_new;
      // next nominal: stage terms are measured to xtarget, not x_terminal, when Q != 0
      cost = HASQR ? w.nominal_cost(X, Uc, xT) : cost_new;
      if constexpr (MERIT) pen = pen_new;
      J = MERIT ? cost + pen : cost;
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
      if constexpr (MERIT) ck.pen.out[j] = pen;
    }
  }
}

// The thirty-two instantiations (two bicycles x two precisions x stage weights x lane layout x barrier
// cost): `extern template` for the launcher, the instantiations in the two units
// (KERNEL: k_lane_iterate_ls with an empty TAIL, k_lane_chunk_ls with the penalty rows)
#define I2LQR_LANE_LS_TAIL(REAL)
#define I2LQR_LANE_LS_TAIL_CHUNK(REAL) , const LaneChunk<REAL>
#define I2LQR_LANE_LS_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, QR, TL, MERIT)               \
  DECL void KERNEL<REAL, SYS<REAL>, QR, TL, MERIT>(                                                \
      const DevCfg<REAL, N_, M_>, const LaneArgs<REAL>, const int, const BoxCfg<REAL, N_>,         \
      const REAL, const int TAIL(REAL));
#define I2LQR_LANE_LS_LAYOUTS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, QR)                          \
  I2LQR_LANE_LS_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, QR, false, false)                  \
  I2LQR_LANE_LS_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, QR, false, true)                   \
  I2LQR_LANE_LS_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, QR, true, false)                   \
  I2LQR_LANE_LS_KERNELS_(DECL, KERNEL, TAIL, REAL, SYS, N_, M_, QR, true, true)
#define I2LQR_LANE_LS_KERNELS_OF(DECL, KERNEL, TAIL, REAL)                                         \
  I2LQR_LANE_LS_LAYOUTS_(DECL, KERNEL, TAIL, REAL, Bicycle4, 4, 2, false)                          \
  I2LQR_LANE_LS_LAYOUTS_(DECL, KERNEL, TAIL, REAL, Bicycle4, 4, 2, true)                           \
  I2LQR_LANE_LS_LAYOUTS_(DECL, KERNEL, TAIL, REAL, Bicycle6, 6, 2, false)                          \
  I2LQR_LANE_LS_LAYOUTS_(DECL, KERNEL, TAIL, REAL, Bicycle6, 6, 2, true)
#define I2LQR_LANE_LS_KERNELS(DECL, REAL)                                                          \
  I2LQR_LANE_LS_KERNELS_OF(DECL, k_lane_iterate_ls, I2LQR_LANE_LS_TAIL, REAL)
// k_lane_chunk_ls where lane_chunks_built() (i2lqr_lane_plan.hpp): with the barrier cost; bicycle6 with
// stage weights in fp64 only (..._B6QR)
#define I2LQR_LANE_LS_CHUNK_(DECL, REAL, SYS, N_, M_, QR)                                          \
  I2LQR_LANE_LS_KERNELS_(DECL, k_lane_chunk_ls, I2LQR_LANE_LS_TAIL_CHUNK, REAL, SYS, N_, M_, QR, false, true) \
  I2LQR_LANE_LS_KERNELS_(DECL, k_lane_chunk_ls, I2LQR_LANE_LS_TAIL_CHUNK, REAL, SYS, N_, M_, QR, true, true)
#define I2LQR_LANE_LS_CHUNK_KERNELS(DECL, REAL)                                                    \
  I2LQR_LANE_LS_CHUNK_(DECL, REAL, Bicycle4, 4, 2, false)                                          \
  I2LQR_LANE_LS_CHUNK_(DECL, REAL, Bicycle4, 4, 2, true)                                           \
  I2LQR_LANE_LS_CHUNK_(DECL, REAL, Bicycle6, 6, 2, false)
#define I2LQR_LANE_LS_CHUNK_KERNELS_B6QR(DECL, REAL) I2LQR_LANE_LS_CHUNK_(DECL, REAL, Bicycle6, 6, 2, true)
template <class T, class Sys, bool HASQR, bool MERIT>
constexpr bool kLaneLsChunkBuilt = lane_chunks_built((int)sizeof(T), Sys::n, HASQR, 2, MERIT);
static_assert(kLaneLsChunkBuilt<double, Bicycle6<double>, true, true> &&
              !kLaneLsChunkBuilt<float, Bicycle6<float>, true, true> &&
              !kLaneLsChunkBuilt<double, Bicycle4<double>, false, false>, "the lists below");

I2LQR_LANE_LS_KERNELS(extern template __global__, double)
I2LQR_LANE_LS_KERNELS(extern template __global__, float)
I2LQR_LANE_LS_CHUNK_KERNELS(extern template __global__, double)
I2LQR_LANE_LS_CHUNK_KERNELS_B6QR(extern template __global__, double)
I2LQR_LANE_LS_CHUNK_KERNELS(extern template __global__, float)

}  // namespace i2lqr
