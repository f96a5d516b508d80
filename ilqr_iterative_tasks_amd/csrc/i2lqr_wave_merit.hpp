// MeritWorker: BoxWorker (i2lqr_wave_box.hpp) with the barrier penalty P(X, U) of the "barrier_cost"
// option (include/i2lqr.h) - the functions whose first derivatives prep, prep_obs and prep_box put
// into the backward pass, summed over the horizon:
//   inputs   t < N,  a < m:      ctrl_q1 (e^{ctrl_q2 (u_t[a] - u_max[a])} + e^{ctrl_q2 (-u_max[a] - u_t[a])})
//   records  t <= N, r[5] >= 0:  obs_q1 e^{obs_q2 h_r(x_t, t)}
//   box      t <= N, i bounded:  box.q1 (e_hi + e_lo)
// Every horizon index has kTerms term SLOTS - 2 m input sides, 2 n box sides, I2LQR_MAX_OBSTACLES
// records - of which a lane evaluates ONE at a time: a lane-selected argument and one exponential.
// Only the slots that can count are handed out (the input sides, the box sides with a bound, the K
// records: 2 m + 3 with a speed limit and one obstacle).  The nominal's penalty spreads the
// (t, slot) pairs over the wavefront; the forward pass spreads the slots of its step over the
// 64 / steps lanes that hold identical copies of a candidate.
// Used by i2lqr_wave_merit.hip (k_iterate_merit) only.
#pragma once
#include "i2lqr_wave_box.hpp"

namespace i2lqr {

template <class T, class Sys, bool HASQR> struct MeritWorker : BoxWorker<T, Sys, HASQR> {
  using Box = BoxWorker<T, Sys, HASQR>;
  using Base = typename Box::Base;
  static constexpr int n = Sys::n, m = Sys::m, NT = Sys::NTRIG;
  static constexpr int kTerms = 2 * m + 2 * n + I2LQR_MAX_OBSTACLES;
  using Base::c;
  using Base::L;
  using Base::N;
  using Base::S;
  using Base::sl;

  __device__ MeritWorker(const typename Base::Cfg& c_, T* smem, int lane) : Box(c_, smem, lane) {}

  // One slot as a lane holds it: the term is coef e^{arg} with
  //   a side of an input or of the box   arg = k2 (sgn v - b),  v = u[idx] (idx < m) or x[idx - m]
  //   a record (rec != NULL)             arg = obs_q2 h_rec(x, t); pa, pb: 1 / rec[2]^2, 1 / rec[3]^2 -
  //                                      the two divisions are the slot's, not every step's
  // on: the slot counts (a side with a bound, a record with rec[5] >= 0, a slot below kTerms).
  struct Term {
    T coef, k2, sgn, b, pa, pb;
    int idx;
    const T* rec;
    bool on;
  };

  // The slots that can count, numbered consecutively: the 2 m input sides, the box sides with a
  // bound (component by component, hi before lo), the K records.  Their number (wave-uniform) ...
  __device__ __forceinline__ int active(const T* g, int K, const BoxCfg<T, n>& b) const {
    return 2 * m + __popc(b.m_hi) + __popc(b.m_lo) + (g ? K : 0);
  }
  // ... and the q-th of them (q lane-dependent) as a slot of term_spec; kTerms: there is none
  __device__ __forceinline__ int slot_of(int q, const T* g, int K, const BoxCfg<T, n>& b) const {
    if (q < 2 * m) return q;
    q -= 2 * m;
    int slot = kTerms, sides = 0;  // sides: wave-uniform, the masks are
#pragma unroll
    for (int i = 0; i < n; i++) {
      if ((b.m_hi >> i) & 1u) {
        slot = sides == q ? 2 * m + 2 * i : slot;
        sides++;
      }
      if ((b.m_lo >> i) & 1u) {
        slot = sides == q ? 2 * m + 2 * i + 1 : slot;
        sides++;
      }
    }
    const int r = q - sides;
    return r >= 0 && g && r < K ? 2 * m + 2 * n + r : slot;
  }

  // Slot e (lane-dependent).  g: obs[K][6] in LDS, or NULL: no obstacle; bl: lo[n], hi[n] in LDS
  // (stage_box: 0 on a side without bound - masked here, never computed with).
  __device__ __forceinline__ Term term_spec(int e, const T* g, int K, const BoxCfg<T, n>& b, T box_q1,
                                            const T* bl) const {
    Term s;
    s.coef = T(0), s.k2 = T(0), s.sgn = T(1), s.b = T(0), s.pa = T(0), s.pb = T(0);
    s.idx = 0, s.rec = nullptr, s.on = false;
    const bool lo = e & 1;
    if (e < 2 * m) {  // e^{q2 (u - u_max)}, e^{q2 (-u_max - u)}
      s.idx = e >> 1;
      s.coef = c.ctrl_q1, s.k2 = c.ctrl_q2, s.sgn = lo ? T(-1) : T(1), s.b = pick(c.u_max, s.idx);
      s.on = true;
    } else if (e < 2 * m + 2 * n) {  // e^{q2 (x - hi)}, e^{q2 (lo - x)}
      const int i = (e - 2 * m) >> 1;
      s.idx = m + i;
      s.coef = box_q1, s.k2 = b.q2, s.sgn = lo ? T(-1) : T(1), s.b = lo ? -bl[i] : bl[n + i];
      s.on = ((lo ? b.m_lo : b.m_hi) >> i) & 1u;
    } else if (e < kTerms) {
      const int r = e - 2 * m - 2 * n;
      if (g && r < K) {
        s.rec = g + r * 6;
        s.coef = c.obs_q1;
        s.pa = T(1) / (s.rec[2] * s.rec[2]), s.pb = T(1) / (s.rec[3] * s.rec[3]);
        s.on = s.rec[5] >= T(0);
      }
    }
    return s;
  }

  // The term of slot s at horizon index t: v the slot's own component, (px, py) the position;
  // with_u false (index N: there is no u_N) drops the input sides.  h is Worker::prep's /
  // ObsWorker::prep_obs's, term for term.
  __device__ __forceinline__ T term_eval(const Term& s, T v, T px, T py, int t, bool with_u) const {
    T arg = s.k2 * (s.sgn * v - s.b);
    if (s.rec) {
      const T* rec = s.rec;
      const int opt = (int)rec[5];
      T dz = px - rec[0], dy = py - rec[1];
      if (opt == 1) dy = py - (rec[1] + T(t) * rec[4]);
      if (opt == 2) dz = px - (rec[0] - T(t) * rec[4]);
      const T h = T(1) + c.safety_margin - (dz * s.pa * dz + dy * s.pb * dy);
      arg = c.obs_q2 * h;
    }
    const T e = t_exp(arg);
    const bool counts = s.on && (with_u || s.idx >= m || s.rec);
    return counts ? s.coef * e : T(0);
  }

  // component idx of (u, x) for a lane-dependent idx: ONE chain of selects (two pick()s under a
  // ternary send both arrays to scratch)
  __device__ __forceinline__ T comp(const T (&u)[m], const T (&x)[n], int idx) const {
    T v = u[0];
#pragma unroll
    for (int q = 1; q < m; q++) v = (idx == q) ? u[q] : v;
#pragma unroll
    for (int q = 0; q < n; q++) v = (idx == m + q) ? x[q] : v;
    return v;
  }

  // P of the trajectory that is rolled out in LDS (the nominal at entry): the (t, slot) pairs
  // spread over the wavefront as prep_box spreads its pairs, then a butterfly - every lane returns
  // the same bits.
  __device__ __forceinline__ T nominal_penalty(int Xo, int Uo, const T* g, int K,
                                               const BoxCfg<T, n>& b, T box_q1, const T* bl) const {
    T p = T(0);
    const int slots = active(g, K, b), pairs = (N + 1) * slots;
    for (int q = sl; q < pairs; q += 64) {
      const int t = q / slots;
      const Term s = term_spec(slot_of(q - t * slots, g, K, b), g, K, b, box_q1, bl);
      const int tu = t < N ? t : N - 1;  // (index N has no input: the value read is dropped)
      const T v = s.idx < m ? S[Uo + tu * m + s.idx] : S[Xo + t * n + (s.idx - m)];
      p += term_eval(s, v, S[Xo + t * n + 0], S[Xo + t * n + 1], t, t < N);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) p += __shfl_xor(p, d);
    return p;
  }

  // LsWorker::forward_ls that also returns the penalty of this lane's candidate (*pen).  The lanes
  // l, l + A, l + 2 A, ... (A step sizes, a power of two) run identical copies of candidate l mod A:
  // copy l / A takes the slots l / A, l / A + 64 / A, ... of every step - one slot per lane unless
  // more than 64 / A slots can count - from the x_t and u_t the step holds in registers, into an accumulator of its
  // own: nothing of it feeds x_{t+1}.  After the loop the copies' partial sums are added up in a
  // butterfly over the strides 32 ... A: one fixed order, the same bits on every copy.  Returns
  // this lane's barrier-free cost, forward_ls's bit for bit.
  template <bool GENERAL>
  __device__ __forceinline__ T forward_merit(int Xo, int Uo, int Xn, int Un, const T (&xT)[n], T alpha,
                                             bool* bad, int A, const T* g, int K,
                                             const BoxCfg<T, n>& b, T box_q1, const T* bl,
                                             T* pen) const {
    T x[n], u[m], xn[n];
#pragma unroll
    for (int i = 0; i < n; i++) x[i] = S[Xo + i];
    this->template publish<n>(Xn, x);
    T cost = T(0), p = T(0);
    const int copies = 64 / A, copy = sl / A;
    const int rounds = (active(g, K, b) + copies - 1) / copies;
    const Term first = term_spec(slot_of(copy, g, K, b), g, K, b, box_q1, bl);  // (the same slot in every step)
    auto terms = [&](const int t, const bool with_u) __attribute__((always_inline)) {
      p += term_eval(first, comp(u, x, first.idx), x[0], x[1], t, with_u);
      for (int r = 1; r < rounds; r++) {
        const Term s = term_spec(slot_of(copy + r * copies, g, K, b), g, K, b, box_q1, bl);
        p += term_eval(s, comp(u, x, s.idx), x[0], x[1], t, with_u);
      }
    };
    T xo[n], uo[m], kk[m][n + 1];
    auto load_step = [&](int t) {
#pragma unroll
      for (int j = 0; j < n; j++) xo[j] = S[Xo + t * n + j];
#pragma unroll
      for (int a = 0; a < m; a++) {
        uo[a] = S[Uo + t * m + a];
#pragma unroll
        for (int j = 0; j <= n; j++) kk[a][j] = S[L.Kk + (t * m + a) * (n + 1) + j];
      }
    };
    load_step(0);
    auto step = [&](const int t) __attribute__((always_inline)) {
#pragma unroll
      for (int a = 0; a < m; a++) {
        T acc = T(0);
#pragma unroll
        for (int j = 0; j < n; j++) acc = t_fma(kk[a][j], x[j] - xo[j], acc);
        u[a] = clip(uo[a] + alpha * kk[a][n] + acc, -c.u_max[a], c.u_max[a]);
      }
      load_step(t + 1 < N ? t + 1 : t);
      this->template publish<m>(Un + t * m, u);
      T tr[NT];
      Sys::template trig_g<GENERAL>(x, tr, bad);
      Sys::step_tr(c, x, u, tr, xn);
      this->template publish<n>(Xn + (t + 1) * n, xn);
      cost = cost + this->stage_cost(x, xT, u);
      terms(t, true);
#pragma unroll
      for (int i = 0; i < n; i++) x[i] = xn[i];
    };
    int t = 0;
    for (; t + 1 < N; t += 2) {
      step(t);
      step(t + 1);
    }
    if (t < N) step(t);
    cost = cost + this->terminal_cost(x, xT);
#pragma unroll
    for (int a = 0; a < m; a++) u[a] = T(0);  // (index N: the input sides are dropped)
    terms(N, false);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const T o = __shfl_xor(p, d);
      if (d >= A) p += o;
    }
    wave_sync();
    *pen = p;
    return cost;
  }
};

}  // namespace i2lqr
