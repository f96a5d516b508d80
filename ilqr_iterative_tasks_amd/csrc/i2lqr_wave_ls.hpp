// LsWorker: the one-problem-per-wavefront Worker (i2lqr_wave.hpp) with the line search's forward
// pass.  Shared by the units that build on it: i2lqr_wave_ls.hip (k_iterate_ls) and
// i2lqr_wave_obs.hip (k_iterate_obs).
#pragma once
#include "i2lqr_wave.hpp"

namespace i2lqr {

constexpr int kLsMaxSteps = 8;

template <class T, class Sys, bool HASQR> struct LsWorker : Worker<T, Sys, 64, HASQR> {
  using Base = Worker<T, Sys, 64, HASQR>;
  static constexpr int n = Sys::n, m = Sys::m, NT = Sys::NTRIG;
  using Base::c;
  using Base::L;
  using Base::N;
  using Base::S;
  using Base::sl;

  __device__ LsWorker(const typename Base::Cfg& c_, T* smem, int lane) : Base(c_, smem, lane) {}

  // Worker::forward with the feed-forward term scaled by this LANE's alpha (a power of two: the
  // product is exact; the association (u + alpha k) + K dx is Worker::forward's).  Lane 0
  // publishes its own candidate to (Xn, Un); returns this lane's cost.
  template <bool GENERAL>
  __device__ __forceinline__ T forward_ls(int Xo, int Uo, int Xn, int Un, const T (&xT)[n], T alpha,
                                          bool* bad) const {
    T x[n], u[m], xn[n];
#pragma unroll
    for (int i = 0; i < n; i++) x[i] = S[Xo + i];
    this->template publish<n>(Xn, x);
    T cost = T(0);
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
    wave_sync();
    return cost;
  }
};

}  // namespace i2lqr
