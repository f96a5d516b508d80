// ObsWorker: LsWorker (i2lqr_wave_ls.hpp) with the several-obstacles prep.  Shared by the units
// that build on it: i2lqr_wave_obs.hip (k_iterate_obs) and i2lqr_wave_box.hip (k_iterate_box).
#pragma once
#include "i2lqr_wave_ls.hpp"

namespace i2lqr {

template <class T, class Sys, bool HASQR> struct ObsWorker : LsWorker<T, Sys, HASQR> {
  using Ls = LsWorker<T, Sys, HASQR>;
  using Base = typename Ls::Base;
  static constexpr int n = Sys::n, m = Sys::m;
  using Base::c;
  using Base::L;
  using Base::N;
  using Base::S;
  using Base::sl;

  __device__ ObsWorker(const typename Base::Cfg& c_, T* smem, int lane) : Ls(c_, smem, lane) {}

  // Worker::prep for record 0 (ob), then records 1 ... K - 1 of this problem (g: obs[K][6] in LDS,
  // or NULL) into the same five words of every t: the lane that wrote them adds to them.
  __device__ __forceinline__ void prep_obs(int Xo, int Uo, const T (&ob)[6], const T* g,
                                           int K) const {
    Base::prep(Xo, Uo, ob);
    if (g) {
      for (int t = sl; t <= N; t += 64) {
        const T px = S[Xo + t * n + 0], py = S[Xo + t * n + 1];
        T o0 = S[L.ob + t * 5 + 0], o1 = S[L.ob + t * 5 + 1], o2 = S[L.ob + t * 5 + 2],
          o3 = S[L.ob + t * 5 + 3], o4 = S[L.ob + t * 5 + 4];
        bool first = !(ob[5] >= T(0));  // nothing written yet: the next record's words are stored
        for (int r = 1; r < K; r++) {
          const T* rec = g + r * 6;
          const T r5 = rec[5];
          if (r5 >= T(0)) {
            // obstacle barrier: control/ilqr_helper.py:32-51 (stage) / :121-147 (terminal, index N)
            const T r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3], r4 = rec[4];
            const int opt = (int)r5;
            T dz = px - r0, dy = py - r1;
            if (opt == 1) dy = py - (r1 + T(t) * r4);
            if (opt == 2) dz = px - (r0 - T(t) * r4);
            const T pa = T(1) / (r2 * r2), pb = T(1) / (r3 * r3);
            const T h = T(1) + c.safety_margin - (dz * pa * dz + dy * pb * dy);
            const T hd0 = T(-2) * pa * dz, hd1 = T(-2) * pb * dy;
            const T e = t_exp(c.obs_q2 * h);
            const T c1 = c.obs_q12 * e, c2 = c.obs_q122 * e;
            const T a0 = c1 * hd0, a1 = c1 * hd1, a2 = c2 * (hd0 * hd0), a3 = c2 * (hd0 * hd1),
                    a4 = c2 * (hd1 * hd1);
            o0 = first ? a0 : o0 + a0;
            o1 = first ? a1 : o1 + a1;
            o2 = first ? a2 : o2 + a2;
            o3 = first ? a3 : o3 + a3;
            o4 = first ? a4 : o4 + a4;
            first = false;
          }
        }
        S[L.ob + t * 5 + 0] = o0;
        S[L.ob + t * 5 + 1] = o1;
        S[L.ob + t * 5 + 2] = o2;
        S[L.ob + t * 5 + 3] = o3;
        S[L.ob + t * 5 + 4] = o4;
      }
    }
    wave_sync();
  }
};

}  // namespace i2lqr
