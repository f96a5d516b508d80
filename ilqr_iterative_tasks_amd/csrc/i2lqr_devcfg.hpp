// Host side: i2lqr_config (include/i2lqr.h) -> the typed device copy the kernels take by value.
#pragma once
#include <cmath>
#include <cstring>
#include <type_traits>

#include "../../include/i2lqr.h"
#include "i2lqr_wave.hpp"

namespace i2lqr {

// Debug build: the device word the kernels record an index violation in (i2lqr_debug.hpp), one
// per process and device, allocated on first use (i2lqr_abi.hip); null in the product build.
unsigned long long* debug_trap_word();

// FLAG_HAS_Q / FLAG_HAS_R: a non-zero entry in the n x n block of Q / the m x m block of R, the
// entries make_dev_cfg hands the kernels (the padding of the I2LQR_MAX_N / I2LQR_MAX_M arrays is
// never read)
inline int stage_weight_flags(const i2lqr_config& h, int n, int m) {
  int flags = 0;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++)
      if (h.Q[i * I2LQR_MAX_N + j] != 0.0) flags |= FLAG_HAS_Q;
  for (int a = 0; a < m; a++)
    for (int b = 0; b < m; b++)
      if (h.R[a * I2LQR_MAX_M + b] != 0.0) flags |= FLAG_HAS_R;
  return flags;
}
// true if the configuration has stage weights (Q or R != 0): DevCfg::flags != 0
inline bool has_stage_weights(const i2lqr_config& h) { return stage_weight_flags(h, h.n, h.m) != 0; }

// f(T()) for the precision a (validated) configuration names
template <class F> auto visit_precision(const i2lqr_config& cfg, F&& f) {
  if (cfg.dtype == I2LQR_F64) return f(double());
  return f(float());
}
// f(T(), Sys()) for the plant and precision a (validated) configuration names; T fixes the
// precision instead.  visit_bicycle: the two m = 2 plants (any other system id: bicycle6).
template <class T = void, class F> auto visit_bicycle(const i2lqr_config& cfg, F&& f) {
  if constexpr (std::is_void_v<T>) {
    return cfg.dtype == I2LQR_F64 ? visit_bicycle<double>(cfg, f) : visit_bicycle<float>(cfg, f);
  } else {
    if (cfg.system_id == I2LQR_SYS_BICYCLE4) return f(T(), Bicycle4<T>());
    return f(T(), Bicycle6<T>());
  }
}
template <class T = void, class F> auto visit_plant(const i2lqr_config& cfg, F&& f) {
  if constexpr (std::is_void_v<T>) {
    return cfg.dtype == I2LQR_F64 ? visit_plant<double>(cfg, f) : visit_plant<float>(cfg, f);
  } else {
    if (cfg.system_id == I2LQR_SYS_QUAD12) return f(T(), Quad12<T>());
    return visit_bicycle<T>(cfg, f);
  }
}

template <class T, int n, int m> inline DevCfg<T, n, m> make_dev_cfg(const i2lqr_config& h) {
  DevCfg<T, n, m> d;
  std::memset(&d, 0, sizeof(d));
  d.N = h.N;
  d.max_iter = h.max_iter;
  d.dt = (T)h.dt;
  d.eps = (T)h.eps;
  d.lamb_factor = (T)h.lamb_factor;
  d.max_lamb = (T)h.max_lamb;
  d.ctrl_q1 = (T)h.ctrl_q1;
  d.ctrl_q2 = (T)h.ctrl_q2;
  d.obs_q1 = (T)h.obs_q1;
  d.obs_q2 = (T)h.obs_q2;
  d.safety_margin = (T)h.safety_margin;
  d.fast_barrier = 1;
  for (int a = 0; a < m; a++) {
    d.u_max[a] = (T)h.u_max[a];
    const double span = 2.0 * h.ctrl_q2 * h.u_max[a];
    d.ctrl_c[a] = (T)std::exp(-span);
    if (!(std::fabs(span) < 600.0)) d.fast_barrier = 0;
  }
  for (int i = 0; i < n; i++) d.xtarget[i] = (T)h.xtarget[i];
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      d.Q[i * n + j] = (T)h.Q[i * I2LQR_MAX_N + j];
      d.Qt[i * n + j] = (T)h.Qt[i * I2LQR_MAX_N + j];
    }
  for (int a = 0; a < m; a++)
    for (int b = 0; b < m; b++) d.R[a * m + b] = (T)h.R[a * I2LQR_MAX_M + b];
  for (int q = 0; q < 8; q++) d.sys_par[q] = (T)h.sys_par[q];
  d.ctrl_q12 = d.ctrl_q1 * d.ctrl_q2;
  d.ctrl_q122 = d.ctrl_q1 * (d.ctrl_q2 * d.ctrl_q2);
  d.obs_q12 = d.obs_q1 * d.obs_q2;
  d.obs_q122 = d.obs_q1 * (d.obs_q2 * d.obs_q2);
  if (h.system_id == I2LQR_SYS_QUAD12) {  // Quad12::step_tr / jac_var / plant_const read these
    const T mass = d.sys_par[0], g = d.sys_par[1], arm = d.sys_par[2];
    const T Ix = d.sys_par[3], Iy = d.sys_par[4], Iz = d.sys_par[5], ct = d.sys_par[6];
    d.pd[0] = T(1) / mass;
    d.pd[1] = arm / Ix;
    d.pd[2] = arm / Iy;
    d.pd[3] = ct / Iz;
    d.pd[4] = (Iy - Iz) / Ix;
    d.pd[5] = (Iz - Ix) / Iy;
    d.pd[6] = (Ix - Iy) / Iz;
    d.pd[7] = mass * g;
    for (int q = 0; q < 6; q++) {
      const T v = q < 2 ? d.dt * arm / Ix : (q < 4 ? d.dt * arm / Iy : d.dt * ct / Iz);
      d.pd[8 + q] = (q & 1) ? -v : v;
    }
  }
  d.flags = stage_weight_flags(h, n, m);
  d.trap = debug_trap_word();
  return d;
}


}  // namespace i2lqr
