// Instantiations and launcher of the eight-lanes-per-problem kernel (i2lqr_group.hpp).
#include "i2lqr_group.h"

#include "i2lqr_devcfg.hpp"
#include "i2lqr_geometry.hpp"
#include "i2lqr_group.hpp"
#include "i2lqr_dryrun.hpp"  // (empty unless -DI2LQR_DRY_RUN: the ASan build)
#include "i2lqr_group_launch.hpp"

namespace i2lqr {

namespace {

template <class T, class Sys, int H, int G = kGroup>
hipError_t launch_h(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  const auto c = make_dev_cfg<T, Sys::n, Sys::m>(cfg);
  const size_t lds = group_lds_bytes<T, Sys, G>(cfg.N);
  if (hipError_t e = raise_lds_limit<k_group_iterate<T, Sys, H, false, G>>(lds); e != hipSuccess)
    return e;
  constexpr int PW = 64 / G;
  const unsigned grid = (unsigned)((a.B + PW - 1) / PW);
  hipLaunchKernelGGL((k_group_iterate<T, Sys, H, false, G>), dim3(grid), dim3(64 * H), lds, s, c, a,
                     (T*)nullptr);
  return hipGetLastError();
}
// (how many wavefronts H a workgroup gets, and which form runs: i2lqr_column_plan.hpp)
// Workspace form (k_group_iterate<.., 1, true>): records and gains in HBM, 4 KB of LDS per problem
template <class T, class Sys>
hipError_t launch_ws(const i2lqr_config& cfg, const IterArgs<T>& a, void* ws, hipStream_t s) {
  const auto c = make_dev_cfg<T, Sys::n, Sys::m>(cfg);
  const size_t lds = (size_t)GLayout<Sys>(cfg.N, true).wave_words() * sizeof(T);
  if (hipError_t e = raise_lds_limit<k_group_iterate<T, Sys, 1, true>>(lds); e != hipSuccess) return e;
  const unsigned grid = (unsigned)((a.B + kGroupsPerWave - 1) / kGroupsPerWave);
  hipLaunchKernelGGL((k_group_iterate<T, Sys, 1, true>), dim3(grid), dim3(64), lds, s, c, a, (T*)ws);
  return hipGetLastError();
}

template <class T, class Sys, int V, int G = kGroup> size_t spec_lds_bytes(int N) {
  return (size_t)GSpecLayout<Sys, V, G>(N).group_words() * sizeof(T);
}

// SETIO: a.count_max problems at most (k_group_spec<.., true>, the tail of the chunked solves)
template <class T, class Sys, int V, bool SETIO, int G>
hipError_t launch_spec_v(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  const auto c = make_dev_cfg<T, Sys::n, Sys::m>(cfg);
  const size_t lds = spec_lds_bytes<T, Sys, V, G>(cfg.N);
  if (hipError_t e = raise_lds_limit<k_group_spec<T, Sys, V, SETIO, G>>(lds); e != hipSuccess)
    return e;
  constexpr int PW = 64 / G;
  const int64_t problems = SETIO ? (int64_t)a.count_max : a.B;
  const unsigned grid = (unsigned)((problems + PW - 1) / PW);
  hipLaunchKernelGGL((k_group_spec<T, Sys, V, SETIO, G>), dim3(grid), dim3(64 * V), lds, s, c, a);
  return hipGetLastError();
}
template <class T, class Sys, bool SETIO, int G>
hipError_t launch_spec(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s, int wavefronts) {
  if (wavefronts == 3) return launch_spec_v<T, Sys, 3, SETIO, G>(cfg, a, s);
  return launch_spec_v<T, Sys, 2, SETIO, G>(cfg, a, s);
}
template <class T, bool SETIO>
hipError_t launch_spec_any(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s, int lanes,
                           int wavefronts) {
  return visit_bicycle<T>(cfg, [&](auto, auto sys) {
    using Sys = decltype(sys);
    return lanes == 16 ? launch_spec<T, Sys, SETIO, 16>(cfg, a, s, wavefronts)
                       : launch_spec<T, Sys, SETIO, kGroup>(cfg, a, s, wavefronts);
  });
}

}  // namespace

static_assert(kGroupsPerWave == kEightLaneProblems && kGroup == 8, "i2lqr_column_plan.hpp");

// The bytes of every form of the eight- / sixteen-lane kernels for a bicycle configuration
void column_fit_group(const i2lqr_config& cfg, ColumnFit& fit) {
  if (fit.plant != ColumnFit::BICYCLE) return;
  fit.fixed_horizon = group16_fixed_horizon(cfg.N);
  visit_bicycle(cfg, [&](auto t, auto sys) {
    using T = decltype(t);
    using Sys = decltype(sys);
    const int N = cfg.N;
    fit.lds_group8 = group_lds_bytes<T, Sys, kGroup>(N);
    fit.lds_group16 = group_lds_bytes<T, Sys, 16>(N);
    fit.lds_group_ws = (size_t)GLayout<Sys>(N, true).wave_words() * sizeof(T);
    fit.ws_group = (int64_t)GLayout<Sys>(N, true).ws_words() * (int64_t)sizeof(T);
    fit.lds_spec8x2 = spec_lds_bytes<T, Sys, 2, kGroup>(N);
    fit.lds_spec8x3 = spec_lds_bytes<T, Sys, 3, kGroup>(N);
    fit.lds_spec16x2 = spec_lds_bytes<T, Sys, 2, 16>(N);
    fit.lds_spec16x3 = spec_lds_bytes<T, Sys, 3, 16>(N);
  });
}

// (the lane launcher asks per call, whatever the handle's layout: the current device's geometry)
int group_spec_tail_lanes(const i2lqr_config& cfg) {
  ColumnFit fit = column_fit_config(cfg);
  column_fit_group(cfg, fit);
  return spec_tail_lanes(device_geometry(), fit);
}
bool group_spec_tail_supported(const i2lqr_config& cfg) { return group_spec_tail_lanes(cfg) != 0; }

// chains (k_group_spec<.., 3, false, 16, true>): the sixteen-lane form with three wavefronts
template <class T, class Sys>
hipError_t launch_spec_chain(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  const auto c = make_dev_cfg<T, Sys::n, Sys::m>(cfg);
  const size_t lds = spec_lds_bytes<T, Sys, 3, 16>(cfg.N);
  if (hipError_t e = raise_lds_limit<k_group_spec<T, Sys, 3, false, 16, true>>(lds); e != hipSuccess)
    return e;
  const unsigned grid = (unsigned)((a.B + 3) / 4);
  hipLaunchKernelGGL((k_group_spec<T, Sys, 3, false, 16, true>), dim3(grid), dim3(64 * 3), lds, s, c, a);
  return hipGetLastError();
}
template <class T>
hipError_t group_spec_chain(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  return visit_bicycle<T>(cfg, [&](auto, auto sys) {
    return launch_spec_chain<T, decltype(sys)>(cfg, a, s);
  });
}
template <class T>
hipError_t group_spec_iterate(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s, int lanes,
                              int wavefronts) {
  return launch_spec_any<T, false>(cfg, a, s, lanes, wavefronts);
}
template <class T>
hipError_t group_spec_tail(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  return launch_spec_any<T, true>(cfg, a, s, group_spec_tail_lanes(cfg), 2);
}

template <class T>
hipError_t group16_iterate(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s, int wavefronts,
                           bool fixed) {
  if (fixed) return group16_iterate_fixed<T>(cfg, a, s, wavefronts);
  return visit_bicycle<T>(cfg, [&](auto, auto sys) {
    using Sys = decltype(sys);
    if (wavefronts == 3) return launch_h<T, Sys, 3, 16>(cfg, a, s);
    if (wavefronts == 2) return launch_h<T, Sys, 2, 16>(cfg, a, s);
    return launch_h<T, Sys, 1, 16>(cfg, a, s);
  });
}

template <class T>
hipError_t group_iterate_ws(const i2lqr_config& cfg, const IterArgs<T>& a, void* ws, hipStream_t s) {
  return visit_bicycle<T>(cfg, [&](auto, auto sys) {
    return launch_ws<T, decltype(sys)>(cfg, a, ws, s);
  });
}

template <class T>
hipError_t group_iterate(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s, int wavefronts) {
  return visit_bicycle<T>(cfg, [&](auto, auto sys) {
    using Sys = decltype(sys);
    if (wavefronts == 3) return launch_h<T, Sys, 3>(cfg, a, s);
    return launch_h<T, Sys, 1>(cfg, a, s);
  });
}

#define I2LQR_GROUP_LAUNCHERS(T)                                                                    \
  template hipError_t group_iterate<T>(const i2lqr_config&, const IterArgs<T>&, hipStream_t, int);  \
  template hipError_t group16_iterate<T>(const i2lqr_config&, const IterArgs<T>&, hipStream_t, int, \
                                         bool);                                                    \
  template hipError_t group_iterate_ws<T>(const i2lqr_config&, const IterArgs<T>&, void*,           \
                                          hipStream_t);                                             \
  template hipError_t group_spec_iterate<T>(const i2lqr_config&, const IterArgs<T>&, hipStream_t,   \
                                            int, int);                                              \
  template hipError_t group_spec_chain<T>(const i2lqr_config&, const IterArgs<T>&, hipStream_t);    \
  template hipError_t group_spec_tail<T>(const i2lqr_config&, const IterArgs<T>&, hipStream_t);
I2LQR_GROUP_LAUNCHERS(double)
I2LQR_GROUP_LAUNCHERS(float)

}  // namespace i2lqr
