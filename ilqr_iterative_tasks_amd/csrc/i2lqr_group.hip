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
// Sixteen lanes per problem (one problem per DPP row, four per wavefront): the backward step
// exchanges nothing through LDS (GroupWorker::backward_row).  One helper wavefront for the record
// phase (2 x 16 lanes >= the 21 records of a problem: one round) while that leaves every wavefront
// a SIMD of its own (<= 512 workgroups = 2048 problems).  Overlapped schedule (k_group_iterate<..,
// 3, false, 16>; overlap = false forces the one-helper form): two helpers take all the records
// while the main wavefront computes the terminal block, and they store the gains at exit — while
// every workgroup has a CU to itself (<= 256 workgroups = 1024 problems: three SIMDs of four).
// fixed: the fixed-horizon kernel (k_group_iterate_fixed, i2lqr_group_fixed.hip) with the same number
// of wavefronts, where the horizon is one it is built for; no effect for any other horizon.
template <class T, class Sys>
hipError_t launch16(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s, bool overlap,
                    bool fixed) {
  const int64_t cus = device_geometry().cus;
  int wavefronts = 1;
#ifndef I2LQR_STAMPS
  if (overlap && (a.B + 3) / 4 <= cus) wavefronts = 3;
  else if ((a.B + 3) / 4 <= 2 * cus) wavefronts = 2;
  if (fixed && group16_fixed_horizon(cfg.N)) return group16_iterate_fixed<T>(cfg, a, s, wavefronts);
#endif
  if (wavefronts == 3) return launch_h<T, Sys, 3, 16>(cfg, a, s);
  if (wavefronts == 2) return launch_h<T, Sys, 2, 16>(cfg, a, s);
  return launch_h<T, Sys, 1, 16>(cfg, a, s);
}
// Two helper wavefronts for the record phase (k_group_iterate<.., 3>) while every workgroup has
// a CU to itself (<= 256 workgroups = 2048 problems): 0.2216 -> 0.2107 ms per 10 iterations at
// 1024 problems (two / four wavefronts: 0.2122 / 0.2102).  With two workgroups per CU the extra
// wavefronts crowd the main ones off their SIMDs: 0.25 -> 0.40 ms at 4096 problems.
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

template <class T, class Sys>
hipError_t launch(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  const int64_t cus = device_geometry().cus;
#ifndef I2LQR_STAMPS  // (the diagnostic build stamps the phases of the lone wavefront)
  if ((a.B + kGroupsPerWave - 1) / kGroupsPerWave <= cus) return launch_h<T, Sys, 3>(cfg, a, s);
#endif
  return launch_h<T, Sys, 1>(cfg, a, s);
}

// Wavefronts per group of eight problems in the speculative kernel.  Three skip two rejects per
// round but share one CU's LDS three ways; the stragglers that decide a solve's duration alternate
// accept / reject, which two wavefronts cover: measured (i2lqr_solve, ms) 16 problems 0.43 (V = 3)
// / 0.46 (V = 2), 256: 0.25 / 0.26, 1024: 0.77 / 0.72, 2048: 0.70 / 0.50, tail of 65536: 2.41 /
// 2.34.  Three up to kSpecWideBatch problems where they fit, two above and in the tail.
constexpr int kSpecWideBatch = 512;

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
hipError_t launch_spec(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  const DeviceGeometry& geo = device_geometry();
  const bool wide = !SETIO && a.B <= geo.scaled(kSpecWideBatch) &&
                    spec_lds_bytes<T, Sys, 3, G>(cfg.N) <= geo.max_dyn_lds;
  if (wide) return launch_spec_v<T, Sys, 3, SETIO, G>(cfg, a, s);
  return launch_spec_v<T, Sys, 2, SETIO, G>(cfg, a, s);
}
template <class T, bool SETIO>
hipError_t launch_spec_any(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s, int lanes) {
  return visit_bicycle<T>(cfg, [&](auto, auto sys) {
    using Sys = decltype(sys);
    return lanes == 16 ? launch_spec<T, Sys, SETIO, 16>(cfg, a, s)
                       : launch_spec<T, Sys, SETIO, kGroup>(cfg, a, s);
  });
}

template <int G> bool spec_lds_fits(const i2lqr_config& cfg) {  // the two-wavefront form
  const size_t lds = visit_bicycle(cfg, [&](auto t, auto sys) {
    return spec_lds_bytes<decltype(t), decltype(sys), 2, G>(cfg.N);
  });
  return lds <= device_geometry().max_dyn_lds;
}
bool spec_plant_ok(const i2lqr_config& cfg) {
  if (cfg.system_id != I2LQR_SYS_BICYCLE4 && cfg.system_id != I2LQR_SYS_BICYCLE6) return false;
  return !has_stage_weights(cfg);
}
// the LDS form of the eight- / sixteen-lane kernel fits: the bicycles, Q = R = 0, problem-major
template <int G> bool group_lds_fits(const i2lqr_config& cfg) {
  if (!spec_plant_ok(cfg) || cfg.layout != I2LQR_LAYOUT_PROBLEM_MAJOR) return false;
  const size_t lds = visit_bicycle(cfg, [&](auto t, auto sys) {
    return group_lds_bytes<decltype(t), decltype(sys), G>(cfg.N);
  });
  return lds <= device_geometry().max_dyn_lds;
}

}  // namespace

bool group_spec_supported(const i2lqr_config& cfg, int lanes) {
  if (!spec_plant_ok(cfg) || cfg.layout != I2LQR_LAYOUT_PROBLEM_MAJOR) return false;
  return lanes == 16 ? spec_lds_fits<16>(cfg) : (group_supported(cfg) && spec_lds_fits<kGroup>(cfg));
}
int group_spec_tail_lanes(const i2lqr_config& cfg) {
  if (!spec_plant_ok(cfg)) return 0;
  return spec_lds_fits<16>(cfg) ? 16 : (spec_lds_fits<kGroup>(cfg) ? kGroup : 0);
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
bool group_spec_chain_supported(const i2lqr_config& cfg, int64_t chains) {
  if (!spec_plant_ok(cfg) || cfg.layout != I2LQR_LAYOUT_PROBLEM_MAJOR) return false;
  const DeviceGeometry& geo = device_geometry();
  if (chains > geo.scaled(kSpecWideBatch)) return false;  // three wavefronts per workgroup
  const size_t lds = visit_bicycle(cfg, [&](auto t, auto sys) {
    return spec_lds_bytes<decltype(t), decltype(sys), 3, 16>(cfg.N);
  });
  return lds <= geo.max_dyn_lds;
}
template <class T>
hipError_t group_spec_chain(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  return visit_bicycle<T>(cfg, [&](auto, auto sys) {
    return launch_spec_chain<T, decltype(sys)>(cfg, a, s);
  });
}
template <class T>
hipError_t group_spec_iterate(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s, int lanes) {
  return launch_spec_any<T, false>(cfg, a, s, lanes);
}
template <class T>
hipError_t group_spec_tail(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  return launch_spec_any<T, true>(cfg, a, s, group_spec_tail_lanes(cfg));
}

bool group16_supported(const i2lqr_config& cfg) { return group_lds_fits<16>(cfg); }
template <class T>
hipError_t group16_iterate(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s, bool overlap,
                           bool fixed) {
  return visit_bicycle<T>(cfg, [&](auto, auto sys) {
    return launch16<T, decltype(sys)>(cfg, a, s, overlap, fixed);
  });
}

bool group_supported(const i2lqr_config& cfg) { return group_lds_fits<kGroup>(cfg); }

int64_t group_workspace_bytes(const i2lqr_config& cfg, int64_t B) {
  if (!group_supported(cfg) || B <= 0) return 0;
  const int64_t probs = (B + kGroupsPerWave - 1) / kGroupsPerWave * kGroupsPerWave;
  const int64_t words = visit_bicycle<double>(cfg, [&](auto, auto sys) {
    return GLayout<decltype(sys)>(cfg.N, true).ws_words();
  });
  const size_t lds = visit_bicycle(cfg, [&](auto t, auto sys) {
    return (size_t)GLayout<decltype(sys)>(cfg.N, true).wave_words() * sizeof(t);
  });
  if (lds > device_geometry().max_dyn_lds) return 0;
  return probs * words * (cfg.dtype == I2LQR_F64 ? 8 : 4);
}
template <class T>
hipError_t group_iterate_ws(const i2lqr_config& cfg, const IterArgs<T>& a, void* ws, hipStream_t s) {
  return visit_bicycle<T>(cfg, [&](auto, auto sys) {
    return launch_ws<T, decltype(sys)>(cfg, a, ws, s);
  });
}

template <class T>
hipError_t group_iterate(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  return visit_bicycle<T>(cfg, [&](auto, auto sys) { return launch<T, decltype(sys)>(cfg, a, s); });
}

#define I2LQR_GROUP_LAUNCHERS(T)                                                                    \
  template hipError_t group_iterate<T>(const i2lqr_config&, const IterArgs<T>&, hipStream_t);       \
  template hipError_t group16_iterate<T>(const i2lqr_config&, const IterArgs<T>&, hipStream_t, bool, \
                                         bool);                                                    \
  template hipError_t group_iterate_ws<T>(const i2lqr_config&, const IterArgs<T>&, void*,           \
                                          hipStream_t);                                             \
  template hipError_t group_spec_iterate<T>(const i2lqr_config&, const IterArgs<T>&, hipStream_t,   \
                                            int);                                                   \
  template hipError_t group_spec_chain<T>(const i2lqr_config&, const IterArgs<T>&, hipStream_t);    \
  template hipError_t group_spec_tail<T>(const i2lqr_config&, const IterArgs<T>&, hipStream_t);
I2LQR_GROUP_LAUNCHERS(double)
I2LQR_GROUP_LAUNCHERS(float)

}  // namespace i2lqr
