// Instantiations and launcher of the fixed-horizon form of the sixteen-lane kernel
// (k_group_iterate_fixed, i2lqr_group.hpp): bicycle4 and bicycle6, fp32 and fp64, H = 1, 2, 3, for
// every horizon of I2LQR_GROUP_FIXED_HORIZONS (i2lqr_group.h) — a translation unit of its own, so
// that these kernels compile beside those of i2lqr_group.hip.
#include "i2lqr_group.h"

#include "i2lqr_devcfg.hpp"
#include "i2lqr_group.hpp"
#include "i2lqr_dryrun.hpp"  // (empty unless -DI2LQR_DRY_RUN: the ASan build)
#include "i2lqr_group_launch.hpp"

namespace i2lqr {

namespace {

template <class T, class Sys, int H, int NH>
hipError_t launch_fixed_h(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s) {
  const auto c = make_dev_cfg<T, Sys::n, Sys::m>(cfg);
  const size_t lds = group_lds_bytes<T, Sys, 16>(cfg.N);  // the layout of the run-time form
  if (hipError_t e = raise_lds_limit<k_group_iterate_fixed<T, Sys, H, NH>>(lds); e != hipSuccess)
    return e;
  const unsigned grid = (unsigned)((a.B + 3) / 4);
  hipLaunchKernelGGL((k_group_iterate_fixed<T, Sys, H, NH>), dim3(grid), dim3(64 * H), lds, s, c, a);
  return hipGetLastError();
}
template <class T, class Sys, int NH>
hipError_t launch_fixed(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s, int helpers) {
  if (helpers == 3) return launch_fixed_h<T, Sys, 3, NH>(cfg, a, s);
  if (helpers == 2) return launch_fixed_h<T, Sys, 2, NH>(cfg, a, s);
  return launch_fixed_h<T, Sys, 1, NH>(cfg, a, s);
}

}  // namespace

bool group16_fixed_horizon(int N) {
#define I2LQR_X(NH) if (N == NH) return true;
  I2LQR_GROUP_FIXED_HORIZONS(I2LQR_X)
#undef I2LQR_X
  return false;
}

template <class T>
hipError_t group16_iterate_fixed(const i2lqr_config& cfg, const IterArgs<T>& a, hipStream_t s,
                                 int wavefronts) {
  return visit_bicycle<T>(cfg, [&](auto, auto sys) -> hipError_t {
    using Sys = decltype(sys);
#define I2LQR_X(NH) if (cfg.N == NH) return launch_fixed<T, Sys, NH>(cfg, a, s, wavefronts);
    I2LQR_GROUP_FIXED_HORIZONS(I2LQR_X)
#undef I2LQR_X
    return hipErrorInvalidValue;  // not a horizon of the list: the caller asks group16_fixed_horizon
  });
}

template hipError_t group16_iterate_fixed<double>(const i2lqr_config&, const IterArgs<double>&,
                                                  hipStream_t, int);
template hipError_t group16_iterate_fixed<float>(const i2lqr_config&, const IterArgs<float>&,
                                                 hipStream_t, int);

}  // namespace i2lqr
