// The launcher of the opt-in forms of the one-problem-per-wavefront kernel (i2lqr_wave_opt.h); host
// code only: the kernels are reached through that header's `extern template` list and compiled in
// their own units.
#include "i2lqr_wave_opt.h"

#include "i2lqr_devcfg.hpp"
#include "i2lqr_dryrun.hpp"  // (empty unless -DI2LQR_DRY_RUN: the ASan build)
#include "i2lqr_group_launch.hpp"  // raise_lds_limit

namespace i2lqr {
namespace {

// One workgroup of one wavefront per problem (or chain); the attribute call is cached per kernel.
template <auto Kernel, class C, class T, class... Tail>
hipError_t launch(size_t lds, hipStream_t s, const C& c, const IterArgs<T>& a,
                  const Tail&... tail) {
  if (hipError_t e = raise_lds_limit<Kernel>(lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)a.B), dim3(64), lds, s, c, a, tail...);
  return hipGetLastError();
}

template <class T, class Sys, bool HASQR>
hipError_t launch_form(const i2lqr_config& cfg, const IterArgs<T>& a, const WaveModel& model,
                       bool chained, size_t lds, hipStream_t s) {
  const auto c = make_dev_cfg<T, Sys::n, Sys::m>(cfg);
  const WaveForm form = model.form(chained);
  lds += model.extra_lds_bytes(form, Sys::n, cfg.N, sizeof(T));  // records, d1, d2 behind the slice
  const int steps = model.steps(), n_obs = model.records();
  switch (form) {
    case WAVE_LS:
      return launch<k_iterate_ls<T, Sys, HASQR>>(lds, s, c, a, steps);
    case WAVE_OBS:
      return launch<k_iterate_obs<T, Sys, HASQR>>(lds, s, c, a, steps, n_obs);
    case WAVE_BOX: {
      const auto box = make_box_cfg<T, Sys::n>(model.box);
      return chained ? launch<k_chain_box<T, Sys, HASQR>>(lds, s, c, a, steps, n_obs, box)
                     : launch<k_iterate_box<T, Sys, HASQR>>(lds, s, c, a, steps, n_obs, box);
    }
    case WAVE_MERIT: {  // (a chained call never gets here: form(true) is the box form)
      const auto box = make_box_cfg<T, Sys::n>(model.box);
      return launch<k_iterate_merit<T, Sys, HASQR>>(lds, s, c, a, steps, n_obs, box, (T)model.box.q1);
    }
    case WAVE_PLAIN:
      break;
  }
  return hipErrorInvalidValue;
}

}  // namespace

template <class T>
hipError_t wave_opt_launch(const i2lqr_config& cfg, const IterArgs<T>& a, const WaveModel& model,
                           bool chained, size_t lds, hipStream_t s) {
  return visit_plant<T>(cfg, [&](auto, auto sys) {
    using Sys = decltype(sys);
    return has_stage_weights(cfg) ? launch_form<T, Sys, true>(cfg, a, model, chained, lds, s)
                                  : launch_form<T, Sys, false>(cfg, a, model, chained, lds, s);
  });
}

template hipError_t wave_opt_launch<double>(const i2lqr_config&, const IterArgs<double>&,
                                            const WaveModel&, bool, size_t, hipStream_t);
template hipError_t wave_opt_launch<float>(const i2lqr_config&, const IterArgs<float>&,
                                           const WaveModel&, bool, size_t, hipStream_t);

}  // namespace i2lqr
