// Launcher of the problem-major layout: one problem per wavefront (i2lqr_wave.hpp), eight or sixteen
// lanes per problem (i2lqr_group.h).  What a call decides from integers — the kernel, its wavefronts
// per workgroup, the workspace, the refusals — is i2lqr_column_plan.hpp, asked with the handle's
// geometry and ColumnFit; this header fills kernel arguments and launches.  Included by
// i2lqr_abi.hip only, behind i2lqr_lane_launch.hpp: the i2lqr_dryrun.hpp that header brings in (with
// the argument blocks of the lane kernels) records the launches below as well.
#pragma once
#include <hip/hip_runtime.h>

#include "i2lqr_column_plan.hpp"
#include "i2lqr_devcfg.hpp"
#include "i2lqr_group.h"
#include "i2lqr_handle.hpp"
#include "i2lqr_host.hpp"
#include "i2lqr_kernels.h"
#include "i2lqr_wave_opt.h"

namespace i2lqr {

// the epilogue of the i2lqr_iterate_pick call this thread is in (i2lqr_handle::Epilogue)
inline thread_local i2lqr_handle::Epilogue* t_epi = nullptr;

inline int64_t registered_ws(const i2lqr_handle* h) { return h->ws ? h->ws_bytes : -1; }
inline ColumnChoice column_kernel(const i2lqr_handle* h, int64_t B, bool early_exit) {
  return column_kernel(h->geo, h->fit, h->col, h->model.form(), registered_ws(h), B, early_exit);
}

// I2LQR_OK if the opt-in form of a call fits the device's dynamic LDS (wave_lds_need), else the
// refusal with the bytes
inline int wave_lds_check(const i2lqr_handle* h, bool chained) {
  const size_t need = wave_lds_need(h->fit, h->model, chained);
  if (need <= h->geo.max_dyn_lds) return I2LQR_OK;
  const WaveForm f = h->model.form(chained);
  const int n_obs = h->model.records();
  char with[64];
  if (f == WAVE_OBS)
    snprintf(with, sizeof(with), "\"obstacles\" = %d", n_obs);
  else
    snprintf(with, sizeof(with), "%s and %d obstacle record%s",
             chained ? "\"wave_chain\"" : wave_phrase(f), n_obs, n_obs > 1 ? "s" : "");
  return fail(I2LQR_ERR_UNSUPPORTED, "horizon %d with %s needs %zu B of LDS per wavefront (> %zu KiB)",
              h->cfg.N, with, need, h->geo.max_dyn_lds / 1024);
}

// One launcher per (dtype, system)
template <class T, class Sys> struct Launch {
  static constexpr int n = Sys::n, m = Sys::m, LANES = 64;  // one problem per wavefront
  static constexpr bool kBicycle = m == 2 && n + m <= 8;
  using Cfg = DevCfg<T, n, m>;

  static unsigned grid(int64_t B) { return (unsigned)B; }

  static int prepare(i2lqr_handle* h) {
    h->lanes = LANES;
    h->fit.lds_wave = (size_t)Layout<Sys>(h->cfg.N).total * sizeof(T);
    h->fit.lds_wave_fstep = kWaveHasFstep<Sys> ? wave_fstep_lds_bytes<T, Sys>(h->cfg.N) : 0;
    const size_t lds = h->fit.lds_wave;
    if (lds > h->geo.max_dyn_lds)
      return fail(I2LQR_ERR_UNSUPPORTED, "horizon %d needs %zu B of LDS per wavefront (> %zu KiB)",
                  h->cfg.N, lds, h->geo.max_dyn_lds / 1024);
    if (lds > h->geo.default_dyn_lds)
      for (const void* kernel :
           {(const void*)k_iterate<T, Sys, LANES, false>, (const void*)k_iterate<T, Sys, LANES, true>,
            (const void*)k_backward<T, Sys, LANES, false>, (const void*)k_backward<T, Sys, LANES, true>,
            (const void*)k_forward<T, Sys, LANES, false>, (const void*)k_forward<T, Sys, LANES, true>,
            (const void*)k_rollout<T, Sys, LANES, false>, (const void*)k_rollout<T, Sys, LANES, true>})
        HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return I2LQR_OK;
  }

  static int iterate(i2lqr_handle* h, const SolveIO& io, hipStream_t s) {
    const int64_t B = io.B;
    IterArgs<T> a = iter_args<T>(io);
    a.chains = h->col.opt_group_chains != 0;
#ifdef I2LQR_STAMPS
    a.dbg = (unsigned long long*)h->ws;  // diagnostic build: caller registers [B][8] u64 here
#endif
    const ColumnChoice choice = column_kernel(h, B, io.early_exit != 0);
    const ColumnKernel fk = choice.kernel;
    if (t_epi && (fk == K_GROUP || fk == K_GROUP16 || fk == K_GROUP_WS)) {  // the eight-lane kernels carry the epilogue
      a.qfun = t_epi->qfun;
      a.outer_iter = t_epi->outer_iter;
      a.max_relax_iter = t_epi->max_relax_iter;
      a.cost_it = (T*)t_epi->cost_it;
      if (t_epi->best_idx) {
        a.pick_part = (MinPair<T>*)t_epi->part;
        a.pick_ticket = h->ticket + h->ticket_next.fetch_add(1, std::memory_order_relaxed) %
                                        i2lqr_handle::kTickets;
        a.best_idx = t_epi->best_idx;
        a.best_cost = (T*)t_epi->best_cost;
      }
      t_epi->fused = true;
    }
    // (the diagnostic build stamps the phases of the lone wavefront of the run-time-horizon kernels)
#ifdef I2LQR_STAMPS
    constexpr bool stamps = true;
#else
    constexpr bool stamps = false;
#endif
    switch (fk) {
      case K_INVALID:
        return fail(I2LQR_ERR_UNSUPPORTED, "%s", choice.why);
      case K_SPEC:
      case K_SPEC16:
        if constexpr (kBicycle) {
          const int lanes = fk == K_SPEC16 ? 16 : 8;
          HIP_TRY(group_spec_iterate<T>(h->cfg, a, s, lanes,
                                        spec_wavefronts(h->geo, h->fit, lanes, B, false)));
          return I2LQR_OK;
        }
        break;
      case K_GROUP:
        if constexpr (kBicycle) {
          HIP_TRY(group_iterate<T>(h->cfg, a, s, stamps ? 1 : group8_wavefronts(h->geo, B)));
          return I2LQR_OK;
        }
        break;
      case K_GROUP16:
        if constexpr (kBicycle) {
          const int wavefronts =
              stamps ? 1 : group16_wavefronts(h->geo, B, h->col.opt_group_overlap != 0);
          HIP_TRY(group16_iterate<T>(h->cfg, a, s, wavefronts, !stamps && group16_fixed(h->fit, h->col)));
          return I2LQR_OK;
        }
        break;
      case K_GROUP_WS:
        if constexpr (kBicycle) {
          HIP_TRY(group_iterate_ws<T>(h->cfg, a, h->ws, s));
          return I2LQR_OK;
        }
        break;
      case K_QUAD:
        if constexpr (n + m == 16) {
          HIP_TRY(quad_iterate<T>(h->cfg, a, h->ws, s));
          return I2LQR_OK;
        }
        break;
      case K_WAVE_OPT:
        if (int rc = wave_lds_check(h, false)) return rc;
        HIP_TRY(wave_opt_launch<T>(h->cfg, a, h->model, false, h->fit.lds_wave, s));
        return I2LQR_OK;
      case K_WAVE:
        break;
    }
    const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
    if constexpr (kWaveHasFstep<Sys>) {
      if (wave_fstep(h->geo, h->fit, h->col, B)) {
        with_weights(c.flags, [&](auto W) {
          hipLaunchKernelGGL((k_iterate<T, Sys, LANES, W, true>), dim3(grid(B)), dim3(64),
                             h->fit.lds_wave_fstep, s, c, a);
        });
        HIP_TRY(hipGetLastError());
        return I2LQR_OK;
      }
    }
    with_weights(c.flags, [&](auto W) {
      hipLaunchKernelGGL((k_iterate<T, Sys, LANES, W>), dim3(grid(B)), dim3(64), h->fit.lds_wave, s, c, a);
    });
    HIP_TRY(hipGetLastError());
    return I2LQR_OK;
  }
  static int names_pair(const i2lqr_handle*, int64_t, int) { return 0; }
  static int names_model_chunks(const i2lqr_handle*, int64_t, int) { return 0; }
  // io.B chains of k problems each in ONE launch (chain_plan)
  static int solve_chained(i2lqr_handle* h, const SolveIO& io, int k, hipStream_t s) {
    const ChainPlan plan = chain_plan(h->geo, h->fit, h->col, h->model.form(), registered_ws(h), io.B);
    if (plan.kind == ChainPlan::REFUSED) return fail(I2LQR_ERR_UNSUPPORTED, "%s", plan.why);
    IterArgs<T> a = iter_args<T>(io);
    a.chain_len = k;
    a.chains = h->col.opt_group_chains != 0;
    if (plan.kind == ChainPlan::WAVE) {
      if (int rc = wave_lds_check(h, true)) return rc;
      HIP_TRY(wave_opt_launch<T>(h->cfg, a, h->model, true, h->fit.lds_wave, s));
    } else if constexpr (kBicycle) {
      HIP_TRY(group_spec_chain<T>(h->cfg, a, s));
    }
    return I2LQR_OK;
  }
  static int rollout(i2lqr_handle* h, int64_t B, void* X, void* U, const void* x_term, void* cost,
                     hipStream_t s) {
    const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
    with_weights(c.flags, [&](auto W) {
      hipLaunchKernelGGL((k_rollout<T, Sys, LANES, W>), dim3(grid(B)), dim3(64), h->fit.lds_wave, s, c,
                         B, (T*)X, (T*)U, (const T*)x_term, (T*)cost);
    });
    HIP_TRY(hipGetLastError());
    return I2LQR_OK;
  }
  static int backward(i2lqr_handle* h, int64_t B, const void* X, const void* U, const void* x_term,
                      const void* lamb, const void* obs, void* K, void* k, hipStream_t s) {
    const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
    with_weights(c.flags, [&](auto W) {
      hipLaunchKernelGGL((k_backward<T, Sys, LANES, W>), dim3(grid(B)), dim3(64), h->fit.lds_wave, s, c,
                         B, (const T*)X, (const T*)U, (const T*)x_term, (const T*)lamb,
                         (const T*)obs, (T*)K, (T*)k);
    });
    HIP_TRY(hipGetLastError());
    return I2LQR_OK;
  }
  static int forward(i2lqr_handle* h, int64_t B, const void* X, const void* U, const void* x_term,
                     const void* K, const void* k, void* Xn, void* Un, void* cost_new,
                     hipStream_t s) {
    const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
    with_weights(c.flags, [&](auto W) {
      hipLaunchKernelGGL((k_forward<T, Sys, LANES, W>), dim3(grid(B)), dim3(64), h->fit.lds_wave, s, c,
                         B, (const T*)X, (const T*)U, (const T*)x_term, (const T*)K, (const T*)k,
                         (T*)Xn, (T*)Un, (T*)cost_new);
    });
    HIP_TRY(hipGetLastError());
    return I2LQR_OK;
  }
};

}  // namespace i2lqr
