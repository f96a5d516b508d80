// Instantiations and launcher of the sixteen-lanes-per-problem kernel (i2lqr_quad.hpp).
#include "i2lqr_geometry.hpp"
#include "i2lqr_group.h"

#include <cstdlib>

#include "i2lqr_devcfg.hpp"
#include "i2lqr_quad.hpp"
#include "i2lqr_dryrun.hpp"  // (empty unless -DI2LQR_DRY_RUN: the ASan build)

namespace i2lqr {

template <class T>
hipError_t quad_iterate(const i2lqr_config& cfg, const IterArgs<T>& a, void* ws, hipStream_t s) {
  using Sys = Quad12<T>;
  const auto c = make_dev_cfg<T, Sys::n, Sys::m>(cfg);
  const size_t lds = (size_t)QLayout<Sys>(cfg.N).lds_total * kQPW * sizeof(T);
  if (lds > device_geometry().default_dyn_lds) {
    hipError_t e = hipFuncSetAttribute((const void*)k_quad_iterate<T, Sys>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const unsigned grid = (unsigned)((a.B + kQPW - 1) / kQPW);
#ifdef I2LQR_STAMPS
  IterArgs<T> a2 = a;  // diagnostic build: [B][8] u64 phase sums at the address in I2LQR_DBG_PTR
  a2.dbg = nullptr;
  if (const char* e = getenv("I2LQR_DBG_PTR")) a2.dbg = (unsigned long long*)strtoull(e, nullptr, 0);
  hipLaunchKernelGGL((k_quad_iterate<T, Sys>), dim3(grid), dim3(64), lds, s, c, a2, (T*)ws);
  return hipGetLastError();
#endif
  hipLaunchKernelGGL((k_quad_iterate<T, Sys>), dim3(grid), dim3(64), lds, s, c, a, (T*)ws);
  return hipGetLastError();
}

static_assert(kQPW == kSixteenLaneProblems, "i2lqr_column_plan.hpp");

void column_fit_quad(const i2lqr_config& cfg, ColumnFit& fit) {
  if (cfg.system_id != I2LQR_SYS_QUAD12) return;
  const QLayout<Quad12<double>> layout(cfg.N);
  fit.lds_quad = (size_t)layout.lds_total * kQPW * (size_t)fit.word;
  fit.ws_quad = (int64_t)layout.ws_total * fit.word;
}

template hipError_t quad_iterate<double>(const i2lqr_config&, const IterArgs<double>&, void*,
                                         hipStream_t);
template hipError_t quad_iterate<float>(const i2lqr_config&, const IterArgs<float>&, void*, hipStream_t);

}  // namespace i2lqr
