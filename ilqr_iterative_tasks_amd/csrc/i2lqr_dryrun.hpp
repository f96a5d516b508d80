// Dry-run launches for the host sanitizers.  Compiled in ONLY with
// -DI2LQR_DRY_RUN (the AddressSanitizer / UBSan build, `make asan`); active only when the environment
// says I2LQR_DRY_RUN=1.  i2lqr_create then skips the device, and every kernel launch of the
// library becomes a RECORD — kernel instantiation, grid, workgroup size, dynamic LDS, arguments
// (tools/dry_run_fuzz.py --trace writes them all) — whose pointer arguments
// (plain pointers and every pointer field of IterArgs / LaneArgs / LaneSet) must lie inside a range
// the driver has declared with i2lqr_dry_run(1, base, bytes): the registered workspace and the
// caller's arrays.  That puts the host code BEHIND a live handle — workspace carving, the chunked
// solve's scheduler, the LDS budgeting, the sharded round — under ASan / UBSan on a box without a
// GPU, and turns "a carved pointer left the workspace" into a reported violation.
// The product build never sees this header's macros.
#pragma once
#ifdef I2LQR_DRY_RUN
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "i2lqr_wave.hpp"

namespace i2lqr {
namespace dry {

bool on();                                      // I2LQR_DRY_RUN=1 (read once)
void allow(const void* base, size_t bytes);     // a range kernel pointers may point into
void reset();                                   // forget ranges, records and violations
// One record per launch: record() opens it with the kernel's instantiation (dladdr on its handle,
// demangled; `expr`, the launch's spelling, where no exported symbol sits at that address), ptr()
// and val() append the arguments, end() files it.  A pointer is written as the declared range it
// lies in plus an offset (r<index>+<bytes>), so two builds of the library give identical records.
void record(const char* expr, const void* kernel, dim3 grid, dim3 block, size_t lds);
void ptr(const char* field, const void* p);
void val(const char* field, int64_t v);
void end();
int64_t report(char* buf, int64_t n);           // text of records + violations; returns #violations

template <class A> inline void arg(const A&) {}  // device configs
inline void arg(int64_t v) { val("int", v); }
inline void arg(int v) { val("int", v); }
template <class P> inline void arg(P* p) { ptr("pointer argument", (const void*)p); }
template <class T> inline void arg(const IterArgs<T>& a) {
  val("IterArgs.B", a.B); val("IterArgs.n_iters", a.n_iters); val("IterArgs.early_exit", a.early_exit);
  ptr("IterArgs.X", a.X); ptr("IterArgs.U", a.U); ptr("IterArgs.x_term", a.x_term);
  ptr("IterArgs.lamb", a.lamb); ptr("IterArgs.obs", a.obs); ptr("IterArgs.cost", a.cost);
  ptr("IterArgs.K", a.K); ptr("IterArgs.k", a.k); ptr("IterArgs.iters", a.iters);
  ptr("IterArgs.status", a.status); ptr("IterArgs.dbg", a.dbg); ptr("IterArgs.count", a.count);
  val("IterArgs.count_max", a.count_max); val("IterArgs.max_total", a.max_total);
  val("IterArgs.set_stride", a.set_stride);
  ptr("IterArgs.orig", a.orig); ptr("IterArgs.out_X", a.out_X);
  ptr("IterArgs.out_U", a.out_U); ptr("IterArgs.out_K", a.out_K);
  ptr("IterArgs.out_k", a.out_k); ptr("IterArgs.out_lamb", a.out_lamb);
  ptr("IterArgs.out_cost", a.out_cost); ptr("IterArgs.out_iters", a.out_iters);
  ptr("IterArgs.out_status", a.out_status);
  val("IterArgs.out_B", a.out_B); val("IterArgs.out_tiled", a.out_tiled);
  ptr("IterArgs.qfun", a.qfun);
  val("IterArgs.outer_iter", a.outer_iter); val("IterArgs.max_relax_iter", a.max_relax_iter);
  ptr("IterArgs.cost_it", a.cost_it); ptr("IterArgs.pick_part", a.pick_part);
  ptr("IterArgs.pick_ticket", a.pick_ticket); ptr("IterArgs.best_idx", a.best_idx);
  ptr("IterArgs.best_cost", a.best_cost); val("IterArgs.chain_len", a.chain_len);
  val("IterArgs.chains", a.chains);
}
#ifdef I2LQR_DRY_RUN_LANE  // (translation units that see i2lqr_lane.hpp)
template <class T> inline void arg(const LaneSet<T>& s) {
  ptr("LaneSet.X", s.X); ptr("LaneSet.U", s.U); ptr("LaneSet.x_term", s.x_term);
  ptr("LaneSet.obs", s.obs); ptr("LaneSet.lamb", s.lamb); ptr("LaneSet.cost", s.cost);
  ptr("LaneSet.K", s.K); ptr("LaneSet.k", s.k); ptr("LaneSet.iters", s.iters);
  ptr("LaneSet.status", s.status); ptr("LaneSet.orig", s.orig); val("LaneSet.B", s.B);
}
template <class T> inline void arg(const LaneArgs<T>& a) {
  val("LaneArgs.B", a.B); val("LaneArgs.n_iters", a.n_iters); val("LaneArgs.early_exit", a.early_exit);
  ptr("LaneArgs.X", a.X); ptr("LaneArgs.U", a.U); ptr("LaneArgs.x_term", a.x_term);
  ptr("LaneArgs.lamb", a.lamb); ptr("LaneArgs.obs", a.obs); ptr("LaneArgs.cost", a.cost);
  ptr("LaneArgs.K", a.K); ptr("LaneArgs.k", a.k); ptr("LaneArgs.iters", a.iters);
  ptr("LaneArgs.status", a.status); ptr("LaneArgs.wsU", a.wsU); ptr("LaneArgs.wsK", a.wsK);
  ptr("LaneArgs.wsk", a.wsk); ptr("LaneArgs.wsX", a.wsX); ptr("LaneArgs.count", a.count);
  val("LaneArgs.resume", a.resume); val("LaneArgs.max_total", a.max_total);
  val("LaneArgs.count_lo", a.count_lo); val("LaneArgs.count_hi", a.count_hi);
  val("LaneArgs.two_max", a.two_max); val("LaneArgs.lds_grow", a.lds_grow);
  ptr("LaneArgs.dbg", a.dbg); val("LaneArgs.defer", a.defer);
  val("LaneArgs.lds_steps", a.lds_steps); val("LaneArgs.reroll", a.reroll);
  val("LaneArgs.merge", a.merge); val("LaneArgs.ckpt", a.ckpt); val("LaneArgs.stagger", a.stagger);
  val("LaneArgs.cp.on", a.cp.on);
  if (a.cp.on) {
    val("LaneArgs.cp.src_is_user", a.cp.src_is_user); val("LaneArgs.cp.user_tiled", a.cp.user_tiled);
    ptr("LaneArgs.cp.orig", a.cp.orig); ptr("LaneArgs.cp.count_out", a.cp.count_out);
    arg(a.cp.dst);
    arg(a.cp.usr);
  }
}
#endif

template <class... A>
inline void launch(const char* expr, const void* kernel, dim3 grid, dim3 block, size_t lds,
                   const A&... a) {
  record(expr, kernel, grid, block, lds);
  (arg(a), ...);
  end();
}

}  // namespace dry
}  // namespace i2lqr

// every launch of the translation unit goes through here
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...)                                  \
  do {                                                                                             \
    if (::i2lqr::dry::on())                                                                        \
      ::i2lqr::dry::launch(#kernel, (const void*)(kernel), dim3(grid), dim3(block), (size_t)(lds), __VA_ARGS__);          \
    else                                                                                           \
      hipLaunchKernelGGLInternal((kernel), (grid), (block), (lds), (stream), __VA_ARGS__);         \
  } while (0)
// ... and the runtime calls between them succeed without a device
#define hipMemsetAsync(...) (::i2lqr::dry::on() ? hipSuccess : hipMemsetAsync(__VA_ARGS__))
#define hipMemcpyAsync(...) (::i2lqr::dry::on() ? hipSuccess : hipMemcpyAsync(__VA_ARGS__))
#define hipFuncSetAttribute(...) (::i2lqr::dry::on() ? hipSuccess : hipFuncSetAttribute(__VA_ARGS__))
#define hipGetLastError() (::i2lqr::dry::on() ? hipSuccess : hipGetLastError())
#define hipEventCreateWithFlags(ev, flags) \
  (::i2lqr::dry::on() ? (*(ev) = (hipEvent_t)0x10, hipSuccess) : hipEventCreateWithFlags(ev, flags))
#define hipEventDestroy(...) (::i2lqr::dry::on() ? hipSuccess : hipEventDestroy(__VA_ARGS__))
#define hipEventRecord(...) (::i2lqr::dry::on() ? hipSuccess : hipEventRecord(__VA_ARGS__))
#define hipStreamWaitEvent(...) (::i2lqr::dry::on() ? hipSuccess : hipStreamWaitEvent(__VA_ARGS__))
#define hipFree(...) (::i2lqr::dry::on() ? hipSuccess : hipFree(__VA_ARGS__))
#define hipGetDevice(p) (::i2lqr::dry::on() ? (*(p) = 0, hipSuccess) : hipGetDevice(p))
#endif  // I2LQR_DRY_RUN
