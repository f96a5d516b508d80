// The handle behind the C-ABI (include/i2lqr.h), the argument block of a solve call and the few
// helpers the launchers of i2lqr_abi.hip share (Launch in i2lqr_column_launch.hpp, LaneLaunch in
// i2lqr_lane_launch.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "../../include/i2lqr.h"
#include "i2lqr_column_plan.hpp"
#include "i2lqr_geometry.hpp"
#include "i2lqr_lane_plan.hpp"
#include "i2lqr_wave.hpp"
#include "i2lqr_wave_model.hpp"

struct i2lqr_handle {
  i2lqr_config cfg;
  int lanes;        // lanes of a wavefront that cooperate on one problem (1: batch-minor layout)
  int device;
  void* ws = nullptr;  // caller-owned scratch of the batch-minor kernels
  int64_t ws_bytes = 0;
  i2lqr::LaneTune lane;  // options of the batch-minor / batch-tiled layouts (i2lqr_lane_plan.hpp)
  i2lqr::ColumnTune col;  // options of the problem-major layout (i2lqr_column_plan.hpp)
  i2lqr::ColumnFit fit;   // what the kernel units know about cfg, filled in i2lqr_create
  i2lqr::WaveModel model;  // one-problem-per-wavefront kernel: "line_search", "obstacles" and the state box (i2lqr_set_state_box), all off by default (i2lqr_wave_model.hpp)
  // "lane_models", "lane_barrier_cost", "lane_line_search": with `model`, what a batch-minor /
  // batch-tiled handle runs on k_lane_iterate_model / _merit / _ls (lane_model(), i2lqr_lane_opt_in.hpp;
  // LaneLaunch::iterate_model)
  i2lqr::LaneOptIn lane_opt;
  // i2lqr_iterate_pick: the epilogue a call asks for; `fused` is set by the launcher that folded
  // it into its kernel, otherwise the call runs the separate kernels.  The pointer to the call's
  // epilogue is THREAD-LOCAL (t_epi in i2lqr_column_launch.hpp), not handle state: two host threads inside
  // i2lqr_iterate_pick on one handle do not see each other's.
  struct Epilogue {
    const int32_t* qfun;
    int outer_iter, max_relax_iter;
    void* cost_it;
    void* part;
    int64_t* best_idx;
    void* best_cost;
    bool fused;
  };
  // Device words of the last-workgroup-done reduction (each wraps to 0 by itself when its launch
  // has drawn all its tickets).  kTickets words, handed out round-robin: calls on one handle that
  // are in flight at the same time (two streams) draw from different words as long as fewer than
  // kTickets of them overlap; their part[] workspaces are the caller's and must differ.
  static constexpr unsigned kTickets = 16;
  unsigned* ticket = nullptr;
  std::atomic<unsigned> ticket_next{0};
  // i2lqr_sharded_round_flat: the event that orders the side stream behind the shard's solve and
  // the one a later round waits for before it reuses the buffers (created on first use)
  hipEvent_t ev_ready = nullptr, ev_side_done = nullptr;
  bool side_pending = false;  // ev_side_done has been recorded at least once
  i2lqr::DeviceGeometry geo;  // of h->device, queried in i2lqr_create (i2lqr_geometry.hpp)
};

namespace i2lqr {

// The caller's arrays and counts of i2lqr_iterate / i2lqr_solve / i2lqr_solve_chained /
// i2lqr_iterate_pick (B: the chains of a chained solve), built once by the entry point; obs, K, k,
// iters and status may be null.
struct SolveIO {
  int64_t B;
  int n_iters, early_exit;
  void* X; void* U; const void* x_term; void* lamb; const void* obs; void* cost; void* K; void* k;
  int32_t* iters; int32_t* status;
};

// IterArgs of a launch on the arrays of `io`, every optional field at its neutral value
template <class T> IterArgs<T> iter_args(const SolveIO& io) {
  IterArgs<T> a;
  a.B = io.B; a.n_iters = io.n_iters; a.early_exit = io.early_exit;
  a.X = (T*)io.X; a.U = (T*)io.U; a.x_term = (const T*)io.x_term; a.lamb = (T*)io.lamb;
  a.obs = (const T*)io.obs; a.cost = (T*)io.cost; a.K = (T*)io.K; a.k = (T*)io.k;
  a.iters = io.iters; a.status = io.status;
  a.dbg = nullptr;
  a.count = nullptr; a.count_max = 0; a.max_total = 0; a.set_stride = 0;
  return a;
}

// f(std::true_type()) for a device config with stage weights (DevCfg::flags), f(std::false_type())
// otherwise: the HASQR parameter of the kernel f launches.  BUILT = false where the stage-weight
// instantiations do not exist (the caller has refused such a configuration): the false one always.
template <bool BUILT = true, class F> void with_weights(int flags, F&& f) {
  if constexpr (BUILT) {
    if (flags) {
      f(std::true_type());
      return;
    }
  }
  f(std::false_type());
}

// One problem per wavefront with per-step Jacobian matrices in LDS (k_iterate<.., FSTEP>; the
// chunked solve's tail runs on it): built for the bicycles, quad12's F is 1.5 KB per step
template <class Sys> constexpr bool kWaveHasFstep = Sys::n <= 6;
template <class T, class Sys> size_t wave_fstep_lds_bytes(int N) {
  return (size_t)Layout<Sys>(N, true).total * sizeof(T);
}

}  // namespace i2lqr
