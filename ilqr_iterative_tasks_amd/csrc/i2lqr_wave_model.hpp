// The opt-in model of the one-problem-per-wavefront kernel as a handle keeps it - line search,
// obstacle records, state box, barrier cost - and every rule the host derives from it: which form of the kernel
// runs, how many step sizes and records it is given, the LDS it takes behind the slice, the name
// it reports and the words the refusals use.  Plain C++17, no HIP: the host test builds it alone
// (tests/test_wave_model_host.py).
#pragma once
#include <stddef.h>

#include "../../include/i2lqr.h"

namespace i2lqr {

// The box as the handle keeps it (i2lqr_set_state_box): doubles, converted by make_box_cfg.
struct StateBox {
  double lo[I2LQR_MAX_N] = {}, hi[I2LQR_MAX_N] = {};  // 0 where the side is unbounded
  double q1 = 1.0, q2 = 1.0;
  unsigned m_lo = 0, m_hi = 0;  // bit i: lo[i] / hi[i] is finite
  bool on() const { return (m_lo | m_hi) != 0; }
};

// The forms in precedence order: each carries the models of the ones before it (k_iterate_box takes
// records and step sizes, k_iterate_obs step sizes; k_iterate_merit is k_iterate_box with the barriers
// in the accept / reject cost).  WAVE_PLAIN: no model is on, k_iterate.
enum WaveForm { WAVE_PLAIN, WAVE_LS, WAVE_OBS, WAVE_BOX, WAVE_MERIT };

struct WaveModel {
  int ls = 0;    // "line_search": 2, 4 or 8 step sizes; 0: off
  int obs = 0;   // "obstacles": 2 ... I2LQR_MAX_OBSTACLES records per problem; 0: off (one record)
  StateBox box;  // i2lqr_set_state_box; box.on(): some bound is finite
  bool barrier_cost = false;  // "barrier_cost": the accept / reject cost carries the barriers

  WaveForm form() const {
    return barrier_cost ? WAVE_MERIT
                        : box.on() ? WAVE_BOX : obs > 1 ? WAVE_OBS : ls > 1 ? WAVE_LS : WAVE_PLAIN;
  }
  // ... of i2lqr_solve_chained with "wave_chain": k_chain_box is the box form whatever is on
  // (it has no barrier cost: chain_plan refuses a chained call with "barrier_cost" on)
  WaveForm form(bool chained) const { return chained ? WAVE_BOX : form(); }
  int steps() const { return ls > 1 ? ls : 1; }      // step sizes per iteration
  int records() const { return obs > 1 ? obs : 1; }  // obstacle records per problem
  // the model without its line search: what a call that has no forward pass sees (no forward
  // pass, no accept / reject step: the barrier cost does not concern it either)
  WaveModel without_line_search() const {
    WaveModel m = *this;
    m.ls = 0;
    m.barrier_cost = false;
    return m;
  }

  // LDS bytes one problem takes behind its slice: nothing, then the records obs[K][6], then behind
  // them the box's d1[N+1][n], d2[N+1][n] and the bounds lo[n], hi[n]
  size_t extra_lds_bytes(WaveForm f, int n, int N, size_t word) const {
    size_t words = f >= WAVE_OBS ? (size_t)records() * 6 : 0;
    if (f >= WAVE_BOX) words += (size_t)2 * n * (N + 1) + (size_t)2 * n;  // (the merit form: the box form's)
    return words * word;
  }
};

// what i2lqr_iterate_kernel / i2lqr_solve_kernel report
inline const char* wave_kernel_name(WaveForm f) {
  switch (f) {
    case WAVE_MERIT: return "k_iterate (barrier cost)";
    case WAVE_BOX: return "k_iterate (state box)";
    case WAVE_OBS: return "k_iterate (several obstacles)";
    case WAVE_LS: return "k_iterate (line search)";
    default: return "k_iterate";
  }
}
// the model as a refusal names it: "<phrase> runs on ...", "<phrase> is built for ..."
inline const char* wave_phrase(WaveForm f) {
  switch (f) {
    case WAVE_MERIT: return "\"barrier_cost\"";
    case WAVE_BOX: return "a state box";
    case WAVE_OBS: return "\"obstacles\"";
    case WAVE_LS: return "\"line_search\"";
    default: return "";
  }
}
// ... and as an entry point without it does: "<entry point> <phrase>, or ..."
inline const char* wave_lack_phrase(WaveForm f) {
  switch (f) {
    case WAVE_MERIT: return "has no barrier cost: switch \"barrier_cost\" off";
    case WAVE_BOX: return "has no state box: clear it (i2lqr_set_state_box with NULL bounds)";
    case WAVE_OBS: return "reads one obstacle record per problem: switch \"obstacles\" off";
    case WAVE_LS: return "has no line search: switch \"line_search\" off";
    default: return "";
  }
}

}  // namespace i2lqr
