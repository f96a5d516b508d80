// The opt-in forms of the one-problem-per-lane kernel as a handle keeps them - "lane_models" with
// obstacle records and the state box, "lane_barrier_cost", "lane_line_search" - and every rule the
// host derives from them: which form runs, the name it reports and which requests are refused, in
// which words.  Plain C++17, no HIP: the host test builds it alone (tests/test_lane_models_host.py).
// The counterpart of i2lqr_wave_model.hpp, whose records and box a lane handle shares.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include "../../include/i2lqr.h"
#include "i2lqr_wave_model.hpp"

namespace i2lqr {

// What a batch-minor / batch-tiled handle keeps of i2lqr_set_option beside its WaveModel
struct LaneOptIn {
  bool models = false;  // "lane_models" 1: the handle accepts model.obs and model.box; never set on a problem-major handle
  bool barrier_cost = false;  // "lane_barrier_cost" 1; only ever set while models is
  int line_search = 0;  // "lane_line_search" 2 / 4 / 8; 0: off; only ever set while models is
  // "lane_rows_models" 1: a handle of a row-block plant (quad12) accepts model.obs and model.box as
  // well, for k_lane_iterate_rows_model; only ever set while models is, never on a bicycle handle
  bool rows_models = false;
};

// The forms in precedence order, as WaveForm ranks them: the barrier cost above the box, the box above
// several records, the line search alone below the others.  LANE_PLAIN: nothing is on, k_lane_iterate
// (or its helper-wavefront / chunked forms).
enum LaneForm { LANE_PLAIN, LANE_LS, LANE_OBS, LANE_BOX, LANE_MERIT };

// The opt-in models of a launch ("lane_models" 1; k_lane_iterate_model, i2lqr_lane_model.hpp):
// `records` obstacle records per problem and the state box, both in the backward pass's derivatives.
// `barrier_cost` ("lane_barrier_cost" 1): the accept / reject step sees the barriers
// (k_lane_iterate_merit, i2lqr_lane_merit.hpp); one record and no box are a model then.
// `line_search` ("lane_line_search" 2 / 4 / 8): that many step sizes per iteration
// (k_lane_iterate_ls, i2lqr_lane_ls.hpp), with or without any of the others.
struct LaneModel {
  int records = 1;   // "obstacles": 2 ... I2LQR_MAX_OBSTACLES; 1: off
  bool box = false;  // i2lqr_set_state_box with a finite bound
  bool barrier_cost = false;  // (the penalty is summed in registers: no LDS, the plan is the same)
  int line_search = 0;  // 2, 4, 8; 0: off (the candidates live in registers: no LDS, the plan is the same)
  bool on() const { return records > 1 || box || barrier_cost || line_search > 1; }
  LaneForm form() const {
    return barrier_cost ? LANE_MERIT
                        : box ? LANE_BOX : records > 1 ? LANE_OBS : line_search > 1 ? LANE_LS : LANE_PLAIN;
  }
};
// ... of a handle (a lane handle without "lane_models" 1 never holds records or a box): what
// LaneLaunch::iterate launches and what the names report
inline LaneModel lane_model(const WaveModel& model, const LaneOptIn& opt) {
  return LaneModel{model.records(), model.box.on(), opt.barrier_cost, opt.line_search};
}

// what i2lqr_iterate_kernel / i2lqr_solve_kernel report for a form that is on
inline const char* lane_kernel_name(LaneForm f) {
  switch (f) {
    case LANE_MERIT: return "k_lane_iterate (barrier cost)";
    case LANE_BOX: return "k_lane_iterate (state box)";
    case LANE_OBS: return "k_lane_iterate (several obstacles)";
    case LANE_LS: return "k_lane_iterate (line search)";
    default: return "k_lane_iterate";
  }
}

// ... of a row-block plant (quad12) with "lane_rows_models" 1: k_lane_iterate_rows_model
// (i2lqr_lane_rows_model.hpp) has the records and the box; a handle with neither runs and reports
// k_lane_iterate_rows
inline const char* lane_rows_kernel_name(LaneForm f) {
  switch (f) {
    case LANE_BOX: return "k_lane_iterate_rows (state box)";
    case LANE_OBS: return "k_lane_iterate_rows (several obstacles)";
    default: return "k_lane_iterate_rows";
  }
}

// ... and i2lqr_solve_kernel where the solve runs as chunks with compaction ("lane_model_chunks")
inline const char* lane_chunked_kernel_name(LaneForm f) {
  switch (f) {
    case LANE_MERIT: return "k_lane_iterate (barrier cost), chunked";
    case LANE_BOX: return "k_lane_iterate (state box), chunked";
    case LANE_OBS: return "k_lane_iterate (several obstacles), chunked";
    case LANE_LS: return "k_lane_iterate (line search), chunked";
    default: return "k_lane_iterate, chunked";
  }
}

// An answer of the rules below: I2LQR_OK, or the error code and the text of i2lqr_last_error
struct LaneRefusal {
  int code = I2LQR_OK;
  char text[320] = "";
};
__attribute__((format(printf, 2, 3))) inline LaneRefusal lane_refuse(int code, const char* fmt, ...) {
  LaneRefusal r;
  r.code = code;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(r.text, sizeof(r.text), fmt, ap);
  va_end(ap);
  return r;
}
// an opt-in form that exists on the one-problem-per-wavefront kernel only, asked of another layout
inline LaneRefusal refuse_layout(const char* what) {
  return lane_refuse(I2LQR_ERR_UNSUPPORTED, "%s is built for the problem-major layout (the "
                     "one-problem-per-wavefront kernel)", what);
}
// LaneLaunch::iterate_model of a row-block plant (quad12): the same rule as lane_refusal's, met by a
// launch instead of a request (a handle without "lane_rows_models" 1)
inline const char* lane_models_rows_text() {
  return "\"lane_models\" is built for the bicycles' one-problem-per-lane kernel, not for the "
         "row-block kernel of this plant (k_lane_iterate_rows): use the problem-major layout";
}

// ... and of a quad12 handle with "lane_rows_models" 1, a model and stage weights: that instantiation of
// k_lane_iterate_rows_model is not built (it compiles with more scratch than k_lane_iterate_rows's)
inline const char* lane_rows_models_weights_text() {
  return "\"lane_rows_models\": k_lane_iterate_rows_model is built for Q = R = 0 (with stage weights "
         "the records and the box run on the problem-major layout)";
}

// What i2lqr_set_option / i2lqr_set_state_box may be asked that concerns the lane forms
enum LaneAsk {
  LANE_ASK_OBSTACLES,     // "obstacles" v
  LANE_ASK_BOX,           // i2lqr_set_state_box: v = 1 for a box with a finite bound, 0 for none
  LANE_ASK_MODELS,        // "lane_models" v
  LANE_ASK_BARRIER_COST,  // "lane_barrier_cost" v
  LANE_ASK_LINE_SEARCH,   // "lane_line_search" v
  WAVE_ASK_BARRIER_COST,  // "barrier_cost" v: a lane handle is pointed at "lane_barrier_cost"
  LANE_ASK_ROWS_MODELS,   // "lane_rows_models" v
};
// `what` as a refusal names it, and for the two lane options their problem-major counterpart
inline const char* lane_ask_phrase(LaneAsk what) {
  switch (what) {
    case LANE_ASK_OBSTACLES: return wave_phrase(WAVE_OBS);
    case LANE_ASK_BOX: return wave_phrase(WAVE_BOX);
    case LANE_ASK_MODELS: return "\"lane_models\"";
    case LANE_ASK_BARRIER_COST: return "\"lane_barrier_cost\"";
    case LANE_ASK_LINE_SEARCH: return "\"lane_line_search\"";
    case LANE_ASK_ROWS_MODELS: return "\"lane_rows_models\"";
    default: return wave_phrase(WAVE_MERIT);
  }
}
inline const char* lane_ask_counterpart(LaneAsk what) {
  return wave_phrase(what == LANE_ASK_LINE_SEARCH ? WAVE_LS : WAVE_MERIT);
}

// May `what` take the value v on a handle of this layout (problem_major) and plant (rows: quad12,
// whose lane kernel is k_lane_iterate_rows) that holds `model` and `opt`?  The one place that knows:
// the values an option takes; that the lane options belong to the lane layouts and "barrier_cost" to
// the other; that records, the box and the two lane options need "lane_models" 1 and the bicycles;
// that "lane_models" stays while any of them is on; that "lane_rows_models" opens records and the box
// (and nothing else) to quad12, needs "lane_models" 1 and stays while either is on.  Off-values are
// accepted everywhere.
inline LaneRefusal lane_refusal(LaneAsk what, int v, bool problem_major, bool rows,
                                const WaveModel& model, const LaneOptIn& opt) {
  const char* const name = lane_ask_phrase(what);
  const bool steps = what == LANE_ASK_LINE_SEARCH;  // valued in step sizes, the others in 0 / 1
  const bool lane_option = what == LANE_ASK_BARRIER_COST || what == LANE_ASK_LINE_SEARCH;
  if (steps && v != -1 && v != 0 && v != 1 && v != 2 && v != 4 && v != 8)
    return lane_refuse(I2LQR_ERR_INVALID, "%s is 2, 4 or 8 step sizes, or -1 / 0 / 1 (off)", name);
  if ((what == LANE_ASK_MODELS || what == LANE_ASK_BARRIER_COST || what == LANE_ASK_ROWS_MODELS) &&
      v != -1 && v != 0 && v != 1)
    return lane_refuse(I2LQR_ERR_INVALID, "%s is 1 (on), or -1 / 0 (off)", name);
  const bool on = steps || what == LANE_ASK_OBSTACLES ? v > 1 : v == 1;
  if (what == LANE_ASK_MODELS) {
    if (on && problem_major)
      return lane_refuse(I2LQR_ERR_UNSUPPORTED, "%s is built for the batch-minor / batch-tiled "
                         "layouts (a problem-major handle runs the models on the "
                         "one-problem-per-wavefront kernels without it)", name);
    const struct { bool on; const char* is; const char* undo; } held[] = {
        {opt.barrier_cost, "\"lane_barrier_cost\" is", "set \"lane_barrier_cost\" to 0"},
        {opt.line_search != 0, "\"lane_line_search\" is", "set \"lane_line_search\" to 0"},
        {opt.models && model.box.on(), "a state box is", "clear it (i2lqr_set_state_box with NULL bounds)"},
        {opt.models && model.obs > 1, "\"obstacles\" is", "set \"obstacles\" to 1"},
        {opt.rows_models, "\"lane_rows_models\" is", "set \"lane_rows_models\" to 0"}};
    for (const auto& h : held)
      if (h.on && !on)
        return lane_refuse(I2LQR_ERR_INVALID, "%s cannot be switched off while %s on: %s first",
                           name, h.is, h.undo);
    return LaneRefusal();
  }
  if (what == LANE_ASK_ROWS_MODELS) {
    if (on && problem_major)
      return lane_refuse(I2LQR_ERR_UNSUPPORTED, "%s is built for the batch-minor / batch-tiled "
                         "layouts of quad12 (a problem-major handle runs the models on the "
                         "one-problem-per-wavefront kernels without it)", name);
    if (on && !rows)
      return lane_refuse(I2LQR_ERR_UNSUPPORTED, "%s is built for quad12's row-block kernel "
                         "(k_lane_iterate_rows): a bicycle handle runs the models with \"lane_models\" "
                         "1 and needs nothing more", name);
    if (on && !opt.models)
      return lane_refuse(I2LQR_ERR_UNSUPPORTED, "%s runs on top of \"lane_models\": set "
                         "\"lane_models\" to 1 first", name);
    const struct { bool on; const char* is; const char* undo; } held[] = {
        {opt.rows_models && model.box.on(), "a state box is", "clear it (i2lqr_set_state_box with NULL bounds)"},
        {opt.rows_models && model.obs > 1, "\"obstacles\" is", "set \"obstacles\" to 1"}};
    for (const auto& h : held)
      if (h.on && !on)
        return lane_refuse(I2LQR_ERR_INVALID, "%s cannot be switched off while %s on: %s first",
                           name, h.is, h.undo);
    return LaneRefusal();
  }
  if (!on) return LaneRefusal();
  if (what == WAVE_ASK_BARRIER_COST)
    return problem_major ? LaneRefusal()
                         : lane_refuse(I2LQR_ERR_UNSUPPORTED, "%s; a batch-minor / batch-tiled handle "
                                       "of the bicycles has \"lane_barrier_cost\" (with "
                                       "\"lane_models\" 1)", refuse_layout(name).text);
  if (problem_major)
    return !lane_option ? LaneRefusal()
                        : lane_refuse(I2LQR_ERR_UNSUPPORTED, "%s is built for the batch-minor / "
                                      "batch-tiled layouts: a problem-major handle takes %s (the "
                                      "one-problem-per-wavefront kernel)", name,
                                      lane_ask_counterpart(what));
  if (!opt.models)
    return !lane_option ? refuse_layout(name)
                        : lane_refuse(I2LQR_ERR_UNSUPPORTED, "%s runs on the kernel of "
                                      "\"lane_models\": set \"lane_models\" to 1 first", name);
  if (rows && (lane_option || !opt.rows_models))  // ("lane_rows_models": records and the box, nothing else)
    return lane_refuse(I2LQR_ERR_UNSUPPORTED, "%s with \"lane_models\" is built for the bicycles' "
                       "one-problem-per-lane kernel, not for quad12's row-block kernel "
                       "(k_lane_iterate_rows): use the problem-major layout", name);
  return LaneRefusal();
}

}  // namespace i2lqr
