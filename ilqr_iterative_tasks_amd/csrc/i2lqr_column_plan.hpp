// What the launcher of the problem-major layout (i2lqr_column_launch.hpp) decides from integers
// alone: which fused kernel a call runs on, with the refusal texts; how many wavefronts a workgroup
// of the eight- / sixteen-lane kernels gets; the per-step-Jacobian form of the wavefront kernel; how
// a chained solve runs; the caller's workspace; the names the library reports; and the crossover
// tables of i2lqr_recommended_layout.  Plain C++17, no HIP: the host test builds it alone
// (tests/test_column_plan_host.py).  Every function takes the DeviceGeometry it decides for: the
// handle's (h->geo), queried in i2lqr_create.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/i2lqr.h"
#include "i2lqr_geometry.hpp"
#include "i2lqr_wave_model.hpp"

namespace i2lqr {

// The handle's options of the problem-major layout (i2lqr_set_option); -1 = automatic
struct ColumnTune {
  int opt_fstep = -1;  // one-problem-per-wavefront kernel: per-step Jacobian matrices in LDS
  int opt_group = -1;  // lanes per problem of the fused kernels: 8, 16, 64
  int opt_spec = -1;   // eight- / sixteen-lane kernel: speculative form (2-3 wavefronts per workgroup)
  int opt_group_ws = -1;  // eight-lane kernel: workspace form (records / gains in HBM)
  int opt_group_overlap = -1;  // sixteen-lane kernel: overlapped schedule (helpers take the records, the terminal block and the gain stores); 0: the one-helper schedule; automatic: on
  int opt_group_fixed = -1;    // sixteen-lane kernel: the fixed-horizon form (k_group_iterate_fixed) where the horizon is one it is built for; 0: the run-time-horizon kernel; automatic: on
  int opt_group_chains = -1;   // eight- / sixteen-lane kernels: the independent chains of a record side by side, the entry rollout's sin / cos spread over the row, sin / cos of x_0 from the nominal's cache (IterArgs::chains); 0: the serial forms; automatic: on
  int opt_wave_chain = 0;  // i2lqr_solve_chained: 1 = what the speculative chain kernel is not built for runs on the one-problem-per-wavefront kernel's chained form (k_chain_box); 0: refused
};

// What only the kernel units know about a configuration, as integers: filled once per handle in
// i2lqr_create by the units that own the layouts (column_fit_group / column_fit_quad of i2lqr_group.h,
// Launch::prepare for Layout<Sys>).  Bytes of dynamic LDS per workgroup; 0: the form is not built
// for the plant.
struct ColumnFit {
  enum Plant { OTHER, BICYCLE, SIXTEEN };  // m = 2 and n + m <= 8 / n + m = 16 (quad12)
  int plant = OTHER;
  bool weights = false;        // stage weights Q, R != 0 (the column kernels are built for Q = R = 0)
  bool problem_major = false;  // the handle's layout
  bool f64 = true;
  int n = 0, N = 0, word = 8;
  bool fixed_horizon = false;  // k_group_iterate_fixed is built for N
  size_t lds_wave = 0, lds_wave_fstep = 0;   // Layout<Sys>: one problem per wavefront; with per-step Jacobians
  size_t lds_group8 = 0, lds_group16 = 0;    // GLayout: eight / four problem slices
  size_t lds_group_ws = 0;                   // eight-lane workspace form
  size_t lds_spec8x2 = 0, lds_spec8x3 = 0;   // GSpecLayout: lanes per problem x wavefronts
  size_t lds_spec16x2 = 0, lds_spec16x3 = 0;
  size_t lds_quad = 0;                       // QLayout, four problems
  int64_t ws_group = 0, ws_quad = 0;  // workspace bytes per problem: eight-lane workspace form, quad
};

// problems per wavefront of the eight- / sixteen-lane forms (kGroupsPerWave, kQPW: asserted in the units)
constexpr int kEightLaneProblems = 8, kSixteenLaneProblems = 4;

// (measured on the 256-CU chip; DeviceGeometry::scaled() where they are used)
constexpr int64_t kAutoGroupBatch = 1024;  // eight-lane kernel from here (automatic)
constexpr int64_t kAutoSpecBatch = 12288;  // speculative form for solves up to here (automatic)
// The sixteen-lane form — one problem per 16-lane DPP row, four per wavefront — is the latency form,
// for batches that leave every wavefront a SIMD of its own (up to kGroup16Batch problems = one round
// of 1024 wavefronts), and — in rounds of kGroup16Batch — wherever whole rounds beat the other forms
// (above kGroupWsTop).
constexpr int64_t kGroup16Batch = 4096;
// Workspace form of the eight-lane kernel (records and gains in a caller-provided HBM workspace: 4 KB
// of LDS per problem, four wavefronts per CU): the choice above kGroupWsBatch problems
constexpr int64_t kGroupWsBatch = 4096;
// ... up to kGroupWsTop problems: the LDS form of the sixteen-lane kernel runs in rounds of 4096
// problems (0.168 ms each), the workspace form's time grows with the batch (0.25 ms + 25 us per
// 1024 problems): 5120 problems 0.285 against 0.330 ms, 6144: 0.306 / 0.339, 8192: 0.354 / 0.348,
// 12288: 0.583 / 0.502, 20480: 0.872 / 0.804 (tools/_diag/mid_check.py).
// Round 5 (tools/threshold_sweep.py, three shapes): at 8192 problems in fp64 the workspace form is
// ahead at every shape measured (bicycle6 N=20: 0.313 against 0.337 ms, bicycle4 N=6: 0.106 / 0.136,
// bicycle4 N=20: 0.279 / 0.314), in fp32 it is behind there (0.250 / 0.197): the top of the range
// depends on the precision.
constexpr int64_t kGroupWsTop = 8192;      // fp64
constexpr int64_t kGroupWsTopF32 = 7168;
// Wavefronts per group of eight problems in the speculative kernel.  Three skip two rejects per
// round but share one CU's LDS three ways; the stragglers that decide a solve's duration alternate
// accept / reject, which two wavefronts cover: measured (i2lqr_solve, ms) 16 problems 0.43 (V = 3)
// / 0.46 (V = 2), 256: 0.25 / 0.26, 1024: 0.77 / 0.72, 2048: 0.70 / 0.50, tail of 65536: 2.41 /
// 2.34.  Three up to kSpecWideBatch problems where they fit, two above and in the tail.
constexpr int kSpecWideBatch = 512;

// ---- what fits: ONE comparison each, of a ColumnFit field with the device's dynamic-LDS limit ------
inline bool lds_fits(const DeviceGeometry& g, size_t bytes) { return bytes <= g.max_dyn_lds; }
// the plants of the eight- / sixteen-lane kernels: the bicycles, Q = R = 0
inline bool column_plant_ok(const ColumnFit& f) { return f.plant == ColumnFit::BICYCLE && !f.weights; }
// the LDS form of the eight- / sixteen-lane kernel (lanes = 8 / 16; four slices: longer horizons)
inline bool group_fits(const DeviceGeometry& g, const ColumnFit& f, int lanes) {
  return column_plant_ok(f) && f.problem_major && lds_fits(g, lanes == 16 ? f.lds_group16 : f.lds_group8);
}
// the speculative form, two wavefronts
inline bool spec_fits(const DeviceGeometry& g, const ColumnFit& f, int lanes) {
  if (!column_plant_ok(f) || !f.problem_major) return false;
  return lanes == 16 ? lds_fits(g, f.lds_spec16x2) : (group_fits(g, f, 8) && lds_fits(g, f.lds_spec8x2));
}
// ... as the tail of the chunked solves, whatever the handle's layout: lanes per problem, 0: none
inline int spec_tail_lanes(const DeviceGeometry& g, const ColumnFit& f) {
  if (!column_plant_ok(f)) return 0;
  return lds_fits(g, f.lds_spec16x2) ? 16 : (lds_fits(g, f.lds_spec8x2) ? 8 : 0);
}
// chains (k_group_spec<.., 3, false, 16, true>): the sixteen-lane form with three wavefronts
inline bool spec_chain_fits(const DeviceGeometry& g, const ColumnFit& f, int64_t chains) {
  if (!column_plant_ok(f) || !f.problem_major) return false;
  return chains <= g.scaled(kSpecWideBatch) && lds_fits(g, f.lds_spec16x3);
}
// workspace of the eight-lane workspace form for B problems (whole wavefronts); 0: not supported
inline int64_t group_ws_bytes(const DeviceGeometry& g, const ColumnFit& f, int64_t B) {
  if (!group_fits(g, f, 8) || B <= 0 || !lds_fits(g, f.lds_group_ws)) return 0;
  return (B + kEightLaneProblems - 1) / kEightLaneProblems * kEightLaneProblems * f.ws_group;
}
inline bool quad_fits(const DeviceGeometry& g, const ColumnFit& f) {
  return f.plant == ColumnFit::SIXTEEN && f.problem_major && !f.weights && lds_fits(g, f.lds_quad);
}
inline int64_t quad_ws_bytes(const DeviceGeometry& g, const ColumnFit& f, int64_t B) {
  if (!quad_fits(g, f)) return 0;
  return (B + kSixteenLaneProblems - 1) / kSixteenLaneProblems * kSixteenLaneProblems * f.ws_quad;
}

// The batches for which the eight-lane workspace form is asked for: the automatic range, above its
// lower edge with "group_lanes" 8, or pinned.  ONE predicate: column_kernel() chooses the form by it
// and column_workspace_bytes() reports a size by it.
inline bool ws_range(const DeviceGeometry& g, const ColumnFit& f, int64_t B) {
  return B > g.scaled(kGroupWsBatch) && B <= g.scaled(f.f64 ? kGroupWsTop : kGroupWsTopF32);
}
inline bool ws_asked(const DeviceGeometry& g, const ColumnFit& f, const ColumnTune& t, int64_t B) {
  return ws_range(g, f, B) || (t.opt_group == 8 && B > g.scaled(kGroupWsBatch)) || t.opt_group_ws == 1;
}

// ---- which fused kernel a problem-major call runs on ---------------------------------------------------
// ONE function, used by the launcher and by i2lqr_iterate_kernel / i2lqr_solve_kernel (what bench.py
// labels its results with).
enum ColumnKernel { K_WAVE, K_WAVE_OPT, K_GROUP, K_GROUP16, K_GROUP_WS, K_SPEC, K_SPEC16, K_QUAD, K_INVALID };
struct ColumnChoice {
  ColumnKernel kernel;
  const char* why;  // the message of K_INVALID (a forced option the configuration cannot honour)
};

// ws_bytes: of the registered workspace, -1 without one
inline ColumnChoice column_kernel(const DeviceGeometry& g, const ColumnFit& fit, const ColumnTune& t,
                                  WaveForm f, int64_t ws_bytes, int64_t B, bool early_exit) {
  // a model is on ("line_search", "obstacles", a state box, "barrier_cost"): every call runs on that form of the
  // one-problem-per-wavefront kernel (i2lqr_wave_opt.h), whatever the batch size
  if (f != WAVE_PLAIN) {
    if (t.opt_group == 8 || t.opt_group == 16) {
      static thread_local char msg[128];
      snprintf(msg, sizeof(msg), "%s runs on the one-problem-per-wavefront kernel: not together "
               "with \"group_lanes\" = 8 or 16", wave_phrase(f));
      return {K_INVALID, msg};
    }
    return {K_WAVE_OPT, ""};
  }
  const bool m2 = fit.plant == ColumnFit::BICYCLE;
  const bool q16 = fit.plant == ColumnFit::SIXTEEN;
  if (m2) {
    // Eight lanes per problem, eight problems per wavefront (i2lqr_group.hpp).  Automatic where it
    // is built (the bicycles, Q = R = 0) from 1024 problems: below that every problem gets a SIMD
    // of its own either way and the one-problem-per-wavefront kernel's iteration is ~8 % shorter
    // (tools/group_ab.py: 0.195 vs 0.212 ms per 10 iterations at 64-256 problems, 0.219 vs 0.213
    // at 1024, 0.63 vs 0.25 at 4096).
    const bool can = group_fits(g, fit, 8);
    if (t.opt_group == 8 && !can)
      return {K_INVALID, "\"group_lanes\" = 8 needs a bicycle plant with Q = R = 0 and a horizon whose "
                         "eight problem slices fit a CU's LDS"};
    // Speculative form (k_group_spec): two or three wavefronts per eight problems run the
    // iterations that follow 0, 1, (2) rejects at once; bit-identical results.  With a FIXED
    // iteration count it measures slower than the plain kernel (0.275 vs 0.215 ms per 10
    // iterations at 1024 problems), so it stays opt-in there.  Automatic for solves to
    // termination (early_exit) of at most kAutoSpecBatch problems: the launch lasts as long as
    // its slowest problem, and the slowest problems alternate accepts and rejects — i2lqr_solve
    // 0.60 -> 0.44 ms at 16 problems, 1.21 -> 0.71 ms at 1024, 1.23 -> 1.17 at 8192.
    // (sixteen lanes per problem — the DPP passes, four problems per workgroup — wherever its
    // buffers fit; "group_lanes" 8 pins the eight-lane form)
    const bool can_spec16 = spec_fits(g, fit, 16), can_spec8 = spec_fits(g, fit, 8);
    const bool spec16 = t.opt_group == 16 || (t.opt_group < 0 && can_spec16);
    const bool can_spec = spec16 ? can_spec16 : can_spec8;
    if (t.opt_spec == 1 && !can_spec)
      return {K_INVALID, "\"speculate\" = 1 needs the eight- / sixteen-lane kernel and a horizon whose "
                         "speculative buffers fit a CU's LDS"};
    if (can_spec && t.opt_group != 64 &&
        (t.opt_spec == 1 ||
         (t.opt_spec < 0 && t.opt_group < 0 && early_exit && B <= g.scaled(kAutoSpecBatch))))
      return {spec16 ? K_SPEC16 : K_SPEC, ""};
    // Sixteen lanes per problem (one problem per DPP row; GroupWorker::backward_row / forward_row):
    // no LDS round trip in the serial chains.  Four problems per wavefront: automatic for every
    // batch that still leaves each wavefront a SIMD of its own (up to kGroup16Batch problems) —
    // its iteration is shorter than the one-problem-per-wavefront kernel's at ANY size (0.145
    // against 0.188 ms per 10 iterations from 1 to 512 problems, n = 6, N = 20; tools/_diag);
    // "group_lanes" 16 / 8 / 64 pins the choice.
    const bool can16 = group_fits(g, fit, 16);  // (four slices: longer horizons than `can`)
    if (t.opt_group == 16 && !can16)
      return {K_INVALID, "\"group_lanes\" = 16 needs a bicycle plant with Q = R = 0 and a horizon whose "
                         "four problem slices fit a CU's LDS"};
    // Beyond one round of 1024 wavefronts the sixteen-lane kernel runs in rounds (0.168 ms per 4096
    // problems); the eight-lane workspace form (four wavefronts of eight problems per CU) is the
    // better choice only between 4096 and kGroupWsTop problems — and only with the caller's
    // workspace registered.
    const int64_t need = can ? group_ws_bytes(g, fit, B) : 0;
    const bool have_ws = need > 0 && ws_bytes >= need;
    if (t.opt_group == 16 ||
        (t.opt_group < 0 && can16 && t.opt_group_ws != 1 && !(ws_range(g, fit, B) && can && have_ws)))
      return {K_GROUP16, ""};
    if (t.opt_group == 8 || (t.opt_group < 0 && can && B >= g.scaled(kAutoGroupBatch))) {
      // "group_workspace" 0 / 1 pins the choice of the eight-lane form
      if (t.opt_group_ws == 1 && !have_ws)
        return {K_INVALID, "\"group_workspace\" = 1 needs a registered workspace of "
                           "i2lqr_workspace_bytes() for this batch"};
      if (have_ws && t.opt_group_ws != 0 && ws_asked(g, fit, t, B)) return {K_GROUP_WS, ""};
      return {K_GROUP, ""};
    }
  } else if (t.opt_group == 8) {
    return {K_INVALID, "\"group_lanes\" = 8 is built for the m = 2 plants only"};
  }
  if (q16) {
    // Sixteen lanes per problem, four problems per wavefront (i2lqr_quad.hpp): needs the caller's
    // workspace (i2lqr_workspace_bytes); automatic whenever it is registered.
    const bool can = quad_fits(g, fit);
    const bool have_ws = ws_bytes >= quad_ws_bytes(g, fit, B);
    if (t.opt_group == 16 && !(can && have_ws))
      return {K_INVALID, "\"group_lanes\" = 16 needs Q = R = 0 and a registered workspace of "
                         "i2lqr_workspace_bytes() for this batch"};
    if ((t.opt_group == 16 || t.opt_group < 0) && can && have_ws) return {K_QUAD, ""};
  } else if (t.opt_group == 16 && !m2) {
    return {K_INVALID, "\"group_lanes\" = 16 is built for the bicycles (DPP row form) and the "
                       "n + m = 16 plant"};
  }
  return {K_WAVE, ""};
}

// what i2lqr_iterate_kernel / i2lqr_solve_kernel report for a problem-major handle
inline const char* column_kernel_name(ColumnKernel k, WaveForm f) {
  switch (k) {
    case K_SPEC: return "k_group_spec";
    case K_SPEC16: return "k_group_spec (sixteen lanes)";
    case K_GROUP: return "k_group_iterate";
    case K_GROUP16: return "k_group_iterate (sixteen lanes)";
    case K_GROUP_WS: return "k_group_iterate (workspace form)";
    case K_QUAD: return "k_quad_iterate";
    case K_WAVE_OPT: return wave_kernel_name(f);
    case K_WAVE: return "k_iterate";
    default: return "unsupported";  // the launch returns I2LQR_ERR_UNSUPPORTED
  }
}

// The caller's workspace of a problem-major handle (i2lqr_workspace_bytes): quad12's sixteen-lane
// kernel; the bicycles' eight-lane workspace form only where column_kernel() asks for it (a
// problem-major batch of 2^20 problems does not need 5.9 GB of scratch it would never use)
inline int64_t column_workspace_bytes(const DeviceGeometry& g, const ColumnFit& f, const ColumnTune& t,
                                      int64_t B) {
  if (f.plant == ColumnFit::SIXTEEN) return quad_ws_bytes(g, f, B);
  return ws_asked(g, f, t, B) ? group_ws_bytes(g, f, B) : 0;
}

// ---- wavefronts per workgroup ------------------------------------------------------------------------
// Eight-lane kernel: two helper wavefronts for the record phase (k_group_iterate<.., 3>) while every
// workgroup has a CU to itself (<= 256 workgroups = 2048 problems): 0.2216 -> 0.2107 ms per 10
// iterations at 1024 problems (two / four wavefronts: 0.2122 / 0.2102).  With two workgroups per CU
// the extra wavefronts crowd the main ones off their SIMDs: 0.25 -> 0.40 ms at 4096 problems.
inline int group8_wavefronts(const DeviceGeometry& g, int64_t B) {
  return (B + kEightLaneProblems - 1) / kEightLaneProblems <= g.cus ? 3 : 1;
}
// Sixteen-lane kernel: one helper wavefront for the record phase (2 x 16 lanes >= the 21 records of
// a problem: one round) while that leaves every wavefront a SIMD of its own (<= 512 workgroups =
// 2048 problems).  Overlapped schedule (k_group_iterate<.., 3, false, 16>; overlap = false forces the
// one-helper form): two helpers take all the records while the main wavefront computes the terminal
// block, and they store the gains at exit — while every workgroup has a CU to itself (<= 256
// workgroups = 1024 problems: three SIMDs of four).
inline int group16_wavefronts(const DeviceGeometry& g, int64_t B, bool overlap) {
  const int64_t workgroups = (B + kSixteenLaneProblems - 1) / kSixteenLaneProblems;
  if (overlap && workgroups <= g.cus) return 3;
  return workgroups <= 2 * (int64_t)g.cus ? 2 : 1;
}
// ... its fixed-horizon form (k_group_iterate_fixed) with the same number of wavefronts, where the
// horizon is one it is built for
inline bool group16_fixed(const ColumnFit& f, const ColumnTune& t) {
  return t.opt_group_fixed != 0 && f.fixed_horizon;
}
// Speculative kernel (kSpecWideBatch above); tail: of the chunked solves, never wide
inline int spec_wavefronts(const DeviceGeometry& g, const ColumnFit& f, int lanes, int64_t B, bool tail) {
  const bool wide = !tail && B <= g.scaled(kSpecWideBatch) &&
                    lds_fits(g, lanes == 16 ? f.lds_spec16x3 : f.lds_spec8x3);
  return wide ? 3 : 2;
}

// ---- the one-problem-per-wavefront kernel ----------------------------------------------------------------
// Per-step F matrices (prep() writes them in parallel over t; the serial recursion then has no
// Jacobian refresh) double the LDS slice: taken when every wavefront of the launch still fits on the
// chip at once, i.e. in the latency-bound regime this variant exists for.
inline bool wave_fstep(const DeviceGeometry& g, const ColumnFit& f, const ColumnTune& t, int64_t B) {
  if (f.lds_wave_fstep == 0 || f.lds_wave_fstep > g.default_dyn_lds) return false;
  if (t.opt_fstep >= 0) return t.opt_fstep != 0;
  const int64_t waves_per_cu = (B + g.cus - 1) / g.cus;
  return (size_t)waves_per_cu * f.lds_wave_fstep <= g.lds_per_cu - 10 * 1024;
}
// The opt-in form of a call (chained: k_chain_box) takes its records and the box's words behind the
// handle's slice: the bytes per wavefront, to fit the device's dynamic LDS
inline size_t wave_lds_need(const ColumnFit& f, const WaveModel& model, bool chained) {
  return f.lds_wave + model.extra_lds_bytes(model.form(chained), f.n, f.N, (size_t)f.word);
}

// i2lqr_solve_chained, `chains` chains in ONE launch: k_group_spec<.., CHAIN> where it is built for
// the handle; otherwise, and with a model on, "wave_chain" 1 runs k_chain_box (i2lqr_wave_chain.hip)
// with the handle's state box, "obstacles" and "line_search"
// Neither chain kernel has the barrier cost (k_chain_box's accept / reject step is k_iterate_box's).
struct ChainPlan {
  enum Kind { SPEC, WAVE, REFUSED } kind;
  const char* why;  // REFUSED: the message
};
constexpr const char* kChainNoBarrierCost =
    "chains have no barrier cost: neither the speculative chain kernel nor \"wave_chain\" "
    "(k_chain_box) carries \"barrier_cost\"; solve the chain steps one after the other instead "
    "(a launch per chain step, lamb carried over)";
inline ChainPlan chain_plan(const DeviceGeometry& g, const ColumnFit& fit, const ColumnTune& t,
                            WaveForm f, int64_t ws_bytes, int64_t chains) {
  if (f == WAVE_MERIT) return {ChainPlan::REFUSED, kChainNoBarrierCost};  // with or without "wave_chain"
  const bool bicycle = fit.plant == ColumnFit::BICYCLE;
  const bool wc = t.opt_wave_chain == 1, model = f != WAVE_PLAIN;
  // (not asked about where "wave_chain" takes the model anyway)
  const bool spec = bicycle && !(wc && model) &&
                    !(t.opt_spec == 0 || t.opt_group == 8 || t.opt_group == 64 ||
                      !spec_chain_fits(g, fit, chains));
  const bool wave = wc && (model || !spec);
  if (!wave && !spec) {
    if (!bicycle) return {ChainPlan::REFUSED, "chains are built for the m = 2 plants"};
    static thread_local char msg[320];
    snprintf(msg, sizeof(msg), "chains run on the sixteen-lane speculative kernel: a "
             "bicycle plant with Q = R = 0, at most %lld chains, a horizon whose three-wavefront "
             "buffers fit a CU's LDS (solve the chain steps one after the other instead)",
             (long long)g.scaled(kSpecWideBatch));
    return {ChainPlan::REFUSED, msg};
  }
  if (wave && model) {  // a model with "group_lanes" 8 or 16: refused as i2lqr_solve refuses it
    const ColumnChoice c = column_kernel(g, fit, t, f, ws_bytes, chains, true);
    if (c.kernel == K_INVALID) return {ChainPlan::REFUSED, c.why};
  }
  return {wave ? ChainPlan::WAVE : ChainPlan::SPEC, ""};
}

// ---- which layout a caller should create the handle in (i2lqr_recommended_layout) -----------------------
// Batch sizes from which the one-problem-per-lane layouts win over the problem-major kernels.
// Round 4 measured ONE shape (fp64, n=6, N=20: 12289 for both entry points) and applied it to every
// bicycle configuration; round 5 measured twelve (tools/threshold_sweep.py: both bicycles x
// horizons 6 / 20 / 50 x fp64 / fp32, interleaved on one device, every launch on its own copy of the
// batch; profiles/r05_threshold_sweep*.json, table in profiles/README.md).  The crossover moves
// with the horizon and the precision by far more than 25 %: the sixteen-lane kernel holds
// 4 x (wavefronts whose LDS slices fit a CU) x 256 problems per round — 4096 at N = 20 in fp64,
// 1024 at N = 50 — while the lane kernels' launch floor grows only linearly with N, and a solve to
// termination on the lane layouts is chunked (compaction) from 4096 problems only.
// Each entry is the first batch size at which the lane layout was ahead (the last size the
// problem-major kernels won, plus one: their time is a staircase in rounds, the lane kernels'
// is flat).  A horizon between the measured ones takes the nearer one on a log scale.
//   quad12 (fp64): the sixteen-lane kernel 13 M it/s at any size, k_lane_iterate_rows 25 M at
//   8192 and 73 M at 65536.
struct LaneFrom { int64_t iterate, solve; };
// (re-measured with the helper-wavefront form of the lane kernel, which moved the bicycle6 N = 20
// crossover from 12289 to 8193 in fp64 and from 16385 to 12289 in fp32: profiles/
// r05_threshold_sweep5.json ... 9.json)
constexpr LaneFrom kLaneFrom[2][3][2] = {
    // bicycle4:          fp64              fp32
    /* N ~ 6  */ {{{8193, 10241}, {8193, 10241}},
    /* N ~ 20 */  {{8193, 4096}, {8193, 10241}},
    /* N ~ 50 */  {{4097, 4096}, {8193, 5121}}},
    // bicycle6
    /* N ~ 6  */ {{{8193, 6145}, {8193, 20481}},
    /* N ~ 20 */  {{8193, 10241}, {12289, 12289}},
    /* N ~ 50 */  {{3073, 4096}, {8193, 5121}}},
};
inline LaneFrom lane_from(const i2lqr_config& cfg) {
  const int sys = cfg.system_id == I2LQR_SYS_BICYCLE6 ? 1 : 0;
  const int nb = cfg.N <= 10 ? 0 : (cfg.N <= 31 ? 1 : 2);  // sqrt(6 x 20) = 10.95, sqrt(20 x 50) = 31.6
  return kLaneFrom[sys][nb][cfg.dtype == I2LQR_F64 ? 0 : 1];
}
// quad12 (round 5, the same sweep: profiles/r05_threshold_sweep3.json, ..4.json; round 4: 8192 for
// everything, measured at N = 50 fp64 fixed counts only).  The problem-major side is the
// sixteen-lane kernel with its HBM workspace (rounds of 4096 problems); solves stay there longer
// because the lane layouts have no latency tail for this plant.  [N <= 31, N > 31][fp64, fp32]
constexpr LaneFrom kLaneFromQuad[2][2] = {
    /* N ~ 20 */ {{4097, 8193}, {8193, 24577}},
    /* N ~ 50 */ {{4097, 6145}, {8193, 12289}},
};
// with stage weights the problem-major side is the one-problem-per-wavefront kernel: 2048 problems
// already fill the chip's SIMDs (as for the bicycles)
constexpr int64_t kLaneFromWeights = 2048;

// What the one-problem-per-lane kernels need of the weights (they store only the upper triangles
// of the value function): nullptr, or what is not symmetric
inline const char* lane_asymmetry(const i2lqr_config& cfg) {
  for (int i = 0; i < cfg.n; i++)
    for (int j = 0; j < i; j++)
      if (cfg.Q[i * I2LQR_MAX_N + j] != cfg.Q[j * I2LQR_MAX_N + i] ||
          cfg.Qt[i * I2LQR_MAX_N + j] != cfg.Qt[j * I2LQR_MAX_N + i])
        return "symmetric Q and Qterminal";
  for (int a = 0; a < cfg.m; a++)
    for (int b = 0; b < a; b++)
      if (cfg.R[a * I2LQR_MAX_M + b] != cfg.R[b * I2LQR_MAX_M + a]) return "a symmetric R";
  return nullptr;
}

// The layout for B problems of a configuration whose system_id is one of the three plants; weights:
// it has stage weights (has_stage_weights, i2lqr_devcfg.hpp)
inline int recommended_layout(const DeviceGeometry& g, const i2lqr_config& cfg, bool weights, int64_t B,
                              bool early_exit) {
  // what the lane layouts cannot run stays problem-major: non-symmetric weights (the kernels keep
  // the upper triangles), and for quad12 (row-block kernel) fp32 WITH stage weights
  bool lane_ok = !lane_asymmetry(cfg);
  int64_t from;
  if (cfg.system_id == I2LQR_SYS_QUAD12) {
    const LaneFrom q = kLaneFromQuad[cfg.N <= 31 ? 0 : 1][cfg.dtype == I2LQR_F64 ? 0 : 1];
    from = weights ? kLaneFromWeights : (early_exit ? q.solve : q.iterate);
    if (cfg.dtype != I2LQR_F64 && weights) lane_ok = false;  // fp32: Q = R = 0 (round 5)
  } else {
    // with stage weights the problem-major side is the one-problem-per-wavefront kernel (the
    // column kernels are built for Q = R = 0): 1024 problems already fill the chip's SIMDs
    from = weights ? kLaneFromWeights : (early_exit ? lane_from(cfg).solve : lane_from(cfg).iterate);
  }
  // measured on the 256-CU chip; on another CU count (a partitioned device) scaled by cus / 256:
  // both sides of the crossover are occupancy effects (i2lqr_geometry.hpp)
  from = g.scaled_from(from);
  if (!lane_ok || B < from) return I2LQR_LAYOUT_PROBLEM_MAJOR;
  return B % 64 == 0 ? I2LQR_LAYOUT_BATCH_TILED : I2LQR_LAYOUT_BATCH_MINOR;
}

}  // namespace i2lqr
