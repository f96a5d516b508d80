// What the launcher of the one-problem-per-lane kernels (i2lqr_lane_launch.hpp) decides from
// integers alone: the scheduling options of a launch, the layout of the caller's workspace and the
// rounds of the chunked solve.  Plain C++17, no HIP: the host test builds it alone
// (tests/test_lane_plan_host.py).
#pragma once
#include <cstddef>
#include <cstdint>

#include "i2lqr_geometry.hpp"
#include "i2lqr_lane_opt_in.hpp"

namespace i2lqr {

// State checkpointing keeps every kSeg-th state in HBM between the passes (i2lqr_lane.hpp)
constexpr int kSeg = 4;
constexpr int kMaxRounds = 24;  // compaction rounds of the chunked solve (one counter each)
constexpr int kFirstChunk = 8;
constexpr int kFinalRound = 3;  // chunked solve: the round (at 24 iterations) whose tail takes everything
// (measured on the 256-CU chip: DeviceGeometry::scaled() where they are used)
constexpr int kAutoWaveTail = 2048;
constexpr int kAutoSpecTail = 12288;  // (round 5: 8192; tools/solve_bench.py --plans)
constexpr int64_t kAutoCompactBatch = 4096;

// The handle's options of the lane layouts (i2lqr_set_option, i2lqr_set_compaction); -1 = automatic
struct LaneTune {
  int64_t compact_min_batch = -1;  // i2lqr_solve uses the chunked, compacting form from this batch; 0: never
  // scheduling options of the one-problem-per-lane kernels
  int opt_defer = -1, opt_reroll = -1, opt_lds_steps = -1, opt_merge = -1, opt_ckpt = -1, opt_stagger = -1;
  int wave_tail = -1;  // chunked solve: finish <= this many survivors with one problem per wavefront (0: off)
  int opt_pair = -1;  // bicycles' lane kernel (fp64 and fp32, with or without stage weights): workgroups of two wavefronts (main + helper)
  int opt_two_x = -1;  // ... its second state buffer (no re-roll of accepted steps)
  int opt_chunk_step = -1;  // chunked solve: length of the chunk that follows the first (automatic: 4); a schedule to measure against
  int opt_fuse = -1;  // chunked solve: compaction folded into the chunk kernels' exit (round 6); 0: k_lane_compact launches; automatic: on
  int opt_final_round = -1;  // chunked solve: the round whose tail kernel takes every survivor and ends the schedule; 0: never
  int opt_first_chunk = -1;  // chunked solve: pinned length of the first chunk, no extension chunks (a hand-tuned schedule to measure the data-driven one against)
  int opt_model_chunks = -1;  // "lane_model_chunks" 1: i2lqr_solve of a model handle (LaneModel::on) runs as the chunked solve where chunked() holds; automatic: off
};

// What a launcher instantiation and the handle's configuration fix
struct LaneShape {
  int n, m, N;
  int word;      // sizeof(T)
  bool rows;     // a row-block plant (Sys::NBLK > 0: quad12), its own fused kernel without LDS
  bool weights;  // stage weights Q, R != 0
  int max_iter;

  // gains of one horizon step, 64 lanes: what a step that stays in LDS takes
  int step_bytes() const { return 64 * m * (n + 1) * word; }
  // k_0 of 64 lanes: step 0 keeps only its feed-forward term in LDS (LaneWorker::lds_k0)
  int k0_bytes() const { return 64 * m * word; }
  // LDS of the state checkpointing: the states of one segment of kSeg steps for 64 lanes
  int seg_bytes() const { return (kSeg + 1) * n * 64 * word; }
};

// The scalar fields of a launch (LaneArgs carries them to the kernel under the same names; the
// functions below that take `class A` read them from either)
struct LaneOptions {
  int defer, reroll, merge, ckpt, stagger, lds_steps, lds_grow, two_max;
};

inline unsigned lane_grid(int64_t B) { return (unsigned)((B + 63) / 64); }

// The helper-wavefront form (k_lane_iterate_pair; round 5): the bicycles in fp64 and fp32 (stage
// weights: its HASQR instantiations), states not checkpointed, and a launch of at most 512 workgroups (32768 problems) - two wavefronts per
// workgroup then still find a SIMD each.  Properties of the chip: half as many workgroups as it
// has SIMDs (512 on 256 CUs); the second state buffer up to one workgroup per CU.
inline unsigned pair_max_grid(const DeviceGeometry& g) { return (unsigned)(g.simds() / 2); }
inline unsigned two_x_max_grid(const DeviceGeometry& g) { return (unsigned)g.cus; }
template <class A> bool pair_built(const LaneShape& s, const A& a, int opt_pair) {
  return !s.rows && !a.ckpt && opt_pair != 0;
}
template <class A>
bool use_pair(const DeviceGeometry& g, const LaneShape& s, const A& a, int64_t B, int opt_pair) {
  return pair_built(s, a, opt_pair) && (opt_pair == 1 || lane_grid(B) <= pair_max_grid(g));
}
template <class A> size_t lane_lds(const LaneShape& s, const A& a) {
  return (size_t)a.lds_steps * s.step_bytes() + s.k0_bytes() + (a.ckpt ? s.seg_bytes() : 0);
}
// A launch of at most 256 / 512 workgroups puts one / two of them on a CU, so each has 160 / 80
// KiB of LDS to itself where a full launch budgets 36 (four wavefronts per CU): the gains of that
// many more horizon steps stay in LDS between the backward and the forward pass instead of going
// through HBM (fp64, n = 6, m = 2: 19 of 20 steps up to 256 workgroups, 8-10 up to 512).
// lds_steps of a launch of `workgroups` workgroups with `fixed` bytes of other dynamic LDS each,
// at most max_dyn bytes of dynamic LDS per workgroup
template <class A>
int grown_lds_steps(const DeviceGeometry& g, const LaneShape& s, const A& a, unsigned workgroups,
                    size_t fixed, size_t max_dyn) {
  if (!a.lds_grow || a.ckpt) return a.lds_steps;
  const unsigned per_cu = (workgroups + (unsigned)g.cus - 1) / (unsigned)g.cus;
  size_t budget = g.lds_per_cu / (per_cu ? per_cu : 1);
  if (budget > max_dyn) budget = max_dyn;
  const size_t need0 = fixed + s.k0_bytes() + 1024;  // (1 KiB: allocation granularity)
  int steps = budget > need0 ? (int)((budget - need0) / (size_t)s.step_bytes()) : 0;
  if (steps > s.N - 1) steps = s.N - 1;
  return steps > a.lds_steps ? steps : a.lds_steps;
}

// i2lqr_solve of B problems runs as the chunked solve (LaneLaunch::solve_compacting).  Automatic:
// from 4096 problems with more than 16 iterations allowed (measured 1.2-1.9x on the bench workload
// from 4096 to 262144 problems; the chunks alone cost ~9 % when nothing terminates early).
inline bool chunked(const DeviceGeometry& g, const LaneShape& s, const LaneTune& t, int64_t B) {
  const int64_t cmin = t.compact_min_batch < 0
      ? (s.max_iter > 16 ? g.scaled(kAutoCompactBatch) : 0) : t.compact_min_batch;
  return cmin > 0 && B >= cmin && s.max_iter > 4;
}

// The options of a launch of B problems.  single_launch_solve: a solve to termination that is not
// chunked — bound by its slowest problem's latency, not by HBM traffic, so the states are neither
// deferred nor re-rolled unless pinned.
inline LaneOptions lane_options(const DeviceGeometry& g, const LaneShape& s, const LaneTune& t,
                                int64_t B, bool single_launch_solve) {
  LaneOptions o;
  o.two_max = 64 * (int)(t.opt_two_x == 1 ? pair_max_grid(g) : two_x_max_grid(g));
  // The gains of the first steps stay in LDS: as many steps as keep the register-limited number
  // of wavefronts per CU (one per SIMD, four per CU) resident in the 160 KiB: 36 KiB each, i.e.
  // 5 steps in fp64 and 10 in fp32 at n=6, m=2.
  o.lds_steps = ((int)g.lds_per_simd_wave() - s.k0_bytes()) / s.step_bytes();  // steps 1..lds_steps; k_0 sits behind them
  if (o.lds_steps < 0) o.lds_steps = 0;
  if (o.lds_steps > s.N - 1) o.lds_steps = s.N - 1;
  // (batch sizes in units of the chip: full = one wavefront per SIMD, 65536 problems on 256 CUs)
  const int64_t full = g.full_batch();
  o.reroll = B >= full / 2 ? 1 : 0;  // pays only where the kernel sits on the HBM roof (32768)
  o.defer = 1;  // the forward pass stores no states; accepted steps re-roll them (see i2lqr_lane.hpp)
  // ... and merge the accepted candidate inputs into the one input buffer.  fp64 (HBM-bound):
  // 7.56 -> 7.23 KB per problem-iteration, +4.8 % it/s at 2^20 problems; fp32 (instruction-bound):
  // the extra row writes cost 6 %, so the per-lane buffer swap stays (tools/ab_bench.py).  Below
  // ~40000 problems the fp64 kernel is instruction-bound as well (one or two wavefronts per CU):
  // 226 -> 237 M it/s at 12800 problems without the merge, 411 -> 426 at 24576, 528 -> 545 at
  // 32768, +-0 from 40960 to 57344, 811 -> 846 WITH it at 65536.
  o.merge = s.word == 8 && B > full / 2 ? 1 : 0;
  if (t.opt_merge >= 0) o.merge = t.opt_merge;
  o.stagger = 0;
  if (s.rows) {
    // automatic where the launch fills the chip (one wavefront per SIMD: 65536 problems)
    o.stagger = B >= full ? 45 : 0;
  } else if (s.word == 8 && B > full * 15 / 16 && B <= full * 5 / 4) {
    // bicycles, fp64, a launch of about one wavefront per SIMD: +3 % (883 -> 912 M it/s at 65536
    // problems, tools/ab_bench.py --cold); fp32 (issue-bound) gains nothing, launches of two
    // and more rounds desynchronise by themselves and only pay the delay (-2 %)
    o.stagger = 8;
  }
  if (t.opt_stagger >= 0) o.stagger = t.opt_stagger > 999 ? 999 : t.opt_stagger;
  if (t.opt_reroll >= 0) o.reroll = t.opt_reroll;
  if (t.opt_defer >= 0) o.defer = t.opt_defer;
  if (t.opt_lds_steps >= 0 && t.opt_lds_steps < o.lds_steps) o.lds_steps = t.opt_lds_steps;
  o.lds_grow = t.opt_lds_steps < 0 ? 1 : 0;
  // State checkpointing (i2lqr_lane.hpp): fp64 with deferred, merged states and the re-rolling
  // forward pass, Q = R = 0; automatic from 65536 problems (where the kernel sits on the HBM
  // roof).
  // (tools/ab_bench.py --cold, round 3: -2 % at 65536 problems, +-0 at 131072, +5 % at 262144,
  // +4-6 % at 2^20; HBM bytes per problem-iteration 6993 -> 6243 (1.41 -> 1.26 x algorithmic):
  // on from 65536 problems, BASELINE's roofline batch and half a per-GPU shard of configs[3] —
  // where the kernel already sits on the HBM roof the bytes are what is left to win)
  const auto ckpt = [&] {
    const bool can = s.word == 8 && !s.weights && o.defer && o.merge && o.reroll && s.N >= 2;
    return can && (t.opt_ckpt >= 0 ? t.opt_ckpt != 0 : B >= full);
  };
  // Its segment buffer takes the place of LDS-resident gain steps.  (The steps are given up with the
  // options of the fixed-count launch, before the single-launch solve switches the checkpoints off
  // again: what the launcher has always done, kept so that every launch stays as it was.)
  if (ckpt()) {
    int steps = ((int)g.lds_per_simd_wave() + 1024 - s.seg_bytes() - s.k0_bytes()) / s.step_bytes();
    if (steps < 0) steps = 0;
    if (o.lds_steps > steps) o.lds_steps = steps;
  }
  if (single_launch_solve) {
    if (t.opt_reroll < 0) o.reroll = 0;
    if (t.opt_defer < 0) o.defer = 0;
  }
  o.ckpt = ckpt();
  return o;
}

// LDS of a model launch (LaneModel, i2lqr_lane_opt_in.hpp) behind the gain steps and k_0: records
// 1 ... K - 1 of 64 lanes, six words each, staged once per launch (record 0 stays in registers as in
// k_lane_iterate; the box is a by-value kernel argument and takes none)
inline size_t lane_model_bytes(const LaneShape& s, const LaneModel& md) {
  return md.records > 1 ? (size_t)64 * 6 * (size_t)(md.records - 1) * (size_t)s.word : 0;
}
// A model launch: k_lane_iterate's one-wavefront form, states not checkpointed.  i2lqr_solve is ONE
// launch with early exit whatever the batch, unless "lane_model_chunks" is 1: then it is the chunked
// solve from the batch chunked() gives, with lane chunks and the fused exit only (k_lane_compact and
// the tail kernels have no models) and the options of a launch that is not a single-launch solve.
// The records take the place of LDS-resident gain steps.
// Which forms have chunk kernels.  k_lane_chunk_model and k_lane_chunk_merit: all.  k_lane_chunk_ls
// (the line search): with the barrier cost only, and not bicycle6 in fp32 with stage weights - the
// other instantiations do not compile without scratch (the soft ones keep a spilled scalar tuple's
// frame, fp32 bicycle6 with weights spills vector registers inside the loop: DESIGN.md 3.5), so they
// are not built and such a solve stays ONE launch.  The one rule: the kernel list
// (i2lqr_lane_ls.hpp), the launcher and the plan below all read it.
constexpr bool lane_chunks_built(int word, int n, bool weights, int line_search, bool barrier_cost) {
  return line_search <= 1 || (barrier_cost && !(word == 4 && n > 4 && weights));
}
struct LaneModelPlan {
  LaneOptions o;
  bool pair;     // always false: the helper-wavefront form has no models
  bool chunked;  // a solve to termination with "lane_model_chunks" 1, chunked() and lane_chunks_built()
  size_t model_bytes;
  size_t lds;   // dynamic LDS the launch asks for before grown_lds_steps(): gain steps + k_0 + records
  bool fits;    // k_0 and the records fit the dynamic LDS a workgroup gets without asking for more
};
inline LaneModelPlan lane_model_plan(const DeviceGeometry& g, const LaneShape& s, const LaneTune& t,
                                     const LaneModel& md, int64_t B, bool solve) {
  LaneModelPlan p;
  LaneTune tm = t;
  tm.opt_ckpt = 0;
  tm.opt_pair = 0;
  p.chunked = solve && t.opt_model_chunks == 1 && chunked(g, s, t, B) &&
              lane_chunks_built(s.word, s.n, s.weights, md.line_search, md.barrier_cost);
  p.o = lane_options(g, s, tm, B, solve && !p.chunked);
  p.model_bytes = lane_model_bytes(s, md);
  const long room = (long)g.lds_per_simd_wave() - (long)s.k0_bytes() - (long)p.model_bytes;
  const int steps = room > 0 ? (int)(room / s.step_bytes()) : 0;
  if (p.o.lds_steps > steps) p.o.lds_steps = steps;
  p.pair = use_pair(g, s, p.o, B, tm.opt_pair);
  p.lds = lane_lds(s, p.o) + p.model_bytes;
  p.fits = (size_t)s.k0_bytes() + p.model_bytes <= g.default_dyn_lds;
  return p;
}

// A model launch of a row-block plant ("lane_rows_models" 1; k_lane_iterate_rows_model,
// i2lqr_lane_rows_model.hpp): ONE launch whatever the batch and whatever "lane_model_chunks" says, the
// grid and the stagger of the plain k_lane_iterate_rows launch of that batch.  The kernel lives on four
// workgroups per CU, so its LDS is static and the model adds nothing to it: records
// 1 ... K - 1 are read from the obs rows at the step that uses them and the box is a by-value kernel
// argument.  What it takes is the row-block pass's own slice, in words per wavefront
// (LaneWorker::kGainWords, which asserts this formula): the step's [Kc | k], the obstacle terms, l_u,
// the sin / cos values, the state entries of the second Jacobian evaluation, u, and the five
// obstacle parameters of the pass - and the 64 words of the warm-up sink (budgeted in both word
// sizes; fp32 never takes the hot pass that warms rows up, and the compiler drops its sink).
constexpr int lane_rows_gain_words(int n, int m, int ntrig, int njx) {
  return (m * (n + 1) + 5 + m + ntrig + njx + m + 5) * 64;
}
struct LaneRowsModelPlan {
  unsigned grid;
  int stagger;
  size_t lds_bytes;  // static LDS of a workgroup (one wavefront)
  bool fits;         // four workgroups per CU still fit: lds_bytes <= LDS per CU / 4
};
// gain_words: lane_rows_gain_words() of the plant
inline LaneRowsModelPlan lane_rows_model_plan(const DeviceGeometry& g, const LaneShape& s,
                                              const LaneTune& t, const LaneModel& md, int64_t B,
                                              int gain_words) {
  LaneRowsModelPlan p;
  p.grid = lane_grid(B);
  p.stagger = lane_options(g, s, t, B, false).stagger;
  (void)md;  // records and the box take no LDS, whatever K and whichever sides are bounded
  p.lds_bytes = (size_t)gain_words * (size_t)s.word + 64 * sizeof(unsigned);
  p.fits = p.lds_bytes <= g.lds_per_cu / 4;
  return p;
}

// Workspace (byte offsets from the registered base) for B problems: candidate inputs + gains
// scratch + the second state buffer of the helper-wavefront form (every call), and for the chunked
// solve two compacted work sets, scratch iters / status and one counter per round.  ONE table:
// i2lqr_workspace_bytes returns `total`, the launcher carves base + offset.
// records, pen: the work sets of a chunked MODEL solve ("lane_model_chunks") hold 6 records rows of
// obs (row q records + r, as the caller's array) and, with the barrier cost, a row for the penalty of
// the nominal behind the cost row; the defaults are the table of every other handle.
struct LaneWorkspace {
  struct Set { int64_t X, U, x_term, obs, lamb, cost, iters, status, orig, pen = -1; };
  int64_t wsU, wsK, wsk;
  // second state buffer of the helper-wavefront form (rows of its own behind the gains scratch
  // since round 6 — the chunks' exits pack survivors into the work set the chunk does not run on,
  // which used to lend its states)
  int64_t wsX;
  Set set[2];
  int64_t uiters, ustatus;
  int64_t count;  // [kMaxRounds]: the live count after each compaction round
  int64_t total;
};
inline LaneWorkspace lane_workspace(const LaneShape& s, int64_t B, int records = 1, bool pen = false) {
  LaneWorkspace w;
  int64_t p = 0;
  const auto take = [&p](int64_t bytes) { const int64_t at = p; p += bytes; return at; };
  const int64_t row = B * s.word, n = s.n, m = s.m, N = s.N;
  w.wsU = take(row * (m * N));
  w.wsK = take(row * (m * n * N));
  w.wsk = take(row * (m * N));
  w.wsX = take(row * (n * (N + 1)));
  for (LaneWorkspace::Set& q : w.set) {
    q.X = take(row * (n * (N + 1)));
    q.U = take(row * (m * N));
    q.x_term = take(row * n);
    q.obs = take(row * 6 * records);
    q.lamb = take(row);
    q.cost = take(row);
    if (pen) q.pen = take(row);
  }
  // the int32 arrays start on the next multiple of 16 (the base is 16-byte aligned); 16 bytes are
  // set aside for that, and what the alignment does not use of them is left behind the counters
  const int64_t pad = (16 - p % 16) % 16;
  p += pad;
  for (LaneWorkspace::Set& q : w.set) {
    q.iters = take(B * 4);
    q.status = take(B * 4);
    q.orig = take(B * 4);
  }
  w.uiters = take(B * 4);
  w.ustatus = take(B * 4);
  w.count = take(kMaxRounds * 4);
  w.total = p + (16 - pad);
  return w;
}

// The schedule of the chunked solve is STRUCTURAL and its decisions are the device's (round 5;
// VERDICT r4 #3 — round 4 sized the first chunk from the bench workload's survivor curve, a
// constant fitted to workloads.make_batch): a first chunk of kFirstChunk iterations on the whole
// batch (never shorter: the tail kernel sums in another order than the lane kernels, and the
// more iterations of a long-horizon problem it runs the further the two solves drift apart in
// the last digits — 2.3e-8 relative at N = 50 with a first chunk of 6 against the suite's 1e-8),
// then rounds of { compaction, tail kernel, lane chunk } with chunk lengths 4, then as many
// iterations as are done (compaction points 8, 12, 24, 48, 96).  Which of the two kernels of a
// round does the work is decided ON THE DEVICE from the live count the compaction leaves: the
// tail kernel is a no-op above its cap ("wave_tail"), the lane chunk skips what the tail has
// finished.  Measured against hand-tuned first chunks of 8 / 10 / 12 / 14 on three
// distributions (the bench's; every problem with the obstacle; targets twice as far) at
// 16384 ... 262144 problems (tools/solve_bench.py --plans, profiles/r05_solve_schedule.txt):
// within 15 % of the best hand-tuned schedule in all 18 cases (worst: 32768 problems, every
// problem with the obstacle, 1.144; 65536: 1.033 / 1.081 / 1.062).  Tried and dropped: up to three in-place
// extension chunks of 2 iterations gated on the survivor count of the chunk before (ahead at
// <= 32768 problems on the hard distribution, 13-41 % behind from 131072, where a chunk over
// the whole batch is several rounds of wavefronts); chunks of 2 behind the first.
struct ChunkRound {
  int len;          // iterations of the round's lane chunk (0: none, the tail ends the schedule)
  bool tail;        // a tail kernel is enqueued in front of the chunk
  bool tail_final;  // ... that takes every survivor, however many, and ends the schedule
  bool last;        // nothing is packed behind this round
};
// round[0] is the chunk that runs in place on the caller's arrays; the chunk of round[i] reads the
// live counter i - 1 and its exit fills counter i.
struct ChunkSchedule {
  int rounds = 0;
  ChunkRound round[kMaxRounds] = {};
};
// tail_on: "wave_tail" > 0; spec_tail: the tail is the speculative sixteen-lane kernel
inline ChunkSchedule chunk_schedule(int max_iter, int opt_first_chunk, int opt_chunk_step,
                                    int opt_final_round, bool tail_on, bool spec_tail) {
  const int first = opt_first_chunk > 0 ? opt_first_chunk : kFirstChunk;
  const int step = opt_chunk_step > 0 ? opt_chunk_step : 4;
  // The LAST round (automatic: the one at 24 iterations; "final_round"): its tail kernel takes
  // whatever is left, however many, and runs it to termination — no lane chunk, no further
  // round is enqueued behind it.  Every round after the one whose tail ran used to be three or
  // four empty launches (14-19 us each round; 65536 problems of the bench workload: the rounds at
  // 24, 48 and 96 iterations).  What survives 24 iterations are the long accept / reject chains
  // the speculative kernel is built for, and their iteration counts spread over 25 ... 150: a
  // lane chunk would idle on its slowest lane.
  const int final_round = (!spec_tail || !tail_on) ? 0
      : (opt_final_round >= 0 ? opt_final_round : kFinalRound);
  ChunkSchedule s;
  int done = max_iter < first ? max_iter : first;
  s.round[s.rounds++] = {done, false, false, done >= max_iter};  // (max_iter <= first chunk: nothing survives it)
  for (int round = 0; done < max_iter; round++) {
    // the tail kernel runs from 4 iterations on; a final round reached before that is not the
    // last (its survivors would be left in the work set, unscattered): a later round takes them
    const bool tail = tail_on && done >= 4;
    if (final_round > 0 && round + 1 >= final_round && tail) {
      s.round[s.rounds++] = {0, true, true, true};
      break;
    }
    // chunk lengths after the first: one chunk of 4 (the tail's second chance), then as many
    // iterations as are done (first chunk 10: compaction points at 10, 14, 28, 56 iterations).
    // Once the tail has run, every further round is three empty launches (14 us), so few of
    // them (the schedule 8, 4, 4, 8, 8, 16, 16, 32, 32, ... spent 0.19 of 2.13 ms there at 65536
    // problems; 10, 4, 4, 10, 20, 40, 12: 85 us of 1.55 ms).  Against 4, 4, 4, 4, ... with a tail
    // of 2048: 1.69 -> 1.35 ms at 16384 problems.
    int len = done < 12 ? step : done;
    if (done + len > max_iter || round + 2 >= kMaxRounds) len = max_iter - done;
    done += len;
    s.round[s.rounds++] = {len, tail, false, done >= max_iter};
  }
  return s;
}

}  // namespace i2lqr
