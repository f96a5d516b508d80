// Launcher of the batch-minor / batch-tiled layouts: one problem per lane (i2lqr_lane.hpp).  What a
// call decides from integers — options, workspace layout, the chunked solve's rounds — is
// i2lqr_lane_plan.hpp; this header turns a plan into kernel arguments and launches.  Included by
// i2lqr_abi.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "i2lqr_devcfg.hpp"
#include "i2lqr_group.h"
#include "i2lqr_handle.hpp"
#include "i2lqr_host.hpp"
#include "i2lqr_kernels.h"
#include "i2lqr_lane12.h"
#include "i2lqr_lane_ls.hpp"
#include "i2lqr_lane_merit.hpp"
#include "i2lqr_lane_model.hpp"
#include "i2lqr_lane_plan.hpp"
#include "i2lqr_lane_rows_model.hpp"

// the launches below are recorded by the dry-run build (empty unless -DI2LQR_DRY_RUN: the ASan build)
#define I2LQR_DRY_RUN_LANE 1
#include "i2lqr_dryrun.hpp"

namespace i2lqr {

template <class T, class Sys, bool TILED> struct LaneLaunch {
  static constexpr int n = Sys::n, m = Sys::m, NT = Sys::NTRIG;
  using Cfg = DevCfg<T, n, m>;
  static unsigned grid(int64_t B) { return lane_grid(B); }
  static LaneShape shape(const i2lqr_handle* h) {
    return LaneShape{n, m, h->cfg.N, (int)sizeof(T), Sys::NBLK > 0, has_stage_weights(h->cfg),
                     h->cfg.max_iter};
  }
  // the caller's arrays as a set (K, k, iters, status may be null)
  static LaneSet<T> user_set(const SolveIO& io) {
    return LaneSet<T>{(T*)io.X, (T*)io.U, (T*)io.x_term, (T*)io.obs, (T*)io.lamb, (T*)io.cost,
                      (T*)io.K, (T*)io.k, io.iters, io.status, nullptr, io.B};
  }
  // the entry fields of a launch on the arrays of `w` (the caller's or a work set)
  static void set_io(LaneArgs<T>& a, int n_iters, int early_exit, const LaneSet<T>& w) {
    a.B = w.B; a.n_iters = n_iters; a.early_exit = early_exit;
    a.X = w.X; a.U = w.U; a.x_term = w.x_term; a.lamb = w.lamb; a.obs = w.obs; a.cost = w.cost;
    a.K = w.K; a.k = w.k; a.iters = w.iters; a.status = w.status;
  }
  // The workspace table of B problems on this handle: a model handle with "lane_model_chunks" 1 has
  // work sets with all its records and, with the barrier cost, the penalty row - whatever the batch, so
  // that the size does not jump at the chunked solve's threshold
  static LaneWorkspace workspace(const i2lqr_handle* h, int64_t B) {
    const LaneModel md = lane_model(h->model, h->lane_opt);
    const bool sets = md.on() && h->lane.opt_model_chunks == 1;
    return lane_workspace(shape(h), B, sets ? md.records : 1, sets && md.barrier_cost);
  }
  // (the tiled layout's arrays are whole tiles of 64 problems)
  static int64_t ws_bytes(const i2lqr_handle* h, int64_t B) {
    return workspace(h, TILED ? (B + 63) / 64 * 64 : B).total;
  }
  static int prepare(i2lqr_handle* h) {
    h->lanes = 1;
    return I2LQR_OK;
  }
  // stage weights Q, R != 0: the bicycles in both precisions; the row-block plant (quad12) in fp64
  // (round 5: instantiations of their own, i2lqr_lane12qr.hip)
  static constexpr bool kStageWeights = Sys::NBLK == 0 || sizeof(T) == 8;
  static int need_ws(i2lqr_handle* h, int64_t B) {
    if (!kStageWeights && has_stage_weights(h->cfg))
      return fail(I2LQR_ERR_UNSUPPORTED, "the one-problem-per-lane kernels of this plant are built "
                  "for Q = R = 0 (use the problem-major layout for stage weights)");
    if (TILED && (B & 63))
      return fail(I2LQR_ERR_INVALID, "the batch-tiled layout needs a batch that is a multiple of "
                  "64 (got %lld)", (long long)B);
    const int64_t need = ws_bytes(h, B);
    if (!h->ws || h->ws_bytes < need)
      return fail(I2LQR_ERR_INVALID, "workspace of %lld B registered, batch %lld needs %lld B "
                  "(i2lqr_workspace_bytes / i2lqr_set_workspace)", (long long)h->ws_bytes,
                  (long long)B, (long long)need);
    return I2LQR_OK;
  }
  struct Carved {
    LaneSet<T> set[2];
    int32_t* uiters;
    int32_t* ustatus;
    int32_t* count;  // [kMaxRounds]: the live count after each compaction round
    T* pen[2];       // penalty rows of the work sets (a chunked model solve with the barrier cost), or null
  };
  // The arguments of a launch of B problems with the options `o`, its scratch carved from the
  // registered workspace (need_ws() has passed); cv: the chunked solve's work sets as well
  static LaneArgs<T> lane_args(const i2lqr_handle* h, int64_t B, const LaneOptions& o,
                               Carved* cv = nullptr) {
    const LaneWorkspace w = workspace(h, B);
    char* const base = (char*)h->ws;
    LaneArgs<T> a;
    a.wsU = (T*)(base + w.wsU);
    a.wsK = (T*)(base + w.wsK);
    a.wsk = (T*)(base + w.wsk);
    a.wsX = h->lane.opt_two_x != 0 ? (T*)(base + w.wsX) : nullptr;
    a.count_lo = -1;
    a.count_hi = 0x7fffffff;
    a.count = nullptr;
    a.resume = 0;
    a.max_total = 0x7fffffff;
    a.defer = o.defer; a.reroll = o.reroll; a.merge = o.merge; a.ckpt = o.ckpt;
    a.stagger = o.stagger; a.lds_steps = o.lds_steps; a.lds_grow = o.lds_grow; a.two_max = o.two_max;
    std::memset(&a.cp, 0, sizeof(a.cp));  // plain exit; solve_compacting() fills it per chunk
    a.dbg = nullptr;
#ifdef I2LQR_STAMPS
    if (const char* e = getenv("I2LQR_DBG_PTR")) a.dbg = (unsigned long long*)strtoull(e, nullptr, 0);
#endif
    if (!cv) return a;
    for (int q = 0; q < 2; q++) {
      const LaneWorkspace::Set& at = w.set[q];
      cv->set[q] = LaneSet<T>{(T*)(base + at.X), (T*)(base + at.U), (T*)(base + at.x_term),
                              (T*)(base + at.obs), (T*)(base + at.lamb), (T*)(base + at.cost),
                              a.wsK, a.wsk, (int32_t*)(base + at.iters),
                              (int32_t*)(base + at.status), (int32_t*)(base + at.orig), B};
      cv->pen[q] = at.pen >= 0 ? (T*)(base + at.pen) : nullptr;
    }
    cv->uiters = (int32_t*)(base + w.uiters);
    cv->ustatus = (int32_t*)(base + w.ustatus);
    cv->count = (int32_t*)(base + w.count);
    return a;
  }
  // More than 64 KiB of dynamic LDS per workgroup has to be asked for; the attribute belongs to
  // the kernel ON THE CURRENT DEVICE, so it is set by every launch that needs it (a process may
  // drive several devices) and a refusal falls back to what 64 KiB hold.
  template <class K>
  static void grow_lds(const DeviceGeometry& g, K kernel, const LaneShape& sh, LaneArgs<T>& a,
                       unsigned workgroups, size_t fixed) {
    const int before = a.lds_steps;
    a.lds_steps = grown_lds_steps(g, sh, a, workgroups, fixed, g.max_dyn_lds);
    if (lane_lds(sh, a) + fixed <= g.default_dyn_lds) return;
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)g.max_dyn_lds) == hipSuccess)
      return;
    (void)hipGetLastError();
    a.lds_steps = before;
    a.lds_steps = grown_lds_steps(g, sh, a, workgroups, fixed, g.default_dyn_lds);
  }
  template <bool TL>
  static void launch_pair(const DeviceGeometry& g, const Cfg& c, const LaneShape& sh,
                          const LaneArgs<T>& a, unsigned workgroups, hipStream_t s) {
    if constexpr (Sys::NBLK == 0) {
      LaneArgs<T> ap = a;
      // stage weights: the record carries 2 Q (x_t - xtarget) as well
      with_weights(c.flags, [&](auto W) {
        using LW = LaneWorker<T, Sys, W, TL>;
        const size_t fixed = 2 * LW::kRec * 64 * sizeof(T) + 65 * sizeof(int) + 12;
        grow_lds(g, &k_lane_iterate_pair<T, Sys, W, TL>, sh, ap, workgroups, fixed);
        hipLaunchKernelGGL((k_lane_iterate_pair<T, Sys, W, TL>), dim3(workgroups), dim3(128),
                           lane_lds(sh, ap) + fixed, s, c, ap);
      });
    }
  }
  template <bool TL>
  static void launch_iterate(const DeviceGeometry& g, const Cfg& c, const LaneShape& sh,
                             const LaneArgs<T>& a, int64_t B, hipStream_t s, int opt_pair = 0) {
    if (use_pair(g, sh, a, B, opt_pair)) {
      launch_pair<TL>(g, c, sh, a, grid(B), s);
      return;
    }
    if constexpr (Sys::NBLK > 0) {  // row-block plants: their own fused kernel, no LDS
      with_weights<kStageWeights>(c.flags, [&](auto W) {
        hipLaunchKernelGGL((k_lane_iterate_rows<T, Sys, W, TL>), dim3(grid(B)), dim3(64), 0, s, c, a);
      });
    } else {
      LaneArgs<T> ag = a;
      with_weights(c.flags, [&](auto W) {
        grow_lds(g, &k_lane_iterate<T, Sys, W, TL>, sh, ag, grid(B), 0);
        hipLaunchKernelGGL((k_lane_iterate<T, Sys, W, TL>), dim3(grid(B)), dim3(64),
                           lane_lds(sh, ag), s, c, ag);
      });
    }
  }

  // Chunked solve with compaction (large batches): ilqr() runs 1..max_iter iterations per
  // problem, so a wavefront of 64 problems would otherwise idle on its slowest lane.  The batch
  // is solved in chunks of 8, 4, then doubling (chunk_schedule, i2lqr_lane_plan.hpp); after every
  // chunk the terminated problems are scattered to the caller's arrays and the survivors are
  // packed into a dense work set (k_lane_compact).  No host synchronisation: the live count stays
  // in device memory and surplus wavefronts exit at once.  Results are bit-identical to the plain
  // launch.
  // One routine for the plain kernels and the model kernels ("lane_model_chunks"): `o` are the
  // options of its launches and chunk(TL, a, opt_pair, pen) launches one lane chunk with the
  // arguments a - TL: std::true_type for chunk 0 of a batch-tiled handle (in place, in the caller's
  // layout), std::false_type for the work sets; pen: the penalty rows the chunk reads and its exit
  // fills.  model: lane chunks and the fused exit only - the tail kernels, k_lane_compact and the
  // helper-wavefront form have no models, so "wave_tail", "final_round", "speculate" and
  // "fused_compaction" have no effect.
  template <class Chunk>
  static int solve_compacting(i2lqr_handle* h, const SolveIO& io, hipStream_t s, const LaneOptions& o,
                              const bool model, Chunk&& chunk) {
    const int64_t B = io.B;
    if (int rc = need_ws(h, B)) return rc;
    const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
    const LaneShape sh = shape(h);
    const LaneTune& tune = h->lane;
    const int N = h->cfg.N, max_iter = h->cfg.max_iter;
    Carved cv;
    LaneArgs<T> a0 = lane_args(h, B, o, &cv);
    LaneSet<T> usr = user_set(io);
    if (!io.iters) usr.iters = cv.uiters;
    if (!io.status) usr.status = cv.ustatus;
    if (!io.obs) { cv.set[0].obs = nullptr; cv.set[1].obs = nullptr; }
    // Latency tail: once few problems survive, the rest of the solve is bound by the slowest
    // problem's iteration latency, which is ~2.8x lower with one problem per WAVEFRONT.  If the
    // packed set holds <= wave_tail problems the one-problem-per-wavefront kernel finishes them
    // (it reads the live count itself and is a no-op otherwise); the lane chunks that follow skip
    // finished problems and the next compaction scatters them to the caller.
    // The survivors are the problems with long accept / reject chains (stragglers alternate
    // accept, reject, accept, ...): the speculative sixteen-lane kernel runs the iteration after
    // a reject beside the current one and needs about half the rounds; bit-identical to the
    // plain kernel.  It takes over from 12288 survivors (workgroups of four problems whose slowest
    // member decides; the hardware backfills), the one-problem-per-wavefront kernel (other
    // plants, stage weights) from 2048.
    bool spec_tail = false;
    if constexpr (m == 2 && n + m <= 8)
      spec_tail = !model && h->col.opt_spec != 0 && c.flags == 0 && group_spec_tail_supported(h->cfg);
    const int wave_tail = model ? 0 : tune.wave_tail < 0
        ? (int)h->geo.scaled(spec_tail ? kAutoSpecTail : kAutoWaveTail) : tune.wave_tail;
    const ChunkSchedule plan = chunk_schedule(max_iter, tune.opt_first_chunk, tune.opt_chunk_step,
                                              tune.opt_final_round, wave_tail > 0, spec_tail);
    // one live counter per compaction round, all cleared by ONE fill in front of the first chunk (a
    // fill per round was a 5 us launch of its own in each of the rounds that follow the tail)
    HIP_TRY(hipMemsetAsync(cv.count, 0, kMaxRounds * sizeof(int32_t), s));
    // Round 6: the compaction is folded into the chunk kernels' EXIT (LaneCompact: a wavefront that
    // has finished its chunk packs its survivors into the next work set and scatters what
    // terminated, one atomic add per wavefront, while the other wavefronts still iterate) — the
    // k_lane_compact launch between every two chunks and the final scatter pass are gone
    // ("fused_compaction" 0 brings them back: the A/B and the fallback).
    const bool fused = model || tune.opt_fuse != 0;
    auto plan_exit = [&](LaneArgs<T>& a, bool src_user, const int32_t* orig, LaneSet<T>* dst,
                         int32_t* count_out) {
      std::memset(&a.cp, 0, sizeof(a.cp));
      if (!fused) return;
      a.cp.on = 1;
      a.cp.src_is_user = src_user ? 1 : 0;
      a.cp.user_tiled = TILED ? 1 : 0;
      a.cp.orig = orig;
      if (dst) a.cp.dst = *dst;
      a.cp.count_out = count_out;
      a.cp.usr = usr;
    };
    // chunk 0 runs in place on the caller's arrays
    set_io(a0, plan.round[0].len, 1, usr);
    a0.max_total = max_iter;
    plan_exit(a0, true, nullptr, plan.round[0].last ? nullptr : &cv.set[0], cv.count);
    chunk(std::integral_constant<bool, TILED>{}, a0, tune.opt_pair, LanePen<T>{nullptr, cv.pen[0]});
    const unsigned cgrid = (unsigned)((B + 255) / 256);
    bool src_user = true;
    const int32_t* count_in = nullptr;
    LaneSet<T> src = usr;
    for (int r = 1; r < plan.rounds; r++) {
      const ChunkRound& round = plan.round[r];
      const int cur = (r - 1) & 1;  // index of the work set this round runs on
      int32_t* const count = cv.count + r - 1;
      if (!fused)
        hipLaunchKernelGGL((k_lane_compact<T, TILED>), dim3(cgrid), dim3(256), 0, s, n, m, N, src,
                           src_user ? 1 : 0, count_in, cv.set[cur], count, usr, c.trap);
      const LaneSet<T>& w = cv.set[cur];
      if (round.tail) {
        const size_t lds_f = wave_fstep_lds_bytes<T, Sys>(N);
        IterArgs<T> t = iter_args<T>(SolveIO{B, max_iter, 1, w.X, w.U, w.x_term, w.lamb, w.obs,
                                             w.cost, w.K, w.k, w.iters, w.status});
        t.count = count; t.count_max = round.tail_final ? (int)B : wave_tail; t.max_total = max_iter;
        t.set_stride = B;
        if (spec_tail) {
          // the speculative tail delivers its problems to the caller's arrays itself (the
          // scatter pass of the next compaction was 82 us for 7938 problems with gains)
          t.orig = w.orig;
          t.out_X = usr.X; t.out_U = usr.U; t.out_K = usr.K; t.out_k = usr.k;
          t.out_lamb = usr.lamb; t.out_cost = usr.cost;
          t.out_iters = usr.iters; t.out_status = usr.status;
          t.out_B = usr.B; t.out_tiled = TILED ? 1 : 0;
          if constexpr (m == 2 && n + m <= 8) HIP_TRY(group_spec_tail<T>(h->cfg, t, s));
        } else if (kWaveHasFstep<Sys> && lds_f <= h->geo.default_dyn_lds) {
          if constexpr (kWaveHasFstep<Sys>) {
            with_weights(c.flags, [&](auto W) {
              hipLaunchKernelGGL((k_iterate<T, Sys, 64, W, true, true>), dim3(wave_tail), dim3(64),
                                 lds_f, s, c, t);
            });
          }
        }
      }
      if (round.tail_final) {  // the tail kernel has delivered everything
        src_user = true;  // (nothing left to scatter)
        break;
      }
      LaneArgs<T> a = a0;
      set_io(a, round.len, 1, w);
      a.K = nullptr; a.k = nullptr;  // gains of work sets go to the scratch buffer (w.K == wsK)
      a.count = count; a.resume = 1;
      // the chunk's exit packs its survivors into the OTHER work set (none behind the last chunk)
      plan_exit(a, false, w.orig, round.last ? nullptr : &cv.set[cur ^ 1], cv.count + r);
      // a batch too large for the helper-wavefront form as a whole: its survivors may not be.
      // Both kernels are enqueued and the live count decides on the device which one runs (the
      // other is an empty launch, ~3 us): 21000 survivors of 65536 problems iterate at 46
      // instead of 67 us per iteration.  The pair's chunk takes the options of a launch of its
      // size (no state checkpoints, no merge, no re-rolling forward pass: all bit-identical).
      LaneArgs<T> ap = a;
      ap.ckpt = 0;
      ap.merge = tune.opt_merge >= 0 ? tune.opt_merge : 0;
      ap.reroll = tune.opt_reroll >= 0 ? tune.opt_reroll : 0;
      const unsigned pair_max = pair_max_grid(h->geo);
      const LanePen<T> pen{cv.pen[cur], cv.pen[cur ^ 1]};
      if (!model && pair_built(sh, ap, tune.opt_pair) && tune.opt_pair < 0 && grid(B) > pair_max) {
        ap.count_hi = 64 * (int)pair_max;
        launch_pair<false>(h->geo, c, sh, ap, pair_max, s);
        a.count_lo = ap.count_hi;
        chunk(std::false_type{}, a, 0, pen);
      } else {
        chunk(std::false_type{}, a, tune.opt_pair, pen);
      }
      src = w;
      src_user = false;
      count_in = count;
    }
    // every remaining problem has a terminal status now: scatter them all
    if (!fused && !src_user) {
      LaneSet<T> none;
      std::memset(&none, 0, sizeof(none));
      hipLaunchKernelGGL((k_lane_compact<T, TILED>), dim3(cgrid), dim3(256), 0, s, n, m, N, src, 0,
                         count_in, none, cv.count + plan.rounds - 1, usr, c.trap);
    }
    HIP_TRY(hipGetLastError());
    return I2LQR_OK;
  }

  // One launch of the model kernel of `md` on the arguments a, in the layout TL: k_lane_iterate_model,
  // with the barrier cost k_lane_iterate_merit, with the line search k_lane_iterate_ls (soft or barrier
  // cost) - same plan, same LDS.  CHUNK selects k_lane_chunk_model / _merit / _ls instead: one chunk of
  // the chunked solve, with LaneArgs' count / resume / max_total and the penalty rows `pen` in a
  // LaneChunk argument.
  template <bool TL, bool CHUNK>
  static void launch_model(const i2lqr_handle* h, const Cfg& c, const LaneShape& sh,
                           const LaneModelPlan& p, const LaneModel& md, LaneArgs<T> a, int64_t B,
                           hipStream_t s, const LanePen<T> pen = LanePen<T>{nullptr, nullptr}) {
    if constexpr (Sys::NBLK == 0) {
      const BoxCfg<T, n> box = make_box_cfg<T, n>(h->model.box);
      // one launch expression: the kernel's address and what follows c, a, md.records and box
      const auto launch = [&](auto kernel, auto... tail) {
        grow_lds(h->geo, kernel, sh, a, grid(B), p.model_bytes);
        hipLaunchKernelGGL(kernel, dim3(grid(B)), dim3(64), lane_lds(sh, a) + p.model_bytes, s,
                           c, a, md.records, box, tail...);
      };
      const T box_q1 = (T)h->model.box.q1;
      with_weights(c.flags, [&](auto W) {
        if constexpr (CHUNK) {
          const LaneChunk<T> ck{a.count, a.resume, a.max_total, pen};
          if (md.line_search > 1) {
            // (lane_chunks_built(): the plan chunks no other line search)
            if constexpr (kLaneLsChunkBuilt<T, Sys, W, true>)
              launch(&k_lane_chunk_ls<T, Sys, W, TL, true>, box_q1, md.line_search, ck);
          } else if (md.barrier_cost) {
            launch(&k_lane_chunk_merit<T, Sys, W, TL>, box_q1, ck);
          } else {
            launch(&k_lane_chunk_model<T, Sys, W, TL>, ck);
          }
        } else {
          if (md.line_search > 1 && md.barrier_cost)
            launch(&k_lane_iterate_ls<T, Sys, W, TL, true>, box_q1, md.line_search);
          else if (md.line_search > 1)
            launch(&k_lane_iterate_ls<T, Sys, W, TL, false>, box_q1, md.line_search);
          else if (md.barrier_cost)
            launch(&k_lane_iterate_merit<T, Sys, W, TL>, box_q1);
          else
            launch(&k_lane_iterate_model<T, Sys, W, TL>);
        }
      });
    }
  }
  // The plan of a model call of n_iters iterations, with or without early exit: the ONE place that
  // says what a solve to termination is (early exit and max_iter iterations; the chunked solve is
  // for nothing else, so any other call is planned with the option off)
  static LaneModelPlan model_plan(const i2lqr_handle* h, const LaneModel& md, int64_t B,
                                  int early_exit, int n_iters) {
    LaneTune tune = h->lane;
    if (!(early_exit && n_iters == h->cfg.max_iter)) tune.opt_model_chunks = -1;
    return lane_model_plan(h->geo, shape(h), tune, md, B, early_exit != 0);
  }
  // i2lqr_iterate / i2lqr_solve with a model on: ONE launch whatever the batch (a solve runs with early
  // exit; "helper_wavefront", "checkpoint_states", "state_buffers" have no effect, and neither has
  // i2lqr_set_compaction) - unless "lane_model_chunks" is 1: then a solve to termination of a batch
  // that chunked() takes runs as solve_compacting's lane chunks
  static int iterate_model(i2lqr_handle* h, const SolveIO& io, const LaneModel& md, hipStream_t s) {
    if constexpr (Sys::NBLK > 0) {
      // "lane_rows_models" 1: k_lane_iterate_rows_model, ONE launch ("lane_model_chunks" has no effect)
      if (!h->lane_opt.rows_models) return fail(I2LQR_ERR_UNSUPPORTED, "%s", lane_models_rows_text());
      if (md.barrier_cost || md.line_search > 1)  // (lane_refusal never lets a quad12 handle hold them)
        return fail(I2LQR_ERR_UNSUPPORTED, "%s", lane_models_rows_text());
      if (has_stage_weights(h->cfg))
        return fail(I2LQR_ERR_UNSUPPORTED, "%s", lane_rows_models_weights_text());
      if (int rc = need_ws(h, io.B)) return rc;
      const LaneShape sh = shape(h);
      using LW = LaneWorker<T, Sys, false, TILED>;
      static_assert(LW::kGainWords == lane_rows_gain_words(n, m, NT, Sys::NJX),
                    "lane_rows_model_plan budgets the row-block pass's LDS slice");
      const LaneRowsModelPlan p = lane_rows_model_plan(h->geo, sh, h->lane, md, io.B, LW::kGainWords);
      if (!p.fits)
        return fail(I2LQR_ERR_UNSUPPORTED, "\"lane_rows_models\": k_lane_iterate_rows_model takes %zu B "
                    "of LDS per wavefront, a quarter of this device's compute unit is %zu B",
                    p.lds_bytes, h->geo.lds_per_cu / 4);
      const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
      LaneOptions o = lane_options(h->geo, sh, h->lane, io.B, io.early_exit != 0);
      o.stagger = p.stagger;
      LaneArgs<T> a = lane_args(h, io.B, o);
      set_io(a, io.n_iters, io.early_exit, user_set(io));
      a.max_total = io.n_iters;
      const BoxCfg<T, n> box = make_box_cfg<T, n>(h->model.box);
      hipLaunchKernelGGL((k_lane_iterate_rows_model<T, Sys, false, TILED>), dim3(p.grid), dim3(64), 0,
                         s, c, a, md.records, box);
      HIP_TRY(hipGetLastError());
      return I2LQR_OK;
    } else {
      if (int rc = need_ws(h, io.B)) return rc;
      const LaneShape sh = shape(h);
      const LaneModelPlan p = model_plan(h, md, io.B, io.early_exit, io.n_iters);
      if (!p.fits)
        return fail(I2LQR_ERR_UNSUPPORTED, "\"lane_models\": %d obstacle records take %zu B of LDS per "
                    "wavefront beside the %d B of k_0, a workgroup of this device gets %zu B",
                    md.records, p.model_bytes, sh.k0_bytes(), h->geo.default_dyn_lds);
      const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
      if (p.chunked)
        return solve_compacting(h, io, s, p.o, true, [&](auto tl, const LaneArgs<T>& a, int, LanePen<T> pen) {
          launch_model<decltype(tl)::value, true>(h, c, sh, p, md, a, io.B, s, pen);
        });
      LaneArgs<T> a = lane_args(h, io.B, p.o);
      set_io(a, io.n_iters, io.early_exit, user_set(io));
      a.max_total = io.n_iters;
      launch_model<TILED, false>(h, c, sh, p, md, a, io.B, s);
      HIP_TRY(hipGetLastError());
      return I2LQR_OK;
    }
  }

  static int iterate(i2lqr_handle* h, const SolveIO& io, hipStream_t s) {
    if (const LaneModel md = lane_model(h->model, h->lane_opt); md.on())
      return iterate_model(h, io, md, s);
    const LaneShape sh = shape(h);
    const bool solve = io.early_exit && io.n_iters == h->cfg.max_iter;
    if (solve && chunked(h->geo, sh, h->lane, io.B)) {
      const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
      return solve_compacting(h, io, s, lane_options(h->geo, sh, h->lane, io.B, false), false,
                              [&](auto tl, const LaneArgs<T>& a, int opt_pair, LanePen<T>) {
                                launch_iterate<decltype(tl)::value>(h->geo, c, sh, a, io.B, s, opt_pair);
                              });
    }
    if (int rc = need_ws(h, io.B)) return rc;
    const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
    LaneArgs<T> a = lane_args(h, io.B, lane_options(h->geo, sh, h->lane, io.B, io.early_exit != 0));
    set_io(a, io.n_iters, io.early_exit, user_set(io));
    a.max_total = io.n_iters;
    launch_iterate<TILED>(h->geo, c, sh, a, io.B, s, h->lane.opt_pair);
    HIP_TRY(hipGetLastError());
    return I2LQR_OK;
  }
  static int solve_chained(i2lqr_handle*, const SolveIO&, int, hipStream_t) {
    return fail(I2LQR_ERR_UNSUPPORTED, "chains are problem-major batches (the controller's path)");
  }
  // 1 if the (first) launch of i2lqr_iterate / i2lqr_solve for B problems is the helper-wavefront
  // kernel: the SAME lane_options + use_pair the launchers above run (no workspace, no launch, no
  // device access) — i2lqr_iterate_kernel / i2lqr_solve_kernel (a hand-written mirror of
  // these conditions had drifted).
  static int names_pair(const i2lqr_handle* h, int64_t B, int early_exit) {
    const LaneShape sh = shape(h);
    const LaneOptions o =
        lane_options(h->geo, sh, h->lane, B, early_exit && !chunked(h->geo, sh, h->lane, B));
    return use_pair(h->geo, sh, o, B, h->lane.opt_pair) ? 1 : 0;
  }
  // 1 if i2lqr_solve of B problems on this handle's model (LaneModel::on) runs as the chunked solve:
  // the plan iterate_model() launches from
  static int names_model_chunks(const i2lqr_handle* h, int64_t B, int early_exit) {
    const LaneModel md = lane_model(h->model, h->lane_opt);
    return md.on() && model_plan(h, md, B, early_exit, h->cfg.max_iter).chunked ? 1 : 0;
  }
  static int rollout(i2lqr_handle* h, int64_t B, void* X, void* U, const void* x_term, void* cost,
                     hipStream_t s) {
    if (int rc = need_ws(h, B)) return rc;
    const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
    with_weights<kStageWeights>(c.flags, [&](auto W) {
      hipLaunchKernelGGL((k_lane_rollout<T, Sys, W, TILED>), dim3(grid(B)), dim3(64), 0, s, c, B,
                         (T*)X, (T*)U, (const T*)x_term, (T*)cost);
    });
    HIP_TRY(hipGetLastError());
    return I2LQR_OK;
  }
  static int backward(i2lqr_handle* h, int64_t B, const void* X, const void* U, const void* x_term,
                      const void* lamb, const void* obs, void* K, void* k, hipStream_t s) {
    if (int rc = need_ws(h, B)) return rc;
    const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
    with_weights<kStageWeights>(c.flags, [&](auto W) {
      hipLaunchKernelGGL((k_lane_backward<T, Sys, W, TILED>), dim3(grid(B)), dim3(64), 0, s, c, B,
                         (const T*)X, (const T*)U, (const T*)x_term, (const T*)lamb, (const T*)obs,
                         (T*)K, (T*)k);
    });
    HIP_TRY(hipGetLastError());
    return I2LQR_OK;
  }
  static int forward(i2lqr_handle* h, int64_t B, const void* X, const void* U, const void* x_term,
                     const void* K, const void* k, void* Xn, void* Un, void* cost_new,
                     hipStream_t s) {
    if (int rc = need_ws(h, B)) return rc;
    const Cfg c = make_dev_cfg<T, n, m>(h->cfg);
    with_weights<kStageWeights>(c.flags, [&](auto W) {
      hipLaunchKernelGGL((k_lane_forward<T, Sys, W, TILED>), dim3(grid(B)), dim3(64), 0, s, c, B,
                         (const T*)X, (const T*)U, (const T*)x_term, (const T*)K, (const T*)k,
                         (T*)Xn, (T*)Un, (T*)cost_new);
    });
    HIP_TRY(hipGetLastError());
    return I2LQR_OK;
  }
};

}  // namespace i2lqr
