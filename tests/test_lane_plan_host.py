"""CPU suite: csrc/i2lqr_lane_plan.hpp, what the launcher of the one-problem-per-lane kernels decides
from integers - the scheduling options of a launch, the layout of the workspace, the rounds of the
chunked solve.  The header is plain C++17: a stand-alone program that includes nothing else of the
library is built with the host compiler under AddressSanitizer and UBSan and run.

Workspace: the total is the size formula the launcher used to carry beside its pointer bumps,
written out here as a literal expression.  That formula sets 16 bytes aside for aligning the int32
arrays; the arrays start on the next multiple of 16 behind the floating-point fields (where they
always did), so the counters are the last kMaxRounds * 4 bytes but for what the alignment left of
those 16 (16 - pad bytes, pad < 16).
Options: literals read from the launcher as it was, on the default (MI355X) geometry.
Schedule: two literal schedules, then every combination of max_iter 1 ... 200 with the values of
"first_chunk", "chunk_step", "final_round" and the three kinds of tail: no more than kMaxRounds
rounds (one counter each), and either the chunks sum to max_iter or a tail kernel that may run
(4 iterations done) takes every survivor."""
from pathlib import Path

from helpers import HOST_CHECK_PRELUDE, run_host_program

CSRC = Path(__file__).resolve().parent.parent / "ilqr_iterative_tasks_amd" / "csrc"

PROGRAM = '#include "i2lqr_lane_plan.hpp"\n' + HOST_CHECK_PRELUDE + r"""
static LaneShape shape(int n, int m, int N, int word, bool weights = false, int max_iter = 150) {
  return LaneShape{n, m, N, word, n == 12, weights, max_iter};
}

static void workspace() {
  const int plants[3][2] = {{4, 2}, {6, 2}, {12, 4}};
  const int horizons[3] = {2, 20, 64};
  const int64_t batches[5] = {1, 64, 200, 4161, 65536};
  for (const auto& p : plants)
    for (int word : {8, 4})
      for (int N : horizons)
        for (int64_t B : batches) {
          const int64_t n = p[0], m = p[1];
          const LaneWorkspace w = lane_workspace(shape(p[0], p[1], N, word), B);
          const int64_t words = B * (m * N + m * n * N + m * N) +
                                2 * (n * (N + 1) + m * N + n + 6 + 2) * B + B * (n * (N + 1));
          CHECK(w.total == words * word + (2 * 3 + 2) * B * 4 + 16 + kMaxRounds * 4);
          // the floating-point fields, back to back from the base, in the launcher's order
          const int64_t rx = B * word * n * (N + 1), ru = B * word * m * N, row = B * word;
          int64_t at = 0;
          const auto next = [&](int64_t field, int64_t bytes) {
            CHECK(field == at);
            at += bytes;
          };
          next(w.wsU, ru);
          next(w.wsK, ru * n);
          next(w.wsk, ru);
          next(w.wsX, rx);
          for (const auto& s : w.set) {
            next(s.X, rx);
            next(s.U, ru);
            next(s.x_term, row * n);
            next(s.obs, row * 6);
            next(s.lamb, row);
            next(s.cost, row);
          }
          CHECK(at == words * word);
          // the int32 arrays: from the next multiple of 16, back to back
          const int64_t pad = w.set[0].iters - at;
          CHECK(pad >= 0 && pad < 16 && w.set[0].iters % 16 == 0);
          at += pad;
          for (const auto& s : w.set) {
            next(s.iters, B * 4);
            next(s.status, B * 4);
            next(s.orig, B * 4);
          }
          next(w.uiters, B * 4);
          next(w.ustatus, B * 4);
          next(w.count, kMaxRounds * 4);
          CHECK(at + (16 - pad) == w.total);
        }
}

static void options() {
  const DeviceGeometry g;  // the MI355X figures
  const LaneTune autom;
  const LaneShape f64 = shape(6, 2, 20, 8), f32 = shape(6, 2, 20, 4);
  {
    const LaneOptions o = lane_options(g, f64, autom, 8192, false);
    CHECK(o.lds_steps == 5 && o.reroll == 0 && o.merge == 0 && o.ckpt == 0 && o.stagger == 0);
    CHECK(o.defer == 1 && o.lds_grow == 1 && o.two_max == 64 * 256);
    CHECK(use_pair(g, f64, o, 8192, autom.opt_pair));
    CHECK(lane_grid(8192) == 128);
    CHECK(grown_lds_steps(g, f64, o, 128, 0, g.max_dyn_lds) == 19);
    CHECK(grown_lds_steps(g, f64, o, 128, 8192, g.max_dyn_lds) == 19);
    CHECK(grown_lds_steps(g, f64, o, 512, 0, g.max_dyn_lds) == 11);   // two workgroups per CU
    CHECK(grown_lds_steps(g, f64, o, 1024, 0, g.max_dyn_lds) == 5);   // four: nothing to grow into
    CHECK(lane_lds(f64, o) == 5u * 7168u + 1024u);
  }
  {
    const LaneOptions o = lane_options(g, f64, autom, 65536, false);
    CHECK(o.reroll == 1 && o.merge == 1 && o.ckpt == 1 && o.lds_steps == 3 && o.stagger == 8);
    CHECK(!use_pair(g, f64, o, 65536, autom.opt_pair));
    CHECK(grown_lds_steps(g, f64, o, 128, 0, g.max_dyn_lds) == 3);  // checkpoints: no growth
    CHECK(lane_lds(f64, o) == 3u * 7168u + 1024u + 15360u);
  }
  CHECK(lane_options(g, f32, autom, 8192, false).lds_steps == 10);
  CHECK(lane_options(g, f32, autom, 65536, false).merge == 0);    // fp32: no merge, so no checkpoints
  CHECK(lane_options(g, f32, autom, 65536, false).ckpt == 0);
  CHECK(lane_options(g, f32, autom, 65536, false).stagger == 0);
  CHECK(lane_options(g, f64, autom, 32768, false).reroll == 1);   // from half a full batch
  CHECK(lane_options(g, f64, autom, 32768, false).merge == 0);    // above it
  CHECK(lane_options(g, f64, autom, 32769, false).merge == 1);
  CHECK(lane_options(g, f64, autom, 61440, false).stagger == 0);  // 15/16 ... 5/4 of a full batch
  CHECK(lane_options(g, f64, autom, 61441, false).stagger == 8);
  CHECK(lane_options(g, f64, autom, 81920, false).stagger == 8);
  CHECK(lane_options(g, f64, autom, 81921, false).stagger == 0);
  CHECK(lane_options(g, shape(6, 2, 20, 8, true), autom, 65536, false).ckpt == 0);  // stage weights
  CHECK(lane_options(g, shape(6, 2, 3, 8), autom, 8192, false).lds_steps == 2);     // at most N - 1
  {  // the row-block plant: its own stagger, never the helper-wavefront form
    const LaneShape q = shape(12, 4, 20, 8);
    CHECK(lane_options(g, q, autom, 65535, false).stagger == 0);
    const LaneOptions o = lane_options(g, q, autom, 65536, false);
    CHECK(o.stagger == 45);
    CHECK(!use_pair(g, q, lane_options(g, q, autom, 64, false), 64, 1));
  }
  {  // the single-launch solve: no re-roll, no deferred states unless pinned, so no checkpoints
    const LaneOptions o = lane_options(g, f64, autom, 65536, true);
    CHECK(o.reroll == 0 && o.defer == 0 && o.ckpt == 0 && o.merge == 1);
    CHECK(o.lds_steps == 3);  // (given up for the checkpoints of the fixed-count options: kept as it was)
    LaneTune t;
    t.opt_reroll = 1;
    CHECK(lane_options(g, f64, t, 65536, true).reroll == 1);
    CHECK(lane_options(g, f64, t, 65536, true).defer == 0 && lane_options(g, f64, t, 65536, true).ckpt == 0);
    t.opt_defer = 1;
    const LaneOptions p = lane_options(g, f64, t, 65536, true);
    CHECK(p.reroll == 1 && p.defer == 1 && p.ckpt == 1 && p.lds_steps == 3);
    CHECK(lane_options(g, f64, autom, 8192, true).defer == 0);
    CHECK(use_pair(g, f64, lane_options(g, f64, autom, 8192, true), 8192, -1));
  }
  {  // each pinned option overrides its automatic value
    LaneTune t;
    t.opt_defer = 0;
    CHECK(lane_options(g, f64, t, 65536, false).defer == 0 && lane_options(g, f64, t, 65536, false).ckpt == 0);
    t = LaneTune();
    t.opt_reroll = 1;
    CHECK(lane_options(g, f64, t, 8192, false).reroll == 1);
    t.opt_reroll = 0;
    CHECK(lane_options(g, f64, t, 65536, false).reroll == 0 && lane_options(g, f64, t, 65536, false).ckpt == 0);
    t = LaneTune();
    t.opt_merge = 1;
    CHECK(lane_options(g, f64, t, 8192, false).merge == 1 && lane_options(g, f32, t, 8192, false).merge == 1);
    t.opt_merge = 0;
    CHECK(lane_options(g, f64, t, 65536, false).merge == 0 && lane_options(g, f64, t, 65536, false).ckpt == 0);
    t = LaneTune();
    t.opt_ckpt = 0;
    CHECK(lane_options(g, f64, t, 65536, false).ckpt == 0 && lane_options(g, f64, t, 65536, false).lds_steps == 5);
    t.opt_ckpt = 1;
    CHECK(lane_options(g, f64, t, 8192, false).ckpt == 0);  // (needs merge and re-roll)
    t.opt_merge = 1;
    t.opt_reroll = 1;
    CHECK(lane_options(g, f64, t, 8192, false).ckpt == 1 && lane_options(g, f64, t, 8192, false).lds_steps == 3);
    CHECK(lane_options(g, f32, t, 8192, false).ckpt == 0);  // fp64 only
    CHECK(!use_pair(g, f64, lane_options(g, f64, t, 8192, false), 8192, -1));  // checkpoints: no pair
    t = LaneTune();
    t.opt_stagger = 45;
    CHECK(lane_options(g, f64, t, 64, false).stagger == 45);
    t.opt_stagger = 5000;
    CHECK(lane_options(g, f64, t, 64, false).stagger == 999);
    t.opt_stagger = 0;
    CHECK(lane_options(g, f64, t, 65536, false).stagger == 0);
    t = LaneTune();
    t.opt_lds_steps = 2;
    CHECK(lane_options(g, f64, t, 8192, false).lds_steps == 2 && lane_options(g, f64, t, 8192, false).lds_grow == 0);
    CHECK(grown_lds_steps(g, f64, lane_options(g, f64, t, 8192, false), 128, 0, g.max_dyn_lds) == 2);
    t.opt_lds_steps = 40;  // (only ever lowers)
    CHECK(lane_options(g, f64, t, 8192, false).lds_steps == 5 && lane_options(g, f64, t, 8192, false).lds_grow == 0);
    t = LaneTune();
    t.opt_two_x = 1;
    CHECK(lane_options(g, f64, t, 8192, false).two_max == 64 * 512);
    t = LaneTune();
    const LaneOptions o = lane_options(g, f64, t, 8192, false);
    CHECK(!use_pair(g, f64, o, 8192, 0));
    CHECK(use_pair(g, f64, o, 32768, -1) && !use_pair(g, f64, o, 32769, -1));  // 512 workgroups
    CHECK(use_pair(g, f64, o, 32769, 1));
  }
  {  // when i2lqr_solve is chunked
    CHECK(chunked(g, f64, autom, 4096) && !chunked(g, f64, autom, 4095));
    CHECK(!chunked(g, shape(6, 2, 20, 8, false, 16), autom, 65536));
    CHECK(chunked(g, shape(6, 2, 20, 8, false, 17), autom, 65536));
    LaneTune t;
    t.compact_min_batch = 64;
    CHECK(chunked(g, f64, t, 64) && !chunked(g, f64, t, 63));
    CHECK(chunked(g, shape(6, 2, 20, 8, false, 5), t, 64) && !chunked(g, shape(6, 2, 20, 8, false, 4), t, 64));
    t.compact_min_batch = 0;
    CHECK(!chunked(g, f64, t, 1 << 20));
  }
}

static void expect(const ChunkSchedule& s, int rounds, const int* len, const int* tail, bool final_tail) {
  CHECK(s.rounds == rounds);
  for (int i = 0; i < rounds && i < s.rounds; i++) {
    const bool end = i == rounds - 1;
    CHECK(s.round[i].len == len[i]);
    CHECK(s.round[i].tail == (tail[i] != 0));
    CHECK(s.round[i].tail_final == (end && final_tail));
    CHECK(s.round[i].last == end);
  }
}

static void schedule() {
  {  // speculative tail, 150 iterations: chunks 8, 4, 12, a tail in front of the second and the
     // third, then the tail that takes everything
    const int len[] = {8, 4, 12, 0}, tail[] = {0, 1, 1, 1};
    expect(chunk_schedule(150, -1, -1, -1, true, true), 4, len, tail, true);
  }
  {
    const int len[] = {8, 4, 12, 24, 48, 54}, tail[] = {0, 1, 1, 1, 1, 1};
    expect(chunk_schedule(150, -1, -1, 0, true, true), 6, len, tail, false);
    expect(chunk_schedule(150, -1, -1, -1, true, false), 6, len, tail, false);  // no final round without the speculative tail
    const int none[] = {0, 0, 0, 0, 0, 0};
    expect(chunk_schedule(150, -1, -1, -1, false, true), 6, len, none, false);
  }
  {  // a final round reached before the tail may run is not the last (the skipped tail)
    const int len[] = {2, 4, 0}, tail[] = {0, 0, 1};
    expect(chunk_schedule(150, 2, -1, 1, true, true), 3, len, tail, true);
  }
  {  // nothing survives a first chunk of max_iter
    const int len[] = {5}, tail[] = {0};
    expect(chunk_schedule(5, -1, -1, -1, true, true), 1, len, tail, false);
  }
  {  // the cap: the chunk that fills the last counter runs whatever is left (doubling from 12, only
     // an iteration limit beyond 12 * 2^11 gets there)
    const ChunkSchedule s = chunk_schedule(1 << 20, 1, 1, 0, true, false);
    CHECK(s.rounds == kMaxRounds && s.round[kMaxRounds - 1].last && !s.round[kMaxRounds - 2].last);
    long done = 0;
    for (int i = 0; i < s.rounds; i++) done += s.round[i].len;
    CHECK(done == 1 << 20);
  }
  const int firsts[] = {-1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 150};
  const int steps[] = {-1, 1, 2, 4, 9};
  const int finals[] = {-1, 0, 1, 2, 3, 4, 5};
  long combos = 0;
  for (int max_iter = 1; max_iter <= 200; max_iter++)
    for (int first : firsts)
      for (int step : steps)
        for (int fin : finals)
          for (int mode = 0; mode < 3; mode++) {  // tail off / on / speculative
            const bool tail_on = mode > 0, spec = mode == 2;
            const ChunkSchedule s = chunk_schedule(max_iter, first, step, fin, tail_on, spec);
            combos++;
            // one counter per round: round i reads counter i - 1 and fills counter i
            CHECK(s.rounds >= 1 && s.rounds <= kMaxRounds);
            const int f = first > 0 ? first : 8;
            CHECK(s.round[0].len == (max_iter < f ? max_iter : f) && !s.round[0].tail);
            int done = 0;
            bool ended = false;
            for (int i = 0; i < s.rounds && i < kMaxRounds; i++) {
              const ChunkRound& r = s.round[i];
              CHECK(!ended);  // nothing behind the round that ends the schedule
              if (i > 0) CHECK(r.tail == (tail_on && done >= 4));
              if (r.tail_final) {
                // a tail that takes every survivor: only the speculative one, once it may run
                CHECK(r.tail && spec && done >= 4 && r.len == 0 && r.last);
                ended = true;
                continue;
              }
              CHECK(r.len > 0);
              done += r.len;
              CHECK(r.last == (done >= max_iter));
              ended = r.last;
            }
            CHECK(ended);
            CHECK(s.round[s.rounds - 1].tail_final || done == max_iter);
            CHECK(done <= max_iter);
          }
  CHECK(combos == 200L * 14 * 5 * 7 * 3);
}

int main() {
  workspace();
  options();
  schedule();
  std::printf("%d failed\n", bad);
  return bad ? 1 : 0;
}
"""


def test_lane_plan_rules_against_literals(tmp_path):
    run_host_program(tmp_path, "lane_plan_check", PROGRAM, [CSRC])
