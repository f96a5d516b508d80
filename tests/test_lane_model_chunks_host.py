"""CPU suite of "lane_model_chunks" (include/i2lqr.h): what i2lqr_lane_plan.hpp decides for the chunked,
compacting solve of a model handle - when the plan is chunked, with which options, on which schedule
and in which workspace.  A stand-alone program under AddressSanitizer and UBSan
(helpers.run_host_program), as in test_lane_models_host.py."""
from pathlib import Path

from helpers import HOST_CHECK_PRELUDE, run_host_program

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ilqr_iterative_tasks_amd" / "csrc"

PROGRAM = '#include "i2lqr_lane_plan.hpp"\n' + HOST_CHECK_PRELUDE + r"""
static LaneShape shape(int n, int m, int N, int word, bool weights = false, int max_iter = 150) {
  return LaneShape{n, m, N, word, false, weights, max_iter};
}
static bool same(const LaneOptions& a, const LaneOptions& b) {
  return a.defer == b.defer && a.reroll == b.reroll && a.merge == b.merge && a.ckpt == b.ckpt &&
         a.stagger == b.stagger && a.lds_grow == b.lds_grow && a.two_max == b.two_max;
}

static void plans() {
  const DeviceGeometry g;  // the MI355X figures
  long combos = 0, chunked_plans = 0;
  for (int word : {8, 4})
    for (int max_iter : {3, 16, 150})
      for (int K : {1, 3})
        for (bool merit : {false, true})
          for (int64_t cmin : {(int64_t)-1, (int64_t)0, (int64_t)64, (int64_t)4096})
            for (int64_t B : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)67, (int64_t)4095,
                              (int64_t)4096, (int64_t)65536})
              for (int option : {-1, 0, 1})
                for (bool solve : {false, true}) {
                  const LaneShape s = shape(6, 2, 20, word, false, max_iter);
                  LaneModel md;
                  md.records = K;
                  md.box = true;
                  md.barrier_cost = merit;
                  LaneTune t;
                  t.compact_min_batch = cmin;
                  t.opt_model_chunks = option;
                  const LaneModelPlan q = lane_model_plan(g, s, t, md, B, solve);
                  combos++;
                  // off is off; on: exactly where the plain solve is chunked, never a fixed count
                  const bool want = option == 1 && solve && chunked(g, s, t, B);
                  CHECK(q.chunked == want);
                  CHECK(!q.pair && q.o.ckpt == 0);
                  // a chunked plan has the options of a launch that is not a single-launch solve
                  LaneTune off = t;
                  off.opt_model_chunks = -1;
                  const LaneModelPlan fixed = lane_model_plan(g, s, off, md, B, false);
                  const LaneModelPlan one = lane_model_plan(g, s, off, md, B, solve);
                  CHECK(same(q.o, want ? fixed.o : one.o));
                  CHECK(q.o.lds_steps == (want ? fixed.o.lds_steps : one.o.lds_steps));
                  CHECK(q.lds == (want ? fixed.lds : one.lds) && q.fits == one.fits);
                  CHECK(q.model_bytes == one.model_bytes);
                  chunked_plans += want;
                }
  CHECK(combos == 2L * 3 * 2 * 2 * 4 * 7 * 3 * 2);
  CHECK(chunked_plans > 0);
  {  // literals: the automatic threshold, and a pinned one
    const LaneShape s = shape(6, 2, 20, 8);
    LaneModel md;
    md.records = 2;
    LaneTune t;
    CHECK(!lane_model_plan(g, s, t, md, 65536, true).chunked);  // default-constructed: off
    t.opt_model_chunks = 1;
    CHECK(lane_model_plan(g, s, t, md, 4096, true).chunked);
    CHECK(!lane_model_plan(g, s, t, md, 4095, true).chunked);
    CHECK(!lane_model_plan(g, s, t, md, 65536, false).chunked);
    LaneModelPlan q = lane_model_plan(g, s, t, md, 65536, true);
    CHECK(q.chunked && q.o.defer == 1 && q.o.reroll == 1 && q.o.merge == 1 && q.o.ckpt == 0 && !q.pair);
    t.compact_min_batch = 64;
    CHECK(lane_model_plan(g, s, t, md, 67, true).chunked && !lane_model_plan(g, s, t, md, 63, true).chunked);
    t.compact_min_batch = 0;
    CHECK(!lane_model_plan(g, s, t, md, 65536, true).chunked);
    // pins of the helper wavefront and the checkpoints do not reach a model's chunks
    t.compact_min_batch = 64;
    t.opt_pair = 1;
    t.opt_ckpt = 1;
    t.opt_merge = 1; t.opt_reroll = 1; t.opt_defer = 1;
    q = lane_model_plan(g, s, t, md, 128, true);
    CHECK(q.chunked && q.o.ckpt == 0 && !q.pair);
  }
}

// which forms have chunk kernels: every model and barrier-cost form; the line search with the barrier
// cost only, and not bicycle6 in fp32 with stage weights - those solves stay ONE launch
static void forms_without_chunk_kernels_stay_a_single_launch() {
  const DeviceGeometry g;
  long combos = 0, refused = 0;
  for (int n : {4, 6})
    for (int word : {8, 4})
      for (bool weights : {false, true})
        for (int A : {0, 2, 4, 8})
          for (bool merit : {false, true})
            for (int K : {1, 3}) {
              const LaneShape s = shape(n, 2, 20, word, weights);
              LaneModel md;
              md.records = K;
              md.box = true;
              md.barrier_cost = merit;
              md.line_search = A;
              LaneTune t;
              t.opt_model_chunks = 1;
              t.compact_min_batch = 64;
              const bool built = A == 0 || (merit && !(word == 4 && n == 6 && weights));
              combos++;
              refused += !built;
              CHECK(lane_chunks_built(word, n, weights, A, merit) == built);
              CHECK(lane_model_plan(g, s, t, md, 128, true).chunked == built);
              CHECK(!lane_model_plan(g, s, t, md, 128, false).chunked);
              // ... with the single launch's options
              LaneTune off = t;
              off.opt_model_chunks = -1;
              if (!built) {
                const LaneModelPlan q = lane_model_plan(g, s, t, md, 128, true);
                const LaneModelPlan one = lane_model_plan(g, s, off, md, 128, true);
                CHECK(same(q.o, one.o) && q.o.lds_steps == one.o.lds_steps && q.lds == one.lds);
              }
            }
  CHECK(combos == 2L * 2 * 2 * 4 * 2 * 2);
  // the soft line search everywhere (2 * 2 * 2 * 3 * 2), fp32 bicycle6 with weights and the barrier cost (3 * 2)
  CHECK(refused == 48 + 6);
}

// the schedule a model solve is built with (tail_on = false): lane chunks only
static void schedule_has_no_tail() {
  for (int max_iter : {5, 9, 17, 150})
    for (int first : {-1, 1, 2, 8})
      for (int step : {-1, 1, 4})
        for (int final_round : {-1, 0, 1, 3})
          for (bool spec : {false, true}) {
            const ChunkSchedule p = chunk_schedule(max_iter, first, step, final_round, false, spec);
            const ChunkSchedule ref = chunk_schedule(max_iter, first, step, -1, false, false);
            CHECK(p.rounds >= 1 && p.rounds <= kMaxRounds && p.rounds == ref.rounds);
            int done = 0;
            for (int r = 0; r < p.rounds; r++) {
              CHECK(!p.round[r].tail && !p.round[r].tail_final);
              CHECK(p.round[r].len >= 1 && p.round[r].len == ref.round[r].len);
              done += p.round[r].len;
              CHECK(p.round[r].last == (r + 1 == p.rounds));
            }
            CHECK(done == max_iter);  // the chunks cover every iteration a problem may take
            CHECK(p.round[0].len == (max_iter < (first > 0 ? first : kFirstChunk)
                                         ? max_iter : (first > 0 ? first : kFirstChunk)));
          }
  // first_chunk 1, chunk_step 1: the most rounds - 1, 1, 1, ... up to 12 iterations, then doubling
  const ChunkSchedule p = chunk_schedule(17, 1, 1, -1, false, false);
  CHECK(p.rounds == 13 && p.round[11].len == 1 && p.round[12].len == 5);
}

struct Block { const char* name; int64_t at, bytes; };

static void workspace() {
  const int64_t B = 192;
  for (int word : {8, 4}) {
    const LaneShape s = shape(6, 2, 20, word);
    const int64_t row = B * word, n = 6, m = 2, N = 20;
    // default arguments: the table as it has always been, block by block
    const LaneWorkspace w = lane_workspace(s, B);
    int64_t p = 0;
    const auto next = [&p](int64_t bytes) { const int64_t at = p; p += bytes; return at; };
    CHECK(w.wsU == next(row * m * N) && w.wsK == next(row * m * n * N) && w.wsk == next(row * m * N));
    CHECK(w.wsX == next(row * n * (N + 1)));
    for (int q = 0; q < 2; q++) {
      CHECK(w.set[q].X == next(row * n * (N + 1)) && w.set[q].U == next(row * m * N));
      CHECK(w.set[q].x_term == next(row * n) && w.set[q].obs == next(row * 6));
      CHECK(w.set[q].lamb == next(row) && w.set[q].cost == next(row));
      CHECK(w.set[q].pen == -1);
    }
    const int64_t pad = (16 - p % 16) % 16;
    p += pad;
    for (int q = 0; q < 2; q++)
      CHECK(w.set[q].iters == next(B * 4) && w.set[q].status == next(B * 4) && w.set[q].orig == next(B * 4));
    CHECK(w.uiters == next(B * 4) && w.ustatus == next(B * 4) && w.count == next(kMaxRounds * 4));
    CHECK(w.total == p + (16 - pad));
    const LaneWorkspace w1 = lane_workspace(s, B, 1, false);
    CHECK(w1.total == w.total && w1.count == w.count && w1.set[1].orig == w.set[1].orig);
    // K records, with and without the penalty row: extents
    for (int K : {1, 2, 3, 8})
      for (bool pen : {false, true}) {
        const LaneWorkspace v = lane_workspace(s, B, K, pen);
        Block blocks[40];
        int nb = 0;
        const auto add = [&](const char* name, int64_t at, int64_t bytes) { blocks[nb++] = {name, at, bytes}; };
        add("wsU", v.wsU, row * m * N); add("wsK", v.wsK, row * m * n * N); add("wsk", v.wsk, row * m * N);
        add("wsX", v.wsX, row * n * (N + 1));
        for (int q = 0; q < 2; q++) {
          const LaneWorkspace::Set& z = v.set[q];
          add("X", z.X, row * n * (N + 1)); add("U", z.U, row * m * N); add("x_term", z.x_term, row * n);
          add("obs", z.obs, row * 6 * K);  // 6 K rows: row q K + r as in the caller's array
          add("lamb", z.lamb, row); add("cost", z.cost, row);
          CHECK((z.pen >= 0) == pen);
          if (pen) add("pen", z.pen, row);
          add("iters", z.iters, B * 4); add("status", z.status, B * 4); add("orig", z.orig, B * 4);
          CHECK(z.iters % 4 == 0 && z.status % 4 == 0 && z.orig % 4 == 0);
          CHECK(z.X % word == 0 && z.obs % word == 0 && z.cost % word == 0 && (!pen || z.pen % word == 0));
        }
        add("uiters", v.uiters, B * 4); add("ustatus", v.ustatus, B * 4);
        add("count", v.count, kMaxRounds * 4);
        int64_t end = 0, sum = 0;
        for (int i = 0; i < nb; i++) {
          CHECK(blocks[i].at >= 0 && blocks[i].bytes > 0);
          if (blocks[i].at + blocks[i].bytes > end) end = blocks[i].at + blocks[i].bytes;
          sum += blocks[i].bytes;
          for (int j = 0; j < i; j++) {
            const bool apart = blocks[i].at + blocks[i].bytes <= blocks[j].at ||
                               blocks[j].at + blocks[j].bytes <= blocks[i].at;
            CHECK(apart);
            if (!apart) std::printf("  %s overlaps %s (K = %d)\n", blocks[i].name, blocks[j].name, K);
          }
        }
        CHECK(v.total >= end);  // total covers the last block
        CHECK(v.total <= sum + 32);  // ... and nothing but the alignment is left over
        CHECK(v.total - w.total == 2 * row * (6 * (K - 1) + (pen ? 1 : 0)));
      }
  }
}

int main() {
  plans();
  forms_without_chunk_kernels_stay_a_single_launch();
  schedule_has_no_tail();
  workspace();
  std::printf("%d failed\n", bad);
  return bad ? 1 : 0;
}
"""


def test_lane_model_chunks_plan(tmp_path):
    run_host_program(tmp_path, "lane_model_chunks_check", PROGRAM, [CSRC])


def test_header_and_docstring_document_the_option():
    hdr = (ROOT / "include" / "i2lqr.h").read_text()
    assert '"lane_model_chunks"' in hdr
    for word in ('"wave_tail"', '"final_round"', '"speculate"', '"fused_compaction"'):
        assert word in hdr[hdr.index('"lane_model_chunks"'):]
    solver = (ROOT / "ilqr_iterative_tasks_amd" / "solver.py").read_text()
    assert '"lane_model_chunks"' in solver
    src = (CSRC / "i2lqr_lane_opt_in.hpp").read_text()
    assert '"k_lane_iterate (state box), chunked"' in src
