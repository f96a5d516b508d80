"""CPU suite of "lane_models" (include/i2lqr.h): the plan of a model launch (i2lqr_lane_plan.hpp: a
stand-alone program under AddressSanitizer and UBSan, helpers.run_host_program), the forms, names and
refusals of the lane options (i2lqr_lane_opt_in.hpp, a second such program), the header's text, and
the conditioning of the two 128-problem sets test_gpu_lane_models.py adds to the sets
test_obstacles_host.py / test_state_box_host.py already pin."""
import functools
from pathlib import Path

import numpy as np
import pytest

from helpers import HOST_CHECK_PRELUDE, run_host_program
from opt_in_cases import RECORDS, TILED, TILED_RUNS, make_case
from opt_in_reference import first_record_only, reference

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ilqr_iterative_tasks_amd" / "csrc"

PROGRAM = '#include "i2lqr_lane_plan.hpp"\n' + HOST_CHECK_PRELUDE + r"""
static LaneShape shape(int n, int m, int N, int word, bool weights = false, int max_iter = 150) {
  return LaneShape{n, m, N, word, false, weights, max_iter};
}

static void model_launches() {
  const DeviceGeometry g;  // the MI355X figures
  const int plants[2][2] = {{4, 2}, {6, 2}};
  long combos = 0;
  for (const auto& p : plants)
    for (int word : {8, 4})
      for (int N : {1, 20, 64})
        for (int K : {1, 2, 8})
          for (bool box : {false, true})
            for (int64_t B : {(int64_t)1, (int64_t)64, (int64_t)4161, (int64_t)65536})
              for (bool solve : {false, true})
                for (int pin : {-1, 0, 1}) {  // "helper_wavefront" / "checkpoint_states" pinned or not
                  const LaneShape s = shape(p[0], p[1], N, word);
                  LaneModel md;
                  md.records = K;
                  md.box = box;
                  CHECK(md.on() == (K > 1 || box));
                  LaneTune t;
                  t.opt_pair = pin;
                  t.opt_ckpt = pin;
                  if (pin == 1) { t.opt_merge = 1; t.opt_reroll = 1; t.opt_defer = 1; }
                  t.compact_min_batch = 64;  // i2lqr_set_compaction(64): ignored by a model launch
                  const LaneModelPlan q = lane_model_plan(g, s, t, md, B, solve);
                  combos++;
                  CHECK(!q.pair && !q.chunked && q.o.ckpt == 0);
                  // the records: 6 words of 64 lanes each but the first, which stays in registers
                  CHECK(q.model_bytes == (size_t)64 * 6 * (size_t)(K - 1) * (size_t)word);
                  CHECK(q.model_bytes == lane_model_bytes(s, md));
                  // LDS: gain steps + k_0 + records, within the budget of one wavefront per SIMD
                  CHECK(q.lds == (size_t)q.o.lds_steps * (size_t)s.step_bytes() + (size_t)s.k0_bytes() +
                                     q.model_bytes);
                  CHECK(q.lds == lane_lds(s, q.o) + q.model_bytes);
                  CHECK(q.lds <= g.lds_per_simd_wave());
                  CHECK(q.fits);
                  CHECK(q.o.lds_steps >= 0 && q.o.lds_steps <= (N > 1 ? N - 1 : 0));
                  // ... and as many gain steps as that budget holds, unless the plain launch keeps fewer
                  LaneTune plain_t = t;
                  plain_t.opt_ckpt = 0;
                  const LaneOptions plain = lane_options(g, s, plain_t, B, solve);
                  const long room = (long)g.lds_per_simd_wave() - s.k0_bytes() - (long)q.model_bytes;
                  const int most = (int)(room / s.step_bytes());
                  CHECK(q.o.lds_steps == (plain.lds_steps < most ? plain.lds_steps : most));
                  // the scheduling options that apply are the plain launch's
                  CHECK(q.o.defer == plain.defer && q.o.reroll == plain.reroll &&
                        q.o.merge == plain.merge && q.o.stagger == plain.stagger &&
                        q.o.lds_grow == plain.lds_grow);
                  // growth through `fixed`: the records and k_0 stay inside what the launch asks for
                  for (unsigned wg : {1u, 256u, 512u, 1024u}) {
                    const int steps = grown_lds_steps(g, s, q.o, wg, q.model_bytes, g.max_dyn_lds);
                    LaneOptions grown = q.o;
                    grown.lds_steps = steps;
                    CHECK(steps >= q.o.lds_steps && steps <= (N > 1 ? N - 1 : 0));
                    if (steps > q.o.lds_steps)
                      CHECK(lane_lds(s, grown) + q.model_bytes + 1024 <= g.max_dyn_lds);
                  }
                }
  CHECK(combos == 2L * 2 * 3 * 3 * 2 * 4 * 2 * 3);
  {  // literals: fp64, n = 6, m = 2, N = 20
    const LaneShape f64 = shape(6, 2, 20, 8), f32 = shape(6, 2, 20, 4);
    const LaneTune autom;
    LaneModel md;
    md.records = 8;
    LaneModelPlan q = lane_model_plan(g, f64, autom, md, 65536, false);
    CHECK(q.model_bytes == 21504 && q.o.lds_steps == 2 && q.lds == 2u * 7168u + 1024u + 21504u);
    CHECK(q.o.reroll == 1 && q.o.merge == 1 && q.o.defer == 1 && q.o.stagger == 8);
    md.records = 2;
    q = lane_model_plan(g, f64, autom, md, 65536, false);
    CHECK(q.model_bytes == 3072 && q.o.lds_steps == 4);
    q = lane_model_plan(g, f64, autom, md, 65536, true);  // a solve: one launch, no re-roll / defer
    CHECK(q.o.reroll == 0 && q.o.defer == 0 && q.o.lds_steps == 4 && !q.chunked);
    q = lane_model_plan(g, f32, autom, md, 8192, false);
    CHECK(q.model_bytes == 1536 && q.o.lds_steps == 9 && !q.pair);
    md.records = 1;
    md.box = true;  // the box alone takes no LDS
    q = lane_model_plan(g, f64, autom, md, 8192, false);
    CHECK(q.model_bytes == 0 && q.o.lds_steps == 5 && q.lds == 5u * 7168u + 1024u && !q.pair);
    // a device whose workgroups get too little LDS: the plan says so
    DeviceGeometry small;
    small.default_dyn_lds = 16 * 1024;
    md.records = 8;
    CHECK(!lane_model_plan(small, f64, autom, md, 64, false).fits);
    CHECK(lane_model_plan(small, f32, autom, md, 64, false).fits);
  }
}

// with no model on the plan is the parent commit's: literals read from it for two shapes
static void plain_launches_are_unchanged() {
  const DeviceGeometry g;
  const LaneTune autom;
  {
    const LaneShape s = shape(6, 2, 20, 8);
    const LaneOptions o = lane_options(g, s, autom, 8192, false);
    CHECK(o.lds_steps == 5 && o.reroll == 0 && o.merge == 0 && o.ckpt == 0 && o.stagger == 0);
    CHECK(o.defer == 1 && o.lds_grow == 1 && o.two_max == 64 * 256);
    CHECK(lane_lds(s, o) == 5u * 7168u + 1024u);
    CHECK(use_pair(g, s, o, 8192, autom.opt_pair));
    const LaneOptions f = lane_options(g, s, autom, 65536, false);
    CHECK(f.reroll == 1 && f.merge == 1 && f.ckpt == 1 && f.lds_steps == 3 && f.stagger == 8);
    CHECK(lane_lds(s, f) == 3u * 7168u + 1024u + 15360u);
    CHECK(chunked(g, s, autom, 4096) && !chunked(g, s, autom, 4095));
  }
  {
    const LaneShape s = shape(4, 2, 6, 4);
    const LaneOptions o = lane_options(g, s, autom, 4161, false);
    CHECK(o.lds_steps == 5 && o.reroll == 0 && o.merge == 0 && o.ckpt == 0 && o.stagger == 0);
    CHECK(o.defer == 1 && o.lds_grow == 1);
    CHECK(s.step_bytes() == 2560 && s.k0_bytes() == 512 && lane_lds(s, o) == 5u * 2560u + 512u);
    const LaneOptions so = lane_options(g, s, autom, 4161, true);
    CHECK(so.defer == 0 && so.reroll == 0 && so.lds_steps == 5);
    CHECK(use_pair(g, s, o, 4161, -1) && !use_pair(g, s, o, 4161, 0));
    // X, U, x_term, obs (six words: the chunked solve has no models), lamb, cost per work set
    const LaneWorkspace w = lane_workspace(s, 64);
    CHECK(w.set[0].lamb - w.set[0].obs == 64 * 4 * 6);
  }
}

int main() {
  model_launches();
  plain_launches_are_unchanged();
  std::printf("%d failed\n", bad);
  return bad ? 1 : 0;
}
"""


def test_lane_model_plan(tmp_path):
    run_host_program(tmp_path, "lane_model_plan_check", PROGRAM, [CSRC])


# The form a handle's options select, its display name and every request the lane forms refuse
# (i2lqr_lane_opt_in.hpp).  The codes and messages are literals copied from i2lqr_set_option,
# i2lqr_set_state_box and refuse_lane_model of csrc/i2lqr_abi.hip as it stood before the rules moved
# (commit a0281da, "Opt-in line search on the one-problem-per-lane kernel"), not from the header.
RULES_PROGRAM = '#include "i2lqr_lane_opt_in.hpp"\n' + HOST_CHECK_PRELUDE + r"""
static WaveModel held(int obs, bool box) {
  WaveModel m;
  m.obs = obs;
  if (box) {
    m.box.hi[2] = 10.0;
    m.box.m_hi = 4u;
  }
  return m;
}

static void forms_and_names() {
  long combos = 0;
  for (int K : {1, 3})
    for (bool box : {false, true})
      for (bool merit : {false, true})
        for (int A : {0, 2, 8}) {
          LaneOptIn opt;
          opt.models = true;
          opt.barrier_cost = merit;
          opt.line_search = A;
          const LaneModel md = lane_model(held(K > 1 ? K : 0, box), opt);
          combos++;
          CHECK(md.records == K && md.box == box && md.barrier_cost == merit && md.line_search == A);
          CHECK(md.on() == (K > 1 || box || merit || A > 1));
          // barrier cost > box > several records > line search alone
          const char* name = "k_lane_iterate";
          LaneForm form = LANE_PLAIN;
          if (A > 1) { form = LANE_LS; name = "k_lane_iterate (line search)"; }
          if (K > 1) { form = LANE_OBS; name = "k_lane_iterate (several obstacles)"; }
          if (box) { form = LANE_BOX; name = "k_lane_iterate (state box)"; }
          if (merit) { form = LANE_MERIT; name = "k_lane_iterate (barrier cost)"; }
          CHECK(md.form() == form);
          CHECK((md.form() == LANE_PLAIN) == !md.on());
          CHECK(!std::strcmp(lane_kernel_name(md.form()), name));
        }
  CHECK(combos == 2L * 2 * 2 * 3);
  CHECK(LANE_PLAIN < LANE_LS && LANE_LS < LANE_OBS && LANE_OBS < LANE_BOX && LANE_BOX < LANE_MERIT);
  // "obstacles" 0 / 1 are one record; a line search of 1 is none
  CHECK(lane_model(held(1, false), LaneOptIn()).form() == LANE_PLAIN);
  CHECK((LaneModel{1, false, false, 1}.form()) == LANE_PLAIN);
}

enum Site { MAJOR, LANE, LANE_MODELS, QUAD_MODELS };  // layout, "lane_models", plant

static LaneRefusal ask(LaneAsk what, int v, Site site, int obs = 0, bool box = false,
                       bool merit = false, int A = 0) {
  LaneOptIn opt;
  opt.models = site == LANE_MODELS || site == QUAD_MODELS;
  opt.barrier_cost = merit;
  opt.line_search = A;
  return lane_refusal(what, v, site == MAJOR, site == QUAD_MODELS, held(obs, box), opt);
}
#define REFUSED(r, want_code, want_text)                                          \
  do {                                                                            \
    const LaneRefusal got = (r);                                                  \
    CHECK(got.code == (want_code));                                               \
    CHECK(!std::strcmp(got.text, (want_text)));                                   \
    if (std::strcmp(got.text, (want_text))) std::printf("  got: %s\n", got.text); \
  } while (0)
#define ACCEPTED(r)                                   \
  do {                                                \
    const LaneRefusal got = (r);                      \
    CHECK(got.code == 0 && got.text[0] == '\0');      \
  } while (0)

static void refusals() {
  const int INVALID = -1, UNSUPPORTED = -2;
  CHECK(I2LQR_ERR_INVALID == INVALID && I2LQR_ERR_UNSUPPORTED == UNSUPPORTED && I2LQR_OK == 0);
  // a problem-major handle
  REFUSED(ask(LANE_ASK_MODELS, 1, MAJOR), UNSUPPORTED,
          "\"lane_models\" is built for the batch-minor / batch-tiled layouts (a problem-major "
          "handle runs the models on the one-problem-per-wavefront kernels without it)");
  REFUSED(ask(LANE_ASK_BARRIER_COST, 1, MAJOR), UNSUPPORTED,
          "\"lane_barrier_cost\" is built for the batch-minor / batch-tiled layouts: a "
          "problem-major handle takes \"barrier_cost\" (the one-problem-per-wavefront kernel)");
  for (int A : {2, 4, 8})
    REFUSED(ask(LANE_ASK_LINE_SEARCH, A, MAJOR), UNSUPPORTED,
            "\"lane_line_search\" is built for the batch-minor / batch-tiled layouts: a "
            "problem-major handle takes \"line_search\" (the one-problem-per-wavefront kernel)");
  // ... takes records, a box and "barrier_cost" on its own kernels
  ACCEPTED(ask(LANE_ASK_OBSTACLES, 8, MAJOR));
  ACCEPTED(ask(LANE_ASK_BOX, 1, MAJOR));
  ACCEPTED(ask(WAVE_ASK_BARRIER_COST, 1, MAJOR));
  ACCEPTED(ask(LANE_ASK_MODELS, 0, MAJOR, 3, true));  // (its records and box are not "lane_models"')
  // a lane handle without "lane_models"
  REFUSED(ask(LANE_ASK_BARRIER_COST, 1, LANE), UNSUPPORTED,
          "\"lane_barrier_cost\" runs on the kernel of \"lane_models\": set \"lane_models\" to 1 "
          "first");
  for (int A : {2, 4, 8})
    REFUSED(ask(LANE_ASK_LINE_SEARCH, A, LANE), UNSUPPORTED,
            "\"lane_line_search\" runs on the kernel of \"lane_models\": set \"lane_models\" to 1 "
            "first");
  for (int K : {2, 8})
    REFUSED(ask(LANE_ASK_OBSTACLES, K, LANE), UNSUPPORTED,
            "\"obstacles\" is built for the problem-major layout (the one-problem-per-wavefront "
            "kernel)");
  REFUSED(ask(LANE_ASK_BOX, 1, LANE), UNSUPPORTED,
          "a state box is built for the problem-major layout (the one-problem-per-wavefront "
          "kernel)");
  // "barrier_cost" on a lane handle, with or without "lane_models", bicycles or quad12
  for (Site site : {LANE, LANE_MODELS, QUAD_MODELS})
    REFUSED(ask(WAVE_ASK_BARRIER_COST, 1, site), UNSUPPORTED,
            "\"barrier_cost\" is built for the problem-major layout (the one-problem-per-wavefront "
            "kernel); a batch-minor / batch-tiled handle of the bicycles has \"lane_barrier_cost\" "
            "(with \"lane_models\" 1)");
  // quad12 with "lane_models" 1 (the switch itself is accepted)
  ACCEPTED(ask(LANE_ASK_MODELS, 1, QUAD_MODELS));
  REFUSED(ask(LANE_ASK_BARRIER_COST, 1, QUAD_MODELS), UNSUPPORTED,
          "\"lane_barrier_cost\" with \"lane_models\" is built for the bicycles' "
          "one-problem-per-lane kernel, not for quad12's row-block kernel (k_lane_iterate_rows): "
          "use the problem-major layout");
  REFUSED(ask(LANE_ASK_LINE_SEARCH, 4, QUAD_MODELS), UNSUPPORTED,
          "\"lane_line_search\" with \"lane_models\" is built for the bicycles' "
          "one-problem-per-lane kernel, not for quad12's row-block kernel (k_lane_iterate_rows): "
          "use the problem-major layout");
  REFUSED(ask(LANE_ASK_OBSTACLES, 2, QUAD_MODELS), UNSUPPORTED,
          "\"obstacles\" with \"lane_models\" is built for the bicycles' one-problem-per-lane "
          "kernel, not for quad12's row-block kernel (k_lane_iterate_rows): use the problem-major "
          "layout");
  REFUSED(ask(LANE_ASK_BOX, 1, QUAD_MODELS), UNSUPPORTED,
          "a state box with \"lane_models\" is built for the bicycles' one-problem-per-lane kernel, "
          "not for quad12's row-block kernel (k_lane_iterate_rows): use the problem-major layout");
  // ... and what a launch on such a plant says
  CHECK(!std::strcmp(lane_models_rows_text(),
                     "\"lane_models\" is built for the bicycles' one-problem-per-lane kernel, not "
                     "for the row-block kernel of this plant (k_lane_iterate_rows): use the "
                     "problem-major layout"));
  // values, on every kind of handle and before anything else is looked at
  for (Site site : {MAJOR, LANE, LANE_MODELS, QUAD_MODELS}) {
    for (int v : {2, 7}) {
      REFUSED(ask(LANE_ASK_MODELS, v, site), INVALID, "\"lane_models\" is 1 (on), or -1 / 0 (off)");
      REFUSED(ask(LANE_ASK_BARRIER_COST, v, site), INVALID,
              "\"lane_barrier_cost\" is 1 (on), or -1 / 0 (off)");
    }
    for (int v : {3, 5, 6, 7, 9, 16})
      REFUSED(ask(LANE_ASK_LINE_SEARCH, v, site), INVALID,
              "\"lane_line_search\" is 2, 4 or 8 step sizes, or -1 / 0 / 1 (off)");
  }
  // "lane_models" 0 / -1 while something runs on its kernel: barrier cost, then line search, then
  // box, then records
  const char* const merit_held = "\"lane_models\" cannot be switched off while "
                                 "\"lane_barrier_cost\" is on: set \"lane_barrier_cost\" to 0 first";
  const char* const ls_held = "\"lane_models\" cannot be switched off while \"lane_line_search\" "
                              "is on: set \"lane_line_search\" to 0 first";
  const char* const box_held = "\"lane_models\" cannot be switched off while a state box is on: "
                               "clear it (i2lqr_set_state_box with NULL bounds) first";
  const char* const obs_held = "\"lane_models\" cannot be switched off while \"obstacles\" is on: "
                               "set \"obstacles\" to 1 first";
  for (int off : {0, -1}) {
    REFUSED(ask(LANE_ASK_MODELS, off, LANE_MODELS, 0, false, true), INVALID, merit_held);
    REFUSED(ask(LANE_ASK_MODELS, off, LANE_MODELS, 0, false, false, 2), INVALID, ls_held);
    REFUSED(ask(LANE_ASK_MODELS, off, LANE_MODELS, 0, true), INVALID, box_held);
    REFUSED(ask(LANE_ASK_MODELS, off, LANE_MODELS, 2), INVALID, obs_held);
    REFUSED(ask(LANE_ASK_MODELS, off, LANE_MODELS, 3, true, true, 8), INVALID, merit_held);
    REFUSED(ask(LANE_ASK_MODELS, off, LANE_MODELS, 3, true, false, 8), INVALID, ls_held);
    REFUSED(ask(LANE_ASK_MODELS, off, LANE_MODELS, 3, true), INVALID, box_held);
    ACCEPTED(ask(LANE_ASK_MODELS, off, LANE_MODELS, 1));
    ACCEPTED(ask(LANE_ASK_MODELS, 1, LANE_MODELS, 3, true, true, 8));  // (on stays on)
  }
  // the off-values are accepted everywhere
  for (Site site : {MAJOR, LANE, LANE_MODELS, QUAD_MODELS})
    for (int off : {0, -1}) {
      for (LaneAsk what : {LANE_ASK_OBSTACLES, LANE_ASK_MODELS, LANE_ASK_BARRIER_COST,
                           LANE_ASK_LINE_SEARCH, WAVE_ASK_BARRIER_COST})
        ACCEPTED(ask(what, off, site));
      ACCEPTED(ask(LANE_ASK_OBSTACLES, 1, site));
      ACCEPTED(ask(LANE_ASK_LINE_SEARCH, 1, site));
      ACCEPTED(ask(LANE_ASK_BOX, 0, site));
    }
  // ... and the on-values on a lane handle of the bicycles with "lane_models" 1
  ACCEPTED(ask(LANE_ASK_MODELS, 1, LANE));
  ACCEPTED(ask(LANE_ASK_BARRIER_COST, 1, LANE_MODELS));
  for (int A : {2, 4, 8}) ACCEPTED(ask(LANE_ASK_LINE_SEARCH, A, LANE_MODELS));
  for (int K : {2, 8}) ACCEPTED(ask(LANE_ASK_OBSTACLES, K, LANE_MODELS));
  ACCEPTED(ask(LANE_ASK_BOX, 1, LANE_MODELS));
}

int main() {
  forms_and_names();
  refusals();
  std::printf("%d failed\n", bad);
  return bad ? 1 : 0;
}
"""


def test_lane_forms_names_and_refusals(tmp_path):
    run_host_program(tmp_path, "lane_opt_in_check", RULES_PROGRAM, [CSRC])


def test_header_documents_the_option_and_the_layouts():
    hdr = (ROOT / "include" / "i2lqr.h").read_text()
    assert '"lane_models"' in hdr
    assert "obs[6][K][B]" in hdr and "obs[B/64][6][K][64]" in hdr
    assert "k_lane_iterate_model" in hdr
    src = (CSRC / "i2lqr_lane_opt_in.hpp").read_text()
    assert '"k_lane_iterate (several obstacles)"' in src and '"k_lane_iterate (state box)"' in src
    units = (CSRC / "Makefile").read_text()
    assert "i2lqr_lane_model_f64" in units and "i2lqr_lane_model_f32" in units


@functools.lru_cache(maxsize=None)
def _reference(name, n_iters, boxed, scale=1.0):
    cfg, host, box = make_case(name, box=True, layout=2)
    host = dict(host, X=host["X"] * scale)  # (only X[:, :, 0] = x0 is non-zero)
    return reference(cfg, host, box=box if boxed else None, max_iter=n_iters,
                     early_exit=n_iters is None)


@pytest.mark.parametrize("name,n_iters,boxed", TILED_RUNS,
                         ids=[f"{c}-{'solve' if n is None else n}-{'box' if b else 'records'}"
                              for c, n, b in TILED_RUNS])
def test_tiled_sets_are_well_conditioned(name, n_iters, boxed):
    """A kernel that differs from the reference by round-off must meet the same accept / reject
    decisions: they do not move when x0 is scaled by 1 + 1e-13 or 1 - 1e-12."""
    ref = _reference(name, n_iters, boxed)
    for scale in (1.0 + 1e-13, 1.0 - 1e-12):
        per = _reference(name, n_iters, boxed, scale)
        assert np.array_equal(per["lamb"], ref["lamb"]), scale
        assert np.array_equal(per["iters"], ref["iters"]), scale


@pytest.mark.parametrize("name", TILED)
def test_tiled_sets_extra_records_and_box_matter(name):
    """The sets exercise what they are for: the records beyond the first and the box each move the
    trajectories of at least a tenth of the problems by more than 1e-6 relative."""
    cfg, host, box = make_case(name, box=True, layout=2)
    assert host["X"].shape[0] == 128 and host["obs"].shape[1:] == (RECORDS[name][1], 6)
    full = _reference(name, 6, False)
    one = reference(cfg, first_record_only(host), max_iter=6, early_exit=False)
    boxed = reference(cfg, host, box=box, max_iter=6, early_exit=False)
    for other in (one, boxed):
        d = (np.abs(full["X"] - other["X"]).reshape(128, -1).max(axis=1) /
             np.abs(full["X"]).reshape(128, -1).max(axis=1))
        assert (d > 1e-6).mean() >= 0.1
