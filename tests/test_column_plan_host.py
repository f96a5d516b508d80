"""CPU suite: csrc/i2lqr_column_plan.hpp, what the launcher of the problem-major layout decides from
integers - which fused kernel a call runs on and the refusal texts, the wavefronts per workgroup of
the eight- / sixteen-lane kernels, the per-step-Jacobian form, how a chained solve runs, the caller's
workspace, the recommended layout.  The header is plain C++17: a stand-alone program that includes
nothing else of the library is built with the host compiler under AddressSanitizer and UBSan and run.

The ColumnFit values are the byte counts of the layouts (Layout / GLayout / GSpecLayout / QLayout of
the kernel headers), printed once from the launcher as it was and pasted here: bicycle6 N = 20 in
fp64 and fp32, bicycle4 N = 6, quad12 N = 20, and bicycle6 N = 50 in fp64, whose eight problem
slices and three-wavefront speculative buffers do not fit a CU's LDS.

Kernel choice: one letter per batch size of {1, 1023, 1024, 4096, 4097, 8192, 8193, 12288, 12289},
read off select_fused() as it stood in i2lqr_abi.hip - G sixteen-lane kernel, W eight-lane workspace
form, 8 eight-lane kernel, S / s speculative form with sixteen / eight lanes, V one problem per
wavefront, X refused.
Workspace: i2lqr_workspace_bytes and the choice read ONE range predicate.  What the launcher always
did and still does: with "group_workspace" 0 a size is reported in the automatic range although the
form is never chosen (asserted as it is)."""
from pathlib import Path

from helpers import HOST_CHECK_PRELUDE, run_host_program

CSRC = Path(__file__).resolve().parent.parent / "ilqr_iterative_tasks_amd" / "csrc"

PROGRAM = '#include "i2lqr_column_plan.hpp"\n' + HOST_CHECK_PRELUDE + r"""
static ColumnFit bicycle(bool f64, int n, int N, size_t wave, size_t fstep, size_t g8, size_t g16,
                         size_t gws, int64_t ws, size_t s8x2, size_t s8x3, size_t s16x2, size_t s16x3) {
  ColumnFit f;
  f.plant = ColumnFit::BICYCLE;
  f.problem_major = true;
  f.f64 = f64;
  f.n = n; f.N = N; f.word = f64 ? 8 : 4;
  f.fixed_horizon = N == 20;
  f.lds_wave = wave; f.lds_wave_fstep = fstep;
  f.lds_group8 = g8; f.lds_group16 = g16; f.lds_group_ws = gws; f.ws_group = ws;
  f.lds_spec8x2 = s8x2; f.lds_spec8x3 = s8x3; f.lds_spec16x2 = s16x2; f.lds_spec16x3 = s16x3;
  return f;
}
// the byte counts of the layouts, as the launcher computed them
static const ColumnFit b6_f64 = bicycle(true, 6, 20, 8736, 16416, 77472, 36384, 33952, 5632, 114912, 152864, 54528, 71968);
static const ColumnFit b6_f32 = bicycle(false, 6, 20, 4368, 8208, 38736, 18192, 16976, 2816, 57456, 76432, 27264, 35984);
static const ColumnFit b4_n6 = bicycle(true, 4, 6, 2752, 3904, 25600, 10368, 13824, 1664, 35392, 47232, 15456, 20096);
// does not fit: eight slices 180896 B and the three-wavefront buffers 173856 B > 160 KiB
static const ColumnFit b6_n50 = bicycle(true, 6, 50, 18576, 37776, 180896, 88096, 72352, 13824, 268512, 356640, 131328, 173856);
static ColumnFit quad12() {
  ColumnFit f;
  f.plant = ColumnFit::SIXTEEN;
  f.problem_major = true;
  f.n = 12; f.N = 20;
  f.lds_wave = 24496; f.lds_quad = 21504; f.ws_quad = 26368;
  return f;
}

static ColumnTune tune(int group = -1, int spec = -1, int ws = -1) {
  ColumnTune t;
  t.opt_group = group; t.opt_spec = spec; t.opt_group_ws = ws;
  return t;
}
static const int64_t kBig = (int64_t)1 << 40;  // a registered workspace that is large enough
static const char* const kWsText =
    "\"group_workspace\" = 1 needs a registered workspace of i2lqr_workspace_bytes() for this batch";

static char letter(const ColumnChoice& c) {
  switch (c.kernel) {
    case K_GROUP16: return 'G';
    case K_GROUP_WS: return 'W';
    case K_GROUP: return '8';
    case K_SPEC16: return 'S';
    case K_SPEC: return 's';
    case K_WAVE: return 'V';
    case K_WAVE_OPT: return 'O';
    case K_QUAD: return 'Q';
    default: return 'X';
  }
}
static const int64_t kBatches[9] = {1, 1023, 1024, 4096, 4097, 8192, 8193, 12288, 12289};
// rows: iterate / solve x workspace not registered / registered
static void expect(int line, const DeviceGeometry& g, const ColumnFit& f, const ColumnTune& t,
                   const char* it, const char* it_ws, const char* so, const char* so_ws) {
  const char* want[2][2] = {{it, it_ws}, {so, so_ws}};
  for (int solve = 0; solve < 2; solve++)
    for (int ws = 0; ws < 2; ws++)
      for (int b = 0; b < 9; b++) {
        const ColumnChoice c = column_kernel(g, f, t, WAVE_PLAIN, ws ? kBig : -1, kBatches[b], solve != 0);
        const bool text = c.kernel == K_INVALID ? !std::strcmp(c.why, kWsText) : c.why[0] == 0;
        if (letter(c) != want[solve][ws][b] || !text) {
          if (bad < 40)
            std::printf("FAILED table of line %d: %s ws %d B %lld: %c, expected %c (\"%s\")\n", line,
                        solve ? "solve" : "iterate", ws, (long long)kBatches[b], letter(c),
                        want[solve][ws][b], c.why);
          bad++;
        }
      }
}
#define EXPECT(...) expect(__LINE__, __VA_ARGS__)

static void choice() {
  const DeviceGeometry g;  // the MI355X figures
  for (const ColumnFit* f : {&b6_f64, &b4_n6}) {
    EXPECT(g, *f, tune(), "GGGGGGGGG", "GGGGWWGGG", "SSSSSSSSG", "SSSSSSSSG");
    EXPECT(g, *f, tune(8), "888888888", "8888WWWWW", "888888888", "8888WWWWW");
    EXPECT(g, *f, tune(16), "GGGGGGGGG", "GGGGGGGGG", "GGGGGGGGG", "GGGGGGGGG");
    EXPECT(g, *f, tune(64), "VVVVVVVVV", "VVVVVVVVV", "VVVVVVVVV", "VVVVVVVVV");
    EXPECT(g, *f, tune(-1, 0), "GGGGGGGGG", "GGGGWWGGG", "GGGGGGGGG", "GGGGWWGGG");
    EXPECT(g, *f, tune(-1, 1), "SSSSSSSSS", "SSSSSSSSS", "SSSSSSSSS", "SSSSSSSSS");
    EXPECT(g, *f, tune(-1, -1, 0), "GGGGGGGGG", "GGGG88GGG", "SSSSSSSSG", "SSSSSSSSG");
    EXPECT(g, *f, tune(-1, -1, 1), "VVXXXXXXX", "VVWWWWWWW", "SSSSSSSSX", "SSSSSSSSW");
  }
  // fp32: the workspace range ends at 7168 problems
  EXPECT(g, b6_f32, tune(), "GGGGGGGGG", "GGGGWGGGG", "SSSSSSSSG", "SSSSSSSSG");
  EXPECT(g, b6_f32, tune(8), "888888888", "8888WWWWW", "888888888", "8888WWWWW");
  EXPECT(g, b6_f32, tune(16), "GGGGGGGGG", "GGGGGGGGG", "GGGGGGGGG", "GGGGGGGGG");
  EXPECT(g, b6_f32, tune(64), "VVVVVVVVV", "VVVVVVVVV", "VVVVVVVVV", "VVVVVVVVV");
  EXPECT(g, b6_f32, tune(-1, 0), "GGGGGGGGG", "GGGGWGGGG", "GGGGGGGGG", "GGGGWGGGG");
  EXPECT(g, b6_f32, tune(-1, 1), "SSSSSSSSS", "SSSSSSSSS", "SSSSSSSSS", "SSSSSSSSS");
  EXPECT(g, b6_f32, tune(-1, -1, 0), "GGGGGGGGG", "GGGG8GGGG", "SSSSSSSSG", "SSSSSSSSG");
  EXPECT(g, b6_f32, tune(-1, -1, 1), "VVXXXXXXX", "VVWWWWWWW", "SSSSSSSSX", "SSSSSSSSW");
  CHECK(column_kernel(g, b6_f32, tune(), WAVE_PLAIN, kBig, 7168, false).kernel == K_GROUP_WS);
  CHECK(column_kernel(g, b6_f32, tune(), WAVE_PLAIN, kBig, 7169, false).kernel == K_GROUP16);
  // a workspace smaller than the batch needs counts as none
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, 4168 * 5632, 4161, false).kernel == K_GROUP_WS);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, 4168 * 5632 - 1, 4161, false).kernel == K_GROUP16);
  // the eight-lane speculative form: pinned lanes and "speculate" 1
  CHECK(column_kernel(g, b6_f64, tune(8, 1), WAVE_PLAIN, -1, 64, false).kernel == K_SPEC);
  CHECK(column_kernel(g, b6_f64, tune(64, 1), WAVE_PLAIN, -1, 64, true).kernel == K_WAVE);

  // what does not fit
  EXPECT(g, b6_n50, tune(), "GGGGGGGGG", "GGGGGGGGG", "SSSSSSSSG", "SSSSSSSSG");
  EXPECT(g, b6_n50, tune(-1, -1, 1), "VVVVVVVVV", "VVVVVVVVV", "SSSSSSSSV", "SSSSSSSSV");
  {
    const ColumnChoice c = column_kernel(g, b6_n50, tune(8), WAVE_PLAIN, kBig, 1024, false);
    CHECK(c.kernel == K_INVALID);
    CHECK(!std::strcmp(c.why, "\"group_lanes\" = 8 needs a bicycle plant with Q = R = 0 and a horizon "
                              "whose eight problem slices fit a CU's LDS"));
    ColumnFit f = b6_n50;
    f.lds_spec16x2 = g.max_dyn_lds + 1;
    const ColumnChoice s = column_kernel(g, f, tune(-1, 1), WAVE_PLAIN, -1, 64, true);
    CHECK(s.kernel == K_INVALID);
    CHECK(!std::strcmp(s.why, "\"speculate\" = 1 needs the eight- / sixteen-lane kernel and a horizon "
                              "whose speculative buffers fit a CU's LDS"));
    CHECK(column_kernel(g, f, tune(), WAVE_PLAIN, -1, 64, true).kernel == K_GROUP16);
    f.lds_group16 = g.max_dyn_lds + 1;
    const ColumnChoice s16 = column_kernel(g, f, tune(16), WAVE_PLAIN, -1, 64, false);
    CHECK(s16.kernel == K_INVALID);
    CHECK(!std::strcmp(s16.why, "\"group_lanes\" = 16 needs a bicycle plant with Q = R = 0 and a horizon "
                                "whose four problem slices fit a CU's LDS"));
    CHECK(column_kernel(g, f, tune(), WAVE_PLAIN, -1, 64, false).kernel == K_WAVE);
    f = b6_f64;  // stage weights: the column kernels are built for Q = R = 0
    f.weights = true;
    CHECK(column_kernel(g, f, tune(), WAVE_PLAIN, kBig, 4161, false).kernel == K_WAVE);
    CHECK(column_kernel(g, f, tune(), WAVE_PLAIN, kBig, 64, true).kernel == K_WAVE);
    CHECK(column_kernel(g, f, tune(16), WAVE_PLAIN, kBig, 64, true).kernel == K_INVALID);
  }
  {  // quad12: the sixteen-lane kernel whenever its workspace is registered
    const ColumnFit q = quad12();
    const int64_t need = quad_ws_bytes(g, q, 4161);
    CHECK(need == 4164 * 26368);
    CHECK(column_kernel(g, q, tune(), WAVE_PLAIN, need, 4161, false).kernel == K_QUAD);
    CHECK(column_kernel(g, q, tune(), WAVE_PLAIN, need, 4161, true).kernel == K_QUAD);
    CHECK(column_kernel(g, q, tune(16), WAVE_PLAIN, need, 4161, false).kernel == K_QUAD);
    CHECK(column_kernel(g, q, tune(), WAVE_PLAIN, need - 1, 4161, false).kernel == K_WAVE);
    CHECK(column_kernel(g, q, tune(), WAVE_PLAIN, -1, 4161, false).kernel == K_WAVE);
    CHECK(column_kernel(g, q, tune(64), WAVE_PLAIN, need, 4161, false).kernel == K_WAVE);
    const ColumnChoice c = column_kernel(g, q, tune(16), WAVE_PLAIN, -1, 4161, false);
    CHECK(c.kernel == K_INVALID);
    CHECK(!std::strcmp(c.why, "\"group_lanes\" = 16 needs Q = R = 0 and a registered workspace of "
                              "i2lqr_workspace_bytes() for this batch"));
    const ColumnChoice c8 = column_kernel(g, q, tune(8), WAVE_PLAIN, need, 4161, false);
    CHECK(c8.kernel == K_INVALID);
    CHECK(!std::strcmp(c8.why, "\"group_lanes\" = 8 is built for the m = 2 plants only"));
    ColumnFit w = q;
    w.weights = true;
    CHECK(quad_ws_bytes(g, w, 4161) == 0);
    CHECK(column_kernel(g, w, tune(), WAVE_PLAIN, kBig, 64, false).kernel == K_WAVE);
    CHECK(column_kernel(g, w, tune(16), WAVE_PLAIN, kBig, 64, false).kernel == K_INVALID);
    ColumnFit big = q;
    big.lds_quad = g.max_dyn_lds + 1;
    CHECK(column_kernel(g, big, tune(), WAVE_PLAIN, kBig, 64, false).kernel == K_WAVE);
    ColumnFit other;  // neither m = 2 nor n + m = 16
    other.problem_major = true;
    const ColumnChoice o = column_kernel(g, other, tune(16), WAVE_PLAIN, -1, 64, false);
    CHECK(o.kernel == K_INVALID);
    CHECK(!std::strcmp(o.why, "\"group_lanes\" = 16 is built for the bicycles (DPP row form) and the "
                              "n + m = 16 plant"));
    CHECK(column_kernel(g, other, tune(), WAVE_PLAIN, -1, 64, false).kernel == K_WAVE);
  }
  {  // a model is on: its form of the wavefront kernel whatever the batch, not with pinned lanes
    for (int64_t B : {1, 4161, 65536}) {
      CHECK(column_kernel(g, b6_f64, tune(), WAVE_LS, kBig, B, false).kernel == K_WAVE_OPT);
      CHECK(column_kernel(g, b6_f64, tune(64), WAVE_BOX, kBig, B, true).kernel == K_WAVE_OPT);
    }
    const ColumnChoice c = column_kernel(g, b6_f64, tune(8), WAVE_LS, -1, 64, false);
    CHECK(c.kernel == K_INVALID);
    CHECK(!std::strcmp(c.why, "\"line_search\" runs on the one-problem-per-wavefront kernel: not "
                              "together with \"group_lanes\" = 8 or 16"));
    const ColumnChoice o = column_kernel(g, quad12(), tune(16), WAVE_OBS, -1, 64, true);
    CHECK(o.kernel == K_INVALID);
    CHECK(!std::strcmp(o.why, "\"obstacles\" runs on the one-problem-per-wavefront kernel: not "
                              "together with \"group_lanes\" = 8 or 16"));
    const ColumnChoice b = column_kernel(g, b6_f64, tune(16), WAVE_BOX, -1, 64, true);
    CHECK(!std::strcmp(b.why, "a state box runs on the one-problem-per-wavefront kernel: not "
                              "together with \"group_lanes\" = 8 or 16"));
  }
  CHECK(!std::strcmp(column_kernel_name(K_GROUP16, WAVE_PLAIN), "k_group_iterate (sixteen lanes)"));
  CHECK(!std::strcmp(column_kernel_name(K_WAVE_OPT, WAVE_BOX), "k_iterate (state box)"));
  CHECK(!std::strcmp(column_kernel_name(K_INVALID, WAVE_PLAIN), "unsupported"));
}

static void helpers() {
  const DeviceGeometry g;
  CHECK(group8_wavefronts(g, 1) == 3 && group8_wavefronts(g, 2048) == 3 && group8_wavefronts(g, 2049) == 1);
  CHECK(group16_wavefronts(g, 1, true) == 3 && group16_wavefronts(g, 1024, true) == 3);
  CHECK(group16_wavefronts(g, 1025, true) == 2 && group16_wavefronts(g, 2048, true) == 2);
  CHECK(group16_wavefronts(g, 2049, true) == 1 && group16_wavefronts(g, 1 << 20, true) == 1);
  for (int64_t B : {1, 1024, 1025, 2048}) CHECK(group16_wavefronts(g, B, false) == 2);  // overlap 0: never 3
  CHECK(group16_wavefronts(g, 2049, false) == 1);
  // the fixed-horizon form: where it is built, unless pinned off
  ColumnTune t;
  CHECK(group16_fixed(b6_f64, t) && !group16_fixed(b4_n6, t) && !group16_fixed(b6_n50, t));
  t.opt_group_fixed = 0;
  CHECK(!group16_fixed(b6_f64, t));
  t.opt_group_fixed = 1;
  CHECK(group16_fixed(b6_f64, t) && !group16_fixed(b4_n6, t));
  // speculative form: three wavefronts up to 512 problems where their buffers fit, never in the tail
  for (int lanes : {8, 16}) {
    CHECK(spec_wavefronts(g, b6_f64, lanes, 1, false) == 3 && spec_wavefronts(g, b6_f64, lanes, 512, false) == 3);
    CHECK(spec_wavefronts(g, b6_f64, lanes, 513, false) == 2 && spec_wavefronts(g, b6_f64, lanes, 64, true) == 2);
    CHECK(spec_wavefronts(g, b6_n50, lanes, 64, false) == 2);  // 173856 / 356640 B do not fit
  }
  ColumnFit f = b6_f64;
  f.lds_spec8x3 = g.max_dyn_lds + 1;  // the eight-lane buffers alone
  CHECK(spec_wavefronts(g, f, 8, 64, false) == 2 && spec_wavefronts(g, f, 16, 64, false) == 3);
  f.lds_spec8x3 = g.max_dyn_lds;
  CHECK(spec_wavefronts(g, f, 8, 64, false) == 3);
  // the tail of the chunked solves: sixteen lanes where they fit, whatever the layout
  ColumnFit lane = b6_f64;
  lane.problem_major = false;
  CHECK(spec_tail_lanes(g, lane) == 16 && spec_tail_lanes(g, b6_f64) == 16);
  CHECK(!spec_fits(g, lane, 16) && !group_fits(g, lane, 8) && group_ws_bytes(g, lane, 4161) == 0);
  lane.lds_spec16x2 = g.max_dyn_lds + 1;
  CHECK(spec_tail_lanes(g, lane) == 8);
  lane.lds_spec8x2 = g.max_dyn_lds + 1;
  CHECK(spec_tail_lanes(g, lane) == 0);
  lane = b6_f64;
  lane.weights = true;
  CHECK(spec_tail_lanes(g, lane) == 0 && spec_tail_lanes(g, quad12()) == 0);
}

static void fstep() {
  const DeviceGeometry g;
  ColumnTune t;
  // automatic: on exactly while waves_per_cu * lds_f <= lds_per_cu - 10 KiB; 16416 B: nine
  // wavefronts per CU (147744 <= 153600 < 164160)
  CHECK(9 * b6_f64.lds_wave_fstep <= g.lds_per_cu - 10240 && 10 * b6_f64.lds_wave_fstep > g.lds_per_cu - 10240);
  CHECK(wave_fstep(g, b6_f64, t, 1) && wave_fstep(g, b6_f64, t, 9 * 256) && !wave_fstep(g, b6_f64, t, 9 * 256 + 1));
  // fp32, 8208 B: eighteen
  CHECK(wave_fstep(g, b6_f32, t, 18 * 256) && !wave_fstep(g, b6_f32, t, 18 * 256 + 1));
  t.opt_fstep = 1;
  CHECK(wave_fstep(g, b6_f64, t, 1 << 20) && wave_fstep(g, b6_n50, t, 1 << 20));
  ColumnFit f = b6_f64;
  f.lds_wave_fstep = g.default_dyn_lds + 1;  // the slice must fit the default limit
  CHECK(!wave_fstep(g, f, t, 1));
  f.lds_wave_fstep = g.default_dyn_lds;
  CHECK(wave_fstep(g, f, t, 1));
  CHECK(!wave_fstep(g, quad12(), t, 1));  // not built for quad12
  t.opt_fstep = 0;
  CHECK(!wave_fstep(g, b6_f64, t, 1));
  // the bytes of an opt-in call: the slice, K records of six words, the box's 2 n (N + 2) words
  WaveModel m;
  CHECK(wave_lds_need(b6_f64, m, false) == 8736);
  m.obs = 3;
  CHECK(wave_lds_need(b6_f64, m, false) == 8736 + 3 * 6 * 8);
  CHECK(wave_lds_need(b6_f64, m, true) == 8736 + (3 * 6 + 2 * 6 * 21 + 2 * 6) * 8);
  CHECK(wave_lds_need(b6_f32, m, true) == 4368 + (3 * 6 + 2 * 6 * 21 + 2 * 6) * 4);
}

static void chains() {
  const DeviceGeometry g;
  const char* const plant = "chains are built for the m = 2 plants";
  const char* const limits =
      "chains run on the sixteen-lane speculative kernel: a bicycle plant with Q = R = 0, at most 512 "
      "chains, a horizon whose three-wavefront buffers fit a CU's LDS (solve the chain steps one after "
      "the other instead)";
  ColumnTune t;
  CHECK(chain_plan(g, b6_f64, t, WAVE_PLAIN, -1, 1).kind == ChainPlan::SPEC);
  CHECK(chain_plan(g, b6_f64, t, WAVE_PLAIN, -1, 512).kind == ChainPlan::SPEC);
  ChainPlan p = chain_plan(g, b6_f64, t, WAVE_PLAIN, -1, 513);
  CHECK(p.kind == ChainPlan::REFUSED && !std::strcmp(p.why, limits));
  p = chain_plan(g, b6_n50, t, WAVE_PLAIN, -1, 8);  // the three-wavefront buffers do not fit
  CHECK(p.kind == ChainPlan::REFUSED && !std::strcmp(p.why, limits));
  for (const ColumnTune& pin : {tune(8), tune(64), tune(-1, 0)}) {
    p = chain_plan(g, b6_f64, pin, WAVE_PLAIN, -1, 8);
    CHECK(p.kind == ChainPlan::REFUSED && !std::strcmp(p.why, limits));
  }
  CHECK(chain_plan(g, b6_f64, tune(16), WAVE_PLAIN, -1, 8).kind == ChainPlan::SPEC);
  ColumnFit w = b6_f64;
  w.weights = true;
  CHECK(chain_plan(g, w, t, WAVE_PLAIN, -1, 8).kind == ChainPlan::REFUSED);
  p = chain_plan(g, quad12(), t, WAVE_PLAIN, kBig, 8);
  CHECK(p.kind == ChainPlan::REFUSED && !std::strcmp(p.why, plant));
  t.opt_wave_chain = 1;  // what the speculative chain is not built for runs on k_chain_box
  CHECK(chain_plan(g, b6_f64, t, WAVE_PLAIN, -1, 512).kind == ChainPlan::SPEC);
  CHECK(chain_plan(g, b6_f64, t, WAVE_PLAIN, -1, 513).kind == ChainPlan::WAVE);
  CHECK(chain_plan(g, b6_n50, t, WAVE_PLAIN, -1, 8).kind == ChainPlan::WAVE);
  CHECK(chain_plan(g, w, t, WAVE_PLAIN, -1, 8).kind == ChainPlan::WAVE);
  CHECK(chain_plan(g, quad12(), t, WAVE_PLAIN, -1, 8).kind == ChainPlan::WAVE);
  for (WaveForm f : {WAVE_LS, WAVE_OBS, WAVE_BOX}) {  // ... and every model
    CHECK(chain_plan(g, b6_f64, t, f, -1, 8).kind == ChainPlan::WAVE);
    CHECK(chain_plan(g, quad12(), t, f, -1, 8).kind == ChainPlan::WAVE);
  }
  t.opt_group = 8;  // a model with pinned lanes: refused as i2lqr_solve refuses it
  p = chain_plan(g, b6_f64, t, WAVE_LS, -1, 8);
  CHECK(p.kind == ChainPlan::REFUSED);
  CHECK(!std::strcmp(p.why, "\"line_search\" runs on the one-problem-per-wavefront kernel: not together "
                            "with \"group_lanes\" = 8 or 16"));
  CHECK(chain_plan(g, b6_f64, t, WAVE_PLAIN, -1, 8).kind == ChainPlan::WAVE);
}

// i2lqr_workspace_bytes and the choice agree, for every batch size around the thresholds
static void workspace() {
  const DeviceGeometry g;
  long checked = 0, ws_form = 0;
  for (const ColumnFit* f : {&b6_f64, &b6_f32})
    for (int group : {-1, 8, 16, 64})
      for (int ws : {-1, 0, 1}) {
        const ColumnTune t = tune(group, -1, ws);
        const auto one = [&](int64_t B) {
          const int64_t bytes = column_workspace_bytes(g, *f, t, B);
          CHECK(bytes >= 0);
          for (int solve = 0; solve < 2; solve++) {
            if (bytes > 0) {  // registered: never the refusal that asks for it
              const ColumnChoice c = column_kernel(g, *f, t, WAVE_PLAIN, bytes, B, solve != 0);
              CHECK(c.kernel != K_INVALID || std::strcmp(c.why, kWsText) != 0);
            }
            // the workspace form is chosen only where a size was reported, and fits into it
            const ColumnChoice big = column_kernel(g, *f, t, WAVE_PLAIN, kBig, B, solve != 0);
            if (big.kernel == K_GROUP_WS) {
              ws_form++;
              CHECK(bytes > 0);
              CHECK(column_kernel(g, *f, t, WAVE_PLAIN, bytes, B, solve != 0).kernel == K_GROUP_WS);
            }
          }
          // the size: whole wavefronts of eight problems, only where the form is asked for
          const int64_t top = f->f64 ? 8192 : 7168;
          const bool asked = (B > 4096 && (B <= top || group == 8)) || ws == 1;
          CHECK(bytes == (asked ? (B + 7) / 8 * 8 * f->ws_group : 0));
          checked++;
        };
        for (int64_t B = 1; B <= 20000; B += 257) one(B);
        for (int64_t edge : {1024, 4096, 7168, 8192, 12288})
          for (int64_t B = edge - 2; B <= edge + 2; B++) one(B);
      }
  CHECK(checked == 2L * 4 * 3 * (78 + 25) && ws_form > 0);
  // what the launcher always did: "group_workspace" 0 reports the range's size and never takes the form
  CHECK(column_workspace_bytes(g, b6_f64, tune(-1, -1, 0), 4161) == 4168 * 5632);
  CHECK(column_kernel(g, b6_f64, tune(-1, -1, 0), WAVE_PLAIN, kBig, 4161, false).kernel == K_GROUP);
  // what does not fit asks for nothing; quad12 whenever it is supported
  CHECK(column_workspace_bytes(g, b6_n50, tune(-1, -1, 1), 4161) == 0);
  CHECK(column_workspace_bytes(g, quad12(), tune(), 1) == 4 * 26368);
  CHECK(column_workspace_bytes(g, quad12(), tune(), 0) == 0);
}

// another CU count: the thresholds follow scaled(), the helper limits the CUs themselves
static void geometry() {
  DeviceGeometry g;
  g.cus = 32;
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, kBig, 512, false).kernel == K_GROUP16);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, kBig, 513, false).kernel == K_GROUP_WS);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, kBig, 1024, false).kernel == K_GROUP_WS);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, kBig, 1025, false).kernel == K_GROUP16);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, -1, 1536, true).kernel == K_SPEC16);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, -1, 1537, true).kernel == K_GROUP16);
  CHECK(column_kernel(g, b6_f64, tune(-1, -1, 1), WAVE_PLAIN, kBig, 127, false).kernel == K_WAVE);
  CHECK(column_kernel(g, b6_f64, tune(-1, -1, 1), WAVE_PLAIN, kBig, 128, false).kernel == K_GROUP_WS);
  CHECK(column_workspace_bytes(g, b6_f64, tune(), 512) == 0 && column_workspace_bytes(g, b6_f64, tune(), 513) > 0);
  CHECK(column_workspace_bytes(g, b6_f64, tune(), 1024) > 0 && column_workspace_bytes(g, b6_f64, tune(), 1025) == 0);
  CHECK(group8_wavefronts(g, 256) == 3 && group8_wavefronts(g, 257) == 1);
  CHECK(group16_wavefronts(g, 128, true) == 3 && group16_wavefronts(g, 129, true) == 2);
  CHECK(group16_wavefronts(g, 256, true) == 2 && group16_wavefronts(g, 257, true) == 1);
  CHECK(spec_wavefronts(g, b6_f64, 16, 64, false) == 3 && spec_wavefronts(g, b6_f64, 16, 65, false) == 2);
  CHECK(chain_plan(g, b6_f64, tune(), WAVE_PLAIN, -1, 64).kind == ChainPlan::SPEC);
  const ChainPlan p = chain_plan(g, b6_f64, tune(), WAVE_PLAIN, -1, 65);
  CHECK(p.kind == ChainPlan::REFUSED && std::strstr(p.why, "at most 64 chains"));
  CHECK(wave_fstep(g, b6_f64, tune(), 9 * 32) && !wave_fstep(g, b6_f64, tune(), 9 * 32 + 1));
  g.cus = 128;
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, kBig, 2048, false).kernel == K_GROUP16);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, kBig, 2049, false).kernel == K_GROUP_WS);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, kBig, 4096, false).kernel == K_GROUP_WS);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, kBig, 4097, false).kernel == K_GROUP16);
  CHECK(column_kernel(g, b6_f32, tune(), WAVE_PLAIN, kBig, 3584, false).kernel == K_GROUP_WS);
  CHECK(column_kernel(g, b6_f32, tune(), WAVE_PLAIN, kBig, 3585, false).kernel == K_GROUP16);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, -1, 6144, true).kernel == K_SPEC16);
  CHECK(column_kernel(g, b6_f64, tune(), WAVE_PLAIN, -1, 6145, true).kernel == K_GROUP16);
  CHECK(column_kernel(g, b6_f64, tune(-1, -1, 1), WAVE_PLAIN, kBig, 511, false).kernel == K_WAVE);
  CHECK(column_kernel(g, b6_f64, tune(-1, -1, 1), WAVE_PLAIN, kBig, 512, false).kernel == K_GROUP_WS);
  CHECK(group8_wavefronts(g, 1024) == 3 && group8_wavefronts(g, 1025) == 1);
  CHECK(group16_wavefronts(g, 512, true) == 3 && group16_wavefronts(g, 513, true) == 2);
  CHECK(group16_wavefronts(g, 1024, true) == 2 && group16_wavefronts(g, 1025, true) == 1);
  CHECK(spec_wavefronts(g, b6_f64, 16, 256, false) == 3 && spec_wavefronts(g, b6_f64, 16, 257, false) == 2);
  CHECK(chain_plan(g, b6_f64, tune(), WAVE_PLAIN, -1, 256).kind == ChainPlan::SPEC);
  CHECK(chain_plan(g, b6_f64, tune(), WAVE_PLAIN, -1, 257).kind == ChainPlan::REFUSED);
  CHECK(wave_fstep(g, b6_f64, tune(), 9 * 128) && !wave_fstep(g, b6_f64, tune(), 9 * 128 + 1));
}

static i2lqr_config config(int system_id, int N, int dtype) {
  i2lqr_config c;
  std::memset(&c, 0, sizeof(c));
  c.system_id = system_id;
  c.n = system_id == I2LQR_SYS_BICYCLE4 ? 4 : (system_id == I2LQR_SYS_BICYCLE6 ? 6 : 12);
  c.m = system_id == I2LQR_SYS_QUAD12 ? 4 : 2;
  c.N = N;
  c.dtype = dtype;
  for (int i = 0; i < c.n; i++) c.Qt[i * I2LQR_MAX_N + i] = 2.0;
  return c;
}

static void layout() {
  const DeviceGeometry g;
  const int PM = I2LQR_LAYOUT_PROBLEM_MAJOR, BM = I2LQR_LAYOUT_BATCH_MINOR, BT = I2LQR_LAYOUT_BATCH_TILED;
  const i2lqr_config b6_50 = config(I2LQR_SYS_BICYCLE6, 50, I2LQR_F64), b6_20 = config(I2LQR_SYS_BICYCLE6, 20, I2LQR_F64);
  const i2lqr_config b6_20f = config(I2LQR_SYS_BICYCLE6, 20, I2LQR_F32), b4_6 = config(I2LQR_SYS_BICYCLE4, 6, I2LQR_F64);
  // (tests/test_layout_table.py::test_horizon_buckets_and_precision_are_read)
  CHECK(recommended_layout(g, b6_50, false, 8192, false) == BT);
  CHECK(recommended_layout(g, b6_20, false, 8192, false) == PM);
  CHECK(recommended_layout(g, b6_20f, false, 12288, false) == PM);
  CHECK(recommended_layout(g, b6_20f, false, 14336, false) == BT);
  CHECK(recommended_layout(g, b6_20, false, 10240, false) == BT);
  CHECK(recommended_layout(g, b4_6, false, 8192, false) == PM);
  CHECK(recommended_layout(g, b4_6, false, 8256, false) == BT);
  CHECK(recommended_layout(g, b4_6, false, 9001, false) == BM);
  // solves have their own crossover; stage weights leave at 2048 problems
  CHECK(recommended_layout(g, b6_20, false, 10240, true) == PM && recommended_layout(g, b6_20, false, 10241, true) == BM);
  CHECK(recommended_layout(g, b6_20, true, 2047, false) == PM && recommended_layout(g, b6_20, true, 2048, false) == BT);
  // non-symmetric weights stay problem-major at any size
  i2lqr_config skew = b6_20;
  skew.Q[0 * I2LQR_MAX_N + 1] = 0.5;
  CHECK(!std::strcmp(lane_asymmetry(skew), "symmetric Q and Qterminal") && !lane_asymmetry(b6_20));
  CHECK(recommended_layout(g, skew, true, 1 << 20, false) == PM);
  skew = b6_20;
  skew.R[1 * I2LQR_MAX_M + 0] = 0.5;
  CHECK(!std::strcmp(lane_asymmetry(skew), "a symmetric R"));
  CHECK(recommended_layout(g, skew, true, 1 << 20, true) == PM);
  // quad12: fp32 with stage weights has no lane kernel
  const i2lqr_config q = config(I2LQR_SYS_QUAD12, 20, I2LQR_F64), qf = config(I2LQR_SYS_QUAD12, 20, I2LQR_F32);
  CHECK(recommended_layout(g, q, false, 4096, false) == PM && recommended_layout(g, q, false, 4097, false) == BM);
  CHECK(recommended_layout(g, q, false, 8192, true) == PM && recommended_layout(g, q, false, 8193, true) == BM);
  CHECK(recommended_layout(g, qf, true, 1 << 20, false) == PM && recommended_layout(g, q, true, 2048, false) == BT);
  DeviceGeometry small;
  small.cus = 32;  // scaled_from: (8193 - 1) / 8 + 1
  CHECK(recommended_layout(small, b6_20, false, 1024, false) == PM && recommended_layout(small, b6_20, false, 1025, false) == BM);
}

int main() {
  choice();
  helpers();
  fstep();
  chains();
  workspace();
  geometry();
  layout();
  std::printf("%d failed\n", bad);
  return bad ? 1 : 0;
}
"""


def test_column_plan_rules_against_literals(tmp_path):
    run_host_program(tmp_path, "column_plan_check", PROGRAM, [CSRC])
