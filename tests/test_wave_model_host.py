"""CPU suite: csrc/i2lqr_wave_model.hpp, what a handle knows about the opt-in model of the
one-problem-per-wavefront kernel (line search, obstacle records, state box) and the rules the host
derives from it.  The header is plain C++17: a stand-alone program that includes nothing else of the
library is built with the host compiler under AddressSanitizer and UBSan and run.  The expected
values are literals: the precedence box > obstacles > line search, the step and record counts, and
the LDS behind a problem's slice - 0, then 6 K words, then 6 K + 2 n (N + 1) + 2 n words."""
from pathlib import Path

from helpers import HOST_CHECK_PRELUDE, run_host_program

CSRC = Path(__file__).resolve().parent.parent / "ilqr_iterative_tasks_amd" / "csrc"

PROGRAM = '#include "i2lqr_wave_model.hpp"\n' + HOST_CHECK_PRELUDE + r"""
static WaveModel model(int ls, int obs, bool box) {
  WaveModel m;
  m.ls = ls;
  m.obs = obs;
  if (box) {
    m.box.hi[0] = 2.5;
    m.box.m_hi = 1u;
  }
  return m;
}

int main() {
  // form and reported kernel, all eight combinations: box > obstacles > line search
  const struct { int ls, obs; bool box; WaveForm form; const char* name; } combos[] = {
      {0, 0, false, WAVE_PLAIN, "k_iterate"},
      {4, 0, false, WAVE_LS, "k_iterate (line search)"},
      {0, 3, false, WAVE_OBS, "k_iterate (several obstacles)"},
      {4, 3, false, WAVE_OBS, "k_iterate (several obstacles)"},
      {0, 0, true, WAVE_BOX, "k_iterate (state box)"},
      {4, 0, true, WAVE_BOX, "k_iterate (state box)"},
      {0, 3, true, WAVE_BOX, "k_iterate (state box)"},
      {4, 3, true, WAVE_BOX, "k_iterate (state box)"},
  };
  for (const auto& c : combos) {
    const WaveModel m = model(c.ls, c.obs, c.box);
    CHECK(m.form() == c.form);
    CHECK(m.form(false) == c.form);
    CHECK(m.form(true) == WAVE_BOX);  // a chained call is the box form whatever is on
    CHECK(!std::strcmp(wave_kernel_name(m.form()), c.name));
  }
  // a default model is off; a lower bound alone switches the box on
  CHECK(WaveModel().form() == WAVE_PLAIN);
  {
    WaveModel m;
    m.box.m_lo = 1u << 3;
    CHECK(m.box.on() && m.form() == WAVE_BOX);
  }
  // a call without a forward pass: the line search does not count
  CHECK(model(4, 0, false).without_line_search().form() == WAVE_PLAIN);
  CHECK(model(4, 3, false).without_line_search().form() == WAVE_OBS);
  CHECK(model(4, 0, true).without_line_search().form() == WAVE_BOX);

  CHECK(model(0, 0, false).steps() == 1);
  CHECK(model(2, 0, false).steps() == 2);
  CHECK(model(4, 0, false).steps() == 4);
  CHECK(model(8, 0, false).steps() == 8);
  CHECK(model(0, 0, false).records() == 1);
  CHECK(model(0, 2, false).records() == 2);
  CHECK(model(0, 8, false).records() == 8);

  // LDS behind the slice
  CHECK(model(8, 0, false).extra_lds_bytes(WAVE_LS, 4, 6, 8) == 0);
  CHECK(model(2, 0, false).extra_lds_bytes(WAVE_LS, 12, 20, 4) == 0);
  CHECK(model(0, 0, false).extra_lds_bytes(WAVE_PLAIN, 6, 50, 8) == 0);
  CHECK(model(0, 8, false).extra_lds_bytes(WAVE_OBS, 4, 6, 4) == 192);
  CHECK(model(0, 2, true).extra_lds_bytes(WAVE_BOX, 4, 6, 8) == 608);
  CHECK(model(0, 0, true).extra_lds_bytes(WAVE_BOX, 12, 20, 4) == 2136);
  {
    const WaveModel off;
    CHECK(off.extra_lds_bytes(off.form(true), 4, 6, 8) == 560);
  }

  // what the refusals name
  CHECK(std::strstr(wave_phrase(WAVE_LS), "\"line_search\""));
  CHECK(std::strstr(wave_phrase(WAVE_OBS), "\"obstacles\""));
  CHECK(std::strstr(wave_phrase(WAVE_BOX), "state box"));
  CHECK(std::strstr(wave_lack_phrase(WAVE_LS), "\"line_search\""));
  CHECK(std::strstr(wave_lack_phrase(WAVE_OBS), "\"obstacles\""));
  CHECK(std::strstr(wave_lack_phrase(WAVE_BOX), "state box"));

  std::printf("%d failed\n", bad);
  return bad ? 1 : 0;
}
"""


def test_wave_model_rules_against_literals(tmp_path):
    run_host_program(tmp_path, "wave_model_check", PROGRAM, [CSRC])
