"""CPU suite: csrc/i2lqr_abi.hip compiles the host layer and the small kernels only.  The fused and
function-level kernels of the wave and lane families are declared `extern template` in
csrc/i2lqr_kernels.h and instantiated in units of their own; a launch in the ABI unit of an
instantiation that header does not declare would compile that kernel into the ABI unit again,
silently, and bring its minutes of compile time back.  Compiles the unit's device code with hipcc
(cross-compiles without a GPU) and inspects the kernels' names."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "ilqr_iterative_tasks_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
         "--cuda-device-only"]
# every kernel template the ABI unit instantiates itself, each in fp64 and fp32
SMALL = ["k_relax_cost", "k_select_candidates", "k_init_candidates", "k_pick_best", "k_pack_problem",
         "k_round_winner", "k_round_prepare", "k_round_pick", "k_argmin_final"]
MOVED = ("k_iterate", "k_rollout", "k_backward", "k_forward", "k_lane_")


def test_the_abi_unit_compiles_the_small_kernels_only(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "i2lqr_abi.s"
    subprocess.run([HIPCC, *FLAGS, "-o", str(out), str(CSRC / "i2lqr_abi.hip")], check=True,
                   capture_output=True, timeout=900)
    symbols = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", out.read_text(), flags=re.M)
    # _ZN5i2lqr<len><name>I... / _ZN<len>_GLOBAL__N_1<len><name>I... -> <name>
    names = []
    for sym in symbols:
        m = re.match(r"_ZN(?:5i2lqr|12_GLOBAL__N_1)(\d+)", sym)
        assert m, f"kernel {sym} is in neither namespace i2lqr nor the unit's anonymous namespace"
        names.append(sym[m.end():m.end() + int(m.group(1))])
    print(len(symbols), "kernels:", sorted(set(names)))
    moved = [s for s, n in zip(symbols, names) if n.startswith(MOVED)]
    assert not moved, f"compiled into the ABI unit again (no extern template declaration?): {moved}"
    expect = sorted(SMALL * 2 + ["k_argmin_partial"] * 4)  # (k_argmin_partial: FINAL and not)
    assert sorted(names) == expect, sorted(names)


def test_the_wave_opt_unit_compiles_no_kernel(tmp_path):
    """csrc/i2lqr_wave_opt.hip is the host-only launcher of the opt-in wavefront kernels: it reaches
    all 48 of them through the `extern template` list of csrc/i2lqr_wave_opt.h.  An instantiation
    that list does not name would compile that kernel a second time, here."""
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "i2lqr_wave_opt.s"
    subprocess.run([HIPCC, *FLAGS, "-o", str(out), str(CSRC / "i2lqr_wave_opt.hip")], check=True,
                   capture_output=True, timeout=900)
    symbols = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", out.read_text(), flags=re.M)
    assert symbols == [], f"compiled into the launcher's unit (no extern template declaration?): {symbols}"
