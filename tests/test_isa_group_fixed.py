"""CPU suite: the compiled gfx950 code of the fixed-horizon form of the sixteen-lane kernel
(k_group_iterate_fixed, csrc/i2lqr_group_fixed.hip).  Its fast passes are straight-line code on
purpose; its general passes and the entry rollout must have stayed loops — unrolled as well they
made the kernel 2.9 times the size of the run-time-horizon one, which the size cap below catches.
Compiles two translation units to ISA with hipcc (cross-compiles without a GPU), side by side."""
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ilqr_iterative_tasks_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
         "--cuda-device-only"]
# k_group_iterate_fixed<double, Bicycle6<double>, 3, 20> / k_group_iterate<double, Bicycle6<double>, 3, false, 16>
FIXED = "_ZN5i2lqr21k_group_iterate_fixedIdNS_8Bicycle6IdEELi3ELi20EEE"
RUNTIME = "_ZN5i2lqr15k_group_iterateIdNS_8Bicycle6IdEELi3ELb0ELi16EEE"


def _isa(tu: str, out_dir: Path) -> str:
    out = out_dir / (tu + ".s")
    subprocess.run([HIPCC, *FLAGS, "-o", str(out), str(CSRC / (tu + ".hip"))], check=True,
                   capture_output=True, timeout=900)
    return out.read_text()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("isa_fixed")
    with ThreadPoolExecutor(2) as ex:
        a, b = ex.map(lambda tu: _isa(tu, d), ["i2lqr_group_fixed", "i2lqr_group"])
    return {"fixed": a, "group": b}


def _kernel_text(text: str, prefix: str) -> str:
    """The listing of the first kernel whose symbol starts with prefix, up to the resource comments
    behind its .Lfunc_end."""
    lines = text.split("\n")
    start = next((i for i, l in enumerate(lines) if l.startswith(prefix) and ":" in l), None)
    assert start is not None, f"no kernel symbol starting with {prefix} in the ISA listing"
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    stop = next((i for i in range(end, len(lines)) if lines[i].startswith("; ScratchSize")), None)
    assert stop is not None, "no resource comments behind the kernel"
    return "\n".join(lines[start:stop + 1])


def _field(kernel_text: str, name: str) -> int:
    m = re.search(r"^; " + re.escape(name) + r"\s*[:=]\s*(\d+)", kernel_text, flags=re.M)
    assert m, name
    return int(m.group(1))


def _metadata_scratch(text: str, prefix: str) -> int:
    """.private_segment_fixed_size of the kernel in the code object's metadata (amdhsa.kernels)."""
    meta = text[text.index("amdhsa.kernels"):]
    entries = re.split(r"\n  - \.", meta)
    mine = [e for e in entries if re.search(r"\.name:\s+" + re.escape(prefix), e)]
    assert len(mine) == 1, (prefix, len(mine))
    m = re.search(r"\.private_segment_fixed_size:\s*(\d+)", mine[0])
    assert m
    return int(m.group(1))


def test_the_headline_fixed_kernel_exists_without_scratch(isa):
    k = _kernel_text(isa["fixed"], FIXED)
    assert _metadata_scratch(isa["fixed"], FIXED) == 0
    assert _field(k, "ScratchSize") == 0
    assert not re.findall(r"^\s+scratch_", k, flags=re.M)


def test_the_fixed_kernels_keep_the_dpp_wait_states(isa):
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_dpp_hazard",
                                                  ROOT / "tools" / "check_dpp_hazard.py")
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    found, bad = lint.check(_kernel_text(isa["fixed"], FIXED))
    assert not bad, bad[:5]
    assert found > 100
    found_all, bad_all = lint.check(isa["fixed"])  # every instantiation of the translation unit
    assert not bad_all, bad_all[:5]
    assert found_all >= found


def test_only_the_fast_passes_are_unrolled(isa):
    """codeLenInByte below twice that of the run-time-horizon kernel compiled in the same run: the
    straight-line fast passes add about half of it again (1.4 x on the compiler this was written
    on), unrolled general passes gave 2.9 x."""
    fixed = _field(_kernel_text(isa["fixed"], FIXED), "codeLenInByte")
    runtime = _field(_kernel_text(isa["group"], RUNTIME), "codeLenInByte")
    print(f"codeLenInByte: fixed {fixed}, run-time {runtime}, ratio {fixed / runtime:.2f}")
    assert fixed < 2 * runtime, (fixed, runtime)
