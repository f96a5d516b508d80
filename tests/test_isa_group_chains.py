"""CPU suite: the record code of the headline kernel, k_group_iterate_fixed<double, Bicycle6, 3, 20>
(csrc/i2lqr_group_fixed.hip), in its compiled gfx950 form.  With "group_chains" on (the default) a
helper wavefront forms a record — three exponentials, two reciprocals — with the chains side by
side (GroupWorker::prep_chains): the record must have stayed ONE basic block, and its Horner steps
three-address multiply-adds with the coefficients read from scalar registers, not a v_mov_b64 +
v_fmac_f64 pair each.  Reads the listing the build writes (csrc/_obj/i2lqr_group_fixed.s) where it
is newer than the sources, and compiles the unit to ISA otherwise (hipcc cross-compiles without a
GPU)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ilqr_iterative_tasks_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
         "--cuda-device-only"]
FIXED = "_ZN5i2lqr21k_group_iterate_fixedIdNS_8Bicycle6IdEELi3ELi20EEE"
# the markers GroupWorker::prep_chains<true> leaves around a record (comments in the listing)
BEGIN, END = "; record, short input barrier", "; record end, short input barrier"


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    built = CSRC / "_obj" / "i2lqr_group_fixed.s"
    sources = [*CSRC.glob("*.hpp"), *CSRC.glob("*.h"), CSRC / "i2lqr_group_fixed.hip"]
    if built.exists() and built.stat().st_mtime >= max(p.stat().st_mtime for p in sources):
        text = built.read_text()
    else:
        if not Path(HIPCC).exists():
            pytest.skip("hipcc not available")
        out = tmp_path_factory.mktemp("isa_chains") / "i2lqr_group_fixed.s"
        subprocess.run([HIPCC, *FLAGS, "-o", str(out), str(CSRC / "i2lqr_group_fixed.hip")],
                       check=True, capture_output=True, timeout=900)
        text = out.read_text()
    lines = text.split("\n")
    start = next((i for i, l in enumerate(lines) if l.startswith(FIXED) and ":" in l), None)
    assert start is not None, "the headline kernel is not in the listing"
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [l.strip() for l in lines[start:end]]


def _records(kernel):
    """The instruction lines of every default-path record of the kernel: (position, lines)."""
    out = []
    for i, l in enumerate(kernel):
        if l == BEGIN:
            j = next((k for k in range(i, len(kernel)) if kernel[k] == END), None)
            assert j is not None, "a record without its end marker"
            out.append((i, [x for x in kernel[i + 1:j]
                            if x and not x.startswith(";;#ASM") and not x.startswith("; ")]))
    return out


def test_the_helpers_record_lies_between_their_two_barriers(kernel):
    """The helper loop: barrier B1, the record, barrier B2, back to B1.  In the listing the loop is
    rotated (B2 and B1 stand in front of the record's block), so: the record's block is part of a
    loop whose header is the block that starts with s_barrier."""
    recs = _records(kernel)
    assert len(recs) == 1, len(recs)  # N = 20, two helpers: one record per lane, no round loop
    pos = recs[0][0]
    header = next((m.group(1) for l in kernel[:pos][::-1]
                   if (m := re.search(r"in Loop: Header=(BB\d+_\d+)", l))), None)
    assert header, "the record is not inside a loop"
    at = next(i for i, l in enumerate(kernel) if l.startswith(f".L{header}:"))
    assert kernel[at + 1].startswith("s_barrier"), kernel[at:at + 3]
    assert sum(l.startswith("s_barrier") for l in kernel[at - 8:at + 2]) == 2  # B2, then B1


def test_a_record_is_one_basic_block(kernel):
    """No branch and no label between the first record load and the last record store, and the
    block is the whole record: its loads, three exponentials (v_ldexp_f64 ends each), the two
    reciprocals of the short input barrier, its stores."""
    for pos, rec in _records(kernel):
        loads = [i for i, l in enumerate(rec) if l.startswith("ds_read")]
        stores = [i for i, l in enumerate(rec) if l.startswith("ds_write")]
        assert loads and stores, pos
        body = rec[loads[0]:stores[-1] + 1]
        assert not [l for l in body if l.startswith(("s_cbranch", "s_branch", "s_setpc"))], pos
        assert not [l for l in rec if l.startswith(".LBB")], pos
        assert sum(l.startswith("v_ldexp_f64") for l in body) == 3, pos
        assert sum(l.startswith("v_rcp_f64") for l in body) == 2, pos


def test_the_horner_steps_of_a_record_copy_no_coefficient(kernel):
    """At most two v_mov_b64 in a record (the serial form has about thirty: one in front of every
    v_fmac_f64 of its three exponentials), and the 3 x 10 middle Horner steps are v_fma_f64 with
    the coefficient in a scalar register pair."""
    for pos, rec in _records(kernel):
        movs = [l for l in rec if l.startswith("v_mov_b64")]
        print(f"record at line {pos}: {len(rec)} instructions, {len(movs)} v_mov_b64")
        assert len(movs) <= 2, movs
        horner = [l for l in rec if re.match(r"v_fma_f64 v\[\d+:\d+\], v\[\d+:\d+\], v\[\d+:\d+\], "
                                             r"s\[\d+:\d+\]$", l)]
        assert len(horner) >= 30, len(horner)
