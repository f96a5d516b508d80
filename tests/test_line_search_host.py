"""CPU suite of the "line_search" option: the host reference the GPU tests compare with
(opt_in_reference.reference with the oracle's backward pass) is the oracle's ilqr() at one step
size, every problem set the GPU tests use is well conditioned (its step choices and lamb survive a
perturbation of x0 far above the kernels' round-off), the sets take short steps, and the header
documents the option."""
import functools
from pathlib import Path

import numpy as np
import pytest

from opt_in_cases import LS_RUNS, candidate_case, make_case
from opt_in_reference import OUTPUTS, reference, short_step_share

ROOT = Path(__file__).resolve().parent.parent


@functools.lru_cache(maxsize=None)
def _reference(case, A, n_iters, scale=1.0):
    cfg, host = make_case(case)[:2] if case != "candidates" else candidate_case()[::4]
    host = dict(host, X=host["X"] * scale)  # (only X[:, :, 0] = x0 is non-zero)
    return reference(cfg, host, A, oracle_backward=True, max_iter=n_iters,
                     early_exit=n_iters is None)


@pytest.mark.parametrize("n_iters", [None, 6])
@pytest.mark.parametrize("case", ["b4_weights", "b4", "b6", "quad12"])
def test_one_step_size_is_the_oracles_ilqr_bit_for_bit(case, n_iters):
    from oracle import oracle as orc
    cfg, host, _ = make_case(case)
    want = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"],
                          max_iter=n_iters, early_exit=n_iters is None)
    got = _reference(case, 1, n_iters)
    for key in OUTPUTS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert (got["jstar"] <= 0).all()


RUNS = list(LS_RUNS) + [("candidates", 4, None, 0.0)]


@pytest.mark.parametrize("case,A,n_iters,share", RUNS,
                         ids=[f"{c}-A{a}-{'solve' if i is None else i}" for c, a, i, _ in RUNS])
def test_gpu_cases_are_well_conditioned_and_take_short_steps(case, A, n_iters, share):
    """A kernel that differs from the reference by round-off (1e-16 relative per operation) must
    meet the same accept / reject and step decisions: they do not move when x0 is scaled by
    1 + 1e-13 or 1 - 1e-12."""
    ref = _reference(case, A, n_iters)
    for scale in (1.0 + 1e-13, 1.0 - 1e-12):
        per = _reference(case, A, n_iters, scale)
        assert np.array_equal(per["jstar"], ref["jstar"]), scale
        assert np.array_equal(per["lamb"], ref["lamb"]), scale
        assert np.array_equal(per["iters"], ref["iters"]), scale
    got = short_step_share(ref)
    print(f"{case} A={A}: short steps in {got:.0%} of the problems, "
          f"status 3 in {(ref['status'] == 3).mean():.1%}, mean iterations {ref['iters'].mean():.1f}")
    if share is None:
        assert (ref["jstar"] <= 0).all()
    else:
        assert got >= share, got


def test_header_documents_the_option_and_the_kernel_name():
    hdr = (ROOT / "include" / "i2lqr.h").read_text()
    assert '"line_search"' in hdr
    assert '"k_iterate (line search)"' in hdr
    src = (ROOT / "ilqr_iterative_tasks_amd" / "csrc" / "i2lqr_abi.hip").read_text()
    assert '!strcmp(name, "line_search")' in src and "wave_kernel_name(" in src
    # (the names of the opt-in forms are written once, in the model's header)
    model = (ROOT / "ilqr_iterative_tasks_amd" / "csrc" / "i2lqr_wave_model.hpp").read_text()
    assert '"k_iterate (line search)"' in model
