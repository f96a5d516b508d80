"""GPU tests of "lane_models" (include/i2lqr.h): k_lane_iterate_model through the C-ABI — several
obstacle records per problem and the state box on the one-problem-per-lane kernel, batch-minor and
batch-tiled.

Off is off, disabled records are inert and a far box is no box, against the plain lane kernels bit
for bit (the far box: as numbers).  K > 1 and a finite bound are compared with
opt_in_reference.reference on the 67-problem sets test_obstacles_host.py / test_state_box_host.py
show to be well conditioned, and on the two 128-problem sets of opt_in_cases.TILED
(test_lane_models_host.py).  Tolerances and the 97 % rule: opt_in_gpu.compare.

The N = 64 sets: no lane kernel has a recorded error at that horizon, so the bound is taken in the
test from the plain lane kernel against the oracle's composition at one record (ten times its
batch_rel_err on X and U, or TOL_SOLVE if that is larger).  Measured on the MI355X: see DESIGN.md §4."""
import functools

import numpy as np
import pytest

from helpers import TOL_SOLVE, batch_rel_err, check_solve_outputs, dev_batch, to_host
from opt_in_cases import BOX_RUNS, OBS_RUNS, SEED, TILED, TILED_RUNS, make_case
from opt_in_gpu import LANE_BOX_NAME as BOX_NAME
from opt_in_gpu import LANE_OBS_NAME as OBS_NAME
from opt_in_gpu import OUTPUTS, checked_lane_solver, compare, lane_solver, records, run, same_bits
from opt_in_reference import Box, first_record_only, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def _reference(case, n_iters, boxed, layout=0):
    """reference() of a RECORDS entry, or (boxed) of a BOXES entry with its box."""
    cfg, host, box = make_case(case, box=boxed, layout=layout)
    return reference(cfg, host, box=box, max_iter=n_iters, early_exit=n_iters is None)


def _model_solver(cfg, host, box=None, layout=1, **options):
    """A model handle for the records of `host` and the box, its names and the shape of obs checked."""
    solver = checked_lane_solver(cfg, host, box, layout, **options)
    B, K = host["X"].shape[0], records(host)
    if K:
        assert solver.shape("obs", B) == ((6, K, B) if layout == 1 else (B // 64, 6, K, 64))
    return solver


def test_off_is_off(torch_mod):
    from ilqr_iterative_tasks_amd.solver import I2lqrError
    cfg, host, box = make_case("b6", box=True)
    B = host["X"].shape[0]
    plain = lane_solver(cfg, models=False)
    names = plain.iterate_kernel(B), plain.solve_kernel(B)
    assert not any("(" in name for name in names)
    # without the option the refusals are today's
    with pytest.raises(I2lqrError, match="obstacles.*problem-major"):
        plain.set_option("obstacles", 2)
    with pytest.raises(I2lqrError, match="state box.*problem-major"):
        plain.set_state_box(box.lo, box.hi)
    for value in (0, -1):
        plain.set_option("lane_models", value)
        with pytest.raises(I2lqrError, match="obstacles.*problem-major"):
            plain.set_option("obstacles", 2)
    want = {n: run(plain, host, n) for n in (6, None)}
    # on, with no model set: the plain kernels
    solver = lane_solver(cfg)
    assert (solver.iterate_kernel(B), solver.solve_kernel(B)) == names
    for n in (6, None):
        same_bits(torch_mod, run(solver, host, n), want[n])
    # a model on, then cleared: the names and the bits return
    solver.set_option("obstacles", 3)
    assert solver.iterate_kernel(B) == solver.solve_kernel(B) == OBS_NAME
    solver.set_state_box(box.lo, box.hi)
    assert solver.iterate_kernel(B) == solver.solve_kernel(B) == BOX_NAME
    solver.set_option("obstacles", 1)
    assert solver.iterate_kernel(B) == BOX_NAME and solver.shape("obs", B) == (6, B)
    solver.set_state_box()
    assert (solver.iterate_kernel(B), solver.solve_kernel(B)) == names
    for n in (6, None):
        same_bits(torch_mod, run(solver, host, n), want[n])
    solver.set_option("lane_models", 0)
    assert (solver.iterate_kernel(B), solver.solve_kernel(B)) == names


def _plain_batch(case, layout):
    """(cfg, host with obs[B, 6]): the 67 problems of the set, or the 128 under the tiled sets."""
    return make_case(case)[:2] if layout == 1 else make_case(case + "_T128", layout=2)[:2]


@pytest.mark.parametrize("layout", [1, 2])
@pytest.mark.parametrize("case", ["b4", "b6"])
def test_disabled_records_are_inert(torch_mod, case, layout):
    """One enabled record in slot 0 of two and in slot 1 of three is that obstacle's k_lane_iterate,
    bit for bit: a wrong record stride in either layout, a wrong record index or a first record read
    twice would show (the disabled records hold other obstacles' numbers, not zeros)."""
    from ilqr_iterative_tasks_amd import workloads
    cfg, host = _plain_batch(case, layout)
    other = workloads.obstacles_on_path(host, 3, 11)
    other[..., 5] = -1.0
    single = dict(host, obs=np.ascontiguousarray(workloads.obstacles_on_path(host, 1, 7)[:, 0]))
    assert (single["obs"][:, 5] >= 0).all()
    middle = other.copy()
    middle[:, 1] = single["obs"]
    first = other[:, :2].copy()
    first[:, 0] = single["obs"]
    plain = lane_solver(cfg, layout=layout, models=False)
    for n in (6, None):
        want = run(plain, single, n)
        for recs in (middle, first):
            batch = dict(host, obs=recs)
            same_bits(torch_mod, run(_model_solver(cfg, batch, layout=layout), batch, n), want)


@pytest.mark.parametrize("layout", [1, 2])
def test_null_obs_is_no_obstacle(torch_mod, layout):
    cfg, host = _plain_batch("b6", layout)
    host = dict(host, obs=None)
    want = run(lane_solver(cfg, layout=layout, models=False), host, 5)
    solver = lane_solver(cfg, layout=layout, obstacles=2)
    assert solver.iterate_kernel(host["X"].shape[0]) == OBS_NAME
    same_bits(torch_mod, run(solver, host, 5), want)


@pytest.mark.parametrize("case", ["b4", "b6"])
def test_a_far_box_is_no_box(torch_mod, case):
    """Bounds of +-1e6 on every component make every barrier term exactly zero: the outputs are the
    plain lane kernel's, with two records the K = 2 model kernel's — as numbers (adding an exact
    zero may turn -0.0 into +0.0).  A term added to the wrong element would show."""
    from ilqr_iterative_tasks_amd import workloads
    cfg, host, _ = make_case(case)
    far = Box(cfg.n, {i: (-1e6, 1e6) for i in range(cfg.n)})
    two = dict(host, obs=workloads.obstacles_on_path(host, 2, 7))
    for batch, base in ((host, lane_solver(cfg, models=False)), (two, _model_solver(cfg, two))):
        boxed = _model_solver(cfg, batch, far)
        for n in (6, None):
            want, got = run(base, batch, n), run(boxed, batch, n)
            for key in OUTPUTS:
                assert torch_mod.equal(got[key], want[key]), (key, n, records(batch))


def _check_records(case, n_iters):
    assert (case, n_iters) in OBS_RUNS
    cfg, host, _ = make_case(case)
    solver = _model_solver(cfg, host)
    buf = run(solver, host, n_iters)
    compare(solver, buf, _reference(case, n_iters, False), n_iters)
    return solver, cfg, host, buf


def _check_box(case, n_iters):
    assert (case, n_iters, 1) in BOX_RUNS
    cfg, host, box = make_case(case, box=True)
    solver = _model_solver(cfg, host, box)
    assert solver.state_box is not None
    buf = run(solver, host, n_iters)
    compare(solver, buf, _reference(case, n_iters, True), n_iters)
    return solver, cfg, host, buf


@pytest.mark.parametrize("case", ["b4_K2", "b4_weights_K2", "b6_K3"])
def test_records_fixed_iterations_match_the_reference(torch_mod, case):
    _check_records(case, 6)


@pytest.mark.parametrize("case", ["b4_N1_K2", "b4_N7_K2", "b6_B1_K3", "b6_B5_K2", "b4_K8"])
def test_records_horizon_batch_and_count_edges_match_the_reference(torch_mod, case):
    _check_records(case, 5)


@pytest.mark.parametrize("case", ["b4", "b4_hi_only", "b4_weights", "b6", "b4_K2"])
def test_box_fixed_iterations_match_the_reference(torch_mod, case):
    _check_box(case, 6)


@pytest.mark.parametrize("case", ["b4_N1", "b6_N1", "b4_N7", "b6_B1", "b6_B5"])
def test_box_horizon_and_batch_edges_match_the_reference(torch_mod, case):
    _check_box(case, 5)


@pytest.mark.parametrize("case", ["b4_K2", "b6_K2"])
def test_records_solve_to_termination_matches_the_reference(torch_mod, case):
    solver, cfg, host, buf = _check_records(case, None)
    check_solve_outputs(solver, cfg, host, buf)


@pytest.mark.parametrize("case", ["b4", "b6"])
def test_box_solve_to_termination_matches_the_reference(torch_mod, case):
    solver, cfg, host, buf = _check_box(case, None)
    check_solve_outputs(solver, cfg, host, buf)


@pytest.mark.parametrize("name", TILED)
def test_tiled_sets_match_the_reference(torch_mod, name):
    """The batch-tiled layout, two wavefronts: the records for 6 iterations, records and box solved."""
    cfg, host, box = make_case(name, box=True, layout=2)
    assert [r[1:] for r in TILED_RUNS if r[0] == name] == [(6, False), (None, True)]
    solver = _model_solver(cfg, host, layout=2)
    compare(solver, run(solver, host, 6), _reference(name, 6, False, layout=2), 6)
    solver = _model_solver(cfg, host, box, layout=2)
    buf = run(solver, host, None)
    compare(solver, buf, _reference(name, None, True, layout=2), None)
    check_solve_outputs(solver, cfg, host, buf)


def _errors(solver, buf, ref):
    """(X, U) batch_rel_err on the problems that took the reference's branches, as compare picks
    them: all iterations run, at least 97 % with the reference's lamb, their status words equal."""
    same = buf["lamb"].cpu().numpy() == ref["lamb"]
    assert (buf["iters"].cpu().numpy() == 5).all()
    assert same.mean() >= 0.97, f"{(~same).sum()} of {len(same)} problems took a different branch"
    assert (buf["status"].cpu().numpy()[same] == ref["status"][same]).all()
    return (batch_rel_err(to_host(solver, buf["X"])[same], ref["X"][same]),
            batch_rel_err(to_host(solver, buf["U"])[same], ref["U"][same]))


@pytest.mark.parametrize("case,boxed", [("b4_N64_K3", False), ("b4_N64", True)])
def test_long_horizon_error_is_the_plain_lane_kernels(torch_mod, case, boxed):
    """N = 64: the model kernel's error on X and U against its reference is at most ten times the
    plain lane kernel's against the oracle's composition at one record on the same batch (the
    extra records and the box add terms of the same size and kind), or TOL_SOLVE if that is larger."""
    cfg, host, box = make_case(case, box=boxed)
    one, ref = host if boxed else first_record_only(host), _reference(case, 5, boxed)
    plain = lane_solver(cfg, models=False)
    base = _errors(plain, run(plain, one, 5), reference(cfg, one, max_iter=5, early_exit=False))
    solver = _model_solver(cfg, host, box)
    got = _errors(solver, run(solver, host, 5), ref)
    print(f"{case}: plain lane kernel X {base[0]:.3e} U {base[1]:.3e}; "
          f"model kernel X {got[0]:.3e} U {got[1]:.3e}")
    for mine, plain_err in zip(got, base):
        assert mine <= max(10.0 * plain_err, TOL_SOLVE)


@pytest.mark.parametrize("K", [3, 8])
def test_scheduling_options_keep_the_bits(torch_mod, K):
    """"defer_states" x "reroll_nominal", "merge_inputs" and no LDS-resident gain steps against the
    automatic choice, with a box and K records: the records' LDS overlapping the gain steps would
    show; K = 8 leaves the fewest gain steps."""
    from ilqr_iterative_tasks_amd import workloads
    cfg, host, box = make_case("b6", box=True)
    host = make_case("b6_K3")[1] if K == 3 else dict(host, obs=workloads.obstacles_on_path(host, 8, SEED))
    variants = [dict(defer_states=d, reroll_nominal=r) for d in (0, 1) for r in (0, 1)]
    variants += [dict(merge_inputs=1), dict(lds_gain_steps=0), dict(stagger=2)]
    for n in (6, None):
        base = _model_solver(cfg, host, box)
        want = run(base, host, n)
        for options in variants + [dict(helper_wavefront=1, checkpoint_states=1, state_buffers=1)]:
            same_bits(torch_mod, run(_model_solver(cfg, host, box, **options), host, n), want)


@pytest.mark.parametrize("layout", [1, 2])
def test_fp32_outputs_are_consistent(torch_mod, layout):
    if layout == 1:
        cfg, host, _ = make_case("b6_K2", dtype="f32")
        _, plain_host, box = make_case("b6", box=True, dtype="f32")
    else:
        cfg, host, box = make_case("b6_T128_K3", box=True, dtype="f32", layout=2)
        plain_host = first_record_only(host)
    for batch, bx in ((host, None), (plain_host, box)):
        solver = _model_solver(cfg, batch, bx, layout=layout)
        buf = run(solver, batch, 6)
        check_solve_outputs(solver, cfg, batch, buf, early_exit=False, n_iters=6)
        buf = run(solver, batch, None)
        check_solve_outputs(solver, cfg, batch, buf)


def test_names_and_refusals(torch_mod):
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config
    from ilqr_iterative_tasks_amd.solver import I2lqrError
    cfg, host, box = make_case("b6_K2", box=True)
    B = host["X"].shape[0]
    solver = lane_solver(cfg, obstacles=2)
    assert solver.iterate_kernel(B) == solver.solve_kernel(B) == OBS_NAME
    solver.set_state_box(box.lo, box.hi)  # the box takes precedence
    assert solver.iterate_kernel(B) == solver.solve_kernel(B) == BOX_NAME
    # a problem-major handle has the wavefront kernels: 1 is refused, 0 / -1 are accepted
    major = BatchedILQR(cfg)
    with pytest.raises(I2lqrError, match="lane_models"):
        major.set_option("lane_models", 1)
    major.set_option("lane_models", 0)
    major.set_option("lane_models", -1)
    with pytest.raises(I2lqrError, match="lane_models"):
        solver.set_option("lane_models", 2)
    # off with a model on: the message names what to clear first
    with pytest.raises(I2lqrError, match="lane_models.*state box"):
        solver.set_option("lane_models", 0)
    solver.set_state_box()
    with pytest.raises(I2lqrError, match="lane_models.*obstacles"):
        solver.set_option("lane_models", 0)
    assert solver.iterate_kernel(B) == OBS_NAME  # a refused switch leaves the handle as it was
    with pytest.raises(I2lqrError, match="obstacles"):
        solver.set_option("obstacles", 9)
    # the other opt-in models stay with the one-problem-per-wavefront kernel
    with pytest.raises(I2lqrError, match="line_search"):
        solver.set_option("line_search", 4)
    with pytest.raises(I2lqrError, match="barrier_cost"):
        solver.set_option("barrier_cost", 1)
    with pytest.raises(I2lqrError, match="wave_chain"):
        solver.set_option("wave_chain", 1)
    buf = dev_batch(solver, host)
    with pytest.raises(I2lqrError, match="obstacles"):
        solver.backward(buf["X"], buf["U"], buf["x_term"], buf["lamb"], buf["obs"])
    solver.set_option("obstacles", 1)
    solver.set_state_box(box.lo, box.hi)
    with pytest.raises(I2lqrError, match="state box"):
        solver.backward(buf["X"], buf["U"], buf["x_term"], buf["lamb"], None)
    # quad12: the row-block kernel has no models
    quad = BatchedILQR(default_config("quad12", 10, dt=0.02, layout=1))
    quad.set_option("lane_models", 1)
    with pytest.raises(I2lqrError, match="obstacles.*quad12"):
        quad.set_option("obstacles", 2)
    with pytest.raises(I2lqrError, match="state box.*quad12"):
        quad.set_state_box(hi=[np.inf, np.inf, 0.05] + [np.inf] * 9)
    assert quad.iterate_kernel(64) == "k_lane_iterate_rows"


def test_solve_stays_a_single_launch(torch_mod):
    """4160 problems (above the automatic compaction threshold): solve() with and without
    set_compaction(64) returns the same bits — the chunked solve has no models and is not taken."""
    from ilqr_iterative_tasks_amd import default_config, workloads
    cfg = default_config("bicycle6", 20, dt=0.25)
    host = workloads.make_batch(cfg, 4160)
    host = dict(host, obs=workloads.obstacles_on_path(host, 2, SEED))
    solver = _model_solver(cfg, host)
    want = run(solver, host, None)
    check_solve_outputs(solver, cfg, host, want)
    solver.set_compaction(64)
    assert solver.solve_kernel(4160) == OBS_NAME
    same_bits(torch_mod, run(solver, host, None), want)
