"""GPU parity tests: the HIP path, called through the C-ABI, against
  (a) golden vectors captured from the reference itself (tests/golden, n=4 m=2), and
  (b) the CPU oracle on identical seeded inputs (all systems), and
  (c) size-independent properties at BASELINE.json's full batch sizes.

Tolerances (fp64): function level 1e-10 rel (G1), whole ilqr() 1e-8 rel with identical iteration
counts and lamb_out (G2-G4) — SURVEY.md §8c: a 1e-13 perturbation of x0 already moves the
reference's own output by 3.4e-9 (chaotic amplification through up to 150 iterations).
"""
import numpy as np
import pytest

from helpers import (TOL_SOLVE, batch_rel_err, check_flipped, check_solve_against_calls,
                     check_solve_outputs, dev_batch, rel_err, to_dev, to_host)

pytestmark = pytest.mark.gpu

TOL_FUNC = 1e-10   # one backward / forward pass, fp64 (TOL_SOLVE, the whole ilqr(): helpers.py)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a HIP device"
    return torch


# problem-major with one problem per wavefront ("wave"), eight problems per wavefront ("group": the
# automatic choice for the bicycles with Q = R = 0 above 4096 problems) or four ("row16": sixteen
# lanes per problem, DPP row broadcasts instead of LDS exchanges; automatic from 1024 to 4096
# problems); batch-minor / batch-tiled: one per lane
LAYOUTS = {"wave": 0, "group": 0, "row16": 0, "spec": 0, "lane": 1, "tiled": 2}
GROUP_LANES = {"wave": 64, "group": 8, "row16": 16, "spec": 8}


@pytest.fixture(params=["wave", "group", "row16", "spec", "lane"])
def layout(request):
    return request.param


def pin_kernel(solver, layout):
    """Problem-major solvers: pin the fused kernels to the family the test names ("spec": the
    speculative form of the eight-lane kernel)."""
    if layout in GROUP_LANES:
        solver.set_option("group_lanes", GROUP_LANES[layout])
        solver.set_option("speculate", 1 if layout == "spec" else 0)
    return solver


def make_solver(system, N, dtype="f64", dt=1.0, layout="wave", **over):
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config
    if layout in ("group", "row16", "spec") and system == "quad12":
        pytest.skip("the eight-lane kernels and their sixteen-lane DPP form are built for the m = 2 plants")
    if layout == "spec" and N > 20:
        pytest.skip("the speculative kernel's buffers fit the LDS up to N = 20 for the bicycles")
    cfg = default_config(system, N, dtype, dt=dt, layout=LAYOUTS[layout])
    for key, val in over.items():
        setattr(cfg, key, val)
    return pin_kernel(BatchedILQR(cfg), layout), cfg


def oracle():
    from oracle import oracle as orc
    return orc


# ------------------------------------------------------------------------------------------------
# (a) golden vectors from the reference
# ------------------------------------------------------------------------------------------------

def test_backward_forward_match_reference_g1(torch_mod, golden_dir, layout):
    g = np.load(golden_dir / "g1_first_iteration.npz")
    solver, cfg = make_solver("bicycle4", 6, layout=layout)
    X, U = to_dev(solver, g["X"]), to_dev(solver, g["U"])
    xt, lamb, obs = to_dev(solver, g["x_term"]), to_dev(solver, g["lamb"]), to_dev(solver, g["obs"])
    k, K = solver.backward(X, U, xt, lamb, obs)
    assert batch_rel_err(to_host(solver, K), g["K"]) < TOL_FUNC
    assert batch_rel_err(to_host(solver, k), g["k"]) < TOL_FUNC
    Xn, Un, cn = solver.forward(X, U, xt, to_dev(solver, g["K"]), to_dev(solver, g["k"]))
    assert batch_rel_err(to_host(solver, Xn), g["X_new"]) < TOL_FUNC
    assert batch_rel_err(to_host(solver, Un), g["U_new"]) < TOL_FUNC
    np.testing.assert_allclose(cn.cpu().numpy(), g["cost_new"], rtol=TOL_FUNC)


def _check_solve_against_calls(g, N, layout, tol=TOL_SOLVE, max_flips=0):
    solver, cfg = make_solver("bicycle4", N, layout=layout)
    return check_solve_against_calls(solver, g, N, tol, max_flips)


def test_solve_matches_reference_g2(torch_mod, golden_dir, layout):
    """384 ilqr() calls of the config-1 closed loop, lamb_in from 1e-29 to 1e4, 1..150 iterations."""
    g = np.load(golden_dir / "g2_ilqr_calls.npz")
    buf = _check_solve_against_calls(g, 6, layout)
    st = buf["status"].cpu().numpy()
    assert set(np.unique(st)) <= {1, 2, 3}
    assert ((st == 2) == (g["iters"] == 150)).all() or (g["iters"] == 150).sum() >= (st == 2).sum()


def test_solve_matches_reference_g3_scenarios(torch_mod, golden_dir, layout):
    """none / static x3 / moving up / moving left obstacles of iterative_ilqr/result/*.py."""
    g = np.load(golden_dir / "g3_scenarios.npz")
    _check_solve_against_calls(g, 6, layout)


@pytest.mark.parametrize("N", [2, 6, 20, 50])
def test_solve_matches_reference_g4_horizons(torch_mod, golden_dir, N, layout):
    g = np.load(golden_dir / f"g4_horizon_N{N}.npz")
    _check_solve_against_calls(g, N, layout)
    # first-iteration gains at this horizon
    solver, cfg = make_solver("bicycle4", N, layout=layout)
    B = len(g["x0"])
    k, K = solver.backward(to_dev(solver, g["first_X"]), to_dev(solver, g["first_U"]),
                           to_dev(solver, g["x_term"]), to_dev(solver, np.ones(B)),
                           to_dev(solver, g["obs"]))
    assert batch_rel_err(to_host(solver, K), g["first_K"]) < TOL_FUNC
    assert batch_rel_err(to_host(solver, k), g["first_k"]) < TOL_FUNC


def test_dynamics_known_answer_g7(torch_mod, golden_dir, layout):
    """rollout of get_traj()'s input schedule reproduces data/closed_loop_feasible.txt (6 decimals,
    utils/base.py:103-138)."""
    g = np.load(golden_dir / "g7_dynamics.npz")
    traj, ucl = g["closed_loop_feasible"], g["ucl"].copy()
    # reference quirk: get_traj() starts its input log with `ucl = u` (an alias of the array it
    # keeps mutating, utils/base.py:132), so the recorded row 0 holds step 1's steering angle;
    # the input actually applied at i = 0 is accel = 1, delta = 0 (utils/base.py:111-128)
    ucl[0] = [1.0, 0.0]
    N = 60
    solver, cfg = make_solver("bicycle4", N, layout=layout)
    x_start = traj[0]  # exactly zero; the second half starts from the computed (unrounded) state
    for s in (0, 60):
        X = np.zeros((1, 4, N + 1))
        X[0, :, 0] = x_start
        U = np.ascontiguousarray(ucl[s:s + N].T[None])
        Xd, Ud = to_dev(solver, X), to_dev(solver, U)
        solver.rollout(Xd, Ud, to_dev(solver, traj[s + N][None]))
        got = to_host(solver, Xd)[0].T
        assert np.abs(got - traj[s:s + N + 1]).max() <= 0.5e-6 + 1e-9  # "%f" rounding only
        x_start = got[-1]


# ------------------------------------------------------------------------------------------------
# (b) oracle on identical seeded inputs
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("system,N,dt,B", [("bicycle4", 6, 1.0, 257), ("bicycle6", 20, 0.25, 1024),
                                           ("quad12", 50, 0.02, 96)])
def test_function_level_vs_oracle(torch_mod, system, N, dt, B, layout):
    from ilqr_iterative_tasks_amd import workloads
    orc = oracle()
    solver, cfg = make_solver(system, N, dt=dt, layout=layout)
    host = workloads.make_batch(cfg, B)
    # a non-trivial nominal: random inputs inside the box, rolled out
    rng = np.random.default_rng(7)
    scale = 0.02 if system == "quad12" else 1.0  # keep the quadrotor away from the Euler singularity
    host["U"] = (rng.uniform(-1, 1, host["U"].shape) * scale *
                 np.array(cfg.u_max[:cfg.m])[None, :, None])
    host["lamb"] = 10.0 ** rng.integers(-6, 3, B).astype(float)
    Xr, Ur, cr = orc.rollout_batch(cfg, host["X"], host["U"], host["x_term"])
    Xd, Ud, xt = to_dev(solver, host["X"]), to_dev(solver, host["U"]), to_dev(solver, host["x_term"])
    cost = solver.rollout(Xd, Ud, xt)
    assert batch_rel_err(to_host(solver, Xd), Xr) < 1e-11
    np.testing.assert_allclose(cost.cpu().numpy(), cr, rtol=1e-11)
    ko, Ko = orc.backward_batch(cfg, Xr, Ur, host["x_term"], host["lamb"], host["obs"])
    Xd, Ud = to_dev(solver, Xr), to_dev(solver, Ur)
    k, K = solver.backward(Xd, Ud, xt, to_dev(solver, host["lamb"]), to_dev(solver, host["obs"]))
    assert batch_rel_err(to_host(solver, K), Ko) < 1e-9
    assert batch_rel_err(to_host(solver, k), ko) < 1e-9
    Xn_o, Un_o, cn_o = orc.forward_batch(cfg, Xr, Ur, host["x_term"], Ko, ko)
    Xn, Un, cn = solver.forward(Xd, Ud, xt, to_dev(solver, Ko), to_dev(solver, ko))
    assert batch_rel_err(to_host(solver, Xn), Xn_o) < 1e-11
    assert batch_rel_err(to_host(solver, Un), Un_o) < 1e-11
    np.testing.assert_allclose(cn.cpu().numpy(), cn_o, rtol=1e-10)


@pytest.mark.parametrize("system,N,dt,B,iters", [("bicycle6", 20, 0.25, 1024, 10),
                                                 ("bicycle4", 6, 1.0, 512, 10),
                                                 ("quad12", 50, 0.02, 64, 4)])
def test_iterate_vs_oracle(torch_mod, system, N, dt, B, iters, layout):
    """BASELINE configs[1] (B=1024, n=6, m=2, N=20, fp64): 10 fused iterations, no early exit."""
    from ilqr_iterative_tasks_amd import workloads
    orc = oracle()
    solver, cfg = make_solver(system, N, dt=dt, layout=layout)
    host = workloads.make_batch(cfg, B)
    ref = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"],
                         max_iter=iters, early_exit=False)
    buf = solver.iterate(dev_batch(solver, host), iters)
    assert (buf["iters"].cpu().numpy() == iters).all()
    lamb = buf["lamb"].cpu().numpy()
    same = lamb == ref["lamb"]
    # an accept/reject decided by a cost difference at round-off level may flip; it must be rare
    assert same.mean() > 0.99, f"{(~same).sum()} of {B} problems took a different branch"
    # ... and where it flips the two branches are equally good: same cost to 1e-6
    check_flipped(buf, ref, same, 1e-6, early_exit=False)
    assert (buf["status"].cpu().numpy()[same] == ref["status"][same]).all()
    for key in ("X", "U"):
        assert batch_rel_err(to_host(solver, buf[key])[same], ref[key][same]) < TOL_SOLVE, key
    np.testing.assert_allclose(buf["cost"].cpu().numpy()[same], ref["cost"][same], rtol=1e-7)
    # gains of the LAST of the fused iterations: K at 1e-6; the feed-forward k -> 0 at a converged
    # solution, so it is compared at the scale of the input box (function-level parity of K, k is
    # pinned at 1e-10 by the G1 / function-level tests above)
    assert batch_rel_err(to_host(solver, buf["K"])[same], ref["K"][same]) < 1e-6
    assert batch_rel_err(to_host(solver, buf["k"])[same], ref["k"][same], floor=1.0) < 1e-6


def test_solve_vs_oracle_bicycle6(torch_mod, layout):
    from ilqr_iterative_tasks_amd import workloads
    orc = oracle()
    solver, cfg = make_solver("bicycle6", 20, dt=0.25, layout=layout)
    host = workloads.make_batch(cfg, 512)
    ref = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"])
    buf = solver.solve(dev_batch(solver, host))
    check_solve_outputs(solver, cfg, host, buf)
    same = (buf["iters"].cpu().numpy() == ref["iters"]) & (buf["lamb"].cpu().numpy() == ref["lamb"])
    assert same.mean() > 0.98
    # a flipped problem may stop one iteration earlier or later than the oracle: its cost is then
    # within the convergence threshold eps (control/iterative_ilqr.py:78) of the oracle's
    check_flipped(buf, ref, same, cfg.eps, early_exit=True)
    assert (buf["status"].cpu().numpy()[same] == ref["status"][same]).all()
    assert batch_rel_err(to_host(solver, buf["X"])[same], ref["X"][same]) < TOL_SOLVE
    assert batch_rel_err(to_host(solver, buf["U"])[same], ref["U"][same]) < 1e-7


# fp32 (BASELINE configs[2]) against the fp64 oracle.  fp32 is narrower than the reference's
# arithmetic, so this is a stated accuracy, not bit parity:
#   one backward pass   K: median 1e-4, k: 5e-3 of the input box (24-bit mantissa through a 20-step
#                       Riccati recursion whose value function spans 4 decades)
#   iterate(10), solve  returned cost within FP32_COST (relative, or relative to the batch's median
#                       initial cost for targets reached to ~0) on FP32_AGREE of the problems
#                       (measured: 99 %) and within 5e-2 on all;
#                       U within FP32_U of the input box (max |u_max|) on FP32_AGREE of the problems;
#                       solve(): exit status equal on FP32_AGREE of the problems; iteration counts
#                       equal on FP32_ITERS of them (measured 94.3 %: at a converged solution
#                       `cost_new < cost` compares values that agree to fp32 round-off, the tie goes
#                       either way and the lamb schedule then exits a few iterations apart) and
#                       never more than 24 apart; every status a legal exit.
FP32_COST, FP32_U, FP32_AGREE, FP32_ITERS = 1e-3, 1e-2, 0.95, 0.92


def _fp32_vs_oracle(solver, cfg, buf, ref, counts, count_share=True):
    """count_share=False (test_gpu_fp32_parity.py, bicycle4): without the share of equal iteration
    counts, FP32_ITERS; everything else, their largest distance included, as stated above."""
    B = len(ref["cost"])
    cost = buf["cost"].double().cpu().numpy()
    assert np.isfinite(cost).all()
    rel = np.abs(cost - ref["cost"]) / np.maximum(np.abs(ref["cost"]), 1e-30)
    # problems that have converged to cost ~ 0 (a reachable target): compare absolutely at the
    # scale of the batch's typical initial cost instead
    scale = np.median(ref["cost0"]) if "cost0" in ref else 1.0
    rel = np.minimum(rel, np.abs(cost - ref["cost"]) / scale)
    assert (rel <= FP32_COST).mean() >= FP32_AGREE, (rel <= FP32_COST).mean()
    assert rel.max() <= 5e-2, rel.max()
    box = max(list(cfg.u_max)[:cfg.m])
    du = np.abs(to_host(solver, buf["U"]).astype(np.float64) - ref["U"]).reshape(B, -1).max(1) / box
    assert (du <= FP32_U).mean() >= FP32_AGREE, (du <= FP32_U).mean()
    st = buf["status"].cpu().numpy()
    assert set(np.unique(st)) <= ({1, 2, 3} if counts else {0, 1, 3}), np.unique(st)
    if counts:
        it = buf["iters"].cpu().numpy()
        if count_share:
            assert (it == ref["iters"]).mean() >= FP32_ITERS, (it == ref["iters"]).mean()
        assert np.abs(it - ref["iters"]).max() <= 24
        assert it.min() >= 1 and it.max() <= cfg.max_iter
        assert (st == ref["status"]).mean() >= FP32_AGREE


@pytest.mark.parametrize("lay", ["wave", "group", "row16", "lane", "tiled"])
def test_fp32_tracks_fp64_oracle(torch_mod, lay):
    """BASELINE configs[2] (n=6, m=2, N=20, fp32) inputs: one backward pass, 10 fused iterations
    and the solve to termination in fp32 against the fp64 oracle, tolerances above."""
    from ilqr_iterative_tasks_amd import workloads
    orc = oracle()
    solver, cfg = make_solver("bicycle6", 20, "f32", dt=0.25, layout=lay)
    B = 2048
    host = workloads.make_batch(cfg, B)
    Xr, Ur, cr = orc.rollout_batch(cfg, host["X"], host["U"], host["x_term"])
    ko, Ko = orc.backward_batch(cfg, Xr, Ur, host["x_term"], host["lamb"], host["obs"])
    k, K = solver.backward(to_dev(solver, Xr), to_dev(solver, Ur), to_dev(solver, host["x_term"]),
                           to_dev(solver, host["lamb"]), to_dev(solver, host["obs"]))
    assert np.median(np.abs(to_host(solver, K) - Ko).reshape(B, -1).max(1) /
                     np.abs(Ko).reshape(B, -1).max(1)) < 1e-4
    box = max(list(cfg.u_max)[:cfg.m])
    assert np.abs(to_host(solver, k) - ko).max() / box < 5e-3
    ref = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"],
                         max_iter=10, early_exit=False)
    ref["cost0"] = cr
    buf = solver.iterate(dev_batch(solver, host), 10)
    assert (buf["iters"].cpu().numpy() == 10).all()
    check_solve_outputs(solver, cfg, host, buf, early_exit=False, n_iters=10)
    _fp32_vs_oracle(solver, cfg, buf, ref, counts=False)
    ref = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"])
    ref["cost0"] = cr
    buf = solver.solve(dev_batch(solver, host))
    check_solve_outputs(solver, cfg, host, buf)
    _fp32_vs_oracle(solver, cfg, buf, ref, counts=True)


def test_relax_cost_and_argmin_vs_oracle(torch_mod, layout):
    from ilqr_iterative_tasks_amd import workloads
    orc = oracle()
    solver, cfg = make_solver("bicycle4", 6, layout=layout)
    B = 4099
    host = workloads.make_batch(cfg, B)
    rng = np.random.default_rng(3)
    X = host["X"].copy()
    X[:, :, -1] = host["x_term"] + rng.normal(0, 1, (B, 4)) * 10.0 ** rng.integers(-3, 4, (B, 1))
    X[5, 0, -1] = np.nan
    qfun = rng.integers(0, 120, B).astype(np.int32)
    for outer in (0, 1, 2):
        want = orc.relax_cost_batch(cfg, X, host["x_term"], qfun, outer)
        got = solver.relax_cost(to_dev(solver, X), to_dev(solver, host["x_term"]),
                                to_dev(solver, qfun), outer)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        idx, val = solver.argmin(got)
        assert int(idx.item()) == int(np.argmin(want))  # first index on ties, like list.index(min)
        assert float(val.item()) == float(np.min(want))


@pytest.mark.parametrize("B", [1, 7, 1027, 4099, 8200])
def test_iterate_pick_equals_iterate_relax_argmin(torch_mod, layout, B):
    """i2lqr_iterate_pick — one launch on the eight- / sixteen-lane kernels (relaxed cost in the
    kernel's exit block, pick by a last-workgroup-done reduction), the three steps as launches on
    the other families — against i2lqr_iterate + i2lqr_relax_cost + i2lqr_argmin and the oracle's
    relaxed cost (utils/base.py:427-437, :462-465): every output bit for bit, empty slots
    (I2LQR_QF_NONE) and non-finite candidates included, repeated launches (the ticket word of the
    reduction resets itself), costs without the pick."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    orc = oracle()
    solver, cfg = make_solver("bicycle4", 6, layout=layout)
    host = workloads.make_batch(cfg, B)
    rng = np.random.default_rng(B)
    qfun = rng.integers(0, 120, B).astype(np.int32)
    qfun[rng.integers(0, B, max(1, B // 9))] = 0x7FFFFFFF
    if B > 5:
        host["x_term"][5, 0] = np.nan
    q = to_dev(solver, qfun)
    for outer in (0, 1, 2, 0):
        a = solver.iterate(dev_batch(solver, host), 4)
        cost_a = solver.relax_cost(a["X"], a["x_term"], q, outer)
        idx_a, val_a = solver.argmin(cost_a)
        b = dev_batch(solver, host)
        cost_b, (idx_b, val_b) = solver.iterate_pick(b, 4, q, outer)
        for key in ("X", "U", "K", "k", "lamb", "cost", "iters", "status"):  # (NaN == NaN here)
            assert torch.equal(a[key].isnan(), b[key].isnan()), (key, outer)
            assert torch.equal(a[key].nan_to_num(7.0), b[key].nan_to_num(7.0)), (key, outer)
        assert torch.equal(cost_a.isnan(), cost_b.isnan())
        assert torch.equal(cost_a.nan_to_num(-1.0), cost_b.nan_to_num(-1.0)), outer
        assert int(idx_a.item()) == int(idx_b.item()) and float(val_a.item()) == float(val_b.item())
        want = orc.relax_cost_batch(cfg, to_host(solver, a["X"]), host["x_term"], qfun, outer)
        want[qfun == 0x7FFFFFFF] = np.inf  # empty candidate slots (a concept of this build)
        np.testing.assert_array_equal(cost_b.cpu().numpy(), want)
        assert int(idx_b.item()) == int(np.argmin(want))
        c = dev_batch(solver, host)
        cost_c, none = solver.iterate_pick(c, 4, q, outer, pick=False)
        assert none is None and torch.equal(cost_c.nan_to_num(-1.0), cost_b.nan_to_num(-1.0))
    if B >= 1024 and layout in ("group", "row16"):
        assert solver.iterate_kernel(B).startswith("k_group_iterate")


# ------------------------------------------------------------------------------------------------
# (c) size-independent properties at full batch sizes, edge cases
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,B", [("f64", 65536), ("f32", 65536)])
def test_properties_full_size(torch_mod, dtype, B, layout):
    """BASELINE configs[2]/[3] sizes: determinism, composition iterate(4)+iterate(6) == iterate(10)
    bit-exactly, returned X is the rollout of returned U, returned cost is its terminal cost."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    solver, cfg = make_solver("bicycle6", 20, dtype, dt=0.25, layout=layout)
    host = workloads.make_batch(cfg, B)
    a = solver.iterate(dev_batch(solver, host), 10)
    b = solver.iterate(dev_batch(solver, host), 10)
    for key in ("X", "U", "lamb", "cost", "K", "k"):
        assert torch.equal(a[key], b[key]), key
    c = solver.iterate(dev_batch(solver, host), 4)
    c = solver.iterate(c, 6)
    for key in ("X", "U", "lamb", "cost", "K", "k"):
        assert torch.equal(a[key], c[key]), key
    X2, U2 = a["X"].clone(), a["U"].clone()
    cost2 = solver.rollout(X2, U2, a["x_term"])
    assert torch.equal(U2, a["U"])            # clipping is idempotent
    assert torch.equal(X2, a["X"])            # same dynamics code path, bit-exact
    assert torch.equal(cost2, a["cost"])      # Q = R = 0: cost is the terminal cost
    assert torch.isfinite(a["cost"]).all()
    assert (a["cost"] >= 0).all()
    u_max = torch.tensor(list(cfg.u_max)[:cfg.m], dtype=solver.dtype, device=solver.device)
    assert (solver.to_problem_major(a["U"]).abs() <= u_max[None, :, None]).all()
    check_solve_outputs(solver, cfg, host, a, early_exit=False, n_iters=10)


@pytest.mark.parametrize("lay,B", [("wave", 131072), ("group", 131072), ("row16", 131072),
                                   ("lane", 131072),
                                   ("tiled", 131072), ("lane", 1 << 20), ("tiled", 1 << 20)])
def test_config4_sizes_properties_and_oracle_sample(torch_mod, lay, B):
    """BASELINE configs[3]: 2^20 problems over 8 GPUs = 131072 per GPU, and the whole 2^20 on one
    (fp64, n=6, m=2, N=20).  Size-independent properties over the full batch — determinism, returned
    X is bit-exactly the rollout of returned U, cost is its terminal cost, inputs inside the box,
    every problem ran exactly 10 iterations — and the CPU oracle on a strided sample of 512
    problems that spans the whole index range, so the row addressing above 65536 problems
    (offsets beyond 2^31 bytes in the batch-minor gains at 2^20) is checked against known answers."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    solver, cfg = make_solver("bicycle6", 20, "f64", dt=0.25, layout=lay)
    host = workloads.make_batch(cfg, B)
    a = solver.iterate(dev_batch(solver, host), 10)
    b = solver.iterate(dev_batch(solver, host), 10)
    for key in ("X", "U", "lamb", "cost", "K", "k"):
        assert torch.equal(a[key], b[key]), key
    del b
    assert int(a["iters"].min()) == 10 == int(a["iters"].max())
    X2, U2 = a["X"].clone(), a["U"].clone()
    cost2 = solver.rollout(X2, U2, a["x_term"])
    assert torch.equal(U2, a["U"]) and torch.equal(X2, a["X"]) and torch.equal(cost2, a["cost"])
    del X2, U2
    assert torch.isfinite(a["cost"]).all() and (a["cost"] >= 0).all()
    u_max = torch.tensor(list(cfg.u_max)[:cfg.m], dtype=solver.dtype, device=solver.device)
    Upm = solver.to_problem_major(a["U"])
    assert (Upm.abs() <= u_max[None, :, None]).all()
    del Upm
    check_solve_outputs(solver, cfg, host, a, early_exit=False, n_iters=10)
    # strided sample incl. the last problem
    idx = np.unique(np.concatenate([np.arange(0, B, B // 511), [B - 1]]))
    ref = oracle().ilqr_batch(cfg, host["X"][idx], host["U"][idx], host["x_term"][idx],
                              host["lamb"][idx], host["obs"][idx], max_iter=10, early_exit=False)
    tidx = torch.as_tensor(idx, device=solver.device)
    got = {key: solver.to_problem_major(a[key])[tidx].cpu().numpy() for key in ("X", "U", "K", "k")}
    sub = {key: a[key][tidx] for key in ("lamb", "cost", "status")}
    same = sub["lamb"].cpu().numpy() == ref["lamb"]
    assert same.mean() > 0.99
    check_flipped(sub, ref, same, 1e-6, early_exit=False)
    for key in ("X", "U"):
        assert batch_rel_err(got[key][same], ref[key][same]) < TOL_SOLVE, key
    np.testing.assert_allclose(sub["cost"].cpu().numpy()[same], ref["cost"][same], rtol=1e-7)
    assert batch_rel_err(got["K"][same], ref["K"][same]) < 1e-6
    assert batch_rel_err(got["k"][same], ref["k"][same], floor=1.0) < 1e-6
    # the solve to termination (chunked + compaction + wave tail on the lane layouts) on the same
    # batch: every problem ends with a legal status, the sample matches the oracle
    s = solver.solve(dev_batch(solver, host, want_gains=False))
    st = s["status"].cpu().numpy()
    assert set(np.unique(st)) <= {1, 2, 3}
    check_solve_outputs(solver, cfg, host, s)
    ref = oracle().ilqr_batch(cfg, host["X"][idx], host["U"][idx], host["x_term"][idx],
                              host["lamb"][idx], host["obs"][idx])
    it = s["iters"][tidx].cpu().numpy()
    same = (it == ref["iters"]) & (s["lamb"][tidx].cpu().numpy() == ref["lamb"])
    assert same.mean() > 0.98
    check_flipped({key: s[key][tidx] for key in ("cost", "status")},
                   ref, same, cfg.eps, early_exit=True)
    Xs = solver.to_problem_major(s["X"])[tidx].cpu().numpy()
    assert batch_rel_err(Xs[same], ref["X"][same]) < TOL_SOLVE


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_tiled_layout_is_bit_identical_to_batch_minor(torch_mod, dtype):
    """The batch-tiled layout runs the same kernels on re-based pointers: results must be
    bit-identical to the batch-minor layout; a ragged batch is rejected."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    from ilqr_iterative_tasks_amd.solver import I2lqrError
    s_l, cfg = make_solver("bicycle6", 20, dtype, dt=0.25, layout="lane")
    s_t, _ = make_solver("bicycle6", 20, dtype, dt=0.25, layout="tiled")
    host = workloads.make_batch(cfg, 4096)
    a = s_l.solve(dev_batch(s_l, host))
    b = s_t.solve(dev_batch(s_t, host))
    for key in ("X", "U", "K", "k"):
        assert torch.equal(s_l.to_problem_major(a[key]), s_t.to_problem_major(b[key])), key
    for key in ("lamb", "cost", "iters", "status"):
        assert torch.equal(a[key], b[key]), key
    c1 = s_l.relax_cost(a["X"], a["x_term"], torch.zeros(4096, dtype=torch.int32, device=s_l.device), 1)
    c2 = s_t.relax_cost(b["X"], b["x_term"], torch.zeros(4096, dtype=torch.int32, device=s_t.device), 1)
    assert torch.equal(c1, c2)
    # the stand-alone phases too
    for s_, buf in ((s_l, a), (s_t, b)):
        buf["k2"], buf["K2"] = s_.backward(buf["X"], buf["U"], buf["x_term"], buf["lamb"], buf["obs"])
        buf["Xn"], buf["Un"], buf["cn"] = s_.forward(buf["X"], buf["U"], buf["x_term"], buf["K2"],
                                                     buf["k2"])
        buf["X3"], buf["U3"] = buf["Xn"].clone(), buf["Un"].clone()
        buf["c3"] = s_.rollout(buf["X3"], buf["U3"], buf["x_term"])
    for key in ("k2", "K2", "Xn", "Un", "X3", "U3"):
        assert torch.equal(s_l.to_problem_major(a[key]), s_t.to_problem_major(b[key])), key
    assert torch.equal(a["cn"], b["cn"]) and torch.equal(a["c3"], b["c3"])
    with pytest.raises((ValueError, I2lqrError)):
        s_t.alloc(100)


@pytest.mark.parametrize("system,N,dt,dtype", [("bicycle4", 50, 1.0, "f64"), ("bicycle6", 20, 0.25, "f32"),
                                               ("bicycle4", 6, 1.0, "f32")])
def test_wave_tail_other_plants_and_precisions(torch_mod, system, N, dt, dtype):
    """The automatic chunked solve (compaction + one-problem-per-wavefront tail) against the single
    launch on the other plant, a long horizon and fp32: identical statuses, iteration counts equal
    on all but 1-2 % of the problems in fp32 (accept / reject ties decided by round-off), trajectories
    within the precision's solve tolerance for the problems whose counts agree."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    solver, cfg = make_solver(system, N, dtype, dt=dt, layout="tiled")
    B = 4096
    host = workloads.make_batch(cfg, B)
    solver.set_compaction(0)
    plain = solver.solve(dev_batch(solver, host))
    solver.set_compaction(-1)
    auto = solver.solve(dev_batch(solver, host))
    it_p, it_a = plain["iters"].cpu().numpy(), auto["iters"].cpu().numpy()
    same = it_p == it_a
    assert same.mean() >= (1.0 if dtype == "f64" else 0.97), same.mean()
    assert it_a.min() >= 1 and (auto["status"].cpu().numpy() != 0).all()
    tol = TOL_SOLVE if dtype == "f64" else 2e-3
    for key in ("X", "U"):
        a, b = to_host(solver, plain[key])[same], to_host(solver, auto[key])[same]
        assert batch_rel_err(b, a, floor=1e-2) < tol, key


@pytest.mark.parametrize("lay,gains", [("lane", True), ("tiled", False)])
def test_chunked_solve_with_wave_tail_matches_oracle_and_plain(torch_mod, lay, gains):
    """Chunked solve with the latency tail on the one-problem-per-wavefront kernel ("wave_tail"):
    problems that survive the first chunks are finished by a different kernel (same algorithm,
    different summation order), so the outputs are compared at the solve tolerance (1e-8) with the
    oracle and with the plain single-launch solve, iteration counts and statuses exactly."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    solver, cfg = make_solver("bicycle6", 20, "f64", dt=0.25, layout=lay)
    B = 4096
    host = workloads.make_batch(cfg, B)
    host["lamb"] = 10.0 ** np.random.default_rng(3).integers(-3, 3, B).astype(float)
    plain = solver.solve(dev_batch(solver, host, want_gains=gains))
    solver.set_compaction(1024)
    solver.set_option("wave_tail", 2048)
    tail = solver.solve(dev_batch(solver, host, want_gains=gains))
    check_solve_outputs(solver, cfg, host, tail)
    it_p, it_t = plain["iters"].cpu().numpy(), tail["iters"].cpu().numpy()
    assert it_t.max() > 16, "the workload must have a tail for this test to mean anything"
    assert (it_p == it_t).all() and torch.equal(plain["status"], tail["status"])
    for key in ("X", "U") + (("K", "k") if gains else ()):
        a, b = to_host(solver, plain[key]), to_host(solver, tail[key])
        floor = 1.0 if key == "k" else 1e-2
        assert batch_rel_err(b, a, floor=floor) < (1e-6 if key in ("K", "k") else TOL_SOLVE), key
    assert rel_err(tail["lamb"].cpu().numpy(), plain["lamb"].cpu().numpy()) == 0.0
    want = oracle().ilqr_batch(cfg, host["X"][:512], host["U"][:512], host["x_term"][:512],
                               host["lamb"][:512], host["obs"][:512])
    assert (want["iters"] == it_t[:512]).all()
    assert batch_rel_err(to_host(solver, tail["X"])[:512], want["X"]) < TOL_SOLVE
    assert batch_rel_err(to_host(solver, tail["U"])[:512], want["U"], floor=1e-2) < TOL_SOLVE


@pytest.mark.parametrize("system,N,dt", [("bicycle6", 20, 0.25), ("bicycle4", 50, 1.0)])
def test_per_step_jacobians_option_is_bit_identical(torch_mod, system, N, dt):
    """One-problem-per-wavefront kernel: with "per_step_jacobians" the [A | B] matrices come from
    the parallel per-step phase instead of the refresh inside the serial recursion — same
    arithmetic, so iterate() and solve() must agree bit for bit with the option forced off."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    solver, cfg = make_solver(system, N, dt=dt, layout="wave")  # pins "group_lanes" to 64
    host = workloads.make_batch(cfg, 512)
    out = {}
    for flag in (0, 1, -1):
        solver.set_option("per_step_jacobians", flag)
        out[flag] = (solver.iterate(dev_batch(solver, host), 6), solver.solve(dev_batch(solver, host)))
    for flag in (1, -1):
        for got, want in zip(out[flag], out[0]):
            for key in ("X", "U", "K", "k", "lamb", "cost", "iters", "status"):
                assert torch.equal(got[key], want[key]), (key, flag)


@pytest.mark.parametrize("lay,dtype", [("lane", "f64"), ("tiled", "f64"), ("tiled", "f32")])
def test_lane_scheduling_options_do_not_change_results(torch_mod, lay, dtype):
    """i2lqr_set_option: deferred state stores, nominal re-roll and the number of LDS-resident gain
    steps only move work around — every combination must reproduce, bit for bit, the plain
    configuration (states read back, candidate written in place, no gains in LDS), for the fused
    iterations and for the solve; an unknown option is an error."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    from ilqr_iterative_tasks_amd.solver import I2lqrError
    solver, cfg = make_solver("bicycle6", 20, dtype, dt=0.25, layout=lay)
    host = workloads.make_batch(cfg, 2048)

    def run(defer, reroll, lds, merge=-1, ckpt=-1):
        solver.set_option("defer_states", defer)
        solver.set_option("reroll_nominal", reroll)
        solver.set_option("lds_gain_steps", lds)
        solver.set_option("merge_inputs", merge)
        solver.set_option("checkpoint_states", ckpt)
        it = solver.iterate(dev_batch(solver, host), 7)
        so = solver.solve(dev_batch(solver, host))
        return it, so

    ref_it, ref_so = run(0, 0, 0)
    for defer, reroll, lds, merge, ckpt in ((1, 1, -1, 1, 0), (1, 0, 3, 0, -1), (0, 1, -1, -1, -1),
                                            (-1, -1, -1, -1, -1), (1, 1, 2, 0, 1), (1, 1, -1, 1, 1),
                                            (1, 1, 1, 1, 1)):
        it, so = run(defer, reroll, lds, merge, ckpt)
        for got, want in ((it, ref_it), (so, ref_so)):
            for key in ("X", "U", "K", "k", "lamb", "cost", "iters", "status"):
                assert torch.equal(got[key], want[key]), (key, defer, reroll, lds, merge, ckpt)
    with pytest.raises(I2lqrError):
        solver.set_option("no_such_option", 1)


@pytest.mark.parametrize("lay,dtype,gains", [("lane", "f64", True), ("lane", "f32", False),
                                             ("tiled", "f64", False), ("tiled", "f32", True)])
def test_chunked_compacting_solve_is_bit_identical_to_plain(torch_mod, lay, dtype, gains):
    """Opt-in chunked solve (i2lqr_set_compaction): chunks of 4, 4, 4, 4, 8, ... iterations with the
    surviving problems packed between chunks (k_lane_compact).  Every output must equal, bit for
    bit, the plain single-launch solve (taken here on sub-batches of 2048, below the threshold),
    and the iteration counts must match the oracle's."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    solver, cfg = make_solver("bicycle6", 20, dtype, dt=0.25, layout=lay)
    B, sub = 8192, 2048
    solver.set_compaction(4096)
    solver.set_option("wave_tail", 0)  # the tail kernel is tested separately (tolerance, not bits)
    host = workloads.make_batch(cfg, B)
    host["lamb"] = 10.0 ** np.random.default_rng(1).integers(-3, 3, B).astype(float)
    big = solver.solve(dev_batch(solver, host, want_gains=gains))
    check_solve_outputs(solver, cfg, host, big)
    keys = ("X", "U") + (("K", "k") if gains else ())
    for lo in range(0, B, sub):
        part = {key: (val[lo:lo + sub] if val is not None else None) for key, val in host.items()}
        ref = solver.solve(dev_batch(solver, part, want_gains=gains))
        for key in keys:
            assert torch.equal(solver.to_problem_major(big[key])[lo:lo + sub],
                               solver.to_problem_major(ref[key])), (key, lo)
        for key in ("lamb", "cost", "iters", "status"):
            assert torch.equal(big[key][lo:lo + sub], ref[key]), (key, lo)
    it = big["iters"].cpu().numpy()
    assert it.min() >= 1 and it.max() > 16 and (big["status"].cpu().numpy() != 0).all()
    if dtype == "f64":
        want = oracle().ilqr_batch(cfg, host["X"][:512], host["U"][:512], host["x_term"][:512],
                                   host["lamb"][:512], host["obs"][:512])
        assert (it[:512] == want["iters"]).mean() > 0.98
    # without an obstacle array as well
    host2 = dict(host)
    host2["obs"] = None
    b2 = dev_batch(solver, host2, want_gains=False)
    solver.solve(b2)
    part = {key: (val[:sub] if val is not None else None) for key, val in host2.items()}
    r2 = solver.solve(dev_batch(solver, part, want_gains=False))
    assert torch.equal(solver.to_problem_major(b2["X"])[:sub], solver.to_problem_major(r2["X"]))
    assert torch.equal(b2["iters"][:sub], r2["iters"])


@pytest.mark.parametrize("lay,B", [("tiled", 192), ("lane", 131)])
def test_quad12_chunked_solve_on_the_lane_layouts_is_bit_identical_to_plain(torch_mod, lay, B):
    """The row-block kernel (k_lane_iterate_rows) as a chunk of the chunked solve: it enters with
    the iteration counts of the earlier chunks, skips what has terminated since and leaves through
    the compaction, fused into its exit or as a launch of its own.  Three wavefronts on the
    batch-tiled layout, two and a ragged tail on the batch-minor one; chunks of two iterations,
    no tail kernel.  Every output must equal, bit for bit, the single launch of the same handle."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    solver, cfg = make_solver("quad12", 10, "f64", dt=0.02, layout=lay)
    assert solver.solve_kernel(B) == "k_lane_iterate_rows"
    host = workloads.make_batch(cfg, B)
    host["lamb"] = 10.0 ** np.random.default_rng(4).integers(-3, 3, B).astype(float)
    solver.set_compaction(0)
    plain = solver.solve(dev_batch(solver, host))
    check_solve_outputs(solver, cfg, host, plain)
    it = plain["iters"].cpu().numpy()
    # chunks of two iterations: a problem with more than four enters a third chunk (so max_iter is
    # above the first chunk too, without which set_compaction(64) would take the single launch)
    assert cfg.max_iter > 4 and B >= 64
    assert it.max() > 4 and len(np.unique(it)) > 2, "several chunks, problems leaving in each"
    solver.set_compaction(64)
    solver.set_option("wave_tail", 0)
    solver.set_option("first_chunk", 2)
    solver.set_option("chunk_step", 2)
    for fused in (1, 0):
        solver.set_option("fused_compaction", fused)
        got = solver.solve(dev_batch(solver, host))
        for key in ("X", "U", "K", "k", "lamb", "cost", "iters", "status"):
            assert torch.equal(got[key], plain[key]), (key, fused)


def test_edge_cases(torch_mod, layout):
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    from ilqr_iterative_tasks_amd.solver import I2lqrError
    orc = oracle()
    # empty batch
    solver, cfg = make_solver("bicycle4", 6, layout=layout)
    solver.solve(solver.alloc(0))
    # ragged batch sizes, B = 1
    for B in (1, 3, 65):
        host = workloads.make_batch(cfg, B)
        ref = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"])
        buf = solver.solve(dev_batch(solver, host))
        assert (buf["iters"].cpu().numpy() == ref["iters"]).all()
        assert batch_rel_err(to_host(solver, buf["X"]), ref["X"]) < TOL_SOLVE
    # no obstacle at all (NULL obs) == every record disabled
    host = workloads.make_batch(cfg, 64)
    b1 = dev_batch(solver, host)
    b1["obs"] = None
    host2 = dict(host)
    host2["obs"] = host["obs"].copy()
    host2["obs"][:, 5] = -1
    b2 = dev_batch(solver, host2)
    solver.solve(b1), solver.solve(b2)
    assert torch.equal(b1["X"], b2["X"]) and torch.equal(b1["lamb"], b2["lamb"])
    # gains may be skipped
    b3 = dev_batch(solver, host2, want_gains=False)
    solver.solve(b3)
    assert torch.equal(b3["X"], b2["X"])
    # non-finite input: a status word, not an error
    host3 = workloads.make_batch(cfg, 8)
    host3["x_term"][2, 0] = np.nan
    b4 = solver.solve(dev_batch(solver, host3))
    assert int(b4["status"][2]) == 4 and (b4["status"].cpu().numpy()[[0, 1, 3]] != 4).all()
    # horizon limits: N = 1 and N = 64 (I2LQR_MAX_HORIZON; the eight problem slices of the
    # eight-lane kernel fit the LDS up to N = 50 for this plant)
    for N in (1, {"group": 50, "spec": 20}.get(layout, 64)):  # (four slices of "row16" fit at 64)
        s2, c2 = make_solver("bicycle4", N, layout=layout)
        h = workloads.make_batch(c2, 33)
        ref = orc.ilqr_batch(c2, h["X"], h["U"], h["x_term"], h["lamb"], h["obs"], max_iter=5,
                             early_exit=False)
        out = s2.iterate(dev_batch(s2, h), 5)
        same = out["lamb"].cpu().numpy() == ref["lamb"]
        assert same.mean() > 0.9
        assert batch_rel_err(to_host(s2, out["X"])[same], ref["X"][same]) < TOL_SOLVE
    # argument errors are error codes -> RuntimeError, never crashes
    with pytest.raises(ValueError):
        solver.rollout(torch.zeros(2, 4, 6, dtype=torch.float64, device=solver.device),
                       torch.zeros(2, 2, 6, dtype=torch.float64, device=solver.device),
                       torch.zeros(2, 4, dtype=torch.float64, device=solver.device))
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config
    bad = default_config("bicycle4", 6)
    bad.N = 1000
    with pytest.raises(I2lqrError):
        BatchedILQR(bad)
    bad = default_config("bicycle4", 6)
    bad.n = 5
    with pytest.raises(RuntimeError):
        BatchedILQR(bad)


def test_group_kernel_selection_and_agreement_with_the_wave_kernel(torch_mod):
    """The speculative form ("speculate" 1) is bit-identical to the plain eight-lane kernel.
    "group_lanes": 8 (eight problems per wavefront) is the automatic choice for the bicycles with
    Q = R = 0 and agrees with 64 (one problem per wavefront) to round-off — K^T Quu K is
    associated differently — with identical iteration counts, statuses and lamb; where it is not
    built, forcing it is an error and the automatic choice falls back."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads
    from ilqr_iterative_tasks_amd.solver import I2lqrError
    for system, N, dt, B in (("bicycle6", 20, 0.25, 1027), ("bicycle4", 6, 1.0, 77),
                             ("bicycle4", 50, 1.0, 9)):
        cfg = default_config(system, N, "f64", dt=dt)
        solver = BatchedILQR(cfg)
        host = workloads.make_batch(cfg, B)
        host["lamb"] = 10.0 ** np.random.default_rng(5).integers(-3, 3, B).astype(float)
        out = {}
        solver.set_option("speculate", 0)
        for lanes in (64, 8, 16, -1):
            solver.set_option("group_lanes", lanes)
            out[lanes] = (solver.iterate(dev_batch(solver, host), 7), solver.solve(dev_batch(solver, host)))
        # the automatic choice: sixteen lanes per problem up to 4096 problems (where its four slices
        # fit the LDS: bicycle4 at N = 50 does), eight lanes above
        auto = 16
        assert solver.iterate_kernel(B) == "k_group_iterate (sixteen lanes)"
        assert solver.iterate_kernel(4097) == "k_group_iterate (sixteen lanes)"  # (no workspace registered)
        for a, b in zip(out[auto], out[-1]):
            for key in ("X", "U", "K", "k", "lamb", "cost", "iters", "status"):
                assert torch.equal(a[key], b[key]), (system, key)
        # the speculative form runs the same iterations in the same order: bit for bit the plain
        # eight-lane kernel, forced and as the automatic choice (<= 2048 problems)
        solver.set_option("group_lanes", 8)
        for spec in (1,):
            if N > 20:
                break  # the speculative buffers do not fit the LDS at this horizon
            solver.set_option("speculate", spec)
            assert solver.iterate_kernel(B) == "k_group_spec"
            got = (solver.iterate(dev_batch(solver, host), 7), solver.solve(dev_batch(solver, host)))
            for a, b in zip(got, out[8]):
                for key in ("X", "U", "K", "k", "lamb", "cost", "iters", "status"):
                    assert torch.equal(a[key], b[key]), (system, key, spec)
        for nit in (1, 2, 3, 4):  # iteration caps that cut a chain of rejects short
            if N > 20:
                break
            solver.set_option("speculate", 1)
            a = solver.iterate(dev_batch(solver, host), nit)
            solver.set_option("speculate", 0)
            b = solver.iterate(dev_batch(solver, host), nit)
            for key in ("X", "U", "K", "k", "lamb", "cost", "iters", "status"):
                assert torch.equal(a[key], b[key]), (system, key, nit)
        solver.set_option("speculate", 0)
        # eight lanes and sixteen lanes (Qux by the symmetry of Vxx, no gain exchange) against one
        # problem per wavefront: round-off apart
        for lanes in (8, 16):
            for a, b in zip(out[lanes], out[64]):
                same = (a["iters"] == b["iters"]) & (a["lamb"] == b["lamb"])
                assert float(same.double().mean()) >= 0.99, (system, lanes)
                assert torch.equal(a["status"][same], b["status"][same])
                sm = same.cpu().numpy()
                for key in ("X", "U"):
                    assert batch_rel_err(to_host(solver, a[key])[sm], to_host(solver, b[key])[sm],
                                         floor=1e-2) < TOL_SOLVE, (system, key, lanes)
    # stage weights: the automatic choice falls back, forcing is an error
    cfg = default_config("bicycle4", 6)
    cfg.set_matrix("R", np.diag([0.05, 0.05]))
    solver = BatchedILQR(cfg)
    host = workloads.make_batch(cfg, 16)
    solver.iterate(dev_batch(solver, host), 2)
    solver.set_option("group_lanes", 8)
    with pytest.raises(I2lqrError, match="group_lanes"):
        solver.iterate(dev_batch(solver, host), 2)
    q = BatchedILQR(default_config("quad12", 10, dt=0.02))
    q.set_option("group_lanes", 8)
    with pytest.raises(I2lqrError, match="group_lanes"):
        q.iterate(dev_batch(q, workloads.make_batch(q.cfg, 4)), 1)
    with pytest.raises(I2lqrError):
        q.set_option("group_lanes", 32)
    # a horizon whose eight problem slices do not fit the LDS: automatic falls back, forcing fails
    big = BatchedILQR(default_config("bicycle4", 64))
    hb = workloads.make_batch(big.cfg, 5)
    big.iterate(dev_batch(big, hb), 2)
    big.set_option("group_lanes", 8)
    with pytest.raises(I2lqrError, match="group_lanes"):
        big.iterate(dev_batch(big, hb), 2)


@pytest.mark.parametrize("B,iters", [(67, 4), (1, 3), (256, 6)])
def test_quad12_sixteen_lane_kernel_vs_oracle_and_wave_kernel(torch_mod, B, iters):
    """BASELINE configs[4] shape (n=12, m=4, N=50, fp64): "group_lanes" 16 — four problems per
    wavefront, each lane a column of the Riccati blocks, records / gains / candidate in the HBM
    workspace — against the CPU oracle (fused iterations and the solve to termination, ragged batch
    sizes) and against the one-problem-per-wavefront kernel.  It is the automatic choice once the
    workspace is registered (BatchedILQR does that)."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads
    orc = oracle()
    cfg = default_config("quad12", 50, "f64", dt=0.02)
    solver = BatchedILQR(cfg)
    host = workloads.make_batch(cfg, B)
    host["lamb"] = 10.0 ** np.random.default_rng(2).integers(-2, 2, B).astype(float)
    out = {}
    for lanes in (64, 16, -1):
        solver.set_option("group_lanes", lanes)
        out[lanes] = (solver.iterate(dev_batch(solver, host), iters), solver.solve(dev_batch(solver, host)))
        assert solver.iterate_kernel(B) == ("k_iterate" if lanes == 64 else "k_quad_iterate")
    for a, b in zip(out[16], out[-1]):  # automatic == 16 (workspace registered): bit for bit
        for key in ("X", "U", "K", "k", "lamb", "cost", "iters", "status"):
            assert torch.equal(a[key], b[key]), key
    ref_it = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"],
                            max_iter=iters, early_exit=False)
    ref_so = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"])
    for lanes in (16, 64):
        it, so = out[lanes]
        assert (it["iters"].cpu().numpy() == iters).all()
        check_solve_outputs(solver, cfg, host, it, early_exit=False, n_iters=iters)
        check_solve_outputs(solver, cfg, host, so)
        same = it["lamb"].cpu().numpy() == ref_it["lamb"]
        assert same.mean() >= 0.97, (lanes, same.mean())
        check_flipped(it, ref_it, same, 1e-6, early_exit=False)
        for key in ("X", "U"):
            assert batch_rel_err(to_host(solver, it[key])[same], ref_it[key][same]) < TOL_SOLVE, (lanes, key)
        np.testing.assert_allclose(it["cost"].cpu().numpy()[same], ref_it["cost"][same], rtol=1e-7)
        assert batch_rel_err(to_host(solver, it["K"])[same], ref_it["K"][same]) < 1e-6, lanes
        assert batch_rel_err(to_host(solver, it["k"])[same], ref_it["k"][same], floor=1.0) < 1e-6
        same = (so["iters"].cpu().numpy() == ref_so["iters"]) & (so["lamb"].cpu().numpy() == ref_so["lamb"])
        assert same.mean() >= 0.97, (lanes, same.mean())
        check_flipped(so, ref_so, same, cfg.eps, early_exit=True)
        assert (so["status"].cpu().numpy()[same] == ref_so["status"][same]).all()
        assert batch_rel_err(to_host(solver, so["X"])[same], ref_so["X"][same]) < TOL_SOLVE, lanes
    # without a registered workspace the automatic choice is the one-problem-per-wavefront kernel
    # and forcing sixteen lanes is an error
    import ctypes as C
    from ilqr_iterative_tasks_amd.solver import I2lqrError
    bare = BatchedILQR(cfg)
    assert bare.iterate_kernel(B) == "k_iterate"
    bare.set_option("group_lanes", 16)
    buf = dev_batch(bare, host)
    bare.ensure_workspace = lambda B: None  # keep the handle without a workspace
    with pytest.raises(I2lqrError, match="group_lanes"):
        bare.iterate(buf, 1)


def test_solves_to_termination_speculate_automatically(torch_mod):
    """i2lqr_solve of a small batch runs on the speculative kernel (three wavefronts per workgroup up
    to 512 problems, two above) without being asked to — in its sixteen-lane form (four problems per
    workgroup, the DPP passes), bit for bit the plain sixteen-lane kernel; pinned to eight lanes, bit
    for bit the plain eight-lane kernel; the chunked solves of the lane layouts finish their
    survivors with it and agree with the one-problem-per-wavefront tail to the solve tolerance."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads
    cfg = default_config("bicycle6", 20, "f64", dt=0.25)
    for B in (5, 100, 1000, 2500):
        host = workloads.make_batch(cfg, B)
        auto = BatchedILQR(cfg)
        assert auto.solve_kernel(B) == "k_group_spec (sixteen lanes)"
        assert auto.iterate_kernel(B) == "k_group_iterate (sixteen lanes)"
        a = auto.solve(dev_batch(auto, host))
        for lanes, spec_name, plain_name in ((16, "k_group_spec (sixteen lanes)", "k_group_iterate (sixteen lanes)"),
                                             (8, "k_group_spec", "k_group_iterate")):
            plain = BatchedILQR(cfg)
            plain.set_option("group_lanes", lanes)
            plain.set_option("speculate", 0)
            assert plain.solve_kernel(B) == plain_name
            b = plain.solve(dev_batch(plain, host))
            forced = BatchedILQR(cfg)
            forced.set_option("group_lanes", lanes)
            forced.set_option("speculate", 1)
            assert forced.solve_kernel(B) == spec_name
            f = forced.solve(dev_batch(forced, host))
            for key in ("X", "U", "K", "k", "lamb", "cost", "iters", "status"):
                assert torch.equal(f[key], b[key]), (B, lanes, key)
                if lanes == 16:
                    assert torch.equal(a[key], b[key]), (B, key)
            check_solve_outputs(plain, cfg, host, b)
        assert B < 100 or int(a["iters"].max()) > 12  # the batch has stragglers to speculate on
    # tail of the chunked solve (batch-tiled layout): speculative tail against the wave-kernel tail
    cfg = default_config("bicycle6", 20, "f64", dt=0.25, layout=2)
    B = 16384
    host = workloads.make_batch(cfg, B)
    res = []
    for spec in (-1, 0):
        solver = BatchedILQR(cfg)
        solver.set_option("speculate", spec)
        res.append(solver.solve(dev_batch(solver, host)))
        check_solve_outputs(solver, cfg, host, res[-1])
    a, b = res
    same = ((a["iters"] == b["iters"]) & (a["lamb"] == b["lamb"])).cpu().numpy()
    assert same.mean() >= 0.99
    assert torch.equal(a["status"].cpu()[same], b["status"].cpu()[same])
    ca, cb = a["cost"].cpu().numpy(), b["cost"].cpu().numpy()
    assert np.max(np.abs(ca - cb)[same] / np.maximum(np.abs(cb[same]), 1e-12)) < TOL_SOLVE
    assert np.max(np.abs(ca - cb) / np.maximum(np.abs(cb), 1.0)) < 1e-6
    assert int(a["iters"].max()) > 40


def test_quad12_full_size_properties_and_oracle_sample(torch_mod):
    """BASELINE configs[4] at its full size: n=12, m=4, N=50, B=65536, fp64 on the sixteen-lane
    kernel.  Size-independent properties over the whole batch (determinism, 2 + 2 == 4 fused
    iterations bit-exactly, returned X is bit-exactly the rollout of returned U, cost is its
    terminal cost, inputs inside the box) and the CPU oracle on a strided sample of 256 problems
    that spans the index range (workspace slots and record addressing of the last wavefronts)."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads
    cfg = default_config("quad12", 50, "f64", dt=0.02)
    solver = BatchedILQR(cfg)
    B, iters = 65536, 4
    host = workloads.make_batch(cfg, B)
    assert solver.iterate_kernel(B) == "k_iterate"  # before the workspace is registered
    a = solver.iterate(dev_batch(solver, host), iters)
    assert solver.iterate_kernel(B) == "k_quad_iterate"
    b = solver.iterate(dev_batch(solver, host), iters)
    for key in ("X", "U", "lamb", "cost", "K", "k"):
        assert torch.equal(a[key], b[key]), key
    c = solver.iterate(solver.iterate(dev_batch(solver, host), 2), 2)
    for key in ("X", "U", "lamb", "cost", "K", "k"):
        assert torch.equal(a[key], c[key]), key
    del b, c
    assert int(a["iters"].min()) == iters == int(a["iters"].max())
    X2, U2 = a["X"].clone(), a["U"].clone()
    cost2 = solver.rollout(X2, U2, a["x_term"])
    assert torch.equal(U2, a["U"]) and torch.equal(X2, a["X"]) and torch.equal(cost2, a["cost"])
    assert torch.isfinite(a["cost"]).all() and (a["cost"] >= 0).all()
    u_max = torch.tensor(list(cfg.u_max)[:cfg.m], dtype=solver.dtype, device=solver.device)
    assert (a["U"].abs() <= u_max[None, :, None]).all()
    check_solve_outputs(solver, cfg, host, a, early_exit=False, n_iters=iters)
    idx = np.unique(np.concatenate([np.arange(0, B, B // 255), [B - 1, B - 2, B - 3]]))
    ref = oracle().ilqr_batch(cfg, host["X"][idx], host["U"][idx], host["x_term"][idx],
                              host["lamb"][idx], host["obs"][idx], max_iter=iters, early_exit=False)
    tidx = torch.as_tensor(idx, device=solver.device)
    same = a["lamb"][tidx].cpu().numpy() == ref["lamb"]
    assert same.mean() >= 0.97
    check_flipped({key: a[key][tidx] for key in ("cost", "status")},
                   ref, same, 1e-6, early_exit=False)
    for key in ("X", "U"):
        assert batch_rel_err(a[key][tidx].cpu().numpy()[same], ref[key][same]) < TOL_SOLVE, key
    assert batch_rel_err(a["K"][tidx].cpu().numpy()[same], ref["K"][same]) < 1e-6
    assert batch_rel_err(a["k"][tidx].cpu().numpy()[same], ref["k"][same], floor=1.0) < 1e-6


@pytest.mark.parametrize("layout_id,B", [(1, 100), (2, 192)])
def test_quad12_one_problem_per_lane_kernel_vs_oracle(torch_mod, layout_id, B):
    """configs[4] shape on the batch-minor / batch-tiled layouts: k_lane_iterate_rows (one problem
    per lane, row-block form of the Riccati step, gains staged through LDS) against the CPU oracle
    — fused iterations with gains, the solve to termination, a ragged batch on the batch-minor
    layout — plus the bit-exact replay properties of the other kernel families."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads
    orc = oracle()
    cfg = default_config("quad12", 50, "f64", dt=0.02, layout=layout_id)
    solver = BatchedILQR(cfg)
    assert solver.iterate_kernel(B) == "k_lane_iterate_rows"
    host = workloads.make_batch(cfg, B)
    host["lamb"] = 10.0 ** np.random.default_rng(2).integers(-2, 2, B).astype(float)
    iters = 4
    it = solver.iterate(dev_batch(solver, host), iters)
    so = solver.solve(dev_batch(solver, host))
    ref_it = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"],
                            max_iter=iters, early_exit=False)
    ref_so = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"])
    assert (it["iters"].cpu().numpy() == iters).all()
    check_solve_outputs(solver, cfg, host, it, early_exit=False, n_iters=iters)
    check_solve_outputs(solver, cfg, host, so)
    same = it["lamb"].cpu().numpy() == ref_it["lamb"]
    assert same.mean() >= 0.97, same.mean()
    check_flipped(it, ref_it, same, 1e-6, early_exit=False)
    for key in ("X", "U"):
        assert batch_rel_err(to_host(solver, it[key])[same], ref_it[key][same]) < TOL_SOLVE, key
    np.testing.assert_allclose(it["cost"].cpu().numpy()[same], ref_it["cost"][same], rtol=1e-7)
    assert batch_rel_err(to_host(solver, it["K"])[same], ref_it["K"][same]) < 1e-6
    assert batch_rel_err(to_host(solver, it["k"])[same], ref_it["k"][same], floor=1.0) < 1e-6
    same = (so["iters"].cpu().numpy() == ref_so["iters"]) & (so["lamb"].cpu().numpy() == ref_so["lamb"])
    assert same.mean() >= 0.97, same.mean()
    check_flipped(so, ref_so, same, cfg.eps, early_exit=True)
    assert (so["status"].cpu().numpy()[same] == ref_so["status"][same]).all()
    assert batch_rel_err(to_host(solver, so["X"])[same], ref_so["X"][same]) < TOL_SOLVE
    # replay properties: 2 + 2 fused iterations == 4, returned X is the rollout of returned U
    two = solver.iterate(solver.iterate(dev_batch(solver, host), 2), 2)
    for key in ("X", "U", "lamb", "cost", "K", "k"):
        assert torch.equal(it[key], two[key]), key
    X2, U2 = it["X"].clone(), it["U"].clone()
    cost2 = solver.rollout(X2, U2, it["x_term"])
    assert torch.equal(U2, it["U"]) and torch.equal(X2, it["X"]) and torch.equal(cost2, it["cost"])
    # stage weights and fp32 run on these layouts since round 5 (tests/test_gpu_round5.py checks them
    # against the oracle); fp32 WITH stage weights is still the problem-major kernels' (a clear
    # error, no fallback)
    from ilqr_iterative_tasks_amd.solver import I2lqrError
    wcfg = default_config("quad12", 50, "f32", dt=0.02, layout=layout_id)
    wcfg.set_matrix("R", 0.01 * np.eye(4))
    with pytest.raises(I2lqrError, match="Q = R = 0"):
        f32 = BatchedILQR(wcfg)
        f32.iterate(dev_batch(f32, workloads.make_batch(wcfg, 64)), 1)


def test_quad12_full_size_on_the_lane_kernel(torch_mod):
    """BASELINE configs[4] at its full size (n=12, m=4, N=50, B=65536, fp64) on the batch-tiled
    layout (what bench.py measures): size-independent properties over the whole batch and the CPU
    oracle on a strided sample of 256 problems spanning the index range; the chunked solve to
    termination against the oracle on the same sample."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads
    cfg = default_config("quad12", 50, "f64", dt=0.02, layout=2)
    solver = BatchedILQR(cfg)
    B, iters = 65536, 4
    host = workloads.make_batch(cfg, B)
    a = solver.iterate(dev_batch(solver, host), iters)
    b = solver.iterate(dev_batch(solver, host), iters)
    for key in ("X", "U", "lamb", "cost", "K", "k"):
        assert torch.equal(a[key], b[key]), key
    del b
    assert int(a["iters"].min()) == iters == int(a["iters"].max())
    X2, U2 = a["X"].clone(), a["U"].clone()
    cost2 = solver.rollout(X2, U2, a["x_term"])
    assert torch.equal(U2, a["U"]) and torch.equal(X2, a["X"]) and torch.equal(cost2, a["cost"])
    assert torch.isfinite(a["cost"]).all() and (a["cost"] >= 0).all()
    U_pm = solver.to_problem_major(a["U"])
    u_max = torch.tensor(list(cfg.u_max)[:cfg.m], dtype=solver.dtype, device=solver.device)
    assert (U_pm.abs() <= u_max[None, :, None]).all()
    idx = np.unique(np.concatenate([np.arange(0, B, B // 255), [B - 1, B - 2, B - 3]]))
    orc = oracle()
    ref = orc.ilqr_batch(cfg, host["X"][idx], host["U"][idx], host["x_term"][idx],
                         host["lamb"][idx], host["obs"][idx], max_iter=iters, early_exit=False)
    tidx = torch.as_tensor(idx, device=solver.device)
    pm = {key: solver.to_problem_major(a[key])[tidx].cpu().numpy() for key in ("X", "U", "K", "k")}
    same = a["lamb"][tidx].cpu().numpy() == ref["lamb"]
    assert same.mean() >= 0.97
    check_flipped({key: a[key][tidx] for key in ("cost", "status")},
                   ref, same, 1e-6, early_exit=False)
    for key in ("X", "U"):
        assert batch_rel_err(pm[key][same], ref[key][same]) < TOL_SOLVE, key
    assert batch_rel_err(pm["K"][same], ref["K"][same]) < 1e-6
    assert batch_rel_err(pm["k"][same], ref["k"][same], floor=1.0) < 1e-6
    del a
    so = solver.solve(dev_batch(solver, host))  # chunked, compacting
    check_solve_outputs(solver, cfg, host, so)
    ref = orc.ilqr_batch(cfg, host["X"][idx], host["U"][idx], host["x_term"][idx],
                         host["lamb"][idx], host["obs"][idx])
    same = (so["iters"][tidx].cpu().numpy() == ref["iters"]) & (so["lamb"][tidx].cpu().numpy() == ref["lamb"])
    assert same.mean() >= 0.97
    check_flipped({key: so[key][tidx] for key in ("cost", "status")},
                   ref, same, cfg.eps, early_exit=True)
    assert (so["status"][tidx].cpu().numpy()[same] == ref["status"][same]).all()
    Xs = solver.to_problem_major(so["X"])[tidx].cpu().numpy()
    assert batch_rel_err(Xs[same], ref["X"][same]) < TOL_SOLVE
    assert set(np.unique(so["status"].cpu().numpy())) <= {1, 2, 3}


def test_negative_curvature_takes_the_eigenvalue_clamping_path(torch_mod, layout):
    """The kernels invert a positive-definite Quu directly and fall back to the reference's
    eig / clamp-negative / add-lamb construction (control/iterative_ilqr.py:118-123) otherwise.
    A negative-definite terminal weight forces the fallback; both paths against the oracle."""
    from ilqr_iterative_tasks_amd import BatchedILQR, workloads
    orc = oracle()
    solver, cfg = make_solver("bicycle4", 6, layout=layout)
    cfg.set_matrix("Qt", 2 * np.diag([1.0, 1.0, 20.0, -2.5]))  # Quu_dd = l_uu + dt^2 Vxx[3][3] < 0
    solver = pin_kernel(BatchedILQR(cfg), layout)
    host = workloads.make_batch(cfg, 192)
    rng = np.random.default_rng(11)
    host["U"] = rng.uniform(-1, 1, host["U"].shape) * np.array(cfg.u_max[:2])[None, :, None]
    host["lamb"] = 10.0 ** rng.integers(-4, 2, 192).astype(float)
    Xr, Ur, _ = orc.rollout_batch(cfg, host["X"], host["U"], host["x_term"])
    ko, Ko = orc.backward_batch(cfg, Xr, Ur, host["x_term"], host["lamb"], host["obs"])
    # the oracle really went through negative eigenvalues somewhere
    Quu_neg = 0
    for b in range(8):
        _, _, d = orc.backward(cfg, Xr[b], Ur[b], host["x_term"][b], host["lamb"][b],
                               obs=host["obs"][b], dump=True)
        Quu_neg += int((d["V_xx"].diagonal() < 0).any())
    assert Quu_neg == 8
    k, K = solver.backward(to_dev(solver, Xr), to_dev(solver, Ur), to_dev(solver, host["x_term"]),
                           to_dev(solver, host["lamb"]), to_dev(solver, host["obs"]))
    # the last three horizon steps (the first three of the recursion): an indefinite value
    # function makes the recursion itself ill-conditioned further back
    # (a clamped eigenvalue contributes 1 / lamb, up to 1e4 here: tolerance 1e-7)
    assert batch_rel_err(to_host(solver, K)[..., 3:], Ko[..., 3:]) < 1e-7
    assert batch_rel_err(to_host(solver, k)[..., 3:], ko[..., 3:]) < 1e-7


def test_nonzero_stage_weights_vs_oracle(torch_mod, layout):
    """Q, R != 0 exercise the stage-cost code paths the reference defaults leave at zero
    (nominal cost measured to xtarget, forward cost to x_terminal: iterative_ilqr.py:43 vs :151)."""
    from ilqr_iterative_tasks_amd import workloads
    orc = oracle()
    if layout in ("group", "row16", "spec"):
        pytest.skip("the eight- / sixteen-lane kernels are built for Q = R = 0 (other weights take "
                    "the one-problem-per-wavefront kernel automatically)")
    solver, cfg = make_solver("bicycle4", 6, layout=layout)
    cfg.set_matrix("Q", np.diag([0.01, 0.02, 0.1, 0.05]) + 0.001)
    cfg.set_matrix("R", np.array([[0.05, 0.01], [0.01, 0.08]]))
    cfg.xtarget[:4] = [1.0, -1.0, 2.0, 0.1]
    from ilqr_iterative_tasks_amd import BatchedILQR
    solver = BatchedILQR(cfg)
    host = workloads.make_batch(cfg, 256)
    ref = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"],
                         max_iter=6, early_exit=False)
    buf = solver.iterate(dev_batch(solver, host), 6)
    same = buf["lamb"].cpu().numpy() == ref["lamb"]
    assert same.mean() > 0.97
    assert batch_rel_err(to_host(solver, buf["X"])[same], ref["X"][same]) < TOL_SOLVE
    np.testing.assert_allclose(buf["cost"].cpu().numpy()[same], ref["cost"][same], rtol=1e-8)


def test_debug_build_reports_index_violations(torch_mod):
    """The index-checked build (make -C ilqr_iterative_tasks_amd/csrc debug) turns a recorded
    violation into I2LQR_ERR_LAUNCH with the decoded record; the product build has no such option
    (and no checks)."""
    import os
    from pathlib import Path
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads, _abi
    from ilqr_iterative_tasks_amd.solver import I2lqrError
    dbg = Path(_abi.__file__).resolve().parent / "csrc" / "libi2lqr_hip_debug.so"
    prod = BatchedILQR(default_config("bicycle4", 6))
    if "debug" not in str(_abi.LIB_PATH):
        with pytest.raises(I2lqrError, match="debug build"):
            prod.set_option("debug_self_test", 1)
    if not dbg.exists():
        pytest.skip("libi2lqr_hip_debug.so not built")
    solver = BatchedILQR(default_config("bicycle4", 6), lib_path=dbg)
    with pytest.raises(I2lqrError, match="index check failed: wave-kernel LDS slice, index 8, limit 8"):
        solver.set_option("debug_self_test", 1)
    # the record is cleared: a clean solve on the debug library passes its checks
    cfg = default_config("bicycle6", 20, dt=0.25)
    s2 = BatchedILQR(cfg, lib_path=dbg)
    host = workloads.make_batch(cfg, 100)
    buf = s2.solve(dev_batch(s2, host))
    assert int(buf["iters"].min()) >= 1


def test_zero_initial_cost_takes_the_reference_exit(torch_mod, layout):
    """x_term = rollout(x0, 0): the nominal cost is exactly 0, no candidate can be strictly better,
    every iteration is a reject and the solve leaves through `lamb > max_lamb` — the relative-
    improvement test `abs((J - J_new) / J) < eps` of control/iterative_ilqr.py:78, whose division
    by zero would yield NaN, is never reached.  Same iteration count, lamb and status as the
    oracle on every kernel family, inputs and states untouched."""
    orc = oracle()
    for system, N, dt in (("bicycle4", 6, 1.0), ("bicycle6", 20, 0.25)):
        solver, cfg = make_solver(system, N, dt=dt, layout=layout)
        B = 128
        rng = np.random.default_rng(3)
        X = np.zeros((B, cfg.n, N + 1))
        # heading 0 and dyadic positions / speeds: sin, cos and every product of the zero-input
        # rollout are exact, so the oracle and the kernels agree on x_N to the last bit and both
        # see a nominal cost of exactly 0
        X[:, :4, 0] = np.stack([rng.integers(0, 200, B) / 4.0, rng.integers(-12, 12, B) / 4.0,
                                rng.integers(0, 32, B) / 4.0, np.zeros(B)], 1)
        U = np.zeros((B, cfg.m, N))
        Xr, Ur, cr = orc.rollout_batch(cfg, X, U, np.zeros((B, cfg.n)))
        host = dict(X=X, U=U, x_term=Xr[:, :, N].copy(), lamb=np.ones(B), obs=None)
        host["lamb"][::3] = 1e-6
        ref = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], None)
        assert (ref["cost"] == 0).all() and (ref["status"] == 3).all()
        buf = solver.solve(dev_batch(solver, host))
        assert (buf["cost"].cpu().numpy() == 0).all()
        assert (buf["status"].cpu().numpy() == 3).all()
        np.testing.assert_array_equal(buf["iters"].cpu().numpy(), ref["iters"])
        np.testing.assert_array_equal(buf["lamb"].cpu().numpy(), ref["lamb"])
        assert (to_host(solver, buf["U"]) == 0).all()
        assert batch_rel_err(to_host(solver, buf["X"]), Xr) < 1e-12


def test_static_obstacle_record_ignores_its_speed(torch_mod, layout):
    """An obs record with moving option 0 is a static obstacle whatever its spd word holds
    (include/i2lqr.h; the reference raises NameError for `spd != 0` with moving_option None,
    control/ilqr_helper.py:34-43, which the Python host mirrors with a ValueError): bit-identical
    results with spd = 0 and spd = 5 on every kernel family."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    from ilqr_iterative_tasks_amd.control import Obstacle
    from ilqr_iterative_tasks_amd.control.iterative_ilqr import obstacle_record
    solver, cfg = make_solver("bicycle6", 20, dt=0.25, layout=layout)
    host = workloads.make_batch(cfg, 256)
    res = []
    for spd in (0.0, 5.0):
        h = dict(host)
        h["obs"] = host["obs"].copy()
        h["obs"][:, 4] = spd
        res.append(solver.iterate(dev_batch(solver, h), 6))
    for key in ("X", "U", "K", "k", "lamb", "cost"):
        assert torch.equal(res[0][key], res[1][key]), key
    with pytest.raises(ValueError):
        obstacle_record(Obstacle(31, -3, 8, 6, spd=1.0, timestep=1, moving_option=None))


def test_inputs_outside_the_box_are_clipped_on_entry(torch_mod, layout):
    """Initial inputs beyond +-u_max are legal: the reference clips them in its first rollout
    (control/iterative_ilqr.py:33-41).  Every kernel family — the eight-lane kernel with helper
    wavefronts (up to 2048 problems) included — must solve from the CLIPPED inputs: compared with
    the oracle and with a solve that was handed the clipped inputs."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import workloads
    orc = oracle()
    solver, cfg = make_solver("bicycle6", 20, dt=0.25, layout=layout)
    B = 1024
    host = workloads.make_batch(cfg, B)
    rng = np.random.default_rng(17)
    u_max = np.array(cfg.u_max[:cfg.m])[None, :, None]
    host["U"] = rng.uniform(-3, 3, host["U"].shape) * u_max  # up to three times the box
    clipped = dict(host)
    clipped["U"] = np.clip(host["U"], -u_max, u_max)
    a = solver.iterate(dev_batch(solver, host), 4)
    b = solver.iterate(dev_batch(solver, clipped), 4)
    for key in ("X", "U", "K", "k", "lamb", "cost"):
        assert torch.equal(a[key], b[key]), key
    ref = orc.ilqr_batch(cfg, host["X"], host["U"], host["x_term"], host["lamb"], host["obs"],
                         max_iter=4, early_exit=False)
    same = a["lamb"].cpu().numpy() == ref["lamb"]
    assert same.mean() > 0.98
    assert batch_rel_err(to_host(solver, a["X"])[same], ref["X"][same]) < TOL_SOLVE


def test_quad12_sixteen_lane_solve_returns_the_gains_of_the_last_executed_iteration(torch_mod):
    """A problem that has terminated keeps running beside its three wavefront neighbours in the
    sixteen-lane kernel; the gains it returns must be those of ITS last executed iteration
    (include/i2lqr.h), as the one-problem-per-wavefront kernel delivers them."""
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads
    cfg = default_config("quad12", 50, "f64", dt=0.02)
    solver = BatchedILQR(cfg)
    B = 64
    host = workloads.make_batch(cfg, B)
    host["lamb"] = 10.0 ** np.random.default_rng(5).integers(-3, 3, B).astype(float)
    out = {}
    for lanes in (64, 16):
        solver.set_option("group_lanes", lanes)
        out[lanes] = solver.solve(dev_batch(solver, host))
    it64, it16 = out[64]["iters"].cpu().numpy(), out[16]["iters"].cpu().numpy()
    assert len(np.unique(it64)) > 3  # the wavefront neighbours stop at different iterations
    same = (it64 == it16) & (out[64]["lamb"].cpu().numpy() == out[16]["lamb"].cpu().numpy())
    assert same.mean() >= 0.97
    assert batch_rel_err(to_host(solver, out[16]["K"])[same], to_host(solver, out[64]["K"])[same]) < 1e-6
    assert batch_rel_err(to_host(solver, out[16]["k"])[same], to_host(solver, out[64]["k"])[same],
                         floor=1.0) < 1e-6


def test_eight_lane_workspace_form_is_bit_identical(torch_mod):
    """The workspace form of the eight-lane kernel (records and gains in HBM, four wavefronts per
    CU; automatic above 4096 problems once the workspace is registered) against the LDS form: bit
    for bit, fused iterations with gains and solves with early exits, ragged batch sizes."""
    torch = torch_mod
    from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads
    for system, N, dt, B in (("bicycle6", 20, 0.25, 8192), ("bicycle6", 20, 0.25, 4101),
                             ("bicycle4", 6, 1.0, 5000)):
        cfg = default_config(system, N, "f64", dt=dt)
        host = workloads.make_batch(cfg, B)
        host["lamb"] = 10.0 ** np.random.default_rng(1).integers(-3, 2, B).astype(float)
        res = {}
        for ws in (0, 1):
            solver = BatchedILQR(cfg)
            solver.set_option("group_lanes", 8)
            solver.set_option("speculate", 0)
            solver.set_option("group_workspace", ws)
            it = solver.iterate(dev_batch(solver, host), 6)
            so = solver.solve(dev_batch(solver, host))
            assert ("workspace" in solver.iterate_kernel(B)) == bool(ws)
            res[ws] = (it, so)
        for a, b in zip(res[0], res[1]):
            for key in ("X", "U", "K", "k", "lamb", "cost", "iters", "status"):
                assert torch.equal(a[key], b[key]), (system, B, key)
    # automatic: the sixteen-lane kernel (rounds of 4096 problems) except between 4097 and 8192
    # problems (fp64; fp32: 7168) with the workspace registered, where the eight-lane workspace
    # form is ahead (round 5: measured at three shapes, tools/threshold_sweep.py)
    auto = BatchedILQR(default_config("bicycle6", 20, "f64", dt=0.25))
    assert auto.iterate_kernel(6144) == "k_group_iterate (sixteen lanes)"  # no workspace registered yet
    auto.ensure_workspace(6144)
    assert auto.iterate_kernel(6144) == "k_group_iterate (workspace form)"
    assert auto.iterate_kernel(4096) == "k_group_iterate (sixteen lanes)"
    assert auto.iterate_kernel(4097) == "k_group_iterate (workspace form)"
    auto.ensure_workspace(8192)
    assert auto.iterate_kernel(8192) == "k_group_iterate (workspace form)"
    assert auto.iterate_kernel(8193) == "k_group_iterate (sixteen lanes)"
    assert int(auto.lib.i2lqr_workspace_bytes(auto._handle, 8193)) == 0  # nothing to allocate there
    f32 = BatchedILQR(default_config("bicycle6", 20, "f32", dt=0.25))
    f32.ensure_workspace(7168)
    assert f32.iterate_kernel(7168) == "k_group_iterate (workspace form)"
    assert f32.iterate_kernel(8192) == "k_group_iterate (sixteen lanes)"


def test_inputs_outside_the_benchmark_distribution_vs_oracle(torch_mod, layout):
    """n = 6 problems the benchmark generator never draws: targets far outside the reachable set
    (hundreds of metres away, behind the vehicle, opposite heading), lamb0 above max_lamb (the first
    reject ends the solve), lamb0 tiny, initial inputs beyond the box, a moving obstacle sitting on
    the start — every kernel family against the oracle, solve to termination."""
    orc = oracle()
    solver, cfg = make_solver("bicycle6", 20, dt=0.25, layout=layout)
    B = 384
    rng = np.random.default_rng(99)
    X = np.zeros((B, 6, 21))
    X[:, 0, 0] = rng.uniform(-50, 50, B)
    X[:, 1, 0] = rng.uniform(-20, 20, B)
    X[:, 2, 0] = rng.uniform(-2, 15, B)
    X[:, 3, 0] = rng.uniform(-3.0, 3.0, B)
    X[:, 4, 0] = rng.uniform(-1, 1, B)
    X[:, 5, 0] = rng.uniform(-0.4, 0.4, B)
    x_term = np.zeros((B, 6))
    x_term[:, 0] = X[:, 0, 0] + rng.choice([-1, 1], B) * rng.uniform(100, 800, B)
    x_term[:, 1] = rng.uniform(-300, 300, B)
    x_term[:, 2] = rng.uniform(-10, 40, B)
    x_term[:, 3] = rng.uniform(-3.1, 3.1, B)
    u_max = np.array(cfg.u_max[:2])[None, :, None]
    U = rng.uniform(-2.5, 2.5, (B, 2, 20)) * u_max
    lamb = 10.0 ** rng.integers(-12, 6, B).astype(float)  # up to 1e5 > max_lamb = 1e3
    obs = np.tile(np.array([0.0, 0.0, 6.0, 4.0, 0.5, 1.0]), (B, 1))
    obs[:, 0] = X[:, 0, 0] + rng.uniform(-3, 3, B)
    obs[:, 1] = X[:, 1, 0] + rng.uniform(-3, 3, B)
    obs[::3, 5] = 2.0
    obs[1::3, 5] = -1.0
    host = dict(X=X, U=U, x_term=x_term, lamb=lamb, obs=obs)
    ref = orc.ilqr_batch(cfg, X, U, x_term, lamb, obs)
    buf = solver.solve(dev_batch(solver, host))
    it, st = buf["iters"].cpu().numpy(), buf["status"].cpu().numpy()
    same = (it == ref["iters"]) & (buf["lamb"].cpu().numpy() == ref["lamb"])
    assert same.mean() > 0.97, same.mean()
    check_flipped(buf, ref, same, cfg.eps, early_exit=True)
    assert (st[same] == ref["status"][same]).all()
    assert set(np.unique(st)) <= {1, 2, 3}
    assert (ref["lamb"] > cfg.max_lamb).any() and (ref["iters"] == 1).any()
    assert batch_rel_err(to_host(solver, buf["X"])[same], ref["X"][same]) < TOL_SOLVE
    assert batch_rel_err(to_host(solver, buf["U"])[same], ref["U"][same], floor=1e-2) < 1e-6
    np.testing.assert_allclose(buf["cost"].cpu().numpy()[same], ref["cost"][same], rtol=1e-7)


def test_random_configurations_every_family_against_the_oracle():
    """tools/parity_campaign.py at a size that takes seconds: random horizons, ragged batches,
    regularisation, obstacles and inputs beyond the box, every kernel family against the oracle —
    deviations within the suite's bounds where the oracle itself is insensitive to one ulp on U0,
    within 100 x that sensitivity elsewhere (profiles/r04_parity_campaign.txt is the long run)."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    out = subprocess.run([sys.executable, str(root / "tools" / "parity_campaign.py"), "12"],
                         capture_output=True, text=True, timeout=900, cwd=str(root))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "held everywhere" in out.stdout
    # 7 + 7 + 4 (plant, family) lines: the bicycles incl. the sixteen-lane DPP form ("row16"), and
    # 3 + 3 with stage weights (round 5: quad12's lane kernels take Q, R != 0)
    assert sum(l.startswith(("bicycle4", "bicycle6", "quad12")) for l in out.stdout.splitlines()) == 24
    assert sum(l.startswith("quad12+QR") for l in out.stdout.splitlines()) == 3
