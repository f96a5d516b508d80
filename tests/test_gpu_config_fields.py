"""Non-default solver constants on every kernel family: eps, lamb_factor, max_lamb, max_iter,
ctrl_q1/q2, obs_q1/q2, safety_margin, u_max[] and sys_par[] of i2lqr_config, with what the host
derives from them (DevCfg::ctrl_q12, obs_q122, ctrl_c[], pd[], fast_barrier), the two-exponential
input barrier (fast_barrier = 0) and the repeat of a fused pass in its general form.

  (1) golden G9 (the reference itself at non-default parameters, oracle/gen_golden_config.py)
      through solve() on every bicycle family, cfg built by config_from_params: no call masked;
  (2) the case table of config_cases.py in comparisons no accept / reject decision can flip: the
      stand-alone phases and the gains of ONE fused iteration, all problems;
  (3) the cases test_config_cases_host.py admits, over several iterations and to termination;
  (4) options that only move work around stay bit-identical under non-default constants.

A deviation is priced against the oracle's own sensitivity (config_cases.bound: the suite's bound
where one ulp on U0 moves the oracle by less than 1e-12, 100 x that sensitivity elsewhere), the rule
and the numbers of tools/parity_campaign.py."""
import numpy as np
import pytest

import config_cases as cc
from config_cases import COST_RATIO, FIXED, LAMB_CASES, MULTI, bound, per_problem
from kernel_families import BICYCLE_FAMILIES, assert_within, families, family_solver
from helpers import (check_flipped, check_solve_against_calls, check_solve_outputs, dev_batch,
                     g9_set, to_dev, to_host)

pytestmark = pytest.mark.gpu

KEYS = ("X", "U", "K", "k", "lamb", "cost", "iters", "status")


def runs(cases):
    """(plant, case, family) of every pair of `cases`."""
    return [(plant, case, fam) for plant, case in cc.pairs(cases) for fam in families(plant)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a HIP device"
    return torch


def rel_cost(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def finite(torch, *tensors):
    return all(bool(torch.isfinite(t).all()) for t in tensors)


# ------------------------------------------------------------------------------------------------
# (1) the reference at non-default parameters
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", list(BICYCLE_FAMILIES))
@pytest.mark.parametrize("name", ["ctrl", "obs", "lamb3", "box", "all"])
def test_solve_matches_reference_g9(torch_mod, golden_dir, name, fam):
    """128 ilqr() calls of the reference per parameter set: iteration count and lamb_out exactly on
    every call (max_flips = 0: the fixture holds only calls on which the reference is stable), X and
    U to 1e-8; and the outputs are consistent with cfg's own lamb_factor, max_lamb, max_iter, u_max."""
    g, cfg = g9_set(golden_dir, name)
    solver, cfg = family_solver(cfg, "bicycle4", fam, len(g["x0"]))
    buf = check_solve_against_calls(solver, g, 6, max_flips=0)
    host = dict(X=np.zeros((len(g["x0"]), 4, 7)), U=np.zeros((len(g["x0"]), 2, 6)),
                x_term=g["x_term"], lamb=g["lamb_in"], obs=g["obs"])
    host["X"][:, :, 0] = g["x0"]
    check_solve_outputs(solver, cfg, host, buf)
    st = buf["status"].cpu().numpy()
    assert ((st == 3) == (g["lamb_out"] > cfg.max_lamb)).all()


# (plant, case) whose U after one fused iteration is compared at the scale of the step that
# produced it, max(|U|, |k|), not at |U| alone.  The accepted U is the nominal plus k + K dx and
# inherits the error the gains are allowed, which is relative to THEIR size; with these stiff
# barriers |k| reaches 46 against |U| <= 2.  Measured at U's own scale, bicycle4, one problem each
# (|k| = 46 / 39), error against bound(sens, 1e-8) = 100 x sensitivity: fast_edge 8.1e-10 (wave),
# 1.0e-9 (group, group-ws, spec), 1.3e-9 (row16), 9.6e-10 (lane, tiled) against 4.6e-10; two_exp
# 1.4e-9 (wave), 1.5e-9 (group, group-ws, spec) against 1.3e-9.  Every other (plant, case) keeps
# U's own scale.
U_AT_STEP_SCALE = (("bicycle4", "fast_edge"), ("bicycle4", "two_exp"))


def _check_neg_qt_trajectory(orc, cfg, host, got, lamb, ref, sens, same, nominal, gains):
    """What one fused iteration returns under neg_qt.  The gains of the first three steps are ill
    conditioned (a clamped eigenvalue contributes 1 / lamb: |k| reaches 4e5) and the candidate is
    rolled out with all of them, so the oracle's trajectory is not the yardstick at the suite's
    bound (measured: X 4e-6 apart with every branch equal).  Two comparisons instead:
    (a) with the gains the kernel itself returned - all steps - the oracle's forward pass gives the
        candidate the kernel must have rolled out: accepted where it is cheaper, X, U and cost at
        the suite's bounds of a fused iterate (U with the rounding floor of its sum, as above).  A
        repeat that returns one set of gains and rolls out another fails here.
    (b) against the oracle's own run at a bound priced by the tolerance the gains are held to: the
        oracle's candidate with its gains moved by 1e-7 of the problem's largest gain (three
        draws); ten times the change it shows in X, U and cost.  A repeat whose early gains are
        wrong by more than the compared ones may be fails here.  (Measured over the seven
        families: X up to 7.7e-6, U 1.4e-4, cost 7.7e-5 from the oracle's, 3.6e-4 of this bound.)"""
    Xr, Ur, cr = nominal
    Ko, ko = gains
    eps = np.finfo(float).eps
    accepted = lamb < host["lamb"]
    Xc, Uc, cc_ = orc.forward_batch(cfg, Xr, Ur, host["x_term"], got["K"], got["k"])
    clear = np.abs(cc_ - cr) > 1e-9 * np.abs(cr)
    assert (accepted == (cc_ < cr))[clear].all()
    ok = clear & np.isfinite(cc_)
    want_X = np.where(accepted[:, None, None], Xc, Xr)
    want_U = np.where(accepted[:, None, None], Uc, Ur)
    want_c = np.where(accepted, cc_, cr)
    S = (np.abs(Ur).max(axis=(1, 2)) + np.abs(got["k"]).max(axis=(1, 2)) +
         cfg.n * np.abs(got["K"]).max(axis=(1, 2, 3)) * np.abs(Xc - Xr).max(axis=(1, 2)))
    u_floor = 16 * eps * S / np.abs(want_U).max(axis=(1, 2))
    assert_within(per_problem(got["X"], want_X)[ok], bound(sens, 1e-8)[ok], "own-gains X")
    assert_within(per_problem(got["U"], want_U)[ok], np.maximum(bound(sens, 1e-8), u_floor)[ok],
                  "own-gains U")
    assert_within(rel_cost(got["cost"], want_c)[ok], bound(sens, 1e-7, COST_RATIO)[ok],
                  "own-gains cost")
    rng = np.random.default_rng(3)
    spread = {key: np.zeros(len(lamb)) for key in ("X", "U", "cost")}
    Xo, Uo, co = orc.forward_batch(cfg, Xr, Ur, host["x_term"], Ko, ko)
    for _ in range(3):
        Kp = Ko + 1e-7 * np.abs(Ko).max(axis=(1, 2, 3), keepdims=True) * rng.uniform(-1, 1, Ko.shape)
        kp = ko + 1e-7 * np.abs(ko).max(axis=(1, 2), keepdims=True) * rng.uniform(-1, 1, ko.shape)
        Xp, Up, cp = orc.forward_batch(cfg, Xr, Ur, host["x_term"], Kp, kp)
        spread["X"] = np.maximum(spread["X"], per_problem(Xp, Xo))
        spread["U"] = np.maximum(spread["U"], per_problem(Up, Uo))
        spread["cost"] = np.maximum(spread["cost"], rel_cost(cp, co))
    both = same & accepted & (ref["lamb"] < host["lamb"])
    for key, tol, ratio in (("X", 1e-8, 100.0), ("U", 1e-8, 100.0), ("cost", 1e-7, COST_RATIO)):
        err = rel_cost(got[key], ref[key]) if key == "cost" else per_problem(got[key], ref[key])
        print("neg_qt", key, "worst error", float(err[both].max()), "worst error / bound",
              float((err / np.maximum(bound(sens, tol, ratio), 10.0 * spread[key]))[both].max()))
        assert_within(err[both], np.maximum(bound(sens, tol, ratio), 10.0 * spread[key])[both],
                      "priced " + key)
    rejected = same & ~accepted
    assert_within(per_problem(got["X"], ref["X"])[rejected], bound(sens, 1e-8)[rejected], "nominal X")


# ------------------------------------------------------------------------------------------------
# (2) comparisons that cannot flip
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plant,case,fam", runs(None))
def test_single_iteration_vs_oracle(torch_mod, plant, case, fam):
    """rollout, backward and forward against the oracle's (test_function_level_vs_oracle's
    tolerances: X 1e-11, gains 1e-9, forward cost 1e-10), then ONE fused iteration: the K and k it
    returns are those of the nominal whatever the accept decision, so they are compared for ALL
    problems - this reaches each fused kernel's own barrier and record code, the two-exponential
    branch and the general-form repeat - and lamb, status, X, U, cost on the problems whose lamb is
    the oracle's (at least 97 %).  Every output is finite.  neg_qt: gains of the last three horizon
    steps at 1e-7, as test_negative_curvature_takes_the_eigenvalue_clamping_path, and the trajectory
    as _check_neg_qt_trajectory says."""
    torch = torch_mod
    from oracle import oracle as orc
    cfg, host, sens, ref = cc.priced(plant, case, 1)
    B = host["X"].shape[0]
    solver, cfg = family_solver(cfg, plant, fam, B)
    tail = slice(3, None) if case == "neg_qt" else slice(None)
    g_tol = 1e-7 if case == "neg_qt" else 1e-9
    # stand-alone phases
    Xr, Ur, cr = orc.rollout_batch(cfg, host["X"], host["U"], host["x_term"])
    Xd, Ud, xt = to_dev(solver, host["X"]), to_dev(solver, host["U"]), to_dev(solver, host["x_term"])
    cost = solver.rollout(Xd, Ud, xt)
    assert finite(torch, Xd, Ud, cost)
    assert np.array_equal(to_host(solver, Ud), Ur)  # clipped to cfg's box
    assert_within(per_problem(to_host(solver, Xd), Xr), bound(sens, 1e-11), "rollout X")
    assert_within(rel_cost(cost.cpu().numpy(), cr), bound(sens, 1e-11), "rollout cost")
    ko, Ko = orc.backward_batch(cfg, Xr, Ur, host["x_term"], host["lamb"], host["obs"])
    Xd, Ud = to_dev(solver, Xr), to_dev(solver, Ur)
    lamb_d, obs_d = to_dev(solver, host["lamb"]), to_dev(solver, host["obs"])
    k, K = solver.backward(Xd, Ud, xt, lamb_d, obs_d)
    assert finite(torch, k, K)
    assert_within(per_problem(to_host(solver, K)[..., tail], Ko[..., tail]), bound(sens, g_tol),
                  "backward K")
    assert_within(per_problem(to_host(solver, k)[..., tail], ko[..., tail]), bound(sens, g_tol),
                  "backward k")
    Xn_o, Un_o, cn_o = orc.forward_batch(cfg, Xr, Ur, host["x_term"], Ko, ko)
    Xn, Un, cn = solver.forward(Xd, Ud, xt, to_dev(solver, Ko), to_dev(solver, ko))
    assert finite(torch, Xn, Un, cn)
    assert_within(per_problem(to_host(solver, Xn), Xn_o), bound(sens, 1e-11), "forward X")
    # U_new = U + k + K (x_new - x) is summed from terms of size S = |U| + |k| + n |K| |x_new - x|
    # and carries their rounding: with stiff barriers |k| reaches 46, under neg_qt (a clamped
    # eigenvalue contributes 1 / lamb) 4e5, against |U| <= 2.  No arithmetic resolves U_new finer
    # than eps S; 16 eps S / |U| is the floor of its bound (default constants: ~1e-13, no change).
    S = (np.abs(Ur).max(axis=(1, 2)) + np.abs(ko).max(axis=(1, 2)) +
         cfg.n * np.abs(Ko).max(axis=(1, 2, 3)) * np.abs(Xn_o - Xr).max(axis=(1, 2)))
    u_floor = 16 * np.finfo(float).eps * S / np.abs(Un_o).max(axis=(1, 2))
    assert_within(per_problem(to_host(solver, Un), Un_o), np.maximum(bound(sens, 1e-11), u_floor),
                  "forward U")
    assert_within(rel_cost(cn.cpu().numpy(), cn_o), bound(sens, 1e-10), "forward cost")
    # one fused iteration
    buf = solver.iterate(dev_batch(solver, host), 1)
    assert finite(torch, *(buf[key] for key in ("X", "U", "K", "k", "lamb", "cost")))
    assert (buf["iters"].cpu().numpy() == 1).all()
    assert_within(per_problem(to_host(solver, buf["K"])[..., tail], Ko[..., tail]),
                  bound(sens, g_tol), "fused K")
    assert_within(per_problem(to_host(solver, buf["k"])[..., tail], ko[..., tail]),
                  bound(sens, g_tol), "fused k")
    same = buf["lamb"].cpu().numpy() == ref["lamb"]
    print(plant, case, fam, "same branch", same.mean())
    assert same.mean() >= 0.97, f"{(~same).sum()} of {B} problems took a different branch"
    assert (buf["status"].cpu().numpy()[same] == ref["status"][same]).all()
    got = {key: to_host(solver, buf[key]) for key in ("X", "U", "K", "k")}
    got["cost"] = buf["cost"].cpu().numpy()
    if case != "neg_qt":
        # the suite's bounds of a fused iterate: X, U 1e-8, cost 1e-7
        assert_within(per_problem(got["X"], ref["X"])[same], bound(sens, 1e-8)[same], "fused X")
        u_err = per_problem(got["U"], ref["U"])
        print(plant, case, fam, "fused U: worst error / bound at U's own scale",
              float((u_err / bound(sens, 1e-8))[same].max()))
        if (plant, case) in U_AT_STEP_SCALE:
            u_scale = np.maximum(np.abs(ref["U"]).max(axis=(1, 2)), np.abs(ko).max(axis=(1, 2)))
            u_err = np.abs(got["U"] - ref["U"]).max(axis=(1, 2)) / u_scale
        assert_within(u_err[same], bound(sens, 1e-8)[same], "fused U")
        assert_within(rel_cost(got["cost"], ref["cost"])[same],
                      bound(sens, 1e-7, COST_RATIO)[same], "fused cost")
    else:
        _check_neg_qt_trajectory(orc, cfg, host, got, buf["lamb"].cpu().numpy(), ref, sens, same,
                                 (Xr, Ur, cr), (Ko, ko))
    check_solve_outputs(solver, cfg, host, buf, early_exit=False, n_iters=1)


# ------------------------------------------------------------------------------------------------
# (3) several iterations
# ------------------------------------------------------------------------------------------------

def _compare_run(solver, cfg, host, buf, ref, sens, n_iters):
    """A fixed count (n_iters) or a solve (None) against the oracle's run `ref`, priced by `sens`."""
    lamb, iters = buf["lamb"].cpu().numpy(), buf["iters"].cpu().numpy()
    if n_iters is None:
        same = (iters == ref["iters"]) & (lamb == ref["lamb"])
    else:
        assert (iters == n_iters).all()
        same = lamb == ref["lamb"]
    print("same branch", same.mean(), "of", len(same))
    assert same.mean() >= (0.98 if n_iters is None else 0.99), \
        f"{(~same).sum()} of {len(same)} problems took a different branch"
    check_flipped(buf, ref, same, cfg.eps if n_iters is None else 1e-6, early_exit=n_iters is None)
    assert (buf["status"].cpu().numpy()[same] == ref["status"][same]).all()
    for key, tol in (("X", 1e-8), ("U", 1e-8), ("K", 1e-6)):
        assert_within(per_problem(to_host(solver, buf[key]), ref[key])[same], bound(sens, tol)[same],
                      key)
    assert_within(rel_cost(buf["cost"].cpu().numpy(), ref["cost"])[same], bound(sens, 1e-7, COST_RATIO)[same],
                  "cost")
    check_solve_outputs(solver, cfg, host, buf, early_exit=n_iters is None, n_iters=n_iters)


@pytest.mark.parametrize("plant,case,fam", runs(MULTI))
def test_fixed_count_and_solve_vs_oracle(torch_mod, plant, case, fam):
    """FIXED[plant] fused iterations and the solve to termination against the oracle on the cases
    that are well conditioned over several iterations (config_cases.MULTI): the oracle's branches on
    at least 99 % / 98 % of the problems, the others as good (_check_flipped), statuses equal, X and
    U within bound(sens, 1e-8), cost 1e-7, K 1e-6, and check_solve_outputs under the case's cfg (it
    reads lamb_factor, max_lamb, max_iter and u_max from it).  The lamb cases leave through every
    exit the oracle takes: all three on the bicycles."""
    n = FIXED[plant]
    cfg, host, sens, ref = cc.priced(plant, case, n)
    B = host["X"].shape[0]
    solver, cfg = family_solver(cfg, plant, fam, B)
    _compare_run(solver, cfg, host, solver.iterate(dev_batch(solver, host), n), ref, sens, n)
    _, _, sens, ref = cc.priced(plant, case, None)
    buf = solver.solve(dev_batch(solver, host))
    _compare_run(solver, cfg, host, buf, ref, sens, None)
    if case in LAMB_CASES:
        st = set(np.unique(buf["status"].cpu().numpy()))
        assert st == set(np.unique(ref["status"])) and (plant == "quad12" or st == {1, 2, 3})


# ------------------------------------------------------------------------------------------------
# (4) options that only move work around
# ------------------------------------------------------------------------------------------------

def _both(solver, host, n_iters):
    """iterate(n_iters) and, for n_iters > 1, the solve to termination."""
    out = [solver.iterate(dev_batch(solver, host), n_iters)]
    if n_iters > 1:
        out.append(solver.solve(dev_batch(solver, host)))
    return out


def _same_bits(torch, got, want, what):
    for a, b in zip(got, want):
        for key in KEYS:
            assert torch.equal(a[key], b[key]), (key, what)
        assert finite(torch, *(a[key] for key in ("X", "U", "K", "k", "lamb", "cost")))


# (plant, family, option, problems: None = SHAPES', "4C" = four per compute unit - the batch at
# which the sixteen-lane kernel takes its overlapped schedule)
OPTIONS = [("bicycle6", "row16", "group_fixed_horizon", "4C"), ("bicycle6", "row16", "group_overlap", "4C"),
           ("bicycle6", "row16", "group_chains", "4C"), ("bicycle6", "row16", "group_chains", None),
           ("bicycle4", "group", "group_chains", None), ("bicycle6", "group", "group_chains", None),
           ("bicycle4", "lane", "helper_wavefront", None), ("bicycle6", "tiled", "helper_wavefront", None),
           ("bicycle4", "wave", "per_step_jacobians", None), ("bicycle6", "wave", "per_step_jacobians", None)]


@pytest.mark.parametrize("case,n_iters", [("all", 6), ("two_exp", 1)])
@pytest.mark.parametrize("plant,fam,option,size", OPTIONS)
def test_scheduling_options_stay_bit_identical(torch_mod, plant, fam, option, size, case, n_iters):
    """The automatic setting of an option against 0: every output equal bit for bit, under `all`
    (fused iterations and the solve) and under `two_exp` (one iteration: fast_barrier = 0)."""
    torch = torch_mod
    cfg, host = cc.problem(plant, case)
    if size == "4C":
        B = 4 * torch.cuda.get_device_properties(0).multi_processor_count
        host = cc.batch(cfg, B, cc.SEED, edge=case in cc.EDGE)
    B = host["X"].shape[0]
    solver, cfg = family_solver(cfg, plant, fam, B)
    out = {}
    for value in (0, -1):
        solver.set_option(option, value)
        out[value] = _both(solver, host, n_iters)
    _same_bits(torch, out[-1], out[0], (option, plant, fam, case))


@pytest.mark.parametrize("case,n_iters", [("all", 6), ("two_exp", 1)])
@pytest.mark.parametrize("plant", list(cc.SHAPES))
def test_tiled_equals_batch_minor(torch_mod, plant, case, n_iters):
    torch = torch_mod
    cfg, host = cc.problem(plant, case)
    B = host["X"].shape[0]
    lane, _ = family_solver(cfg, plant, "lane", B)
    tiled, _ = family_solver(cfg, plant, "tiled", B)
    for a, b in zip(_both(lane, host, n_iters), _both(tiled, host, n_iters)):
        for key in ("X", "U", "K", "k"):
            assert torch.equal(lane.to_problem_major(a[key]), tiled.to_problem_major(b[key])), key
        for key in ("lamb", "cost", "iters", "status"):
            assert torch.equal(a[key], b[key]), key


# ------------------------------------------------------------------------------------------------
# (5) the opt-in forms under `all`
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", list(cc.OPT_IN_RUNS))
def test_opt_in_forms_under_all(torch_mod, form):
    """One small run per opt-in form with every constant of `all` set (config_cases.OPT_IN_RUNS:
    three iterations, shown to be well conditioned by test_config_cases_host.py), through the forms'
    own harness: opt_in_reference.reference reads the same cfg, opt_in_gpu.compare as it stands."""
    import opt_in_gpu as og
    cfg, host, box, A, merit, layout, _ = cc.opt_in_case(form)
    B = host["X"].shape[0]
    if layout == 0:
        solver = og.make_solver(cfg, box, barrier_cost=1 if merit else None, **og.options_for(host, A))
        name = og.MERIT_NAME if merit else og.BOX_NAME if box is not None else \
            og.OBS_NAME if og.records(host) else og.LS_NAME
        assert solver.iterate_kernel(B) == name
    else:
        solver = og.checked_lane_solver(cfg, host, box, layout, A, merit)
    buf = og.run(solver, host, cc.OPT_IN_ITERS)
    assert finite(torch_mod, *(buf[key] for key in ("X", "U", "K", "k", "lamb", "cost")))
    og.compare(solver, buf, cc.opt_in_reference(form), cc.OPT_IN_ITERS)


def test_wave_chain_under_all_equals_the_per_step_launches(torch_mod):
    """A chain of dependent solves in one launch ("wave_chain") against chain_len calls of solve()
    with lamb carried by hand, under `all`: bit for bit, as under the defaults."""
    import opt_in_gpu as og
    from opt_in_cases import make_chain
    cfg, host, box, A, chains, chain_len = make_chain(cc.OPT_IN_CHAIN)
    cc.apply(cfg, "all")
    solver = og.make_solver(cfg, box, wave_chain=1, **og.options_for(host, A))
    chained = solver.solve_chained(dev_batch(solver, host), chains, chain_len)
    og.same_bits(torch_mod, chained, og.step_by_step(solver, host, chains, chain_len), "all")
    it = chained["iters"].cpu().numpy()
    assert (it >= 1).all() and (it <= cfg.max_iter).all()
