"""CPU suite of the non-default-constants table (config_cases.py): the oracle alone stays inside
every cap test_gpu_config_fields.py puts on the kernels, and every case bites.

The GPU suite prices a kernel's deviation against the oracle's own sensitivity (the same problem
with U0 moved by one ulp) and asks for the oracle's accept / reject branches.  That only means
something if the oracle's own one-ulp run keeps its branches and most problems are well
conditioned; and a case only tests a field if the field moves the result."""
import numpy as np
import pytest

import config_cases as cc
from config_cases import FIXED, LAMB_CASES, MULTI, SINGLE


@pytest.mark.parametrize("plant,case", cc.pairs(MULTI))
def test_reference_is_well_conditioned_where_several_iterations_are_compared(plant, case):
    """No branch changes under one ulp after 1 iteration and after the fixed count, at most 3 %
    after a solve; at least 90 % of the problems have a sensitivity below 1e-12 after the fixed
    count; everything is finite."""
    for n_iters, most in ((1, 0.0), (FIXED[plant], 0.0), (None, 0.03)):
        _, _, sens, ref = cc.priced(plant, case, n_iters)
        changed = sens == 1.0
        print(plant, case, n_iters, "changed", int(changed.sum()), "well conditioned",
              float((sens < 1e-12).mean()), "largest", float(sens[~changed].max(initial=0.0)))
        assert changed.mean() <= most, (n_iters, int(changed.sum()))
        assert all(np.isfinite(ref[key]).all() for key in ("X", "U", "K", "k", "cost", "lamb"))
        if n_iters == FIXED[plant]:
            assert (sens < 1e-12).mean() >= 0.90


@pytest.mark.parametrize("plant,case", cc.pairs(SINGLE))
def test_single_iteration_cases_keep_their_branches_and_are_priced(plant, case):
    """The cases config_cases.py restricts to one iteration: their one-ulp run changes no branch
    within that iteration and is finite, and the restriction is still called for (fewer than 90 %
    well-conditioned problems after the fixed count, or changed branches)."""
    _, _, sens, ref = cc.priced(plant, case, 1)
    assert not (sens == 1.0).any()
    assert all(np.isfinite(ref[key]).all() for key in ("X", "U", "K", "k", "cost", "lamb"))
    sens_n, _ = cc.priced(plant, case, FIXED[plant])[2:]
    print(plant, case, "after", FIXED[plant], "well conditioned", float((sens_n < 1e-12).mean()),
          "changed", int((sens_n == 1.0).sum()), "largest", float(sens_n[sens_n < 1.0].max()))
    assert (sens_n < 1e-12).mean() < 0.90 or (sens_n == 1.0).any()


@pytest.mark.parametrize("plant,case", cc.pairs())
def test_every_case_bites(plant, case):
    """The oracle's K after one iteration differs from the default configuration's by more than 1e-4
    (relative, per problem) on at least half the problems - for the cases that only change the
    accept / reject constants, lamb or the iteration count of the solve on at least a quarter - so a
    kernel that ignored the field could not pass."""
    cfg, host = cc.problem(plant, case)
    dflt = cc.make_cfg(plant)
    if case in LAMB_CASES:
        a, b = cc.oracle_run(cfg, host, None), cc.oracle_run(dflt, host, None)
        moved = (a["lamb"] != b["lamb"]) | (a["iters"] != b["iters"])
        assert moved.mean() >= 0.25
    else:
        a, b = cc.oracle_run(cfg, host, 1), cc.oracle_run(dflt, host, 1)
        assert (cc.per_problem(a["K"], b["K"]) > 1e-4).mean() >= 0.5


@pytest.mark.parametrize("plant", ["bicycle4", "bicycle6"])
@pytest.mark.parametrize("case", LAMB_CASES)
def test_lamb_cases_reach_every_exit(plant, case):
    """CONVERGED, MAX_ITER and LAMB_OVERFLOW all occur in the oracle's solve on the bicycles (quad12's
    64 problems converge or overflow before max_iter: two exits)."""
    ref = cc.priced(plant, case, None)[3]
    assert set(np.unique(ref["status"])) == {1, 2, 3}


def test_quad12_lamb_cases_reach_two_exits():
    for case in LAMB_CASES:
        assert set(np.unique(cc.priced("quad12", case, None)[3]["status"])) == {1, 3}


def test_two_exp_and_fast_edge_sit_where_the_table_says():
    """2 ctrl_q2 u_max: 596 < 600 on bicycle4 and quad12 under `fast_edge` (DevCfg::fast_barrier
    stays 1), at least 600 for some input of every plant under `two_exp`; and a quarter of their U
    entries sit exactly on the box, both signs."""
    for plant in cc.SHAPES:
        edge, host = cc.problem(plant, "fast_edge")
        spans = [2 * edge.ctrl_q2 * edge.u_max[a] for a in range(edge.m)]
        assert max(spans) < 600 and (plant == "bicycle6" or max(spans) == 596.0)
        two, host = cc.problem(plant, "two_exp")
        assert max(2 * two.ctrl_q2 * two.u_max[a] for a in range(two.m)) >= 600
        u_max = np.array(two.u_max[:two.m])[None, :, None]
        for sign in (-1.0, 1.0):
            assert 0.08 < (host["U"] == sign * u_max).mean() < 0.17


def test_neg_qt_goes_through_negative_eigenvalues():
    """As test_gpu_parity.py::test_negative_curvature_...: V_xx has a negative diagonal entry on
    every sampled problem."""
    from oracle import oracle as orc
    cfg, host = cc.problem("bicycle4", "neg_qt")
    Xr, Ur, _ = orc.rollout_batch(cfg, host["X"], host["U"], host["x_term"])
    for b in range(0, 192, 12):
        d = orc.backward(cfg, Xr[b], Ur[b], host["x_term"][b], host["lamb"][b], obs=host["obs"][b],
                         dump=True)[2]
        assert (d["V_xx"].diagonal() < 0).any()


def test_bound_is_the_campaigns_rule():
    b = cc.bound(np.array([0.0, 9.9e-13, 1e-12, 3e-9, 1.0]), 1e-8)
    assert list(b) == [1e-8, 1e-8, 100 * 1e-12, 100 * 3e-9, 100.0]


def test_apply_scales_the_box_and_sets_the_fields():
    cfg = cc.make_cfg("quad12", "all")
    assert list(cfg.u_max[:4]) == [2.0 * 0.6, 2.0 * (0.9 / 1.57), 2.0 * 0.6, 2.0 * (0.9 / 1.57)]
    assert (cfg.lamb_factor, cfg.max_lamb, cfg.eps, cfg.safety_margin) == (4.0, 300.0, 1e-3, 0.2)
    b4 = cc.make_cfg("bicycle4", "all")
    assert abs(b4.u_max[0] - 1.2) < 1e-15 and abs(b4.u_max[1] - 0.9) < 1e-15
    assert list(cc.make_cfg("quad12", "plant").sys_par[:7]) == cc.CASES["plant"]["sys_par"][:7]


@pytest.mark.parametrize("form", list(cc.OPT_IN_RUNS))
def test_opt_in_runs_under_all_bite_and_are_well_conditioned(form):
    """opt_in_reference.reference() of every OPT_IN_RUNS entry: under `all` it differs from the run
    at the defaults (gains by more than 1e-4, or lamb) on at least half the problems, its one-ulp
    run keeps at least 97 % of the problems on their branch, at least 97 % decide with a margin of
    opt_in_cases.MARGIN, and everything is finite."""
    from opt_in_cases import MARGIN
    ref, dflt = cc.opt_in_reference(form), cc.opt_in_reference(form, None)
    moved = (cc.per_problem(ref["K"], dflt["K"]) > 1e-4) | (ref["lamb"] != dflt["lamb"])
    assert moved.mean() >= 0.5
    assert (cc.opt_in_reference(form, "all", True)["lamb"] == ref["lamb"]).mean() >= 0.97
    assert (ref["margin"] >= MARGIN).mean() >= 0.97
    assert all(np.isfinite(ref[key]).all() for key in ("X", "U", "K", "k", "cost", "lamb"))
