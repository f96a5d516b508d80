#!/usr/bin/env python3
"""Golden G9: the reference's ilqr() at NON-DEFAULT parameters, captured by running the reference
itself (build container only; see oracle/gen_golden.py for how the reference is imported).  Writes
tests/golden/g9_config_fields.npz: plain arrays only.

Five parameter sets (SETS below) x 128 calls: 64 states traj[s] of data/closed_loop_feasible.txt,
x_term = traj[min(s + 6, 120)], lamb_in in {1, 1e-3}, N = 6, dt = 1; the static obstacle
(31,-3,8,6) on every other state, the moving record (35,-16,34,34,1,1,1) on the rest.  Per set:
  <set>_params                 the parameters as numbers, in the order of `param_names`
  <set>_<pack_calls' arrays>   x0, x_term, lamb_in, obs, U, X, lamb_out, iters
  <set>_iter_*                 X, U, lamb, k, K, X_new, U_new, cost_new, x_term, obs of the first
                               and third iteration of 16 of the calls (as G1); <set>_iter_iteration
                               says which (1 or 3)

Calls on which the reference is its own round-off tie are not captured.  An accept / reject
decision `cost_new < cost` (control/iterative_ilqr.py:74) taken on two costs that agree to round-off
goes either way under a perturbation of one ulp, and no restatement of the arithmetic can be held
to it.  So every call is run five times by the reference: as it stands, with x0 moved by one ulp
up and down (np.nextafter on every component) and with x0 scaled by 1 +- 1e-13 (the kernels that
are held to this fixture sum in another order than NumPy: a few hundred ulp of margin).  It enters
the fixture only if iteration count and lamb_out are the same in all five runs.  The states are
taken in a fixed order (64 spread over the lap first, obstacle alternating, both lamb_in; then the
states in between; then the same states with the other obstacle) until 64 calls per obstacle are
found.  The tests then compare EVERY call of the fixture: none is masked.

This also settles the one call on which oracle and reference were seen to differ before this
fixture existed (lamb_factor 3, max_lamb 50, eps 1e-4, max_ilqr_iter 40: oracle 9 iterations,
reference 13).  The states of the data file are rounded to six decimals, so the first Newton step
lands on x_term to ~4e-8 and leaves a cost of ~3e-15: a squared difference of positions ~1e2 that
carry 1e-14 of round-off, known to ~3e-7 relative.  At the default eps = 1e-2 the solve exits
there.  At eps = 1e-4 the first step's relative change (3.4e-4) is not small enough, and every
later iteration compares two costs that differ by that noise: an "accept" exits as converged, a
"reject" multiplies lamb until it passes max_lamb.  The count is a sequence of coin flips: on
state 16, lamb_in 1e-3 the reference itself takes 14 iterations, and 11 with x0 one ulp up or
down.  50 of the 178 `lamb3` candidates tried are dropped for that reason (the run prints the
count); the sets with eps >= 1e-3 drop none under one ulp and at most 2 under 1e-13.  The oracle
was not wrong, and is unchanged.  (The stable calls take at most 20 iterations: none reaches
max_ilqr_iter, so that field is pinned by the oracle comparisons of the kernels, not here.)
"""
import builtins
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from gen_golden import REF, Capture, _setup_reference, pack_calls  # noqa: E402

N = 6
STATIC = (31, -3, 8, 6)
MOVING = (35, -16, 34, 34, 1, 1, 1)  # spd 1, timestep 1, option 1 (up)
PARAM_NAMES = ("tuning_ctrl_q1", "tuning_ctrl_q2", "tuning_obs_q1", "tuning_obs_q2", "safety_margin",
               "lamb_factor", "max_lamb", "eps", "max_ilqr_iter", "a_max", "delta_max")
SYS_NAMES = ("a_max", "delta_max")
# set -> non-default parameters (the rest: the reference's defaults, read back from its objects).
# delta_max 0.904: the reference clips and barriers at round(delta_max, 2) = 0.9
SETS = {
    "ctrl": dict(tuning_ctrl_q1=0.3, tuning_ctrl_q2=2.5),
    "obs": dict(tuning_obs_q1=1.3, tuning_obs_q2=0.9, safety_margin=0.35),
    "lamb3": dict(lamb_factor=3, max_lamb=50, eps=1e-4, max_ilqr_iter=40),
    "box": dict(a_max=0.8, delta_max=0.6),
    "all": dict(tuning_ctrl_q1=2.0, tuning_ctrl_q2=0.5, tuning_obs_q1=0.7, tuning_obs_q2=4.0,
                safety_margin=0.2, lamb_factor=4, max_lamb=300, eps=1e-3, a_max=1.2,
                delta_max=0.904),
}
N_STATES, N_FIRST = 64, 16


def make_params(base, over):
    ilqr = base.iLqrParam(num_horizon=N, timestep=1,
                          **{k: v for k, v in over.items() if k not in SYS_NAMES})
    plant = base.KineticBicycleParam(**{k: v for k, v in over.items() if k in SYS_NAMES})
    return ilqr, plant


def call(base, cap, ilqr, plant, x0, x_term, lamb, oargs):
    """The reference's ilqr() the way iLqr.calc_input calls it (utils/base.py:405-426)."""
    uvar = np.zeros((2, N))
    xvar = np.zeros((4, N + 1))
    xvar[:, 0] = x0
    dX = np.zeros((4, N + 1))
    dX[:, 0] = xvar[:, 0]
    n_before = len(cap.calls)
    base.ilqr(ilqr, N, np.array([0, 0, 0, 0]), 1, base.Obstacle(*oargs), plant,
              np.array(x_term, float), dX, uvar, xvar, lamb)
    return cap.calls[n_before]


def main():
    out = Path(__file__).resolve().parent.parent / "tests" / "golden"
    _setup_reference()
    real_print = builtins.print
    builtins.print = lambda *a, **k: None  # the reference prints in its hot loop
    from utils import base
    import control.iterative_ilqr as core

    cap = Capture(base, core)
    traj = np.loadtxt(REF / "data" / "closed_loop_feasible.txt")
    # preferred states: 64 spread over the lap; replacements: the states in between, in order
    first = [int(s) for s in (np.arange(N_STATES) * 15) // 8]
    order = first + [s for s in range(120) if s not in first]
    res = {"param_names": np.array(PARAM_NAMES)}
    for name, over in SETS.items():
        ilqr, plant = make_params(base, over)
        res[name + "_params"] = np.array([float(getattr(plant if p in SYS_NAMES else ilqr, p))
                                          for p in PARAM_NAMES])
        recs, dropped = [], 0
        quota = {STATIC: N_STATES, MOVING: N_STATES}
        for swap in (0, 1):
            for pos, s in enumerate(order):
                oargs = (STATIC, MOVING)[(pos + swap) % 2]
                x_term = traj[min(s + N, 120)]
                for lamb in (1.0, 1e-3):
                    if quota[oargs] == 0:
                        break
                    runs = [call(base, cap, ilqr, plant, x0, x_term, lamb, oargs)
                            for x0 in (traj[s], np.nextafter(traj[s], np.inf),
                                       np.nextafter(traj[s], -np.inf), traj[s] * (1 + 1e-13),
                                       traj[s] * (1 - 1e-13))]
                    if all(r["iters"] == runs[0]["iters"] and r["lamb_out"] == runs[0]["lamb_out"]
                           for r in runs[1:]):
                        recs.append(runs[0])
                        quota[oargs] -= 1
                    else:
                        dropped += 1
            if not any(quota.values()):
                break
        assert not any(quota.values()), (name, quota)
        real_print(f"{name}: {len(recs)} calls, iterations {min(r['iters'] for r in recs)}.."
                   f"{max(r['iters'] for r in recs)}; {dropped} round-off ties of the reference dropped")
        for key, arr in pack_calls(recs).items():
            res[f"{name}_{key}"] = arr
        firsts, src, which = [], [], []
        for i in range(0, len(recs), len(recs) // N_FIRST):
            for key, itn in (("_first", 1), ("_third", 3)):
                if key in recs[i] and "X_new" in recs[i][key]:
                    firsts.append(recs[i][key])
                    src.append(i)
                    which.append(itn)
        for key in ("X", "U", "lamb", "k", "K", "X_new", "U_new", "cost_new"):
            res[f"{name}_iter_{key}"] = np.stack([np.asarray(f[key], float) for f in firsts])
        res[f"{name}_iter_x_term"] = np.stack([recs[i]["x_term"] for i in src])
        res[f"{name}_iter_obs"] = np.stack([recs[i]["obs"] for i in src])
        res[f"{name}_iter_iteration"] = np.array(which, np.int32)
    cap.restore()
    builtins.print = real_print
    path = out / "g9_config_fields.npz"
    np.savez_compressed(path, **res)
    print("wrote", path.name, f"{path.stat().st_size / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
