"""The run tables of "lane_barrier_cost" and "lane_line_search" (include/i2lqr.h: k_lane_iterate_merit
and k_lane_iterate_ls, the barrier cost and the line search on the one-problem-per-lane kernel), not
a test module: test_lane_barrier_cost_host.py / test_lane_line_search_host.py show every run to be
well conditioned on the CPU, test_gpu_lane_barrier_cost.py / test_gpu_lane_line_search.py run them
on the kernels.  The problem sets, the boxes, the tiled sets (TILED) and the conditioning rule (MARGIN,
MAX_LEFT_OUT) are opt_in_cases.py's; every set is boxed."""
import functools

import numpy as np

from opt_in_cases import SEED, TILED, make_case
from opt_in_reference import Box, reference

# bicycle6 in fp64 with stage weights: the instantiations whose trial passes hold two candidates, not
# four (kLaneLsGroup, csrc/i2lqr_lane_ls.hpp) - A = 4 is two passes there and A = 8 four.  No set of
# opt_in_cases.py has this plant with weights, so the two sets are built here as make_case builds
# b4_weights: name -> (problems, layout); N = 20, dt = 0.25, two records, the box v in [0, 10].
WEIGHTED_B6 = {"b6_weights_K2": (67, 1), "b6_T128_weights_K2": (128, 2)}


def make_lane_case(name, layout=1, dtype="f64"):
    """(cfg, host batch, Box): make_case(name, box=True) for a BOXES entry, or a WEIGHTED_B6 set."""
    if name not in WEIGHTED_B6:
        return make_case(name, box=True, dtype=dtype, layout=layout)
    from ilqr_iterative_tasks_amd import default_config, workloads
    cfg = default_config("bicycle6", 20, dtype, dt=0.25, layout=layout)
    cfg.set_matrix("Q", np.diag([0.01, 0.02, 0.1, 0.05, 0.03, 0.04]) + 0.001)
    cfg.set_matrix("R", np.array([[0.05, 0.01], [0.01, 0.08]]))
    cfg.xtarget[:6] = [1.0, -1.0, 2.0, 0.1, 0.0, 0.0]
    host = workloads.make_batch(cfg, WEIGHTED_B6[name][0])
    host = dict(host, obs=workloads.obstacles_on_path(host, 2, SEED, None))
    return cfg, host, Box(cfg.n, {2: (0.0, 10.0)})


def run_id(case, n_iters, layout, A=None, merit=None):
    """case-3-minor of a barrier-cost row; case-A4-solve-tiled-soft of a line-search row."""
    return "-".join([case] + ([] if A is None else [f"A{A}"]) +
                    ["solve" if n_iters is None else str(n_iters), "minor" if layout == 1 else "tiled"] +
                    ([] if merit is None else ["merit" if merit else "soft"]))


# "lane_barrier_cost":
# (BOXES entry, fixed iterations or None for a solve to termination, layout: 1 batch-minor, 2
# batch-tiled).  The fixed counts are short on purpose, as MERIT_RUNS' are: near the optimum J_new
# and J agree to round-off and the branch is not decidable.
LANE_MERIT_RUNS = (
    [(case, 3, 1) for case in ("b4", "b4_hi_only", "b4_weights", "b6", "b4_N7", "b6_B1", "b6_B5",
                               "b4_K2", "b6_K2")] +
    [(case, 2, 1) for case in ("b4_N1", "b6_N1")] +
    [(case, None, 1) for case in ("b4", "b6", "b4_K2", "b6_K2")] +
    [(case, n, 2) for case in TILED for n in (3, None)])
LANE_MERIT_TERMINATION_RUNS = [run for run in LANE_MERIT_RUNS if run[1] is None]
LANE_MERIT_IDS = [run_id(*run) for run in LANE_MERIT_RUNS]
LANE_MERIT_TERMINATION_IDS = [run_id(*run) for run in LANE_MERIT_TERMINATION_RUNS]

# LAMB_OVERFLOW exits of the termination runs on the host reference with the box on, soft accept
# test -> barrier cost (README.md)
LANE_MERIT_LAMB_OVERFLOW_EXITS = {"b4": (19, 9), "b6": (17, 5), "b4_K2": (39, 17), "b6_K2": (38, 0),
                                  "b4_T128_K2": (80, 28), "b6_T128_K3": (84, 2)}


def _rows(merit, n_iters, layout, table):
    return [(case, A, n_iters, layout, merit) for cases, steps in table for case in cases for A in steps]


# "lane_line_search":
# (BOXES entry, step sizes, fixed iterations or None for a solve to termination, layout: 1 batch-minor,
# 2 batch-tiled, barrier cost).  The fixed counts are short on purpose, as MERIT_RUNS' are: near the
# optimum J_new and J agree to round-off and the branch is not decidable.  Not in the table, because
# the reference alone breaks the conditioning rule: b6 with the barrier cost (2 of 67 problems under
# the margin at 3 iterations), b4 A = 8 and b4_N7 A = 4 with it (1), b6_T128_K3 A = 8 soft (1), b4 / b6
# to termination with it (24 / 25 %); b4 and b4_weights soft at A = 8 (margins of 2-3e-7: too thin).
SOFT_RUNS = (
    _rows(False, 3, 1, [(("b4", "b4_weights"), (2, 4)), (("b4_hi_only",), (4,)),
                        (("b6", "b6_K2"), (2, 4, 8)), (("b4_K2", "b4_N7"), (8,)),
                        (("b4_N64", "b6_B1", "b6_B5"), (4,))]) +
    _rows(False, 2, 1, [(("b4_N1", "b6_N1"), (8,))]) +
    _rows(False, None, 1, [(("b4", "b6", "b4_K2", "b6_K2"), (4,))]) +
    _rows(False, 3, 2, [(TILED, (4,))]) + _rows(False, None, 2, [(TILED, (4,))]))
# (opt_in_cases.MERIT_RUNS is the wavefront kernel's table: these are the line search's merit rows)
LS_MERIT_RUNS = (
    _rows(True, 3, 1, [(("b4",), (2, 4)), (("b4_weights", "b4_K2", "b6_K2"), (2, 4, 8)),
                       (("b4_hi_only",), (4,)), (("b4_N7",), (2, 8)),
                       (("b4_N64", "b6_B1", "b6_B5"), (4,))]) +
    _rows(True, 2, 1, [(("b4_N1", "b6_N1"), (8,))]) +
    _rows(True, None, 1, [(("b4_K2", "b6_K2"), (4,))]) +
    _rows(True, 3, 2, [(TILED, (4, 8))]) + _rows(True, None, 2, [(TILED, (4,))]))
# The weighted bicycle6 sets, both layouts, soft and barrier cost, A = 4 and 8.  On the host reference
# every 3-iteration run keeps all its problems but the tiled set with the barrier cost at A = 8 (1 of
# 128 under the margin), which runs 2 iterations instead.  No solves to termination: with A = 4 they
# are not decidable (44 ... 88 problems end on a tie), and with A = 8 the sets take up to the 150
# iterations allowed, 5 ... 14 s of host reference for one row.
WEIGHTED_RUNS = [
    (case, A, 2 if (case, A, merit) == ("b6_T128_weights_K2", 8, True) else 3, layout, merit)
    for case, (_, layout) in WEIGHTED_B6.items() for merit in (False, True) for A in (4, 8)]
LANE_LS_RUNS = SOFT_RUNS + LS_MERIT_RUNS + WEIGHTED_RUNS
# the reference never takes a short step on them: they must equal k_lane_iterate_merit's run bit for bit
FULL_STEP_RUNS = [run for run in LS_MERIT_RUNS if run[0] in ("b4_N1", "b6_N1")]

# problems the conditioning rule leaves out of the termination runs, on the host reference
LEFT_OUT = {("b4", 4, None, 1, False): 0, ("b6", 4, None, 1, False): 0,
            ("b4_K2", 4, None, 1, False): 0, ("b6_K2", 4, None, 1, False): 0,
            ("b4_K2", 4, None, 1, True): 6, ("b6_K2", 4, None, 1, True): 2,
            ("b4_T128_K2", 4, None, 2, True): 12, ("b6_T128_K3", 4, None, 2, True): 7}

# LAMB_OVERFLOW exits of the solves to termination on the host reference, box on: set -> (layout,
# (soft A = 1, soft A = 4, barrier cost A = 1, barrier cost A = 4)) (README.md)
LANE_LS_LAMB_OVERFLOW_EXITS = {"b4_T128_K2": (2, (80, 53, 28, 20)), "b6_T128_K3": (2, (84, 69, 2, 0)),
                               "b4_K2": (1, (39, 31, 17, 8)), "b4": (1, (19, 13, 9, 4))}


def ls_run_ids(runs):
    """The test ids of line-search rows (case, A, n_iters, layout, merit)."""
    return [run_id(case, n_iters, layout, A, merit) for case, A, n_iters, layout, merit in runs]


@functools.lru_cache(maxsize=None)
def _reference(case, A, n_iters, layout, merit, boxed):
    cfg, host, box = make_lane_case(case, layout)
    return reference(cfg, host, A, box=box if boxed else None, merit=merit, max_iter=n_iters,
                     early_exit=n_iters is None)


def lane_reference(case, A=1, n_iters=None, layout=1, merit=False, boxed=True):
    """reference() of a BOXES entry or a WEIGHTED_B6 set (boxed: with its box) and A step sizes;
    computed once per run, however the arguments are spelled, and shared - callers do not modify it."""
    return _reference(case, A, n_iters, layout, merit, boxed)
