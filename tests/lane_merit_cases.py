"""The run table of "lane_barrier_cost" (include/i2lqr.h: k_lane_iterate_merit, the barrier cost on the
one-problem-per-lane kernel), not a test module: test_lane_barrier_cost_host.py shows every run to be
well conditioned on the CPU, test_gpu_lane_barrier_cost.py runs them on the kernel.  The problem sets,
the boxes and the conditioning rule (MARGIN, MAX_LEFT_OUT) are opt_in_cases.py's."""
import functools

from opt_in_cases import make_case
from opt_in_reference import reference

# (BOXES entry, fixed iterations or None for a solve to termination, layout: 1 batch-minor, 2
# batch-tiled).  The fixed counts are short on purpose, as MERIT_RUNS' are: near the optimum J_new
# and J agree to round-off and the branch is not decidable.
LANE_MERIT_RUNS = (
    [(case, 3, 1) for case in ("b4", "b4_hi_only", "b4_weights", "b6", "b4_N7", "b6_B1", "b6_B5",
                               "b4_K2", "b6_K2")] +
    [(case, 2, 1) for case in ("b4_N1", "b6_N1")] +
    [(case, None, 1) for case in ("b4", "b6", "b4_K2", "b6_K2")] +
    [(case, n, 2) for case in ("b4_T128_K2", "b6_T128_K3") for n in (3, None)])
LANE_MERIT_TERMINATION_RUNS = [run for run in LANE_MERIT_RUNS if run[1] is None]
LANE_MERIT_TILED = ("b4_T128_K2", "b6_T128_K3")

# LAMB_OVERFLOW exits of the termination runs on the host reference with the box on, soft accept
# test -> barrier cost (README.md)
LAMB_OVERFLOW_EXITS = {"b4": (19, 9), "b6": (17, 5), "b4_K2": (39, 17), "b6_K2": (38, 0),
                       "b4_T128_K2": (80, 28), "b6_T128_K3": (84, 2)}


def run_id(case, n_iters, layout):
    return f"{case}-{'solve' if n_iters is None else n_iters}-{'minor' if layout == 1 else 'tiled'}"


IDS = [run_id(*run) for run in LANE_MERIT_RUNS]
TERMINATION_IDS = [run_id(*run) for run in LANE_MERIT_TERMINATION_RUNS]


@functools.lru_cache(maxsize=None)
def lane_merit_reference(case, n_iters, layout=1, merit=True, boxed=True):
    """reference() of a BOXES entry (boxed: with its box), one step size; computed once per run and
    shared - callers do not modify it."""
    cfg, host, box = make_case(case, box=True, layout=layout)
    return reference(cfg, host, box=box if boxed else None, merit=merit, max_iter=n_iters,
                     early_exit=n_iters is None)
