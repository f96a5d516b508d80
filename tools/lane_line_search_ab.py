#!/usr/bin/env python3
"""A/B of "lane_line_search" (include/i2lqr.h) against the lane kernels it extends and against the
one-problem-per-wavefront kernel with the same line search, in ONE process:

    lane_line_search_ab.py [--out FILE] [--reps R] [--batches 4096,16384,65536] [--step-limit SECONDS]
                           [--dtypes f64,f32] [--weights]

bicycle6, N = 20, fp64 and fp32, the same problems for every variant (workloads.make_batch, two
records of workloads.obstacles_on_path, the box v in [0, 10]), with the soft accept test and with the
barrier cost, time per 10 fixed iterations of
  lane A1          k_lane_iterate_model / k_lane_iterate_merit: the option off   (batch-minor handle)
  lane A2, A4, A8  k_lane_iterate_ls: the same handle with "lane_line_search" A
  wave A2, A4, A8  k_iterate_box / k_iterate_merit with "line_search" A          (problem-major handle)
- device events, median over the repetitions, the variants alternating inside every repetition,
every launch on a fresh copy of the batch (copied outside the timed region).  Every GPU step (a
copy, a launch and its wait) runs under an alarm of --step-limit seconds whose default action ends
the process: a step that hangs is not followed by another.  After the timed repetitions every
variant solves the batch once to termination: its LAMB_OVERFLOW exits.
Writes JSON (default profiles/lane_line_search_ab.json) with, per precision, accept test and batch,
each variant's time, accepted share and LAMB_OVERFLOW exits, "lane A" as a multiple of "lane A1" (the
cost of the candidates: near A would mean the loads are repeated per candidate) and of "wave A" (the
gain of the feature).  --weights: the same with stage weights Q, R != 0 (in fp64 the instantiations of
bicycle6 whose trial passes hold two candidates: A = 4 is two passes, A = 8 four).  Not part of
bench.py, not a test.
"""
import argparse
import json
import signal
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads
from lane_models_ab import base_set, fresh
from obstacles_ab import timed

STEPS = (2, 4, 8)
VARIANTS = ("lane A1",) + tuple(f"lane A{A}" for A in STEPS) + tuple(f"wave A{A}" for A in STEPS)
RECORDS = 2
ST_LAMB_OVERFLOW = 3


def make_solver(cfg, variant, merit):
    lane, A = variant.startswith("lane"), int(variant.split("A")[1])
    c = cfg.copy()
    c.layout = 1 if lane else 0
    solver = BatchedILQR(c)
    if lane:
        solver.set_option("lane_models", 1)
    solver.set_option("obstacles", RECORDS)
    lo, hi = np.full(cfg.n, -np.inf), np.full(cfg.n, np.inf)
    lo[2], hi[2] = 0.0, 10.0
    solver.set_state_box(lo, hi)
    if merit:
        solver.set_option("lane_barrier_cost" if lane else "barrier_cost", 1)
    if A > 1:
        solver.set_option("lane_line_search" if lane else "line_search", A)
    return solver


def measure(cfg, B, merit, reps, limit):
    host = workloads.make_batch(cfg, B)
    obs = workloads.obstacles_on_path(host, RECORDS)
    solvers = {v: make_solver(cfg, v, merit) for v in VARIANTS}
    base = {v: base_set(solvers[v], host, obs) for v in VARIANTS}
    ms = {v: [] for v in VARIANTS}
    last = {}
    for r in range(reps + 1):  # (repetition 0 warms every variant up)
        for v in VARIANTS:
            signal.alarm(limit)  # (no handler: a step that does not return ends the process)
            work = fresh(base[v])
            ms[v].append(timed(lambda: solvers[v].iterate(work, 10)))
            signal.alarm(0)
            last[v] = work
    rows = {}
    for v in VARIANTS:
        t = np.array(ms[v][1:])
        # lamb_out = lamb_in * factor^(rejects - accepts) over 10 iterations, lamb_in = 1
        j = np.rint(np.log(last[v]["lamb"].double().cpu().numpy()) / np.log(cfg.lamb_factor))
        signal.alarm(limit)
        work = fresh(base[v])
        solvers[v].solve(work)
        exits = int((work["status"] == ST_LAMB_OVERFLOW).sum().item())
        signal.alarm(0)
        rows[v] = dict(kernel=solvers[v].iterate_kernel(B), iterate10_ms_median=float(np.median(t)),
                       iterate10_ms_min=float(t.min()), iterate10_ms_max=float(t.max()),
                       accepted_share=float(((10 - j) / 2).mean() / 10),
                       solve_lamb_overflow_exits=exits)
    med = lambda v: rows[v]["iterate10_ms_median"]
    for A in STEPS:
        row = rows[f"lane A{A}"]
        row["iterate10_over_lane_A1"] = med(f"lane A{A}") / med("lane A1")
        row["iterate10_over_wave"] = med(f"lane A{A}") / med(f"wave A{A}")
        # the two kernels with the line search run the same problems: how far their branches agree
        same = (last[f"lane A{A}"]["lamb"].double().cpu().numpy() ==
                last[f"wave A{A}"]["lamb"].double().cpu().numpy())
        row["same_lamb_as_wave"] = float(same.mean())
    for s in solvers.values():
        s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" /
                                         "lane_line_search_ab.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="4096,16384,65536")
    ap.add_argument("--step-limit", type=int, default=60)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--weights", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lane_line_search_ab.py needs a HIP device")
    batches = [int(b) for b in args.batches.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "stage_weights": args.weights,
           "note": "bicycle6 N=20, two records and the box v in [0, 10], batch-minor; \"lane A1\": "
                   "k_lane_iterate_model (soft) / k_lane_iterate_merit (barrier cost), the option off; "
                   "\"lane A\": k_lane_iterate_ls on the same handle with \"lane_line_search\" A; "
                   "\"wave A\": k_iterate_box / k_iterate_merit on a problem-major handle with "
                   "\"line_search\" A and the same problems; ms per 10 fixed iterations from device "
                   "events, median of the repetitions; solve_lamb_overflow_exits: one solve to "
                   "termination of the same batch",
           "configurations": []}
    for dtype in args.dtypes.split(","):
        cfg = default_config("bicycle6", 20, dtype, dt=0.25)
        if args.weights:
            cfg.set_matrix("Q", np.diag([0.01, 0.02, 0.1, 0.05, 0.03, 0.04]) + 0.001)
            cfg.set_matrix("R", np.array([[0.05, 0.01], [0.01, 0.08]]))
            cfg.xtarget[:6] = [1.0, -1.0, 2.0, 0.1, 0.0, 0.0]
        for merit in (False, True):
            for B in batches:
                rows = measure(cfg, B, merit, args.reps, args.step_limit)
                doc["configurations"].append(dict(
                    name=f"bicycle6 N=20 {dtype}" + (" stage weights" if args.weights else ""),
                    dtype=dtype, B=B,
                    accept="barrier cost" if merit else "soft", variants=rows))
                for v, row in rows.items():
                    print(f"{dtype} {'merit' if merit else 'soft ':5s} B={B:6d} {v:8s}: 10 iterations "
                          f"{row['iterate10_ms_median']:9.4f} ms [{row['iterate10_ms_min']:.4f}, "
                          f"{row['iterate10_ms_max']:.4f}]  x lane A1 "
                          f"{row.get('iterate10_over_lane_A1', float('nan')):6.3f}  x wave "
                          f"{row.get('iterate10_over_wave', float('nan')):6.3f}  accepted "
                          f"{row['accepted_share']:.0%}  overflow exits "
                          f"{row['solve_lamb_overflow_exits']}  {row['kernel']}", flush=True)
                # (written after every configuration: a run that is cut short keeps what it measured)
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
