#!/usr/bin/env python3
"""A/B of the state box (i2lqr_set_state_box, include/i2lqr.h) against k_iterate and k_iterate_obs in
ONE process:

    state_box_ab.py [--out FILE] [--reps R]

For bicycle6 N = 20 fp64 at 256 and 1024 problems and bicycle4 N = 6 fp64 at 16 (obstacles_ab.py's
configurations), one obstacle record per problem everywhere: k_iterate as dispatched ("group_lanes"
64), k_iterate_obs with that one record ("obstacles" 2, the second record disabled), and
k_iterate_box with 1 bounded component (v in [0, 10]) and with all n bounded (+-1000 on the others:
the barrier's arithmetic runs, its terms vanish): time per 10 fixed iterations — device events,
median over the repetitions, the variants alternating inside every repetition, every launch on its
own copy of the batch — and the share of the 10 iterations that were accepted.
Writes JSON (default profiles/state_box_ab.json).  Not part of bench.py, not a test.
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from ilqr_iterative_tasks_amd import BatchedILQR, workloads
from obstacles_ab import configurations, device_sets, timed

VARIANTS = ("k_iterate", "obs 1", "box 1", "box n")


def make_solver(cfg, variant):
    solver = BatchedILQR(cfg)
    solver.set_option("group_lanes", 64)
    if variant == "obs 1":
        solver.set_option("obstacles", 2)
    if variant.startswith("box"):
        lo, hi = np.full(cfg.n, -np.inf), np.full(cfg.n, np.inf)
        if variant == "box n":
            lo[:], hi[:] = -1000.0, 1000.0
        lo[2], hi[2] = 0.0, 10.0
        solver.set_state_box(lo, hi)
    return solver


def records(host, variant):
    one = np.ascontiguousarray(workloads.obstacles_on_path(host, 2)[:, 0])
    if variant != "obs 1":
        return one
    two = np.stack([one, one], axis=1)
    two[:, 1, 5] = -1.0  # the second record is disabled: one record's work
    return two


def measure(cfg, B, reps):
    host = workloads.make_batch(cfg, B)
    solvers = {v: make_solver(cfg, v) for v in VARIANTS}
    sets = {v: device_sets(solvers[v], host, records(host, v), reps + 1) for v in VARIANTS}
    ms = {v: [] for v in VARIANTS}
    for r in range(reps + 1):  # (repetition 0 warms every variant up)
        for v in VARIANTS:
            ms[v].append(timed(lambda: solvers[v].iterate(sets[v][r], 10)))
    rows = {}
    for v in VARIANTS:
        t = np.array(ms[v][1:])
        # lamb_out = lamb_in * factor^(rejects - accepts) over 10 iterations, lamb_in = 1
        j = np.rint(np.log(sets[v][-1]["lamb"].cpu().numpy()) / np.log(cfg.lamb_factor))
        rows[v] = dict(kernel=solvers[v].iterate_kernel(B), iterate10_ms_median=float(np.median(t)),
                       iterate10_ms_min=float(t.min()), iterate10_ms_max=float(t.max()),
                       accepted_share=float(((10 - j) / 2).mean() / 10))
    for v in VARIANTS[1:]:
        rows[v]["iterate10_over_k_iterate"] = (rows[v]["iterate10_ms_median"] /
                                               rows["k_iterate"]["iterate10_ms_median"])
        rows[v]["iterate10_over_k_iterate_obs"] = (rows[v]["iterate10_ms_median"] /
                                                   rows["obs 1"]["iterate10_ms_median"])
    for s in solvers.values():
        s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" /
                                         "state_box_ab.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("state_box_ab.py needs a HIP device")
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "note": "\"k_iterate\": as dispatched with \"group_lanes\" 64; \"obs 1\": k_iterate_obs "
                   "with one enabled record; \"box 1\" / \"box n\": k_iterate_box with 1 / n bounded "
                   "components; times from device events",
           "configurations": []}
    for name, cfg, B in configurations():
        rows = measure(cfg, B, args.reps)
        doc["configurations"].append(dict(name=name, B=B, variants=rows))
        for v, row in rows.items():
            print(f"{name:20s} B={B:5d} {v:10s}: 10 iterations {row['iterate10_ms_median']:.4f} ms "
                  f"[{row['iterate10_ms_min']:.4f}, {row['iterate10_ms_max']:.4f}]  x k_iterate "
                  f"{row.get('iterate10_over_k_iterate', 1.0):.3f}  x k_iterate_obs "
                  f"{row.get('iterate10_over_k_iterate_obs', 1.0):.3f}  accepted "
                  f"{row['accepted_share']:.0%}  {row['kernel']}", flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
