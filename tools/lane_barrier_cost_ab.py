#!/usr/bin/env python3
"""A/B of "lane_barrier_cost" (include/i2lqr.h) against the lane kernel it extends and against the
one-problem-per-wavefront kernel with the same merit, in ONE process:

    lane_barrier_cost_ab.py [--out FILE] [--reps R] [--batches 4096,16384,65536] [--step-limit SECONDS]

bicycle6, N = 20, fp64 and fp32, the same problems for every variant (workloads.make_batch, two
records of workloads.obstacles_on_path, the box v in [0, 10]), time per 10 fixed iterations of
  model        k_lane_iterate_model: "lane_models" 1, soft accept test      (batch-minor handle)
  merit        k_lane_iterate_merit: the same handle with "lane_barrier_cost" 1
  wave merit   k_iterate_merit: "barrier_cost" 1                           (problem-major handle)
- device events, median over the repetitions, the variants alternating inside every repetition,
every launch on a fresh copy of the batch (copied outside the timed region).  Every GPU step (a
copy, a launch and its wait) runs under an alarm of --step-limit seconds whose default action ends
the process: a step that hangs is not followed by another.
Writes JSON (default profiles/lane_barrier_cost_ab.json) with, per precision and batch, each
variant's time and accepted share (it moves with the merit), "merit" as a multiple of "model" (the
cost of the penalty) and of "wave merit" (the gain of the feature), and per precision the smallest
measured batch from which "merit" is ahead of "wave merit".  Not part of bench.py, not a test.
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

VARIANTS = ("model", "merit", "wave merit")
RECORDS = 2


def make_solver(cfg, variant):
    lane = variant != "wave merit"
    c = cfg.copy()
    c.layout = 1 if lane else 0
    solver = BatchedILQR(c)
    if lane:
        solver.set_option("lane_models", 1)
    solver.set_option("obstacles", RECORDS)
    lo, hi = np.full(cfg.n, -np.inf), np.full(cfg.n, np.inf)
    lo[2], hi[2] = 0.0, 10.0
    solver.set_state_box(lo, hi)
    if variant != "model":
        solver.set_option("lane_barrier_cost" if lane else "barrier_cost", 1)
    return solver


def measure(cfg, B, reps, limit):
    host = workloads.make_batch(cfg, B)
    obs = workloads.obstacles_on_path(host, RECORDS)
    solvers = {v: make_solver(cfg, v) for v in VARIANTS}
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
        rows[v] = dict(kernel=solvers[v].iterate_kernel(B), iterate10_ms_median=float(np.median(t)),
                       iterate10_ms_min=float(t.min()), iterate10_ms_max=float(t.max()),
                       accepted_share=float(((10 - j) / 2).mean() / 10))
    med = lambda v: rows[v]["iterate10_ms_median"]
    rows["merit"]["iterate10_over_model"] = med("merit") / med("model")
    rows["merit"]["iterate10_over_wave_merit"] = med("merit") / med("wave merit")
    # the two kernels with the merit run the same problems: how far their branches agree
    same = last["merit"]["lamb"].double().cpu().numpy() == last["wave merit"]["lamb"].double().cpu().numpy()
    rows["merit"]["same_lamb_as_wave_merit"] = float(same.mean())
    for s in solvers.values():
        s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" /
                                         "lane_barrier_cost_ab.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="4096,16384,65536")
    ap.add_argument("--step-limit", type=int, default=60)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lane_barrier_cost_ab.py needs a HIP device")
    batches = [int(b) for b in args.batches.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "note": "bicycle6 N=20, two records and the box v in [0, 10]; \"model\": "
                   "k_lane_iterate_model (soft accept test); \"merit\": k_lane_iterate_merit on the "
                   "same handle shape; \"wave merit\": k_iterate_merit on a problem-major handle with "
                   "the same problems; ms per 10 fixed iterations from device events, median of the "
                   "repetitions",
           "configurations": [], "lane_side_wins_from": {}}
    for dtype in ("f64", "f32"):
        cfg = default_config("bicycle6", 20, dtype, dt=0.25)
        wins = {}
        for B in batches:
            rows = measure(cfg, B, args.reps, args.step_limit)
            doc["configurations"].append(dict(name=f"bicycle6 N=20 {dtype}", dtype=dtype, B=B,
                                              variants=rows))
            wins[B] = rows["merit"]["iterate10_over_wave_merit"] < 1.0
            for v, row in rows.items():
                print(f"{dtype} B={B:6d} {v:10s}: 10 iterations {row['iterate10_ms_median']:9.4f} ms "
                      f"[{row['iterate10_ms_min']:.4f}, {row['iterate10_ms_max']:.4f}]  x model "
                      f"{row.get('iterate10_over_model', float('nan')):6.3f}  x wave merit "
                      f"{row.get('iterate10_over_wave_merit', float('nan')):6.3f}  accepted "
                      f"{row['accepted_share']:.0%}  {row['kernel']}", flush=True)
        # the smallest measured batch from which the lane side wins at every larger one too
        first = None
        for B in sorted(batches, reverse=True):
            if not wins[B]:
                break
            first = B
        doc["lane_side_wins_from"][dtype] = first
        print(f"{dtype}: the lane kernel with the barrier cost wins from {first} problems "
              f"(measured: {sorted(batches)})", flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
