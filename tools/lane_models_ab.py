#!/usr/bin/env python3
"""A/B of "lane_models" (include/i2lqr.h) against the plain lane kernel and against the
one-problem-per-wavefront kernels of the same models, in ONE process:

    lane_models_ab.py [--out FILE] [--reps R] [--batches 4096,16384,65536] [--step-limit SECONDS]

bicycle6, N = 20, fp64 and fp32, the same problems for every variant (workloads.make_batch, records
of workloads.obstacles_on_path), time per 10 fixed iterations of
  lane 1w / lane       k_lane_iterate in its one-wavefront form ("helper_wavefront" 0) / as
                       dispatched, one record                              (batch-minor handle)
  model K2 / K4 / K8   k_lane_iterate_model with 2 / 4 / 8 records
  model box 1 / box n  k_lane_iterate_model with one record and 1 / n bounded components
  wave K2 / K4 / K8    k_iterate_obs with the same records              (problem-major handle)
  wave box 1 / box n   k_iterate_box with the same box
— device events, median over the repetitions, the variants alternating inside every repetition,
every launch on a fresh copy of the batch (copied outside the timed region).  Every GPU step (a
copy, a launch and its wait) runs under an alarm of --step-limit seconds whose default action ends
the process: a step that hangs is not followed by another.
Writes JSON (default profiles/lane_models_ab.json) with, per precision and batch, each model
variant as a multiple of "lane 1w" (the cost of the model) and of its wavefront counterpart (the gain
of the feature), and per precision the smallest measured batch from which every model variant is
ahead of its wavefront counterpart.  Not part of bench.py, not a test.
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
from obstacles_ab import timed

LANE = ("lane 1w", "lane")
MODEL = ("model K2", "model K4", "model K8", "model box 1", "model box n")
WAVE = {"model K2": "wave K2", "model K4": "wave K4", "model K8": "wave K8",
        "model box 1": "wave box 1", "model box n": "wave box n"}
VARIANTS = LANE + MODEL + tuple(WAVE.values())


def make_solver(cfg, variant):
    lane = not variant.startswith("wave")
    c = cfg.copy()
    c.layout = 1 if lane else 0
    solver = BatchedILQR(c)
    if variant == "lane 1w":
        solver.set_option("helper_wavefront", 0)
    if variant in LANE:
        return solver
    if lane:
        solver.set_option("lane_models", 1)
    else:
        solver.set_option("group_lanes", 64)
    what = variant.split(" ", 1)[1]
    if what.startswith("K"):
        solver.set_option("obstacles", int(what[1:]))
    else:
        lo, hi = np.full(cfg.n, -np.inf), np.full(cfg.n, np.inf)
        if what == "box n":
            lo[:], hi[:] = -1000.0, 1000.0
        lo[2], hi[2] = 0.0, 10.0
        solver.set_state_box(lo, hi)
    return solver


def records(host, variant):
    what = variant.split(" ", 1)[-1]
    if what.startswith("K"):
        return workloads.obstacles_on_path(host, int(what[1:]))
    return np.ascontiguousarray(workloads.obstacles_on_path(host, 2)[:, 0])


def base_set(solver, host, obs):
    B = host["X"].shape[0]
    dev = lambda a: solver.to_native(torch.as_tensor(np.ascontiguousarray(a)).to(solver.device,
                                                                                 solver.dtype))
    base = solver.alloc(B, want_gains=False)
    for key in ("X", "U", "x_term", "lamb"):
        base[key].copy_(dev(host[key]))
    base["obs"] = dev(obs)
    return base


def fresh(base):
    b2 = dict(base)
    b2.update({k: base[k].clone() for k in ("X", "U", "lamb", "cost", "iters", "status")})
    return b2


def measure(cfg, B, reps, limit):
    host = workloads.make_batch(cfg, B)
    solvers = {v: make_solver(cfg, v) for v in VARIANTS}
    base = {v: base_set(solvers[v], host, records(host, v)) for v in VARIANTS}
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
    rows["lane"]["iterate10_over_lane_1w"] = med("lane") / med("lane 1w")
    for v in MODEL:
        rows[v]["iterate10_over_lane_1w"] = med(v) / med("lane 1w")
        rows[v]["iterate10_over_wave"] = med(v) / med(WAVE[v])
    for s in solvers.values():
        s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" /
                                         "lane_models_ab.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="4096,16384,65536")
    ap.add_argument("--step-limit", type=int, default=60)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lane_models_ab.py needs a HIP device")
    batches = [int(b) for b in args.batches.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "note": "bicycle6 N=20; \"lane 1w\" / \"lane\": k_lane_iterate with \"helper_wavefront\" 0 / "
                   "as dispatched, one record; \"model ...\": k_lane_iterate_model; \"wave ...\": "
                   "k_iterate_obs / k_iterate_box on a problem-major handle with the same problems; "
                   "ms per 10 fixed iterations from device events, median of the repetitions",
           "configurations": [], "lane_side_wins_from": {}}
    for dtype in ("f64", "f32"):
        cfg = default_config("bicycle6", 20, dtype, dt=0.25)
        wins = {}
        for B in batches:
            rows = measure(cfg, B, args.reps, args.step_limit)
            doc["configurations"].append(dict(name=f"bicycle6 N=20 {dtype}", dtype=dtype, B=B,
                                              variants=rows))
            wins[B] = all(rows[v]["iterate10_over_wave"] < 1.0 for v in MODEL)
            for v, row in rows.items():
                print(f"{dtype} B={B:6d} {v:12s}: 10 iterations {row['iterate10_ms_median']:9.4f} ms "
                      f"[{row['iterate10_ms_min']:.4f}, {row['iterate10_ms_max']:.4f}]  x lane 1w "
                      f"{row.get('iterate10_over_lane_1w', 1.0):6.3f}  x wave "
                      f"{row.get('iterate10_over_wave', float('nan')):6.3f}  accepted "
                      f"{row['accepted_share']:.0%}  {row['kernel']}", flush=True)
        # the smallest measured batch from which the lane side wins at every larger one too
        first = None
        for B in sorted(batches, reverse=True):
            if not wins[B]:
                break
            first = B
        doc["lane_side_wins_from"][dtype] = first
        print(f"{dtype}: the lane side wins from {first} problems (measured: {sorted(batches)})",
              flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
