#!/usr/bin/env python3
"""A/B of "lane_rows_models" (include/i2lqr.h) against quad12's plain row-block lane kernel, against
the parent commit's build of it and against the one-problem-per-wavefront kernels of the same models,
in ONE process:

    lane_rows_models_ab.py [--parent-lib FILE] [--out FILE] [--reps R] [--batches 4096,16384,65536]
                           [--step-limit SECONDS]

quad12, N = 50, dt = 0.02, fp64 and fp32, the same problems for every variant (workloads.make_batch,
records of workloads.obstacles_on_path), time per 10 fixed iterations of
  rows parent / parent'  k_lane_iterate_rows of the library --parent-lib names (the parent commit's
                         build), two handles: their ratio is the run's A/A band
  rows off               k_lane_iterate_rows of this build, "lane_models" 1 and "lane_rows_models" 1
                         with no model set                                   (batch-minor handles)
  model K2 / K4 / K8     k_lane_iterate_rows_model with 2 / 4 / 8 records
  model box 1 / box n    k_lane_iterate_rows_model with one record and 1 / 12 bounded components
  wave K2 / K4 / K8      k_iterate_obs with the same records              (problem-major handle)
  wave box 1 / box n     k_iterate_box with the same box
- device events, median over the repetitions, the variants alternating inside every repetition,
every launch on a fresh copy of the batch (copied outside the timed region).  Every GPU step (a copy,
a launch and its wait) runs under an alarm of --step-limit seconds whose default action ends the
process: a step that hangs is not followed by another.
Writes JSON (default profiles/lane_rows_models_ab.json) with, per precision and batch, the A/A band,
"rows off" as a multiple of "rows parent", each model variant as a multiple of "rows off" (the cost
of the model) and of its wavefront counterpart (the gain of the feature), and per precision the
smallest measured batch from which every model variant is ahead of its wavefront counterpart.  Not
part of bench.py, not a test.
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

PARENT = ("rows parent", "rows parent'")
MODEL = ("model K2", "model K4", "model K8", "model box 1", "model box n")
WAVE = {"model K2": "wave K2", "model K4": "wave K4", "model K8": "wave K8",
        "model box 1": "wave box 1", "model box n": "wave box n"}


def make_solver(cfg, variant, parent_lib):
    lane = not variant.startswith("wave")
    c = cfg.copy()
    c.layout = 1 if lane else 0
    if variant in PARENT:
        return BatchedILQR(c, lib_path=parent_lib)
    solver = BatchedILQR(c)
    if lane:
        solver.set_option("lane_models", 1)
        solver.set_option("lane_rows_models", 1)
    else:
        solver.set_option("group_lanes", 64)
    if variant == "rows off":
        return solver
    what = variant.split(" ", 1)[1]
    if what.startswith("K"):
        solver.set_option("obstacles", int(what[1:]))
    else:
        lo, hi = np.full(cfg.n, -np.inf), np.full(cfg.n, np.inf)
        if what == "box n":
            lo[:], hi[:] = -1000.0, 1000.0
        lo[2], hi[2] = -0.05, 0.05  # z, the box of the tests
        solver.set_state_box(lo, hi, 1.0, 20.0)
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


def measure(cfg, B, reps, limit, parent_lib):
    variants = (PARENT if parent_lib else ()) + ("rows off",) + MODEL + tuple(WAVE.values())
    host = workloads.make_batch(cfg, B)
    solvers = {v: make_solver(cfg, v, parent_lib) for v in variants}
    base = {v: base_set(solvers[v], host, records(host, v)) for v in variants}
    ms = {v: [] for v in variants}
    last = {}
    for r in range(reps + 1):  # (repetition 0 warms every variant up)
        for v in variants:
            signal.alarm(limit)  # (no handler: a step that does not return ends the process)
            work = fresh(base[v])
            ms[v].append(timed(lambda: solvers[v].iterate(work, 10)))
            signal.alarm(0)
            last[v] = work
    rows = {}
    for v in variants:
        t = np.array(ms[v][1:])
        # lamb_out = lamb_in * factor^(rejects - accepts) over 10 iterations, lamb_in = 1
        j = np.rint(np.log(last[v]["lamb"].double().cpu().numpy()) / np.log(cfg.lamb_factor))
        rows[v] = dict(kernel=solvers[v].iterate_kernel(B), iterate10_ms_median=float(np.median(t)),
                       iterate10_ms_min=float(t.min()), iterate10_ms_max=float(t.max()),
                       M_it_per_s=float(B * 10 / np.median(t) / 1e3),
                       accepted_share=float(((10 - j) / 2).mean() / 10))
    med = lambda v: rows[v]["iterate10_ms_median"]
    summary = {}
    if parent_lib:
        summary["aa_band"] = med(PARENT[1]) / med(PARENT[0])
        summary["off_over_parent"] = med("rows off") / med(PARENT[0])
        # the option-off kernel must not differ from the parent's by more than the parent from itself
        spread = abs(summary["aa_band"] - 1.0)
        summary["off_inside_aa_band"] = bool(abs(summary["off_over_parent"] - 1.0) <= max(spread, 0.01))
    for v in MODEL:
        rows[v]["iterate10_over_rows_off"] = med(v) / med("rows off")
        rows[v]["iterate10_over_wave"] = med(v) / med(WAVE[v])
    for s in solvers.values():
        s.close()
    return rows, summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" /
                                         "lane_rows_models_ab.json"))
    ap.add_argument("--parent-lib", default=None, help="libi2lqr_hip.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="4096,16384,65536")
    ap.add_argument("--step-limit", type=int, default=60)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lane_rows_models_ab.py needs a HIP device")
    batches = [int(b) for b in args.batches.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "note": "quad12 N=50 dt=0.02; \"rows parent\" / \"rows parent'\": k_lane_iterate_rows of the "
                   "parent commit's library, two handles (their ratio: the A/A band; \"off inside the "
                   "band\" allows max(|band - 1|, 1 %)); \"rows off\": this build with "
                   "\"lane_rows_models\" 1 and no model; \"model ...\": k_lane_iterate_rows_model; "
                   "\"wave ...\": k_iterate_obs / k_iterate_box on a problem-major handle with the "
                   "same problems; ms per 10 fixed iterations from device events, median of the "
                   "repetitions, variants interleaved in one process",
           "configurations": [], "lane_side_wins_from": {}}
    for dtype in ("f64", "f32"):
        cfg = default_config("quad12", 50, dtype, dt=0.02)
        wins = {}
        for B in batches:
            rows, summary = measure(cfg, B, args.reps, args.step_limit, args.parent_lib)
            doc["configurations"].append(dict(name=f"quad12 N=50 {dtype}", dtype=dtype, B=B,
                                              variants=rows, **summary))
            wins[B] = all(rows[v]["iterate10_over_wave"] < 1.0 for v in MODEL)
            for v, row in rows.items():
                print(f"{dtype} B={B:6d} {v:13s}: 10 iterations {row['iterate10_ms_median']:9.4f} ms "
                      f"[{row['iterate10_ms_min']:.4f}, {row['iterate10_ms_max']:.4f}] "
                      f"{row['M_it_per_s']:6.1f} M it/s  x off "
                      f"{row.get('iterate10_over_rows_off', float('nan')):6.3f}  x wave "
                      f"{row.get('iterate10_over_wave', float('nan')):6.3f}  accepted "
                      f"{row['accepted_share']:.0%}  {row['kernel']}", flush=True)
            if summary:
                print(f"{dtype} B={B:6d} A/A band {summary['aa_band']:.4f}, off / parent "
                      f"{summary['off_over_parent']:.4f}, inside: {summary['off_inside_aa_band']}",
                      flush=True)
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
