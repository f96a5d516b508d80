#!/usr/bin/env python3
"""Host time per call of the one-problem-per-lane launcher (csrc/i2lqr_lane_launch.hpp, its decisions
in csrc/i2lqr_lane_plan.hpp) against another build of the library, in ONE process:

    lane_plan_host_ab.py --other LIB [--out FILE] [--reps R]

The sibling of tools/wave_opt_host_ab.py for the lane layouts; same method, same rule.  LIB is the
parent commit's libi2lqr_hip.so, whose kernels are the same instructions
(tools/compare_kernel_listings.py), so only the host path of a call can differ.  Two calls on a
batch-minor bicycle6, N = 20, dt = 0.25, fp64 handle with 4161 problems:
  iterate   i2lqr_iterate, 10 iterations             (one launch)
  solve     i2lqr_solve with set_compaction(64)      (the chunked solve: about seven launches)
Three variants: "parent", "parent again" (two handles on LIB: their difference is the run's A/A
spread) and "new" (this tree's library).  Every repetition restores each variant's inputs, waits for
the device, then takes the host clock around the C call alone (call_us: the enqueue, what the
launcher's host code costs) and around the call and the synchronisation that follows (call_sync_us);
the variants alternate inside a repetition and their order rotates.  The arguments are converted to
ctypes once, outside the clock.  Rule of profiles/iterate_refactor.md: "new" may exceed the faster
parent median by no more than the two parent medians differ.  All three must return the same bits.
Writes JSON (default profiles/lane_plan_host_ab.json).  Not part of bench.py, not a test.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from ilqr_iterative_tasks_amd import BatchedILQR, _abi, workloads

B, HORIZON = 4161, 20
VARIANTS = ("parent", "parent again", "new")
KEYS = ("X", "U", "lamb", "cost", "iters", "status", "K", "k")


def make(cfg, host, lib_path, solve):
    solver = BatchedILQR(cfg, lib_path=lib_path)
    if solve:
        solver.set_compaction(64)
    buf = solver.alloc(B)
    for key in ("X", "U", "x_term", "lamb"):
        buf[key].copy_(solver.to_native(torch.as_tensor(host[key]).to(solver.device, solver.dtype)))
    buf["obs"] = solver.to_native(torch.as_tensor(host["obs"]).to(solver.device, solver.dtype))
    start = {k: buf[k].clone() for k in ("X", "U", "lamb")}
    args = solver._iter_args(buf, B)
    stream = solver._stream()
    if solve:
        call = lambda: solver.lib.i2lqr_solve(solver._handle, B, *args, stream)
    else:
        call = lambda: solver.lib.i2lqr_iterate(solver._handle, B, 10, *args, stream)
    return dict(solver=solver, buf=buf, start=start, call=call)


def measure(cfg, host, libs, solve, reps):
    runs = {v: make(cfg, host, libs[v], solve) for v in VARIANTS}
    us = {v: ([], []) for v in VARIANTS}
    for r in range(reps + 20):  # (the first 20 repetitions warm every variant up)
        order = [VARIANTS[(r + i) % 3] for i in range(3)]
        for v in order:
            run = runs[v]
            for k, t in run["start"].items():
                run["buf"][k].copy_(t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = run["call"]()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert rc == 0, (v, rc, run["solver"].lib.i2lqr_last_error())
            if r >= 20:
                us[v][0].append((t1 - t0) * 1e6)
                us[v][1].append((t2 - t0) * 1e6)
    outs = {v: {k: runs[v]["buf"][k].cpu().numpy() for k in KEYS} for v in VARIANTS}
    same = all(np.array_equal(outs["new"][k], outs[v][k], equal_nan=True)
               for v in VARIANTS for k in KEYS)
    new = runs["new"]["solver"]
    kernel = new.solve_kernel(B) if solve else new.iterate_kernel(B)
    row = dict(kernel=kernel, identical_outputs=bool(same), variants={})
    for v in VARIANTS:
        c, s = np.array(us[v][0]), np.array(us[v][1])
        row["variants"][v] = dict(
            call_us_median=float(np.median(c)), call_us_q1=float(np.quantile(c, 0.25)),
            call_us_q3=float(np.quantile(c, 0.75)), call_sync_us_median=float(np.median(s)),
            call_sync_us_q1=float(np.quantile(s, 0.25)), call_sync_us_q3=float(np.quantile(s, 0.75)))
    for metric in ("call_us_median", "call_sync_us_median"):
        a, b = (row["variants"][v][metric] for v in VARIANTS[:2])
        new_us = row["variants"]["new"][metric]
        row[metric.replace("_median", "_verdict")] = dict(
            parent_aa_us=abs(a - b), new_minus_faster_parent_us=new_us - min(a, b),
            within=bool(new_us - min(a, b) <= abs(a - b)))
    for run in runs.values():
        run["solver"].close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="the parent commit's libi2lqr_hip.so")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" /
                                         "lane_plan_host_ab.json"))
    ap.add_argument("--reps", type=int, default=1000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lane_plan_host_ab.py needs a HIP device")
    cfg = _abi.default_config("bicycle6", HORIZON, "f64", dt=0.25, layout=_abi.LAYOUT_BATCH_MINOR)
    host = workloads.make_batch(cfg, B)
    libs = {"parent": args.other, "parent again": args.other, "new": None}
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "shape": f"{B} problems, bicycle6, N = {HORIZON}, dt = 0.25, fp64, batch-minor layout",
           "note": "host clock around the C call (call_us) and around the call and the "
                   "synchronisation after it (call_sync_us), inputs restored and the device idle "
                   "before every call; \"parent\" / \"parent again\": two handles on the parent "
                   "commit's library, \"new\": this tree's; the variants alternate, their order rotates",
           "calls": {}}
    for name, solve in (("iterate", False), ("solve", True)):
        row = doc["calls"][name] = measure(cfg, host, libs, solve, args.reps)
        for v in VARIANTS:
            t = row["variants"][v]
            print(f"{name:8s} {v:13s}: call {t['call_us_median']:.2f} us [q1 {t['call_us_q1']:.2f}, "
                  f"q3 {t['call_us_q3']:.2f}]  call + sync {t['call_sync_us_median']:.2f} us "
                  f"[q1 {t['call_sync_us_q1']:.2f}, q3 {t['call_sync_us_q3']:.2f}]", flush=True)
        for metric in ("call_us_verdict", "call_sync_us_verdict"):
            print(f"{name:8s} {metric}: {row[metric]}  identical outputs {row['identical_outputs']}",
                  flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
