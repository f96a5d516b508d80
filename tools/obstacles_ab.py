#!/usr/bin/env python3
"""A/B of the "obstacles" option (include/i2lqr.h) against k_iterate in ONE process:

    obstacles_ab.py [--out FILE] [--reps R] [--other LIB]

For bicycle6 N = 20 fp64 at 256 and 1024 problems and bicycle4 N = 6 fp64 at 16, k_iterate with one
obstacle record per problem ("group_lanes" 64: as dispatched, and with "per_step_jacobians" 0, the
form k_iterate_obs is built on) against k_iterate_obs with K = 2, 4 and 8 records
(workloads.obstacles_on_path; the one-record runs carry record 0 of the K = 2 set):
time per 10 fixed iterations — device events, median over the repetitions, the variants
alternating inside every repetition, every launch on its own copy of the batch — and the share of
the 10 iterations that were accepted (only an accepted iteration computes the barrier terms again).
--other LIB (another build of the library, e.g. tools/_diag/libi2lqr_<name>.so): the K = 2, 4, 8
variants run on LIB as well, twice (the pair gives the run's A/A spread), interleaved with the rest.
Writes JSON (default profiles/obstacles_ab.json).  Not part of bench.py, not a test.
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from ilqr_iterative_tasks_amd import BatchedILQR, default_config, workloads

VARIANTS = ("1", "1 pj0", "2", "4", "8")  # records per problem; "1 ...": k_iterate


def variants(other):
    """{name: (records variant, library path or None)}; with `other`, K > 1 twice more on it."""
    out = {v: (v, None) for v in VARIANTS}
    if other:
        for k in ("2", "4", "8"):
            out[f"{k} other"] = (k, other)
            out[f"{k} other again"] = (k, other)
    return out


def configurations():
    b6 = default_config("bicycle6", 20, "f64", dt=0.25)
    b4 = default_config("bicycle4", 6, "f64")
    return [("bicycle6 N=20 fp64", b6, 256), ("bicycle6 N=20 fp64", b6, 1024),
            ("bicycle4 N=6 fp64", b4, 16)]


def make_solver(cfg, variant, lib_path=None):
    solver = BatchedILQR(cfg, lib_path=lib_path)
    solver.set_option("group_lanes", 64)
    if variant == "1 pj0":
        solver.set_option("per_step_jacobians", 0)
    elif variant != "1":
        solver.set_option("obstacles", int(variant))
    return solver


def records(host, variant):
    if variant.startswith("1"):
        return np.ascontiguousarray(workloads.obstacles_on_path(host, 2)[:, 0])
    return workloads.obstacles_on_path(host, int(variant))


def device_sets(solver, host, obs, count):
    B = host["X"].shape[0]
    dev = lambda a: torch.as_tensor(a).to(solver.device, solver.dtype)
    base = solver.alloc(B, want_gains=False)
    for key in ("X", "U", "x_term", "lamb"):
        base[key].copy_(dev(host[key]))
    base["obs"] = dev(obs)
    sets = []
    for _ in range(count):
        b2 = dict(base)
        b2.update({k: base[k].clone() for k in ("X", "U", "lamb", "cost", "iters", "status")})
        sets.append(b2)
    return sets


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(cfg, B, reps, runs):
    host = workloads.make_batch(cfg, B)
    solvers = {v: make_solver(cfg, *runs[v]) for v in runs}
    sets = {v: device_sets(solvers[v], host, records(host, runs[v][0]), reps + 1) for v in runs}
    ms = {v: [] for v in runs}
    for r in range(reps + 1):  # (repetition 0 warms every variant up)
        for v in runs:
            ms[v].append(timed(lambda: solvers[v].iterate(sets[v][r], 10)))
    rows = {}
    for v in runs:
        t = np.array(ms[v][1:])
        # lamb_out = lamb_in * factor^(rejects - accepts) over 10 iterations, lamb_in = 1
        j = np.rint(np.log(sets[v][-1]["lamb"].cpu().numpy()) / np.log(cfg.lamb_factor))
        rows[v] = dict(kernel=solvers[v].iterate_kernel(B), iterate10_ms_median=float(np.median(t)),
                       iterate10_ms_min=float(t.min()), iterate10_ms_max=float(t.max()),
                       accepted_share=float(((10 - j) / 2).mean() / 10))
    for v in list(runs)[1:]:
        rows[v]["iterate10_over_k_iterate"] = rows[v]["iterate10_ms_median"] / rows["1"]["iterate10_ms_median"]
        rows[v]["iterate10_over_k_iterate_pj0"] = (rows[v]["iterate10_ms_median"] /
                                                   rows["1 pj0"]["iterate10_ms_median"])
    for s in solvers.values():
        s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" /
                                         "obstacles_ab.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--other", default=None, help="a second library to run the K > 1 variants on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("obstacles_ab.py needs a HIP device")
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "other": args.other,
           "note": "records per problem; \"1\" = k_iterate (\"group_lanes\" 64), \"1 pj0\" the same "
                   "with \"per_step_jacobians\" 0; times from device events",
           "configurations": []}
    runs = variants(args.other)
    for name, cfg, B in configurations():
        rows = measure(cfg, B, args.reps, runs)
        doc["configurations"].append(dict(name=name, B=B, records=rows))
        for v, row in rows.items():
            print(f"{name:20s} B={B:5d} records {v:5s}: 10 iterations {row['iterate10_ms_median']:.4f} ms "
                  f"[{row['iterate10_ms_min']:.4f}, {row['iterate10_ms_max']:.4f}]  x k_iterate "
                  f"{row.get('iterate10_over_k_iterate', 1.0):.3f}  accepted "
                  f"{row['accepted_share']:.0%}  {row['kernel']}", flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
