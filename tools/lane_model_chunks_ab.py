#!/usr/bin/env python3
"""A/B of "lane_model_chunks" (include/i2lqr.h): i2lqr_solve of a lane handle with a model on as ONE
launch with early exit (the option off) against the chunked, compacting solve (the option on), in ONE
process:

    lane_model_chunks_ab.py [--out FILE] [--reps R] [--batches 4096,16384,65536] [--step-limit SECONDS]
                            [--dtypes f64,f32]

bicycle6, N = 20, batch-minor, the same problems for both variants (workloads.make_batch, two records of
workloads.obstacles_on_path, the box v in [0, 10]); soft accept test and barrier cost; one and four step
sizes; fp64 and fp32.  Time of one solve to termination - device events, median over the repetitions,
the two variants alternating inside every repetition, every solve on a fresh copy of the batch (copied
outside the timed region).  Every GPU step (a copy, a solve and its wait) runs under an alarm of
--step-limit seconds whose default action ends the process: a step that hangs is not followed by
another.  Per variant the mean and maximum iteration count and the status totals of the last solve are
recorded; the two variants must agree on them (and on every output, bit for bit), else the tool ends
with an error.  (A form without chunk kernels - the soft accept test with four step sizes - is ONE launch
with the option on as well: its "kernel" has no ", chunked" and the two times are one measurement twice.)
Writes JSON (default profiles/lane_model_chunks_ab.json) under "configurations".

    lane_model_chunks_ab.py --libraries parent=PATH,this=PATH [--order parent,this,parent] ...

The option-off A/B of two builds of the library: for every name in --order a fresh child process with
I2LQR_LIB_PATH set to that build times 10 fixed iterations (the option off, the same handles and
batches) and prints its rows; the parent process, which never opens the device, merges them into the
same file under "option_off_ab" with the spread of the runs of the same build beside the difference
between the builds - what the chunk protocol costs the existing model kernels while the option is off
(it decided that the chunk kernels are copies in units of their own: profiles/README.md).  Not part
of bench.py, not a test.
"""
import argparse
import json
import os
import signal
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
RECORDS = 2
FORMS = [(False, 1), (False, 4), (True, 1), (True, 4)]  # (barrier cost, step sizes)


def form_name(merit, A):
    return f"{'barrier cost' if merit else 'soft'} A{A}"


def make_solver(cfg, merit, A):
    import numpy as np
    from ilqr_iterative_tasks_amd import BatchedILQR
    c = cfg.copy()
    c.layout = 1
    solver = BatchedILQR(c)
    solver.set_option("lane_models", 1)
    solver.set_option("obstacles", RECORDS)
    lo, hi = np.full(cfg.n, -np.inf), np.full(cfg.n, np.inf)
    lo[2], hi[2] = 0.0, 10.0
    solver.set_state_box(lo, hi)
    if merit:
        solver.set_option("lane_barrier_cost", 1)
    if A > 1:
        solver.set_option("lane_line_search", A)
    return solver


def summary(work):
    it = work["iters"].cpu().numpy()
    st = work["status"].cpu().numpy()
    return dict(iters_mean=float(it.mean()), iters_max=int(it.max()),
                status={str(s): int((st == s).sum()) for s in (1, 2, 3, 4)})


def measure_solve(cfg, B, merit, A, reps, limit):
    import numpy as np
    import torch
    from ilqr_iterative_tasks_amd import workloads
    from lane_models_ab import base_set, fresh
    from obstacles_ab import timed
    host = workloads.make_batch(cfg, B)
    obs = workloads.obstacles_on_path(host, RECORDS)
    solvers = {"single launch": make_solver(cfg, merit, A), "chunked": make_solver(cfg, merit, A)}
    solvers["chunked"].set_option("lane_model_chunks", 1)
    base = {v: base_set(s, host, obs) for v, s in solvers.items()}
    ms = {v: [] for v in solvers}
    last = {}
    for r in range(reps + 1):  # (repetition 0 warms both variants up)
        for v in solvers:
            signal.alarm(limit)  # (no handler: a step that does not return ends the process)
            work = fresh(base[v])
            ms[v].append(timed(lambda: solvers[v].solve(work)))
            signal.alarm(0)
            last[v] = work
    rows = {}
    for v, s in solvers.items():
        t = np.array(ms[v][1:])
        rows[v] = dict(kernel=s.solve_kernel(B), solve_ms_median=float(np.median(t)),
                       solve_ms_min=float(t.min()), solve_ms_max=float(t.max()), **summary(last[v]))
    a, b = last["single launch"], last["chunked"]
    same = all(torch.equal(a[k], b[k]) for k in ("X", "U", "lamb", "cost", "iters", "status"))
    for key in ("iters_mean", "iters_max", "status"):
        if rows["single launch"][key] != rows["chunked"][key]:
            sys.exit(f"B={B} {form_name(merit, A)}: {key} differs: {rows['single launch'][key]} "
                     f"against {rows['chunked'][key]}")
    if not same:
        sys.exit(f"B={B} {form_name(merit, A)}: the chunked solve's outputs are not the single launch's")
    rows["chunked"]["solve_over_single_launch"] = (rows["chunked"]["solve_ms_median"] /
                                                   rows["single launch"]["solve_ms_median"])
    rows["chunked"]["bit_identical"] = True
    for s in solvers.values():
        s.close()
    return rows


def measure_fixed(cfg, B, merit, A, reps, limit):
    """10 fixed iterations, the option off: what a build of the library costs where nothing is chunked."""
    import numpy as np
    from ilqr_iterative_tasks_amd import workloads
    from lane_models_ab import base_set, fresh
    from obstacles_ab import timed
    host = workloads.make_batch(cfg, B)
    solver = make_solver(cfg, merit, A)
    base = base_set(solver, host, workloads.obstacles_on_path(host, RECORDS))
    ms = []
    for r in range(reps + 1):
        signal.alarm(limit)
        work = fresh(base)
        ms.append(timed(lambda: solver.iterate(work, 10)))
        signal.alarm(0)
    t = np.array(ms[1:])
    row = dict(kernel=solver.iterate_kernel(B), iterate10_ms_median=float(np.median(t)),
               iterate10_ms_min=float(t.min()), iterate10_ms_max=float(t.max()))
    solver.close()
    return row


def configurations(args):
    from ilqr_iterative_tasks_amd import default_config
    for dtype in args.dtypes.split(","):
        cfg = default_config("bicycle6", 20, dtype, dt=0.25)
        for merit, A in FORMS:
            for B in (int(b) for b in args.batches.split(",")):
                yield dtype, cfg, merit, A, B


def child(args):
    """One build's rows of the option-off A/B, as one JSON line on stdout."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("lane_model_chunks_ab.py needs a HIP device")
    rows = []
    for dtype, cfg, merit, A, B in configurations(args):
        row = measure_fixed(cfg, B, merit, A, args.reps, args.step_limit)
        rows.append(dict(dtype=dtype, form=form_name(merit, A), B=B, **row))
        print(f"# {dtype} {form_name(merit, A):15s} B={B:6d}: 10 iterations "
              f"{row['iterate10_ms_median']:9.4f} ms  {row['kernel']}", file=sys.stderr, flush=True)
    print(json.dumps(rows))


def library_ab(args, out):
    libs = dict(item.split("=", 1) for item in args.libraries.split(","))
    order = args.order.split(",")
    runs = []
    for name in order:
        env = dict(os.environ, I2LQR_LIB_PATH=str(Path(libs[name]).resolve()))
        cmd = [sys.executable, __file__, "--child", "--reps", str(args.reps), "--batches", args.batches,
               "--dtypes", args.dtypes, "--step-limit", str(args.step_limit)]
        # a fresh process per build: a child that fails or runs out of time ends the A/B
        done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=args.run_limit, check=True)
        runs.append(dict(library=name, rows=json.loads(done.stdout.decode().strip().splitlines()[-1])))
    doc = json.loads(out.read_text()) if out.exists() else {}
    table = []
    for i, first in enumerate(runs[0]["rows"]):
        med = {}
        for run in runs:
            med.setdefault(run["library"], []).append(run["rows"][i]["iterate10_ms_median"])
        mean = {name: sum(v) / len(v) for name, v in med.items()}
        spread = {name: max(v) - min(v) for name, v in med.items()}
        names = list(med)
        table.append(dict(dtype=first["dtype"], form=first["form"], B=first["B"], kernel=first["kernel"],
                          iterate10_ms_median=med, run_to_run_ms=spread,
                          difference_ms=mean[names[-1]] - mean[names[0]] if len(names) > 1 else 0.0))
    doc["option_off_ab"] = dict(
        note="10 fixed iterations, the option off, one fresh process per run with I2LQR_LIB_PATH set to "
             "the build; iterate10_ms_median lists every run's median per build in the order run; "
             "run_to_run_ms: largest minus smallest median of the runs of one build; difference_ms: mean "
             "of the last-named build's runs minus mean of the first-named build's",
        order=order, reps=args.reps, rows=table)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    for row in table:
        print(f"{row['dtype']} {row['form']:15s} B={row['B']:6d}: {row['iterate10_ms_median']}  "
              f"difference {row['difference_ms']:+.4f} ms, run to run {row['run_to_run_ms']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lane_model_chunks_ab.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", default="4096,16384,65536")
    ap.add_argument("--step-limit", type=int, default=60)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--libraries", default="")
    ap.add_argument("--order", default="parent,this,parent")
    ap.add_argument("--run-limit", type=int, default=240)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    out = Path(args.out)
    if args.child:
        return child(args)
    if args.libraries:
        return library_ab(args, out)
    import torch
    if not torch.cuda.is_available():
        sys.exit("lane_model_chunks_ab.py needs a HIP device")
    doc = json.loads(out.read_text()) if out.exists() else {}
    doc.update({"device": torch.cuda.get_device_name(0), "reps": args.reps,
                "note": "bicycle6 N=20, two records and the box v in [0, 10], batch-minor; one solve to "
                        "termination of the same batch as ONE launch with early exit (\"single launch\": "
                        "\"lane_model_chunks\" off) and as chunks with compaction (\"chunked\": the option "
                        "on, automatic schedule); ms from device events, median of the repetitions, the "
                        "variants alternating; iters_mean / iters_max / status: iteration counts and "
                        "status totals (1 converged, 2 max_iter, 3 lamb overflow, 4 non-finite) of the "
                        "last solve, equal between the variants by construction of the tool",
                "configurations": []})
    for dtype, cfg, merit, A, B in configurations(args):
        rows = measure_solve(cfg, B, merit, A, args.reps, args.step_limit)
        doc["configurations"].append(dict(name=f"bicycle6 N=20 {dtype}", dtype=dtype, B=B,
                                          form=form_name(merit, A), variants=rows))
        one, ch = rows["single launch"], rows["chunked"]
        print(f"{dtype} {form_name(merit, A):15s} B={B:6d}: single launch {one['solve_ms_median']:9.3f} ms, "
              f"chunked {ch['solve_ms_median']:9.3f} ms  x {ch['solve_over_single_launch']:.3f}  iterations "
              f"mean {one['iters_mean']:.1f} max {one['iters_max']}  status {one['status']}  {ch['kernel']}",
              flush=True)
        # (written after every configuration: a run that is cut short keeps what it measured)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
