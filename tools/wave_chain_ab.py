#!/usr/bin/env python3
"""A/B of the chained control round in one launch ("wave_chain", include/i2lqr.h: k_chain_box) against
the launch per chain step, replayed as a graph, in ONE process:

    wave_chain_ab.py [--out FILE] [--reps R]

The round is config 1's of the reference scenario (--num-ss-iters 2 --num-ss-points 8: 2 laps of 8
candidates, bicycle4, N = 6, fp64, chained lamb) with the models the speculative chain kernel
refuses: the speed limit of examples/speed_limit_laps.py (v in [0, 8]) and the two obstacles of
examples/two_obstacle_laps.py.  Timed is HipCandidateSolver.solve_chained, host arrays in, host
arrays out (one copy up, the launches, one copy down, one synchronisation): host clock around the
call, 5 warm-up rounds per variant (the per-step form captures its graph in the first), then R
rounds with the two variants alternating, their order swapped every round; medians, quartiles and
the medians by order.  Both variants must return the same bits.
Writes JSON (default profiles/wave_chain_ab.json).  Not part of bench.py, not a test.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from ilqr_iterative_tasks_amd import default_config, workloads
from ilqr_iterative_tasks_amd.control import StateBox
from ilqr_iterative_tasks_amd.control.iterative_ilqr import HipCandidateSolver

LAPS, POINTS, HORIZON = 2, 8, 6
VARIANTS = ("one_launch", "per_step")


def rounds():
    """name -> (solver keywords, obstacle record(s)) of the two scenarios; and the shared round."""
    cfg = default_config("bicycle4", HORIZON)
    host = workloads.make_batch(cfg, LAPS * POINTS)
    x0 = host["X"][0, :, 0].copy()
    chains = [host["x_term"][a * POINTS:(a + 1) * POINTS] for a in range(LAPS)]
    first = np.array([31.0, -3.0, 8.0, 6.0, 0.0, 0.0])
    second = np.array([x0[0] + 10.0, x0[1] + 1.0, 4.0, 3.0, 0.2, 1.0])
    inf = np.full(4, np.inf)
    limit = StateBox(np.where(np.arange(4) == 2, 0.0, -inf), np.where(np.arange(4) == 2, 8.0, inf))
    return cfg, x0, chains, {"speed_limit": (dict(state_box=limit), first),
                             "two_obstacles": (dict(), np.stack([first, second]))}


def measure(cfg, x0, chains, keywords, rec, reps):
    solvers = {"one_launch": HipCandidateSolver(wave_chain=True, **keywords),
               "per_step": HipCandidateSolver(wave_chain=False, **keywords)}

    def one(v):
        t0 = time.perf_counter()
        out = solvers[v].solve_chained(cfg, x0, chains, 1.0, rec)
        return (time.perf_counter() - t0) * 1e3, out

    outs = {}
    for v in VARIANTS:
        for _ in range(5):
            outs[v] = one(v)[1]
    info = {v: dict(solvers[v].chain_info) for v in VARIANTS}
    assert info["one_launch"]["one_launch"] is True, info
    assert info["per_step"]["one_launch"] is False, info
    same = all(np.array_equal(a[key], b[key]) for a, b in zip(outs["one_launch"], outs["per_step"])
               for key in ("U", "X", "lamb", "cost", "iters", "status"))
    ms = {v: [] for v in VARIANTS}
    for r in range(reps):
        for v in (VARIANTS if r % 2 == 0 else VARIANTS[::-1]):
            ms[v].append(one(v)[0])
    rows = {}
    for v in VARIANTS:
        t = np.array(ms[v])
        rows[v] = dict(round_ms_median=float(np.median(t)), round_ms_q1=float(np.quantile(t, 0.25)),
                       round_ms_q3=float(np.quantile(t, 0.75)), round_ms_min=float(t.min()),
                       round_ms_max=float(t.max()),
                       round_ms_median_when_first=float(np.median(t[(0 if v == VARIANTS[0] else 1)::2])),
                       round_ms_median_when_second=float(np.median(t[(1 if v == VARIANTS[0] else 0)::2])),
                       graph=bool(info[v]["graph"]), graph_error=info[v]["graph_error"])
    iters = np.concatenate([o["iters"] for o in outs["one_launch"]])
    return dict(variants=rows, identical_outputs=bool(same),
                iterations_per_chain=[int(o["iters"].sum()) for o in outs["one_launch"]],
                iterations_total=int(iters.sum()),
                one_launch_over_per_step=rows["one_launch"]["round_ms_median"] /
                rows["per_step"]["round_ms_median"],
                saved_us_per_chain_step=(rows["per_step"]["round_ms_median"] -
                                         rows["one_launch"]["round_ms_median"]) * 1e3 / POINTS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" /
                                         "wave_chain_ab.json"))
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wave_chain_ab.py needs a HIP device")
    cfg, x0, chains, scenarios = rounds()
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "round": f"{LAPS} chains x {POINTS} candidates, bicycle4, N = {HORIZON}, fp64",
           "note": "\"one_launch\": HipCandidateSolver(wave_chain=True).solve_chained (k_chain_box); "
                   "\"per_step\": wave_chain=False, a launch and a lamb copy per chain step replayed "
                   "as a graph; host clock around the call (copy up, launches, copy down, "
                   "synchronise), the variants alternating, their order swapped every round",
           "scenarios": {}}
    for name, (keywords, rec) in scenarios.items():
        row = doc["scenarios"][name] = measure(cfg, x0, chains, keywords, rec, args.reps)
        for v in VARIANTS:
            t = row["variants"][v]
            print(f"{name:14s} {v:10s}: {t['round_ms_median']:.4f} ms per round "
                  f"[q1 {t['round_ms_q1']:.4f}, q3 {t['round_ms_q3']:.4f}]  first "
                  f"{t['round_ms_median_when_first']:.4f}  second {t['round_ms_median_when_second']:.4f}"
                  f"  graph {t['graph']}", flush=True)
        print(f"{name:14s} one launch / per step {row['one_launch_over_per_step']:.3f}, "
              f"{row['saved_us_per_chain_step']:.2f} us saved per chain step, identical outputs "
              f"{row['identical_outputs']}, {row['iterations_total']} iterations", flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
