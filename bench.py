#!/usr/bin/env python3
"""bench.py — batched iLQR iterations/s on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Started plainly with --gpus N > 1 (no RANK / WORLD_SIZE in the environment) this process becomes the
launcher: it starts N fresh rank processes through torch.distributed.run BEFORE anything touches the
GPU (it never imports torch itself) and relays rank 0's JSON line.  Under a launcher whose world
differs from --gpus it exits non-zero instead of reporting a smaller world.

A "step" is one pass of the hot path over one batch of synthetic problems that is already resident
in HBM: `iters` fused iLQR iterations per problem (i2lqr_iterate: rollout + cost, backward Riccati
pass with dynamics Jacobians and cost quadratisation, forward rollout, accept/reject), the relaxed
terminal cost of every candidate, the all-gather of those costs across ranks (one RCCL
ncclAllGather through the C-ABI, i2lqr_allgather_costs, on a side stream) and the arg-min every
rank evaluates locally (utils/base.py:462-469).  Default workload = BASELINE.json configs[1]: batch
1024 per GPU, kinematic bicycle n=6 m=2 N=20, fp64.  Weak scaling: every rank owns its own `batch`
problems; `extra.config4_strong` adds the strong-scaled configs[3] (2^20 problems over all ranks).

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step handed its caller
(the batch's X, U, lamb, costs, iteration counts, status and gains, the relaxed costs and the pick;
with an exchange also the gathered costs and the winner's trajectory) as DIR/<name>.npy.  The
inputs are seeded, so two builds run with the same arguments can be compared array for array.

Rank 0 prints ONE JSON line.  `roofline` prices the dominant kernel against the HBM peak with the
ALGORITHMIC bytes of SURVEY.md §8(d) (4968 B per iteration per problem at n=6, m=2, N=20, fp64);
`roofline_issue` prices the same kernel against the instruction-issue peak of its wavefronts (the
bound that matters while a launch is one wavefront per SIMD); `cpu_baseline` (--full) times the CPU
oracle (a port, oracle/ilqr_oracle.c) on the host cores of the same box on a bounded sample of the
same workload.

A plain run does what its headline figure needs: set-up, warm-up, the timed steps, --dump-outputs
and the JSON line, whose `roofline` and `roofline_issue` come from event brackets inside the timed
steps.  --full adds everything that takes runs of its own: `cpu_baseline`, the secondary workloads
(`extra`, `roofline_large_batch`, `roofline_solve` and their claim scalars in `roofline`) and, with
--gpus N, the `long_run` and the host-driven and two-collective forms of the round
(`exchange.phases_ms`, `host_driven_variant`, `broadcast_variant`).  --no-cpu-baseline and
--no-extra leave parts of that out again.

--exchange-only (no GPU needed; gloo): the multi-rank harness alone — launcher, process group,
barriers, max-over-ranks timing, all-gather of synthetic cost shards, local arg-min — with the
solve left out.  It exists so that the N > 1 plumbing of this file is testable on a CPU box; its
JSON line says so and is not a throughput figure of the solver.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
SIMDS = 256 * 4        # CUs x SIMDs per CU
CLOCK_GHZ = 2.4        # max clock; one wavefront alone on a SIMD issues one instruction per 4 cycles
LIB = ROOT / "ilqr_iterative_tasks_amd" / "csrc" / "libi2lqr_hip.so"


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="config2",
                    help="config2 (default: B=1024 fp64), config3 (B=65536 fp32), config4, config5")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default: workload's)")
    ap.add_argument("--dtype", default=None, choices=[None, "f64", "f32"])
    ap.add_argument("--iters", type=int, default=10, help="fused iLQR iterations per step")
    ap.add_argument("--layout", default="auto", choices=["auto", "wave", "lane", "tiled"],
                    help="kernel family: wave = one problem per wavefront (problem-major), lane = "
                         "one problem per lane (batch-minor); auto picks by batch size")
    ap.add_argument("--exchange", default="native", choices=["native", "torch"],
                    help="all-gather of the costs: native = i2lqr_allgather_costs (RCCL through the "
                         "C-ABI), torch = torch.distributed.all_gather_into_tensor")
    ap.add_argument("--handoff", default="gather", choices=["gather", "broadcast"],
                    help="--gpus N: how the winner reaches every rank in the TIMED step: gather = the "
                         "local winners' packs ride in the grouped all-gather (one collective, no "
                         "host round trip; the default), broadcast = all-gather of the costs, pick "
                         "read back, ONE ncclBroadcast from the owner (two collectives: the form to "
                         "fall back on should grouped collectives misbehave on a node)")
    ap.add_argument("--exchange-only", action="store_true",
                    help="CPU/gloo dry run of the multi-rank harness without the solve (see above)")
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline: CPU baseline, secondary workloads and their claim "
                         "scalars; --gpus N: long run, host-driven and two-collective rounds")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the secondary workloads")
    ap.add_argument("--cpu-seconds", type=float, default=15.0,
                    help="--full: CPU baseline time budget")
    ap.add_argument("--test-hooks", action="store_true",
                    help="tests only: honour I2LQR_BENCH_TEST_HANG (an attempt that never returns)")
    ap.add_argument("--launch-timeout", type=float, default=900.0,
                    help="--gpus N > 1 without a launcher: seconds one attempt of the N ranks may "
                         "take before its process group is ended")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as "
                         "DIR/<name>.npy (float32 / float64, at most 64 MB in all: a fixed, seeded "
                         "sample of the problems when the batch is larger); rank 0 only")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


# ------------------------------------------------------------------------------------------------
# launcher: python bench.py --gpus N  ->  N rank processes
# ------------------------------------------------------------------------------------------------

def _run_ranks(args, extra_argv, timeout_s):
    """One attempt: N fresh rank processes through torch.distributed.run, in a process group of
    their own so that a hung attempt (a rank stuck in a communicator bootstrap) can be ended as a
    whole.  Returns (returncode or None on timeout, stdout)."""
    import signal
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["I2LQR_BENCH_LAUNCHER"] = "1"  # the ranks may leave (exit 75) and count on a fresh start
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port",
           str(port), str(Path(__file__).resolve())] + sys.argv[1:] + extra_argv
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=timeout_s)
        return proc.returncode, out
    except subprocess.TimeoutExpired:
        for sig in (signal.SIGTERM, signal.SIGKILL):  # exactly the group this attempt started
            try:
                os.killpg(proc.pid, sig)
            except ProcessLookupError:
                break
            try:
                proc.wait(timeout=10)
                break
            except subprocess.TimeoutExpired:
                continue
        out = ""
        try:
            out, _ = proc.communicate(timeout=5)
        except Exception:  # noqa: BLE001
            pass
        return None, out or ""


def spawn_ranks(args) -> int:
    """Start args.gpus ranks of this script as fresh processes and relay rank 0's JSON line.  Runs
    before torch is imported: the launcher never initialises a GPU, and nothing is exec'ed from a
    process that has.  An attempt that fails or exceeds --launch-timeout is ended (its whole
    process group) and, if it used the native exchange, repeated ONCE as a fresh set of processes
    with --exchange torch (torch.distributed's all-gather instead of the library's own RCCL
    communicator); the JSON line then carries the story under "launcher".  Exit code non-zero if
    that fails too."""
    attempts = []
    plans = [[]]
    if args.exchange == "native":
        plans.append(["--exchange", "torch"])
    for extra_argv in plans:
        t0 = time.perf_counter()
        rc, out = _run_ranks(args, extra_argv, args.launch_timeout)
        lines = [ln for ln in out.splitlines() if ln.startswith('{"metric"')]
        attempts.append({"argv": extra_argv, "returncode": rc, "timed_out": rc is None,
                         "seconds": round(time.perf_counter() - t0, 1)})
        if rc == 0 and lines:
            d = json.loads(lines[-1])
            d["launcher"] = {"attempts": attempts,
                             "fallback": None if not extra_argv else
                             "first attempt failed or timed out: ranks restarted with "
                             "--exchange torch"}
            print(result_line(d), flush=True)
            return 0
        sys.stderr.write(out[-4000:])
        sys.stderr.write(f"bench.py: the {args.gpus}-rank run "
                         f"{'timed out after %g s' % args.launch_timeout if rc is None else 'failed (exit %s)' % rc}"
                         f"{' [' + ' '.join(extra_argv) + ']' if extra_argv else ''}\n")
    return (attempts[-1]["returncode"] or 1) if attempts else 1


# ------------------------------------------------------------------------------------------------
# one rank
# ------------------------------------------------------------------------------------------------

# per-GPU batch from which the one-problem-per-lane kernels win over the eight-problems-per-
# wavefront kernel (tools/ab_bench.py, tools/solve_bench.py; fp64, n=6, N=20):
#   iterate: 8192: 165 vs 152 M it/s, 12288: 171 vs 223;  solve: 8192: 1.18 vs 1.68 ms,
#   16384: 1.80 vs 1.81 ms, 65536: 5.6 vs 2.5 ms
# The kernel's launch duration is measured live with HIP events on the launch stream around
# KERNEL_SAMPLES evenly spaced timed steps (an event pair around EVERY launch costs the timed region
# 5 us per step in marker packets, 3 % of a 0.136 ms step): 10 samples at the driver's --steps 20,
# 20 at the default 200.  The cost of an EMPTY event pair (measured after the timed region, smallest of 30) is
# subtracted: the two marker packets themselves sit inside the bracket, and at 0.2 ms per launch
# they are 5 % of it (rocprofv3's kernel duration, profiles/, is the check).  Secondary workloads:
# EXTRA_LAUNCHES individually bracketed launches after EXTRA_WARMUP, median and spread reported.
KERNEL_SAMPLES = 10       # at fewer than 100 timed steps (the driver's --steps 20: every second step)
KERNEL_SAMPLES_LONG = 20  # from 100 timed steps
LONG_RUN_STEPS = 200  # --gpus N > 1: a second timed loop of this many steps ("long_run")
EXTRA_LAUNCHES = 20
EXTRA_WARMUP = 3
FP64_VECTOR_PEAK_TFLOPS = 78.6  # MI355X fp64 vector peak (spec; = 1024 SIMDs x 16 lanes x 2 x 2.4 GHz)
LAYOUT_ID = {"wave": 0, "lane": 1, "tiled": 2}
LAYOUT_NAME = {"wave": "problem-major (one problem per wavefront)",  # 4 / 8 per wavefront from 1024
               "lane": "batch-minor (one problem per lane)",
               "tiled": "batch-tiled x64 (one problem per lane)"}


def pick_layout(args, B, solve=False, cfg=None):
    """wave: problem-major (one problem per wavefront below 1024 problems, four / eight per
    wavefront from there: the library's per-call choice); lane / tiled: one problem per lane over
    batch-minor rows / tiles of 64 problems.  The crossover between the layouts is the LIBRARY's
    (i2lqr_recommended_layout: measured thresholds live behind the C-ABI, not here)."""
    if args.layout != "auto":
        return args.layout
    from ilqr_iterative_tasks_amd import _abi
    rc = _abi.load_library().i2lqr_recommended_layout(cfg, int(B), 1 if solve else 0)
    if rc < 0:
        raise RuntimeError(f"i2lqr_recommended_layout failed ({rc})")
    return {0: "wave", 1: "lane", 2: "tiled"}[rc]


def kernel_label(kernel, layout):
    if kernel.startswith("k_group_iterate (sixteen"):
        return "problem-major (four problems per wavefront, sixteen lanes each)"
    if kernel.startswith("k_group_iterate"):
        return "problem-major (eight problems per wavefront)"
    if kernel == "k_quad_iterate":
        return "problem-major (four problems per wavefront)"
    return LAYOUT_NAME[layout]


def waves_of(kernel, B):
    """Main wavefronts of a launch (helper wavefronts not counted)."""
    if kernel == "k_iterate":
        return B
    if "(sixteen lanes)" in kernel or kernel == "k_quad_iterate":
        return (B + 3) // 4
    if kernel.startswith(("k_group_iterate", "k_group_spec")):
        return (B + 7) // 8
    return (B + 63) // 64


def accepted_fraction(lamb, lamb0, iters, factor):
    """Share of the `iters` fixed-count iterations that were accepted steps: every accept divides
    lamb by `factor`, every reject multiplies it (control/iterative_ilqr.py:76, :82), so
    accepts - rejects = log(lamb0 / lamb) / log(factor)."""
    import torch
    d = torch.log(lamb0.double() / lamb.double()) / torch.log(torch.tensor(float(factor), dtype=torch.float64))
    acc = (iters + torch.round(d)) / 2.0
    return float((acc / iters).mean())


def make_step_buffers(solver, host, n_sets, torch, want_gains=True):
    """n_sets independent copies of the in/out state (X, U, lamb) + shared read-only inputs and
    shared outputs, all resident in HBM before the timed region starts."""
    dev, dt = solver.device, solver.dtype
    B = host["X"].shape[0]
    native = lambda a: solver.to_native(torch.as_tensor(a).to(dev, dt))
    shared = dict(
        x_term=native(host["x_term"]),
        obs=native(host["obs"]),
        cost=torch.zeros(B, dtype=dt, device=dev),
        K=torch.zeros(solver.shape("K", B), dtype=dt, device=dev) if want_gains else None,
        k=torch.zeros(solver.shape("k", B), dtype=dt, device=dev) if want_gains else None,
        iters=torch.zeros(B, dtype=torch.int32, device=dev),
        status=torch.zeros(B, dtype=torch.int32, device=dev),
    )
    X0, U0, l0 = native(host["X"]), native(host["U"]), native(host["lamb"])
    sets = []
    for _ in range(n_sets):
        buf = dict(shared)
        buf.update(X=X0.clone(), U=U0.clone(), lamb=l0.clone())
        sets.append(buf)
    return sets


DUMP_BUDGET_BYTES = 64_000_000  # --dump-outputs: all files together
DUMP_SAMPLE_SEED = 20240229   # the problems kept when a batch's outputs exceed the budget
DUMP_WHOLE = ("best_idx", "best_cost", "winner_U", "winner_X")  # not indexed by problem


def dump_step_outputs(out_dir, outs, B, torch):
    """Write the outputs of one step (problem-major tensors, batch axis first, except DUMP_WHOLE)
    as out_dir/<name>.npy: floating arrays keep their precision, integer arrays become float64
    (exact).  Over DUMP_BUDGET_BYTES the per-problem arrays keep the same fixed sample of problems,
    drawn with DUMP_SAMPLE_SEED and stored in ascending order as sample_index.npy."""
    import numpy as np
    host = {}
    for name, t in outs.items():
        t = t.detach()
        host[name] = t.to(t.dtype if t.is_floating_point() else torch.float64)
    per = [n for n, t in host.items() if n not in DUMP_WHOLE and t.dim() >= 1 and t.shape[0] == B]
    header = 128  # bytes of .npy header per file
    fixed = sum(t.numel() * t.element_size() + header for n, t in host.items() if n not in per)
    row = sum(host[n][0].numel() * host[n].element_size() for n in per)
    keep = B
    if fixed + B * row + header * len(per) > DUMP_BUDGET_BYTES:
        keep = (DUMP_BUDGET_BYTES - fixed - header * (len(per) + 1)) // (row + 8)
        if keep < 1:
            raise ValueError("--dump-outputs: the step's outputs do not fit in the budget")
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    arrays = {}
    if keep < B:
        sample = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(B, keep, replace=False))
        idx = torch.as_tensor(sample, device=host[per[0]].device)
        for n in per:
            host[n] = host[n].index_select(0, idx)
        arrays["sample_index"] = sample.astype(np.float64)
    arrays.update((name, t.cpu().numpy()) for name, t in host.items())
    for name, a in arrays.items():
        np.save(out / f"{name}.npy", a)
    return {"bytes": sum(a.nbytes for a in arrays.values()), "problems": int(keep), "batch": B,
            "sampled": keep < B}


def event_stride_for(steps):
    return max(1, steps // (KERNEL_SAMPLES_LONG if steps >= 100 else KERNEL_SAMPLES))


def empty_bracket_ms(torch, n=30):
    """Smallest duration HIP reports for an event pair with nothing in between, on a BUSY stream (a
    small kernel is enqueued in front of every pair, as in the timed loop where the previous step's
    kernels are still in flight): the two marker packets themselves.  On an idle stream the same
    pair reads 2-3 times longer (wake-up), which is not what the brackets of the timed region pay."""
    x = torch.zeros(1024, device="cuda")
    pairs = []
    for _ in range(n):
        x.add_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    vals = sorted(a.elapsed_time(b) for a, b in pairs)
    # the smallest reading is the markers' own cost; the median of the same samples moves between
    # 5 and 13 us from run to run (whatever else the queue processor is doing)
    return vals[0]


def spread(vals):
    """median, min, max and (max - min) / median of a list of durations."""
    v = sorted(vals)
    med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    return {"median": med, "mean": sum(v) / len(v), "min": v[0], "max": v[-1],
            "rel_spread": (v[-1] - v[0]) / med, "samples": len(v)}


SECONDARY_DIGITS = 6  # significant digits of the secondary figures: well below their run-to-run noise


def round_sig(x, digits=SECONDARY_DIGITS):
    """The floats of a (nested) result rounded to `digits` significant digits."""
    if isinstance(x, float):
        return float(f"{x:.{digits}g}")
    if isinstance(x, dict):
        return {k: round_sig(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [round_sig(v, digits) for v in x]
    return x


def result_line(d):
    """The JSON result line, without padding: it must stay well below 16 KiB so that a reader that
    keeps a bounded window of the output still holds all of it."""
    return json.dumps(d, separators=(",", ":"))


def run_gpu(args, cfg, B, rank, world, torch, dist_mod, steps, warmup, with_tail=True,
            event_stride=1, dump_dir=None):
    """Time `steps` steps; returns dict(seconds, kernel_ms, iterations, ...).  dump_dir: write the
    outputs of the last timed step there (dump_step_outputs) before anything reuses its buffers."""
    import torch.distributed as dist
    from ilqr_iterative_tasks_amd import BatchedILQR, workloads
    cfg = cfg.copy()
    layout = pick_layout(args, B, cfg=cfg)
    cfg.layout = LAYOUT_ID[layout]
    solver = BatchedILQR(cfg, torch.device("cuda", torch.cuda.current_device()))
    host = workloads.make_batch(cfg, B, offset=rank * B)
    sets = make_step_buffers(solver, host, steps + warmup, torch)
    l0_first = sets[-1]["lamb"].clone()
    qfun = torch.zeros(B, dtype=torch.int32, device=solver.device)
    # one cost vector per step: the exchange of step i (all-gather + arg-min) runs on a side
    # stream and overlaps the solve of step i+1 (the steps are independent candidate batches)
    cost_its = [torch.zeros(B, dtype=solver.dtype, device=solver.device)
                for _ in range(steps + warmup)]
    main_stream = torch.cuda.current_stream()
    grouped = dist.is_available() and dist.is_initialized()
    exchange, native_error = None, None
    if grouped and with_tail:
        exchange = "torch"
        if args.exchange == "native":
            # the communicator behind i2lqr_allgather_costs is created here by every rank at once;
            # if RCCL cannot be bound or bootstrapped that way on this node, all ranks fall back
            # to torch.distributed's all-gather together and the JSON line says so
            poisoned = False
            try:  # (raises on every rank or on none: CostExchange agrees on each bring-up step)
                with quiet_stdout():
                    exchange = dist_mod.CostExchange(solver)
                ok = 1
            except dist_mod.CostExchangePoisoned as e:
                native_error, ok, poisoned = f"{type(e).__name__}: {e}", 0, True
            except Exception as e:  # noqa: BLE001
                native_error, ok = f"{type(e).__name__}: {e}", 0
            # agreement over the HOST-side channel (no device collective next to a bootstrap that
            # may still be running in an abandoned thread)
            all_ok, none_poisoned = dist_mod._agree([ok == 1, not poisoned], dist_mod.host_group())
            if not none_poisoned and os.environ.get("I2LQR_BENCH_LAUNCHER") == "1":
                # some rank's ncclCommInitRank never returned: this set of processes is not to be
                # trusted with the device any more.  Under bench.py's own launcher every rank
                # leaves (non-zero) and the launcher starts FRESH ranks on the torch exchange.
                sys.stderr.write(f"bench.py rank {rank}: {native_error}; leaving for a fresh start\n")
                sys.stderr.flush()
                os._exit(75)
            if not all_ok:
                if exchange != "torch" and not isinstance(exchange, str):
                    exchange.close()
                exchange = "torch"
                native_error = native_error or "another rank could not create the communicator"
    # the exchange stream is PROBED (dist.exchange_stream): two HIP streams may share a hardware
    # queue — every fourth stream a process creates lands on the launch stream's — and the exchange
    # then runs BEHIND the next solve instead of beside it (+10 % at 8192 problems per rank)
    comm_stream = dist_mod.exchange_stream(solver.device) if exchange is not None else None
    # The multi-rank step IS the product's sharded round (HipCandidateSolver.sharded_round — what
    # control.iLqr(sharded=...) calls): shard solve + relaxed costs + local pick (one launch on the
    # fused kernels), the local winner's pack, ONE grouped all-gather of costs and packs, the pick
    # on the gathered vector and the winner's hand-off (i2lqr_round_winner) — every rank ends the
    # step holding best_idx and the winner's (U, X) as device tensors.  No host round trip: the
    # exchange of step i runs on a side stream beside the solve of step i+1.
    from ilqr_iterative_tasks_amd.control.iterative_ilqr import HipCandidateSolver
    rounds = HipCandidateSolver(solver.device)
    xch = None
    if exchange is not None:
        xch = dist_mod.TorchExchange() if exchange == "torch" else exchange
    P = cfg.m * cfg.N + cfg.n * (cfg.N + 1)
    zt = lambda *shape, dtype=None: torch.zeros(*shape, dtype=dtype or solver.dtype,
                                                device=solver.device)
    xbufs = ([solver.round_buffers(B, B * world, world) for _ in range(steps + warmup)]
             if exchange is not None else None)
    cost_alls = [b["cost_all"] for b in xbufs] if xbufs else None
    # the round as ONE C-ABI call (i2lqr_sharded_round_flat; round 6): its argument block is built
    # once per buffer set, like the buffers themselves; every step in flight has its own buffers, so
    # no round waits for the previous round's exchange (guard_previous off)
    one_call = exchange is not None and dist_mod.native_comm(xch)[1]
    plans = ([solver.plan_round(sets[i], qfun, cost_its[i], world * B, world, rank, args.iters,
                                bufs=xbufs[i], guard_previous=False)
              for i in range(steps + warmup)] if one_call else None)
    ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    xev = {name: [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
           for name in ("start", "gathered", "picked", "handed_over")}
    picks, winners = [], []
    last_round = {}  # the sharded round's result of the latest step (--dump-outputs)

    fused = solver.iterate_kernel(B).startswith("k_group_iterate")
    bests = [(torch.zeros(1, dtype=torch.int64, device=solver.device),
              torch.zeros(1, dtype=solver.dtype, device=solver.device))
             for _ in range(steps + warmup)] if with_tail and exchange is None else None

    def step(i_set, i_timed=None, handoff="gather"):
        buf, cost_it = sets[i_set], cost_its[i_set]
        bracket = i_timed is not None and i_timed % event_stride == 0
        if with_tail and exchange is not None:
            # (the kernel bracket of the sharded step is taken around the whole shard solve: the
            # event pair sits on the launch stream in front of and behind it)
            if bracket:
                ev0[i_timed].record()
            mark = ((lambda name: (ev1 if name == "solved" else xev[name])[i_timed].record())
                    if bracket else None)
            if handoff == "gather" and one_call:
                res = rounds.sharded_round(cfg, None, None, None, None, xch, world * B,
                                           n_iters=args.iters, plan=plans[i_set],
                                           exchange_stream=comm_stream, on_phase=mark)
            elif handoff in ("gather", "gather_host"):  # the same steps driven from Python
                res = rounds.sharded_round(cfg, None, None, None, None, xch, world * B,
                                           n_iters=args.iters, prepared=(solver, buf, qfun, cost_it),
                                           bufs=xbufs[i_set], exchange_stream=comm_stream,
                                           on_phase=mark, host_driven=True)
            else:  # the two-collective form: pick read back, ONE broadcast from the owner
                res = rounds.sharded_round(
                    cfg, None, None, None, None, xch, world * B, n_iters=args.iters,
                    prepared=(solver, buf, qfun, cost_it),
                    lexi=lambda cost_all: int(solver.argmin(cost_all, side=True)[0]), on_phase=mark)
            picks.append(res["best_idx"])
            winners.append(res["pack"])
            last_round["res"] = res
            return
        if bracket:
            ev0[i_timed].record()
        # One call per control round (i2lqr_iterate_pick).  On the eight- / sixteen-lane kernels it
        # is ONE launch — relaxed cost in the kernel's exit block, the pick a last-workgroup-done
        # reduction — and the bracket holds that launch; the other families run iterate,
        # relax_cost and argmin as launches and the bracket holds the dominant one.
        if not with_tail:
            solver.iterate(buf, args.iters)
        elif fused:
            picks.append(solver.iterate_pick(buf, args.iters, qfun, 0, 55, cost_it,
                                             best=bests[i_set])[1])
        else:
            solver.iterate(buf, args.iters)
        if bracket:
            ev1[i_timed].record()
        if with_tail and not fused:
            solver.relax_cost(buf["X"], buf["x_term"], qfun, 0, 55, cost_it)
            picks.append(solver.argmin(cost_it))

    def timed_loop(handoff="gather"):
        for i in range(warmup):
            step(i, None, handoff)
        torch.cuda.synchronize()
        if grouped:
            dist.barrier()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(warmup + i, i, handoff)
        torch.cuda.synchronize()  # both streams: every step's exchange, pick and hand-off is complete
        if grouped:
            dist.barrier()
            torch.cuda.synchronize()
        return time.perf_counter() - t0

    seconds = timed_loop(args.handoff if exchange is not None else "gather")
    dumped = None
    if dump_dir is not None:
        last = sets[warmup + steps - 1]
        outs = {name: solver.to_problem_major(last[key]) for name, key in (
            ("X", "X"), ("U", "U"), ("lamb", "lamb"), ("cost", "cost"), ("iters", "iters"),
            ("status", "status"), ("K_feedback", "K"), ("k_feedforward", "k"))
            if last[key] is not None}
        if exchange is None:
            outs["cost_it"] = cost_its[warmup + steps - 1]
            outs["best_idx"], outs["best_cost"] = picks[-1]
        else:
            r = last_round["res"]
            outs.update(cost_it=r["cost_local"], cost_all=r["cost_all"],
                        best_idx=torch.as_tensor(r["best_idx"]).reshape(-1),
                        winner_U=r["U"], winner_X=r["X"])
            if r.get("best_cost") is not None:
                outs["best_cost"] = r["best_cost"]
        dumped = dump_step_outputs(dump_dir, outs, B, torch)
    rank_seconds = [seconds]
    if grouped:
        t = torch.tensor([seconds], dtype=torch.float64,
                         device=solver.device if dist.get_backend() == "nccl" else "cpu")
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        rank_seconds = [float(x.item()) for x in allt]
        seconds = max(rank_seconds)
    timed = range(0, steps, event_stride)
    overhead = empty_bracket_ms(torch)
    raw = [ev0[i].elapsed_time(ev1[i]) for i in timed]
    kstat = spread([max(v - overhead, 0.0) for v in raw])
    kern_ms = kstat["median"]
    # every problem executes exactly `iters` iterations (no early exit): check on the last set
    assert int(sets[-1]["iters"].min()) == args.iters == int(sets[-1]["iters"].max())
    kernel = solver.iterate_kernel(B)
    res = dict(seconds=seconds, kernel_ms=kern_ms, kernel_ms_stats=kstat,
               kernel_ms_raw_median=spread(raw)["median"], event_pair_overhead_ms=overhead,
               iterations=world * B * args.iters * steps,
               rank_seconds=rank_seconds, kernel=kernel, layout=kernel_label(kernel, layout),
               # launches of ONE step: the fused round is one launch only on a single GPU; a sharded
               # step adds the winner's pack, the grouped all-gather, the pick on the gathered
               # vector and i2lqr_round_winner
               # (... the one-call round: local winner's pack, grouped gather, pick + hand-off; driven
               # from Python: pack, gather, arg-min, round winner)
               launches_per_step=((1 if fused else 3) +
                                  ((3 if one_call else 4) if exchange is not None else 0))
               if with_tail else 1,
               # share of the fixed-count iterations that were accepted steps (a rejected step of
               # the one-problem-per-lane kernels stores no states: "defer_states")
               accepted_fraction=accepted_fraction(sets[-1]["lamb"], l0_first, args.iters,
                                                   cfg.lamb_factor))
    if dumped is not None:
        res["dump_outputs"] = dumped
    if with_tail and exchange is None:
        # the pick of the last step is the first-index arg-min of its relaxed costs
        idx, val = picks[-1]
        first, best = dist_mod.select_best_flat(cost_its[warmup + steps - 1])
        assert int(idx.item()) == first and float(val.item()) == best, "fused pick mismatch"
    if exchange is not None:
        ms = lambda a, b: sum(xev[a][i].elapsed_time(xev[b][i]) for i in timed) / len(timed)
        res["one_call_round"] = bool(one_call)
        # the pick is the same on every rank, is the first-index arg-min of the gathered vector, and
        # the pack every rank holds is the trajectory its owner solved
        if args.handoff == "gather":
            idx, owner = (int(v) for v in picks[-1].cpu())
            first, best = dist_mod.select_best_flat(cost_alls[warmup + steps - 1])
        else:  # (two-collective form: the pick is a host integer, the costs are gathered again here)
            idx = int(picks[-1])
            owner = idx // B
            first, best = dist_mod.select_best_flat(xch.allgather(cost_its[warmup + steps - 1]))
        assert idx == first, f"exchange / pick mismatch: {idx} vs {first}"
        assert owner == idx // B, (owner, idx, B)
        if owner == rank:
            mine = solver.pack_problem(sets[warmup + steps - 1], torch.tensor(
                [idx - rank * B], dtype=torch.int64, device=solver.device))
            assert torch.equal(mine, winners[-1]), "the handed-over pack is not the owner's trajectory"
        assert bool(torch.isfinite(winners[-1]).all())
        res["handoff"] = ("--handoff broadcast: all-gather of the costs + i2lqr_argmin + 8-byte read-back "
                          "+ i2lqr_pack_problem on the owner + ONE ncclBroadcast (i2lqr_broadcast_winner)"
                          if args.handoff == "broadcast" else
                          "winner packs ride in the all-gather: ONE grouped collective "
                          "(i2lqr_allgather_round) + pick + owner's pack (i2lqr_round_pick), no host "
                          "round trip; the whole round is one C-ABI call" if one_call else
                          "winner packs ride in the all-gather (i2lqr_allgather_round / torch) + "
                          "i2lqr_argmin + i2lqr_round_winner, driven from Python, no host round trip")

        def fresh_sets():
            picks.clear(), winners.clear()
            for dst, src in zip(sets, make_step_buffers(solver, host, steps + warmup, torch)):
                dst.update(src)
            if plans:  # (the plans hold the addresses of the sets' tensors)
                for i in range(steps + warmup):
                    plans[i] = solver.plan_round(sets[i], qfun, cost_its[i], world * B, world, rank,
                                                 args.iters, bufs=xbufs[i], guard_previous=False)

        # The same round driven from Python (five enqueues: iterate_pick, pack, event + gather,
        # arg-min, round winner; what round 5 timed) on fresh copies of the batch: the phase marks
        # of the exchange come from here, and its ms_per_step beside the one-call form's is what
        # the C entry point buys on this box.
        if args.full and B <= 65536 and args.handoff == "gather":
            fresh_sets()
            h_seconds = timed_loop("gather_host")
            res["exchange_ms"] = ms("start", "picked")
            res["exchange_phases_ms"] = {"gather_costs_and_packs": ms("start", "gathered"),
                                         "pick_and_winner": ms("gathered", "picked")}
            res["host_driven_variant"] = {"ms_per_step": h_seconds / steps * 1e3,
                                          "one_call_ms_per_step": seconds / steps * 1e3}
        # The two-collective form for comparison (the pick read back, ONE ncclBroadcast from the
        # owner: i2lqr_broadcast_winner — what the controller's list-of-lists rounds use), on fresh
        # copies of the batch, same steps: its host round trip per step serialises the pipeline.
        if args.full and B <= 65536 and args.handoff == "gather":
            fresh_sets()
            b_seconds = timed_loop("broadcast")
            res["broadcast_variant"] = {
                "ms_per_step": b_seconds / steps * 1e3,
                "phases_ms": {"gather_costs": ms("start", "gathered"),
                              "pick_and_read_back": ms("gathered", "picked"),
                              "broadcast_winner": ms("picked", "handed_over")},
                "step": "sharded_round(lexi=flat pick on the host): all-gather(costs) + i2lqr_argmin "
                        "+ 8-byte read-back + i2lqr_pack_problem on the owner + "
                        "i2lqr_broadcast_winner"}
            assert int(picks[-1]) == dist_mod.select_best_flat(
                xch.allgather(cost_its[warmup + steps - 1]))[0]
        if exchange != "torch":
            res["nccl_world"] = exchange.comm_world
            res["exchange_path"] = "native"
            exchange.close()
        else:
            res["nccl_world"] = dist.get_world_size()
            res["exchange_path"] = "torch"
            if native_error:
                res["native_exchange_error"] = native_error
            if dist_mod.abandoned_bring_ups() or (native_error and "Poisoned" in native_error):
                # foreign launcher: nobody can restart the ranks, the run goes on over torch's
                # exchange and the process leaves through os._exit at the end
                res["poisoned_bring_up"] = True
    solver.close()
    return res


def time_launches(args, cfg, B, torch, iters, launches=EXTRA_LAUNCHES, warmup=EXTRA_WARMUP):
    """`launches` individually bracketed i2lqr_iterate launches after `warmup` untimed ones, each
    on its OWN copy of the batch (allocated and filled before the first launch: no launch finds its
    inputs warm in the 256 MB Infinity Cache because a restore copy has just written them):
    median / min / max kernel time (empty-bracket overhead subtracted)."""
    from ilqr_iterative_tasks_amd import BatchedILQR, workloads
    cfg = cfg.copy()
    layout = pick_layout(args, B, cfg=cfg)
    cfg.layout = LAYOUT_ID[layout]
    solver = BatchedILQR(cfg, torch.device("cuda", torch.cuda.current_device()))
    host = workloads.make_batch(cfg, B)
    sets = make_step_buffers(solver, host, warmup + launches, torch)
    l0 = sets[-1]["lamb"].clone()
    overhead = empty_bracket_ms(torch)
    vals = []
    for i in range(warmup + launches):
        buf = sets[i]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        solver.iterate(buf, iters)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            vals.append(max(e0.elapsed_time(e1) - overhead, 0.0))
    assert int(sets[-1]["iters"].min()) == iters == int(sets[-1]["iters"].max())
    kernel = solver.iterate_kernel(B)
    name = kernel_label(kernel, layout)
    acc = accepted_fraction(sets[-1]["lamb"], l0, iters, cfg.lamb_factor)
    solver.close()
    st = spread(vals)
    return {"kernel": kernel, "layout": name, "kernel_ms": st["median"],
            "kernel_ms_mean": st["mean"],  # (what a kernel-trace summary's AverageNs compares with)
            "kernel_ms_min": st["min"],
            "kernel_ms_max": st["max"], "kernel_ms_rel_spread": st["rel_spread"],
            "launches": st["samples"], "warmup": warmup, "accepted_fraction": acc,
            "waves_per_simd": waves_of(kernel, B) / SIMDS,
            "iterations_per_s": B * iters / (st["median"] * 1e-3)}


def time_candidate_round(args, B, torch, rounds=20, warmup=3):
    """Wall time of whole control rounds through control.iterative_ilqr.HipCandidateSolver (events
    around `rounds` consecutive calls; inputs resident on the device)."""
    import numpy as np
    from ilqr_iterative_tasks_amd import workloads
    from ilqr_iterative_tasks_amd.control.iterative_ilqr import HipCandidateSolver
    cfg = workloads.config_for(args.workload, "f64")
    host = workloads.make_batch(cfg, B)
    x0 = torch.as_tensor(host["X"][0, :, 0]).cuda()
    x_terms = torch.as_tensor(host["x_term"]).cuda()
    qfun = torch.zeros(B, dtype=torch.int32, device="cuda")
    hs = HipCandidateSolver(device=torch.device("cuda", torch.cuda.current_device()))
    obs = (31.0, -3.0, 8.0, 6.0, 0.0, 0.0)
    for _ in range(warmup):
        out = hs.candidate_round(cfg, x0, x_terms, qfun, 1.0, obs_rec=obs, n_iters=args.iters)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        out = hs.candidate_round(cfg, x0, x_terms, qfun, 1.0, obs_rec=obs, n_iters=args.iters)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / rounds
    s = out["solver"]
    return {"iterations_per_s": B * args.iters / (ms * 1e-3), "ms_per_round": ms, "batch": B,
            "kernel": s.iterate_kernel(B), "layout": LAYOUT_NAME[{0: "wave", 1: "lane", 2: "tiled"}[s.cfg.layout]],
            # device tensors in, cost_it / pick / winner's U, X out; layout chosen by
            # i2lqr_recommended_layout; the round = initial state in the chosen layout +
            # i2lqr_iterate_pick + winner gather
            "entry": "HipCandidateSolver.candidate_round"}


class quiet_stdout:
    """RCCL prints a version banner to the C stdout when a communicator comes up (buffered: it
    would land BEHIND the JSON line when stdout is a file).  Around a bring-up: fd 1 points at
    stderr, the C buffers are flushed inside, fd 1 comes back — stdout carries the JSON line only."""

    def __enter__(self):
        import ctypes
        self._libc = ctypes.CDLL(None)
        sys.stdout.flush()
        self._libc.fflush(None)
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush()
        self._libc.fflush(None)
        os.dup2(self._saved, 1)
        os.close(self._saved)
        return False


def measure_sharded_overhead(args, cfg, B, torch, dist_mod, steps=50, reps=4, options=None):
    """Per-rank cost of the SHARDED step beside the unsharded one, in ONE process on ONE GPU
    (the only evidence for the >= 6x-at-8-GPUs target obtainable without the node —
    weak scaling needs the sharded pipeline to sustain the unsharded step's rate per rank).  A world
    of one over the library's own RCCL communicator (the all-gathers are self-copies inside RCCL;
    without RCCL: device copies), `reps` x `steps` steps of each form, interleaved, every step on
    its own copy of the batch, restored before each run:
      unsharded          i2lqr_iterate_pick                      (bench.py --gpus 1's step)
      sharded_one_call   HipCandidateSolver.sharded_round -> i2lqr_sharded_round_flat, exchange on
                         a side stream                           (bench.py --gpus N's step)
      sharded_host_driven  the same round as five Python-driven enqueues (round 5's step)
    step_ms = wall time of the run / steps (enqueue loop + final synchronise); host_enqueue_ms =
    wall time of the enqueue loop alone / steps (what the host needs per step: it must stay below
    the GPU's step for the pipeline to be fed).  Medians over the reps."""
    from ilqr_iterative_tasks_amd import BatchedILQR, workloads
    from ilqr_iterative_tasks_amd.control.iterative_ilqr import HipCandidateSolver
    cfg = cfg.copy()
    layout = pick_layout(args, B, cfg=cfg)
    cfg.layout = LAYOUT_ID[layout]
    solver = BatchedILQR(cfg, torch.device("cuda", torch.cuda.current_device()))
    for key, val in (options or {}).items():  # (tools/sharded_overhead.py: A/B of a scheduling option)
        solver.set_option(key, int(val))
    host = workloads.make_batch(cfg, B)
    sets = make_step_buffers(solver, host, steps, torch, want_gains=False)
    pristine = {k: sets[0][k].clone() for k in ("X", "U", "lamb")}
    qfun = torch.zeros(B, dtype=torch.int32, device=solver.device)
    cost_its = [torch.zeros(B, dtype=solver.dtype, device=solver.device) for _ in range(steps)]
    bests = [(torch.zeros(1, dtype=torch.int64, device=solver.device),
              torch.zeros(1, dtype=solver.dtype, device=solver.device)) for _ in range(steps)]
    path, err = "native (RCCL world of one)", None
    try:
        with quiet_stdout():
            xch = dist_mod.CostExchange(solver)
    except Exception as e:  # noqa: BLE001
        xch, path, err = dist_mod.TorchExchange(), "device copies (no RCCL)", f"{type(e).__name__}: {e}"
    xbufs = [solver.round_buffers(B, B, 1) for _ in range(steps)]
    plans = [solver.plan_round(sets[i], qfun, cost_its[i], B, 1, 0, args.iters, bufs=xbufs[i],
                               guard_previous=False) for i in range(steps)]
    rounds = HipCandidateSolver(solver.device)
    side = dist_mod.exchange_stream(solver.device)  # (probed: not on the launch stream's hardware queue)

    def unsharded(i):
        solver.iterate_pick(sets[i], args.iters, qfun, 0, 55, cost_its[i], best=bests[i])

    def one_call(i):
        rounds.sharded_round(cfg, None, None, None, None, xch, B, n_iters=args.iters, plan=plans[i],
                             exchange_stream=side)

    def host_driven(i):
        rounds.sharded_round(cfg, None, None, None, None, xch, B, n_iters=args.iters,
                             prepared=(solver, sets[i], qfun, cost_its[i]), bufs=xbufs[i],
                             exchange_stream=side, host_driven=True)

    modes = {"unsharded": unsharded, "sharded_one_call": one_call, "sharded_host_driven": host_driven}
    samples = {m: {"step_ms": [], "host_enqueue_ms": []} for m in modes}
    picks = {}
    for rep in range(reps + 1):  # (the first repetition warms everything up and is dropped)
        for name, fn in modes.items():
            for b in sets:
                for k, v in pristine.items():
                    b[k].copy_(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                fn(i)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep:
                samples[name]["step_ms"].append((t2 - t0) / steps * 1e3)
                samples[name]["host_enqueue_ms"].append((t1 - t0) / steps * 1e3)
            picks[name] = (int(bests[-1][0]) if name == "unsharded"
                           else int(xbufs[-1]["best_global"][0]))
    assert len(set(picks.values())) == 1, f"the three forms disagree on the pick: {picks}"
    if hasattr(xch, "close"):
        xch.close()
    solver.close()
    med = lambda v: spread(v)["median"]
    out = {"batch": B, "steps_per_run": steps, "runs_per_form": reps, "exchange": path,
           "forms": {m: {"step_ms": med(v["step_ms"]), "host_enqueue_ms": med(v["host_enqueue_ms"]),
                         "step_ms_runs": v["step_ms"], "host_enqueue_ms_runs": v["host_enqueue_ms"]}
                     for m, v in samples.items()}}
    f = out["forms"]
    out["sharded_over_unsharded"] = f["sharded_one_call"]["step_ms"] / f["unsharded"]["step_ms"]
    out["host_driven_over_unsharded"] = f["sharded_host_driven"]["step_ms"] / f["unsharded"]["step_ms"]
    if err:
        out["native_exchange_error"] = err
    return out


def closed_loop_config1(torch):
    """BASELINE.json configs[0] — the reference's own CPU-runnable case and its only timing
    ("time to solve" per control step, utils/base.py:145-150) — through the product: three laps of
    tests/ilqr_test.py's set-up (--lap-number 3 --num-ss-iters 2 --num-ss-points 8, obstacle
    (31, -3, 8, 6)) driven by control.iLqr in its three host modes.  Wall seconds, mean / p95
    control-step milliseconds, lap lengths (asserted for the reference's semantics, chained lamb:
    121 / 54 / 29 / 23)."""
    import numpy as np
    from ilqr_iterative_tasks_amd import harness
    from ilqr_iterative_tasks_amd.control import KineticBicycleParam, Obstacle, iLqr, iLqrParam

    def run(lamb_mode, device_rounds):
        ego = harness.KineticBicycle(system_param=KineticBicycleParam())
        ego.set_state(np.zeros(4))
        ego.set_timestep(1)
        ego.get_traj()
        ego.set_zero_noise()
        ctrl = iLqr(iLqrParam(num_ss_points=8, num_ss_iter=2, timestep=1, num_horizon=6),
                    obstacle=Obstacle(31, -3, 8, 6), system_param=KineticBicycleParam(),
                    lamb_mode=lamb_mode, device_rounds=device_rounds)
        ctrl.add_trajectory(ego.xcl, ego.ucl)
        ctrl.set_timestep(1)
        ego.set_ctrl_policy(ctrl)
        t0 = time.perf_counter()
        laps = harness.run_laps(ego, ctrl, 3)
        wall = time.perf_counter() - t0
        t = np.concatenate([np.ravel(x) for x in ego.diagnostics["solver_time"]])
        return laps, t, wall

    # The reference: BASELINE.md section 2, the reference itself (NumPy) on 1 thread of an 8-core
    # Xeon @ 2.1 GHz; not measured here, its Python does not travel.  The three modes:
    #   chained        lamb chained across the candidates of a lap (the reference's exact semantics):
    #                  8 dependent chain steps per round over the two laps, the chain carried on the
    #                  device (HipCandidateSolver.solve_chained: one upload, 8 launches replayed as a
    #                  hipGraph, one read-back per round)
    #   independent    independent lamb per candidate, one batched solve per round, host rounds
    #   device_rounds  independent lamb, the three rounds chained on the GPU and replayed as a hipGraph
    out = {"workload": "BASELINE.json configs[0]: ilqr_test.py --lap-number 3 --num-ss-iters 2 "
                       "--num-ss-points 8",
           "reference": {"wall_s": 74.4, "control_step_ms_mean": 700.0, "cores": 1,
                         "provenance": "BASELINE.md section 2 (not measured here)"}}
    for key, mode, dev in (("chained", "chained", False), ("independent", "independent", False),
                           ("device_rounds", "independent", True)):
        run(mode, dev)  # warm-up: library load, allocator, graph capture
        laps, t, wall = run(mode, dev)
        if key == "chained":
            assert [int(v) for v in laps] == [121, 54, 29, 23], laps
        out[key] = {"laps": [int(v) for v in laps], "wall_s": wall, "control_steps": int(len(t)),
                    "control_step_ms_mean": float(t.mean() * 1e3),
                    "control_step_ms_median": float(np.median(t) * 1e3),
                    "control_step_ms_p95": float(np.percentile(t, 95) * 1e3),
                    "control_step_ms_max": float(t.max() * 1e3)}
    return out


def roofline_entry(cfg, B, iters, r, traffic):
    """HBM (and fp64) fractions of one timed workload from its median kernel time."""
    from ilqr_iterative_tasks_amd import workloads
    bts = workloads.algorithmic_bytes_per_iteration(cfg)
    ach = bts * B * iters / (r["kernel_ms"] * 1e-3) / 1e9
    out = dict(r)
    out.update({"batch": B, "iterations_per_launch": iters,
                "algorithmic_bytes_per_iteration": bts, "achieved_GBs": ach,
                "hbm_frac": ach / HBM_PEAK_GBS,
                "hbm_frac_of_mean": bts * B * iters / (r["kernel_ms_mean"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "traffic": traffic})
    if traffic:
        out["traffic_over_algorithmic"] = traffic / (bts * B * iters)
    return out


def run_solve(args, cfg, B, torch, reps=3, single_launch=False, want_gains=False):
    """One solve to termination per rep, each on its own copy of the batch.  Outputs = what the
    reference's ilqr() returns (uvar, xvar, lamb: control/iterative_ilqr.py:85) plus cost, iteration
    count and status per problem; the gains of the last backward pass are an extra of this library
    (want_gains: +0.05-0.09 ms at 65536 problems for their scatter to the caller's arrays)."""
    from ilqr_iterative_tasks_amd import BatchedILQR, workloads
    cfg = cfg.copy()
    layout = pick_layout(args, B, solve=True, cfg=cfg)
    cfg.layout = LAYOUT_ID[layout]
    solver = BatchedILQR(cfg, torch.device("cuda", torch.cuda.current_device()))
    if single_launch:
        solver.set_compaction(0)
    host = workloads.make_batch(cfg, B)
    sets = make_step_buffers(solver, host, reps + 1, torch, want_gains=want_gains)
    solver.solve(sets[0])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        solver.solve(sets[1 + i])
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    it = sets[1]["iters"].double()
    executed = float(it.sum())
    kernel = solver.solve_kernel(B)
    if kernel.startswith("k_lane_iterate") and not single_launch:
        kernel += " chunks (compaction folded into their exit) + k_group_spec tail"
    solver.close()
    return {"executed_iterations_per_s": executed / (ms * 1e-3), "ms_per_solve": ms,
            "iterations_mean": executed / B, "iterations_max": int(it.max()), "kernel": kernel,
            "outputs": "U, X, lamb, cost, iters, status" + (", K, k" if want_gains else "")}


def lib_sha256():
    try:
        return hashlib.sha256(LIB.read_bytes()).hexdigest()
    except OSError:
        return None


class PmcFile:
    """profiles/pmc_traffic.json: per-launch HBM bytes (FETCH_SIZE / WRITE_SIZE) and SQ counters
    from separate `rocprofv3 --pmc` passes (tools/collect_profiles.sh), stamped with the sha256 of
    the library they were collected on.  Counters of another build are not reported: `traffic`
    becomes null and `traffic_stale` true."""

    def __init__(self):
        try:
            self.data = json.loads((ROOT / "profiles" / "pmc_traffic.json").read_text())
        except Exception:
            self.data = {}
        self.collected_on = (self.data.get("_meta") or {}).get("lib_sha256")
        self.running = lib_sha256()
        self.stale = self.collected_on is None or self.collected_on != self.running

    def get(self, key, field="hbm_bytes_per_launch"):
        rec = self.data.get(key)
        if self.stale or not rec:
            return None
        return rec.get(field)

    def stamp(self):
        return {"traffic_stale": self.stale,
                "traffic_source": "profiles/pmc_traffic.json (rocprofv3 --pmc passes, "
                                  f"library sha256 {str(self.collected_on)[:16]})",
                "library_sha256": str(self.running)[:16]}


def issue_roofline(pmc, key, kernel_ms, waves):
    """Instruction-issue roofline of a launch whose wavefronts each sit alone on a SIMD: such a
    wavefront issues at most one instruction per 4 cycles, whatever the instruction
    (MI355X_MICROARCH.md, 'vector-instruction ISSUE cost').  achieved = wavefront-instructions
    issued per second (SQ_INSTS_VALU + SALU + LDS + ... = SQ_INSTS of the --pmc pass, per launch,
    / the kernel time measured here); peak = SIMDs occupied by ALL launched wavefronts x clock / 4
    (helper wavefronts included: their instructions are in the numerator, so their SIMDs are in
    the denominator)."""
    insts = pmc.get(key, "wave_instructions_per_launch")
    launched = pmc.get(key, "waves_per_launch")
    occupied = int(launched) if launched and launched > waves else waves
    simds = min(occupied, SIMDS)
    peak = simds * CLOCK_GHZ / 4.0  # G wave-instructions / s
    out = {"bound": "issue", "unit": "G wavefront-instructions/s", "peak": peak,
           "simds_occupied": simds, "achieved": None, "frac": None,
           "wave_instructions_per_launch": insts}
    if occupied > waves:
        # k_group_iterate up to 2048 problems: two helper wavefronts per workgroup take a share of
        # the per-step records and sleep at a barrier otherwise
        out["helper_wavefronts"] = int(occupied - waves)
        out["main_wavefronts"] = int(waves)
    if insts:
        out["achieved"] = insts / (kernel_ms * 1e-3) / 1e9
        out["frac"] = out["achieved"] / peak
    return out


def cpu_quota():
    """CPUs this process may actually use: the affinity mask capped by the cgroup CPU quota (a
    container that SEES 256 logical CPUs may be allowed 16 CPUs' worth of time: threads beyond
    the quota are throttled, which reads as an OpenMP port that does not scale)."""
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = Path("/sys/fs/cgroup/cpu.max").read_text().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except Exception:  # noqa: BLE001
        try:
            q = int(Path("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read_text())
            per = int(Path("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read_text())
            if q > 0:
                quota = q / per
        except Exception:  # noqa: BLE001
            pass
    usable = avail if quota is None else max(1, min(avail, int(quota)))
    return avail, quota, usable


def cpu_baseline(cfg, B, iters, budget_s):
    """The CPU oracle (a port of the reference algorithm, oracle/ilqr_oracle.c, OpenMP over the
    batch, static chunks, threads pinned: OMP_PROC_BIND=spread) on the host cores of this box:
    same synthetic workload, same fixed iteration count, sweeps of 65536 problems for about
    `budget_s` seconds of wall time.  Threads = the CPUs the cgroup quota grants this process."""
    os.environ.setdefault("OMP_PROC_BIND", "spread")  # before libgomp starts its first team
    os.environ.setdefault("OMP_PLACES", "cores")
    from ilqr_iterative_tasks_amd import workloads
    from oracle import oracle as orc
    avail, quota, usable = cpu_quota()
    NB = 65536
    host = workloads.make_batch(cfg, NB)

    def run(nprob):
        sl = slice(0, nprob)
        t0 = time.perf_counter()
        orc.ilqr_batch(cfg, host["X"][sl], host["U"][sl], host["x_term"][sl], host["lamb"][sl],
                       host["obs"][sl], max_iter=iters, early_exit=False, want_gains=True)
        return time.perf_counter() - t0

    orc.set_threads(1)
    run(256)
    one_thread = 1024 * iters / run(1024)
    # the quota's thread count, and half / twice of it (SMT siblings, a quota below the mask):
    # keep the fastest
    probes = {}
    for nt in sorted({max(1, usable // 2), usable, min(avail, 2 * usable)}):
        orc.set_threads(nt)
        run(min(NB, 1024 * nt))  # warm the team
        probes[nt] = NB * iters / run(NB)
    best_t = max(probes, key=probes.get)
    threads = orc.set_threads(best_t)
    t_all = NB * iters / probes[best_t]
    sweeps = max(1, min(400, int(budget_s / max(t_all, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(sweeps):
        run(NB)
    dt = time.perf_counter() - t0
    return dict(value=NB * sweeps * iters / dt, unit="iLQR iterations/s", cores=threads,
                kind="port",
                sample=f"{NB} problems x {iters} iterations x {sweeps} sweeps of the bench "
                       f"workload, OpenMP (static chunks, OMP_PROC_BIND=spread) on {threads} "
                       f"threads; {avail} logical CPUs visible, cgroup quota "
                       f"{'none' if quota is None else f'{quota:g} CPUs'}; {dt:.1f} s wall",
                value_1thread=one_thread, logical_cpus=avail, cgroup_cpu_quota=quota,
                threads_probed={str(k): v for k, v in probes.items()},
                # the reference's own ilqr() (NumPy) on 1 thread of an
                # 8-core Xeon @ 2.1 GHz, config 1: n=4, m=2, N=6, 56073 iterations in 74.16 s; 268
                # it/s at N=20.  Not measured here: the reference's Python does not travel.
                reference_python={
                    "value": 756.0, "unit": "iLQR iterations/s", "cores": 1,
                    "provenance": "BASELINE.md section 2 (config 1, not measured here)"})


def run_exchange_only(args, rank, world, torch, dist_mod):
    # test hook of the launcher's timeout / fresh-process fallback (tests/test_dist_gloo.py): a
    # "native" attempt that never returns, as a rank stuck in a communicator bootstrap would
    if args.test_hooks and os.environ.get("I2LQR_BENCH_TEST_HANG") == args.exchange:
        time.sleep(3600)
    """The multi-rank harness without the solve (CPU tensors, gloo): per step every rank
    contributes a synthetic cost shard, all-gathers, and picks; the pick is checked against the
    shards every rank can regenerate from the seeds."""
    import numpy as np
    import torch.distributed as dist
    B = args.batch or 1024
    total = B * world

    def shard(step, r):
        return np.random.default_rng([20230228, step, r]).uniform(1.0, 1e4, B)

    grouped = dist.is_available() and dist.is_initialized()

    def step(i):
        cost_all = dist_mod.allgather_costs(torch.as_tensor(shard(i, rank)))
        return dist_mod.select_best_flat(cost_all)

    for i in range(args.warmup):
        step(i)
    if grouped:
        dist.barrier()
    t0 = time.perf_counter()
    pick = None
    for i in range(args.steps):
        pick = step(args.warmup + i)
    if grouped:
        dist.barrier()
    seconds = time.perf_counter() - t0
    if grouped:
        t = torch.tensor([seconds], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        seconds = float(t.item())
    full = np.concatenate([shard(args.warmup + args.steps - 1, r) for r in range(world)])
    assert pick == (int(np.argmin(full)), float(full.min())), "all-gather / pick mismatch"
    return {
        "metric": "exchange-only dry run: candidates/s through all-gather + arg-min (NO solve; "
                  "harness check, not a solver throughput)",
        "value": total * args.steps / seconds, "unit": "candidates/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": seconds / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic cost shards (no GPU, gloo)",
        "config": {"workload": "exchange-only", "batch_per_gpu": B, "global_batch": total,
                   "backend": dist.get_backend() if grouped else "none",
                   "parallelism": f"batch-sharded x{world}, one all-gather of terminal costs"},
    }


def run_rank(args) -> int:
    import torch
    from ilqr_iterative_tasks_amd import dist as dist_mod, workloads

    gpu_mode = not args.exchange_only
    want = int(os.environ.get("WORLD_SIZE", "1"))
    # I2LQR_BENCH_SHARE_GPU=1 (test hook for single-GPU boxes): the ranks take the visible devices
    # round-robin and the process group runs on gloo — RCCL refuses two ranks on one device, so
    # the native exchange's bring-up fails on the real library and every rank falls back together
    share_gpu = gpu_mode and os.environ.get("I2LQR_BENCH_SHARE_GPU") == "1" and torch.cuda.device_count() > 0
    if gpu_mode and not share_gpu and torch.cuda.device_count() < want:  # (counting devices initialises nothing)
        if int(os.environ.get("RANK", "0")) == 0:
            print(f"bench.py: {want} ranks but {torch.cuda.device_count()} HIP devices are "
                  "visible (use --exchange-only for the CPU dry run of the harness)",
                  file=sys.stderr)
        return 3
    rank, world, local = dist_mod.init_from_env("nccl" if gpu_mode and not share_gpu else "gloo")
    if share_gpu:
        local %= torch.cuda.device_count()
    if world != max(1, args.gpus):
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks",
                  file=sys.stderr)
        return 2
    import torch.distributed as dist
    if not gpu_mode:
        out = run_exchange_only(args, rank, world, torch, dist_mod)
        if rank == 0:
            print(result_line(out), flush=True)
        if dist.is_available() and dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
        return 0
    torch.cuda.set_device(local)
    wl = workloads.CONFIGS[args.workload]
    cfg = workloads.config_for(args.workload, args.dtype)
    B = args.batch or wl["batch"]
    dtype = "f64" if cfg.dtype == 0 else "f32"
    pmc = PmcFile()

    res = run_gpu(args, cfg, B, rank, world, torch, dist_mod, args.steps, args.warmup,
                  event_stride=event_stride_for(args.steps),
                  dump_dir=args.dump_outputs if rank == 0 else None)
    value = res["iterations"] / res["seconds"]
    alg_bytes = workloads.algorithmic_bytes_per_iteration(cfg)
    achieved = alg_bytes * B * args.iters / (res["kernel_ms"] * 1e-3) / 1e9
    key = f"{args.workload}:{dtype}:B{B}:it{args.iters}"
    waves = waves_of(res["kernel"], B)

    out = {
        "metric": "batched iLQR iterations/s (n=6,m=2,N=20)" if wl["system"] == "bicycle6"
        else f"batched iLQR iterations/s ({wl['system']}, N={wl['N']})",
        "value": value,
        "unit": "iLQR iterations/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": res["seconds"] / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": dtype,
        "data": "synthetic",
        "config": {"workload": f"BASELINE.json configs[{int(args.workload[-1]) - 1}] ({args.workload}): "
                               f"{wl['system']} n={cfg.n} m={cfg.m} N={cfg.N} dt={cfg.dt}",
                   "batch_per_gpu": B, "global_batch": B * world, "layout": res["layout"],
                   "iterations_per_step": args.iters,
                   "step": ("i2lqr_iterate_pick: ONE launch (iterations + relaxed cost + pick)"
                            if res["launches_per_step"] == 1 and "exchange_path" not in res else
                            "i2lqr_iterate + i2lqr_relax_cost + i2lqr_argmin"
                            if "exchange_path" not in res else
                            "HipCandidateSolver.sharded_round (the product's sharded control round) "
                            "= ONE C-ABI call, i2lqr_sharded_round_flat: i2lqr_iterate_pick on the "
                            "shard (iterations + relaxed cost + local pick) on the launch stream; "
                            "local winner's pack + ONE grouped all-gather of costs and packs + pick "
                            "and owner's pack (i2lqr_round_pick) on the exchange stream: pick AND "
                            "the winner's hand-off inside the timed step, no host round trip"
                            if res.get("one_call_round") else
                            "HipCandidateSolver.sharded_round driven from Python (torch exchange): "
                            "i2lqr_iterate_pick + i2lqr_pack_problem + all-gather of costs and "
                            "local-winner packs + i2lqr_argmin + i2lqr_round_winner"),
                   "launches_per_step": res["launches_per_step"],
                   "parallelism": f"batch-sharded x{world}, one all-gather of terminal costs"},
    }
    # (the driver keeps the head of the line: the multi-rank facts come before the long objects)
    out["per_rank_iterations_per_s"] = [B * args.iters * args.steps / s for s in res["rank_seconds"]]
    if "exchange_path" in res:
        item = 8 if dtype == "f64" else 4
        out["exchange"] = {"path": res["exchange_path"], "nccl_world": res["nccl_world"],
                           "one_call_round": res.get("one_call_round"),
                           # (phase marks: from the host-driven form of the same round, see there)
                           "ms_per_step": res.get("exchange_ms"),
                           "phases_ms": res.get("exchange_phases_ms"),
                           "what": ("i2lqr_allgather_round (RCCL: two ncclAllGather in one group, via "
                                    "the C-ABI)" if res["exchange_path"] == "native" else
                                    "torch.distributed all-gathers (costs, packs)") +
                                   " + pick + owner's pack on a side stream",
                           "handoff": res["handoff"],
                           "bytes_per_rank": (B + cfg.m * cfg.N + cfg.n * (cfg.N + 1)) * item}
        for k in ("native_exchange_error", "poisoned_bring_up", "host_driven_variant",
                  "broadcast_variant"):
            if k in res:
                out["exchange"][k] = res[k]
    if args.full and world > 1 and args.steps < LONG_RUN_STEPS:
        # the contract's K timed steps may be a few milliseconds, of which the two barriers are a
        # visible share: the same loop once more over LONG_RUN_STEPS steps, reported beside it
        lr = run_gpu(args, cfg, B, rank, world, torch, dist_mod, LONG_RUN_STEPS, args.warmup,
                     event_stride=event_stride_for(LONG_RUN_STEPS))
        out["long_run"] = {"steps": LONG_RUN_STEPS, "value": lr["iterations"] / lr["seconds"],
                           "ms_per_step": lr["seconds"] / LONG_RUN_STEPS * 1e3,
                           "per_rank_iterations_per_s": [B * args.iters * LONG_RUN_STEPS / s
                                                         for s in lr["rank_seconds"]],
                           "exchange_path": lr.get("exchange_path"),
                           "exchange_ms_per_step": lr.get("exchange_ms")}
    out.update({
        "roofline": {"bound": "hbm", "kernel": res["kernel"], "achieved": achieved,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                     "traffic": pmc.get(key), "algorithmic_bytes_per_iteration": alg_bytes,
                     # median of the sampled launches of the timed region, empty event pair
                     # subtracted (kernel_ms_raw_median is what the events report as is)
                     "kernel_ms_avg": res["kernel_ms"],
                     "kernel_ms_samples": res["kernel_ms_stats"]["samples"],
                     "kernel_ms_mean": res["kernel_ms_stats"]["mean"],
                     "kernel_ms_min": res["kernel_ms_stats"]["min"],
                     "kernel_ms_max": res["kernel_ms_stats"]["max"],
                     "kernel_ms_raw_median": res["kernel_ms_raw_median"],
                     "event_pair_overhead_ms": res["event_pair_overhead_ms"],
                     "step_ms_outside_kernel": res["seconds"] / args.steps * 1e3 - res["kernel_ms"],
                     "accepted_fraction": res["accepted_fraction"],
                     "waves_per_simd": waves / SIMDS, **pmc.stamp()},
        "roofline_issue": issue_roofline(pmc, key, res["kernel_ms"], waves),
    })
    # SQ counters of the same kernel (separate --pmc pass): shares of the wavefronts' lifetime spent
    # issuing (any / VALU), parked on s_waitcnt, stalled
    out["roofline_issue"]["sq_shares_of_wave_cycles"] = pmc.get(key, "sq_shares_of_wave_cycles")

    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg, B, args.iters, args.cpu_seconds)
    with_extra = args.full and not args.no_extra
    extra = {}
    if with_extra:
        # configs[3] strong-scaled: 2^20 problems over all ranks, exchange included
        total = 1 << 20
        ecfg = workloads.config_for(args.workload, "f64")
        r = run_gpu(args, ecfg, total // world, rank, world, torch, dist_mod, 3, 2)
        eb_bytes = workloads.algorithmic_bytes_per_iteration(ecfg)
        ach = eb_bytes * (total // world) * args.iters / (r["kernel_ms"] * 1e-3) / 1e9
        extra["config4_strong"] = {
            "iterations_per_s": r["iterations"] / r["seconds"], "global_batch": total,
            "batch_per_gpu": total // world, "scaling": "strong", "kernel": r["kernel"],
            "layout": r["layout"], "kernel_ms": r["kernel_ms"], "achieved_GBs_per_gpu": ach,
            "hbm_frac_per_gpu": ach / HBM_PEAK_GBS,
            "exchange_ms_per_step": r.get("exchange_ms"), "nccl_world": r.get("nccl_world")}
    if world == 1 and with_extra:
        # secondary single-GPU workloads (not the headline): EXTRA_LAUNCHES individually timed
        # launches each after EXTRA_WARMUP, median kernel time (min / max / spread beside it)
        def timed(workload, edt, eb, iters):
            ecfg = workloads.config_for(workload, edt)
            r = time_launches(args, ecfg, eb, torch, iters)
            return roofline_entry(ecfg, eb, iters, r, pmc.get(f"{workload}:{edt}:B{eb}:it{iters}"))

        for name, eb, edt in (("B4096_f64", 4096, "f64"), ("B8192_f64", 8192, "f64"),
                              ("B12288_f64", 12288, "f64"), ("B16384_f64", 16384, "f64"),
                              ("B24576_f64", 24576, "f64"), ("B32768_f64", 32768, "f64"),
                              ("B65536_f32", 65536, "f32"),
                              ("B1048576_f64", 1 << 20, "f64"), ("B1048576_f32", 1 << 20, "f32")):
            extra[name] = timed(args.workload, edt, eb, args.iters)
        # the large-batch fp64 regime as a first-class object: BASELINE's roofline batch (65536)
        # and the per-GPU shard of configs[3] (2^20 / 8 = 131072)
        out["roofline_large_batch"] = {
            "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "dtype": "f64",
            "B65536": timed(args.workload, "f64", 65536, args.iters),
            "B131072": timed(args.workload, "f64", 131072, args.iters)}
        # ilqr() to termination (1..98 iterations per problem) is what the reference actually
        # calls (control/iterative_ilqr.py:7-85): executed iterations per second of one solve of
        # 65536 problems against the fixed-count rate of the same batch; where the solve's time
        # goes by kernel comes from the kernel trace under profiles/ (same library only)
        rs = run_solve(args, workloads.config_for(args.workload, "f64"), 65536, torch, reps=5)
        rs["ms_per_solve_with_gains_out"] = run_solve(
            args, workloads.config_for(args.workload, "f64"), 65536, torch, reps=5,
            want_gains=True)["ms_per_solve"]
        fixed = out["roofline_large_batch"]["B65536"]["iterations_per_s"]
        # kernel_time_shares: rocprofv3 kernel trace of 10 solves
        # (profiles/<round>_kstats_solve_f64_B65536.csv); k_group_spec is the speculative tail that
        # finishes the stragglers, k_lane_iterate the first chunk of the whole batch
        rs.update({"batch": 65536, "dtype": "f64", "fixed_count_iterations_per_s": fixed,
                   "frac_of_fixed_count_rate": rs["executed_iterations_per_s"] / fixed,
                   "kernel_time_shares": pmc.get("solve:f64:B65536", "kernel_time_shares"),
                   "kernels_ms_per_solve": pmc.get("solve:f64:B65536", "kernels_ms_per_solve")})
        out["roofline_solve"] = rs
        # BASELINE configs[4]: quadrotor-sized n=12, m=4, N=50, B=65536, fp64 (33912 algorithmic
        # bytes and 600 k algorithmic flops per iteration); 4 fused iterations per launch
        q = timed("config5", "f64", 65536, 4)
        qflops = workloads.algorithmic_flops_per_iteration(workloads.config_for("config5", "f64"))
        q["algorithmic_flops_per_iteration"] = qflops
        q["achieved_fp64_TFLOPs"] = q["iterations_per_s"] * qflops / 1e12
        q["fp64_vector_peak_TFLOPs"] = FP64_VECTOR_PEAK_TFLOPS
        q["dense_form_fp64_flop_frac"] = q["achieved_fp64_TFLOPs"] / FP64_VECTOR_PEAK_TFLOPS
        # what the kernel EXECUTES (fp64 instruction counters of a separate --pmc pass, 64 lanes
        # per wavefront-instruction, a multiply-add = 2): the sparsity of [A | B] is folded into the
        # instruction stream, so this is the figure to hold against the vector peak
        ex = pmc.get("config5:f64:B65536:it4", "executed_fp64_flops_per_problem_iteration")
        q["executed_fp64_flops_per_iteration"] = ex
        q["executed_fp64_TFLOPs"] = q["iterations_per_s"] * ex / 1e12 if ex else None
        # fp64_flop_frac = EXECUTED flops (profiles/pmc_traffic.json) / 78.6 TFLOP/s; dense_form_*
        # prices the reference's dense form (600 k flops per iteration), of which the
        # kernel executes a part
        q["fp64_flop_frac"] = (q["executed_fp64_TFLOPs"] / FP64_VECTOR_PEAK_TFLOPS) if ex else None
        extra["config5_quad12_B65536_f64"] = q
        # the same plant in fp32 on the lane layouts (round 5: new there; VERDICT r5 Weak #9: it had
        # no roofline entry): 16956 algorithmic bytes per iteration
        extra["config5_quad12_B65536_f32"] = timed("config5", "f32", 65536, 4)
        # the product surface: HipCandidateSolver.candidate_round — 65536 candidates of one control
        # round handed over as device tensors (x0, x_term[B, n], qfun[B]); the library picks the
        # layout (i2lqr_recommended_layout), the round stays on the device: initial state written
        # in that layout, 10 fused iterations, relaxed costs, flat pick, the winner's trajectory
        extra["candidate_round_B65536_f64"] = time_candidate_round(args, 65536, torch)
        # solve to termination (reference exits: 1..150 iterations per problem): executed
        # iterations per second — lanes that finish early idle until their wavefront's slowest
        # problem is done, so this is below the fixed-count rate.  Default = chunked solve with
        # compaction and the one-problem-per-wavefront tail; single launch beside it.
        f64 = workloads.config_for(args.workload, "f64")
        for sb in (1024, 4096, 16384):
            extra[f"solve_to_termination_B{sb}_f64"] = run_solve(args, f64, sb, torch)
        extra["solve_to_termination_B65536_f64"] = "see roofline_solve"
        # the sharded step's per-rank overhead, beside the unsharded step
        extra["sharded_overhead"] = measure_sharded_overhead(args, cfg, B, torch, dist_mod)
        extra["sharded_overhead_B131072"] = measure_sharded_overhead(
            args, workloads.config_for(args.workload, "f64"), 131072, torch, dist_mod, steps=8, reps=3)
        # (the medians only: the per-run samples are tools/sharded_overhead.py's to report)
        for key in ("sharded_overhead", "sharded_overhead_B131072"):
            for form in extra[key]["forms"].values():
                del form["step_ms_runs"], form["host_enqueue_ms_runs"]
        # the reference's own metric (per-control-step "time to solve") on configs[0]
        extra["config1_closed_loop"] = closed_loop_config1(torch)
        extra["solve_to_termination_B65536_f64_single_launch"] = run_solve(
            args, f64, 65536, torch, single_launch=True)
    # The secondary figures at SECONDARY_DIGITS (the headline keeps full precision), rounded before
    # the claims below copy them; with the line compact, it stays below 16 KiB.
    for key in ("roofline_large_batch", "roofline_solve"):
        if key in out:
            out[key] = round_sig(out[key])
    extra = round_sig(extra)
    if extra:
        out["extra"] = extra
    if "dump_outputs" in res:
        out["dump_outputs"] = res["dump_outputs"]
    if world == 1 and with_extra:
        # The figures that carry the claims, as FLAT scalars of `roofline` IMMEDIATELY behind `frac`
        # (a consumer that keeps the first scalars of `roofline` still finds every
        # one; round 5's sat behind a dict and were cut): the full objects stay where they are.
        lb = out["roofline_large_batch"]
        so = extra["sharded_overhead"]
        claims = {
            "large_batch_B65536_f64_frac": lb["B65536"]["hbm_frac"],
            "large_batch_B131072_f64_frac": lb["B131072"]["hbm_frac"],
            "f32_B65536_frac": extra["B65536_f32"]["hbm_frac"],
            "quad12_frac": extra["config5_quad12_B65536_f64"]["hbm_frac"],
            "quad12_Mits": extra["config5_quad12_B65536_f64"]["iterations_per_s"] / 1e6,
            "quad12_f32_frac": extra["config5_quad12_B65536_f32"]["hbm_frac"],
            # per-rank cost of the sharded step beside the unsharded one (one process, one GPU)
            "sharded_step_ms": so["forms"]["sharded_one_call"]["step_ms"],
            "unsharded_step_ms": so["forms"]["unsharded"]["step_ms"],
            "sharded_host_enqueue_ms": so["forms"]["sharded_one_call"]["host_enqueue_ms"],
            "sharded_over_unsharded": so["sharded_over_unsharded"],
            "sharded_over_unsharded_B131072": extra["sharded_overhead_B131072"]["sharded_over_unsharded"],
            # the reference's own metric through the product: control-step latency on configs[0]
            "control_step_ms": extra["config1_closed_loop"]["chained"]["control_step_ms_mean"],
            "control_step_ms_device_rounds":
                extra["config1_closed_loop"]["device_rounds"]["control_step_ms_mean"],
            "solve_B65536_ms": out["roofline_solve"]["ms_per_solve"],
            "solve_B1024_ms": extra["solve_to_termination_B1024_f64"]["ms_per_solve"],
            "solve_frac_of_fixed_count_rate": out["roofline_solve"]["frac_of_fixed_count_rate"]}
        # the curve VERDICT r4 #4 asked to be monotone from 8192 to 32768 problems (M it/s)
        for b in (4096, 8192, 12288, 16384, 24576, 32768):
            claims[f"mid_{b}_Mits"] = round(extra[f"B{b}_f64"]["iterations_per_s"] / 1e6, 1)
        rf, head = out["roofline"], {}
        for k, v in rf.items():
            head[k] = v
            if k == "frac":
                head.update(claims)
        out["roofline"] = head
    if rank == 0:
        import ctypes
        ctypes.CDLL(None).fflush(None)  # (anything a library left in the C stdout buffer goes first)
        print(result_line(out), flush=True)
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
        if dist_mod.abandoned_bring_ups():
            # a thread of this rank is still inside an ncclCommInitRank that never returned: the
            # regular teardown (process group, library destructors) may wait for it
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(0)
        dist.destroy_process_group()
    return 0


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    sys.exit(run_rank(args))


if __name__ == "__main__":
    main()
