#!/usr/bin/env python3
"""The host code BEHIND a live handle under AddressSanitizer + UBSan:
drives the dry-run form of the ASan build of the library (csrc/i2lqr_dryrun.hpp: I2LQR_DRY_RUN=1 —
i2lqr_create skips the device, every kernel launch becomes a record whose pointer arguments must
lie inside a declared range) through random configurations: plant x horizon x precision x layout x
batch x scheduling options x entry point (rollout / backward / forward / iterate / solve /
iterate_pick / sharded round).  The caller's arrays and the workspace are FAKE address ranges of
exactly the sizes the layout prescribes; a carved or derived pointer that leaves them is a
violation, an out-of-bounds host access or undefined behaviour is the sanitizers' report.

    tools/run_host_sanitizers.sh            (builds the ASan library, preloads the runtime)
    python tools/dry_run_fuzz.py --configs 1000"""
import argparse
import ctypes as C
import os
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
os.environ["I2LQR_DRY_RUN"] = "1"
import numpy as np

from ilqr_iterative_tasks_amd import _abi

ap = argparse.ArgumentParser()
ap.add_argument("--configs", type=int, default=1000)
ap.add_argument("--seed", type=int, default=20260406)
ap.add_argument("--verbose", action="store_true")
ap.add_argument("--trace", metavar="FILE",
                help="write every launch record (instantiation, shape, arguments), every refusal's "
                     "text and the kernels every handle reports to FILE: two builds of the library "
                     "that enqueue the same launches and say the same write identical files")
args = ap.parse_args()

lib = _abi.load_library()
P = C.c_void_p
assert lib.i2lqr_dry_run(0, None, 0) == 1, \
    "this library has no dry-run form (needs the ASan build and I2LQR_DRY_RUN=1): " + \
    lib.i2lqr_last_error().decode()

rng = np.random.default_rng(args.seed)
STREAM = P(0x1000)
SIDE = P(0x2000)
OPTIONS = {"defer_states": (0, 1), "reroll_nominal": (0, 1), "lds_gain_steps": (0, 1, 3, 7, 19, 40),
           "merge_inputs": (0, 1), "checkpoint_states": (0, 1), "stagger": (0, 8, 45),
           "per_step_jacobians": (0, 1), "wave_tail": (0, 512, 2048, 12288, 65536),
           "first_chunk": (1, 4, 8, 12, 150), "helper_wavefront": (0, 1), "state_buffers": (0, 1),
           "chunk_step": (1, 2, 4, 9), "speculate": (0, 1), "group_workspace": (0, 1),
           "group_lanes": (8, 16, 64), "fused_compaction": (0, 1), "final_round": (0, 1, 2, 3, 5),
           "line_search": (0, 2, 4, 8), "obstacles": (0, 2, 3, 8), "group_overlap": (0, 1),
           "group_fixed_horizon": (0, 1), "wave_chain": (0, 1), "group_chains": (0, 1)}


class Arena:
    """Fake device addresses: every array gets its own range, declared to the library."""

    def __init__(self):
        self.next = 0x7000_0000_0000

    def take(self, nbytes):
        base = self.next
        self.next += (int(nbytes) + 0xFFFF) // 0x10000 * 0x10000 + 0x10000  # a gap behind each
        if nbytes > 0:
            assert lib.i2lqr_dry_run(1, P(base), int(nbytes)) == 0
        return P(base) if nbytes > 0 else P(None)


trace = open(args.trace, "w") if args.trace else None


def note(line):
    """A line of the trace that is no launch: a refusal's text, the kernels a handle reports."""
    if trace:
        trace.write(f"# {line}\n")


def report(label=""):
    # (the library keeps up to 2 MiB of records between two reports: the trace takes all of them)
    buf = C.create_string_buffer(1 << 22 if trace else 1 << 16)
    bad = lib.i2lqr_dry_run(3, buf, len(buf))
    text = buf.value.decode(errors="replace")
    if trace:
        trace.write(f"# {label}\n{text}")
    return int(bad), text


FIELD = re.compile(r" ([A-Za-z_][A-Za-z_.]*)=(\S+)")


def records(text):
    """Launch records of a report -> [(kernel, {field: value})]; pointers stay strings."""
    out = []
    for line in text.splitlines():
        if not line.startswith("launch ") or " grid " not in line:
            continue
        kernel, rest = line[7:].split(" grid ", 1)
        out.append((kernel, {k: (int(v) if re.fullmatch(r"-?\d+", v) else v)
                             for k, v in FIELD.findall(" grid " + rest)}))
    return out


def schedule_gap(text):
    """The chunked solve must leave no survivor behind: the lane chunks of a solve (LaneArgs with
    early_exit; the helper-wavefront and plain kernel of one round, enqueued as a pair, count once)
    sum to max_iter, or the last chunk or tail launch is a tail kernel (IterArgs with a live count)
    that takes every problem (count_max == B) to max_iter.  Returns a description of the gap, or
    None (also for calls without a lane solve)."""
    chunks, last, prev = 0, None, None
    total = None
    for kernel, f in records(text):
        if f.get("LaneArgs.early_exit") == 1:
            if total is None:
                total = f["LaneArgs.max_total"]
            partner = (prev is not None and f["LaneArgs.count_lo"] >= 0
                       and prev.get("LaneArgs.count_hi") == f["LaneArgs.count_lo"]
                       and prev.get("LaneArgs.n_iters") == f["LaneArgs.n_iters"])
            if not partner:
                chunks += f["LaneArgs.n_iters"]
            last = ("chunk", f)
        elif total is not None and f.get("IterArgs.count", 0) != 0 and \
                f.get("IterArgs.early_exit") == 1:
            last = ("tail", f)
        prev = f
    if total is None or chunks == total:
        return None
    if last[0] == "tail" and last[1]["IterArgs.count_max"] == last[1]["IterArgs.B"] and \
            last[1]["IterArgs.max_total"] == total:
        return None
    what = "a lane chunk" if last[0] == "chunk" else \
        f"a tail kernel with count_max {last[1]['IterArgs.count_max']}"
    return (f"the lane chunks run {chunks} of {total} iterations and the last launch is {what}: "
            "survivors are left unsolved")


def solve_records(options, B=8192, max_iter=150):
    """The records of one i2lqr_solve on a batch-tiled bicycle6 handle with `options`."""
    assert lib.i2lqr_dry_run(2, None, 0) == 0
    cfg = _abi.default_config("bicycle6", 20, "f64", dt=0.25, layout=2)
    cfg.max_iter = max_iter
    h = P()
    assert lib.i2lqr_create(C.byref(cfg), C.byref(h)) == 0, lib.i2lqr_last_error()
    for name, v in options.items():
        assert lib.i2lqr_set_option(h, name.encode(), v) == 0
    arena = Arena()
    X, U = arena.take(B * 6 * 21 * 8), arena.take(B * 2 * 20 * 8)
    xt, lamb, cost = arena.take(B * 6 * 8), arena.take(B * 8), arena.take(B * 8)
    wsb = int(lib.i2lqr_workspace_bytes(h, B))
    assert lib.i2lqr_set_workspace(h, arena.take(wsb), wsb) == 0
    assert lib.i2lqr_solve(h, B, X, U, xt, lamb, None, cost, None, None, None, None, STREAM) == 0, \
        lib.i2lqr_last_error()
    bad, text = report(f"schedule {options} B={B} max_iter={max_iter}")
    assert bad == 0, text[:400]
    assert lib.i2lqr_destroy(h) == 0
    return text


# The checker must be live: a workspace DECLARED at half the size the library carves it to has to
# come back as violations (the second work set of the chunked solve lies behind the declared half).
cfg = _abi.default_config("bicycle6", 20, "f64", dt=0.25, layout=2)
h = P()
assert lib.i2lqr_create(C.byref(cfg), C.byref(h)) == 0, lib.i2lqr_last_error()
B0 = 8192
wsb = int(lib.i2lqr_workspace_bytes(h, B0))
base = 0x6000_0000_0000
assert lib.i2lqr_dry_run(1, P(base), wsb // 2) == 0
assert lib.i2lqr_set_workspace(h, P(base), wsb) == 0
arrs = []
for nbytes in (B0 * 6 * 21 * 8, B0 * 2 * 20 * 8, B0 * 6 * 8, B0 * 8, B0 * 8):
    a = 0x6800_0000_0000 + len(arrs) * 0x1000_0000
    assert lib.i2lqr_dry_run(1, P(a), nbytes) == 0
    arrs.append(P(a))
assert lib.i2lqr_solve(h, B0, arrs[0], arrs[1], arrs[2], arrs[3], None, arrs[4], None, None, None, None,
                       STREAM) == 0, lib.i2lqr_last_error()
bad, text = report("self-check")
assert bad > 0 and "VIOLATION" in text and "LaneArgs" in text, (bad, text[:400])
assert lib.i2lqr_destroy(h) == 0
print(f"self-check: a workspace declared at half its size is reported ({bad} violations, e.g. "
      f"{text.splitlines()[0][:110]})")



def padding_records(system, dtype, B, pad):
    """The records of i2lqr_iterate and i2lqr_solve on a batch-minor handle; pad: a non-zero Q
    entry outside the plant's n x n block, which no kernel reads."""
    assert lib.i2lqr_dry_run(2, None, 0) == 0
    cfg = _abi.default_config(system, 20, dtype, dt=0.25, layout=1)
    if pad:
        cfg.Q[_abi.MAX_N * _abi.MAX_N - 1] = 1.0
    h = P()
    assert lib.i2lqr_create(C.byref(cfg), C.byref(h)) == 0, lib.i2lqr_last_error()
    item, n, m, N = (8 if dtype == "f64" else 4), cfg.n, cfg.m, cfg.N
    arena = Arena()
    X, U = arena.take(B * n * (N + 1) * item), arena.take(B * m * N * item)
    xt, lamb, cost = arena.take(B * n * item), arena.take(B * item), arena.take(B * item)
    wsb = int(lib.i2lqr_workspace_bytes(h, B))
    assert lib.i2lqr_set_workspace(h, arena.take(wsb), wsb) == 0
    assert lib.i2lqr_iterate(h, B, 5, X, U, xt, lamb, None, cost, None, None, None, None, STREAM) == 0, \
        lib.i2lqr_last_error()
    assert lib.i2lqr_solve(h, B, X, U, xt, lamb, None, cost, None, None, None, None, STREAM) == 0, \
        lib.i2lqr_last_error()
    bad, text = report(f"padding {system} {dtype} B={B} pad={pad}")
    assert bad == 0 and text.count("launch ") >= 2, text[:400]
    assert lib.i2lqr_destroy(h) == 0
    return text


# Stage weights are read from the n x n / m x m blocks only (has_stage_weights): a non-zero entry
# in the padding of Q changes no launch — fp64 at 65536 problems keeps its state checkpoints.
for system, dtype in (("bicycle6", "f64"), ("bicycle4", "f32")):
    plain = padding_records(system, dtype, 65536, False)
    assert padding_records(system, dtype, 65536, True) == plain
    assert dtype != "f64" or "LaneArgs.ckpt=1" in plain, plain[:400]
print("self-check: a non-zero entry in the padding of Q changes no launch")

# Every survivor of the chunked solve is covered: the automatic schedule, and the schedules whose
# final round comes before the tail kernel may run (4 iterations)
for opts in ({}, {"first_chunk": 2, "final_round": 1},
             {"first_chunk": 1, "chunk_step": 1, "final_round": 2},
             {"first_chunk": 3, "final_round": 1, "fused_compaction": 0}):
    gap = schedule_gap(solve_records(opts))
    assert gap is None, f"chunked solve with {opts}: {gap}"
print("self-check: the chunked solve's schedules cover every survivor (automatic; final round "
      "before 4 iterations)")



def column_case(system, options, B, entry, workspace=True, chain_len=1, N=20, dtype="f64"):
    """One call on a problem-major handle, its records and words in the trace: `entry` is
    "iterate", "solve" or "chained" (B chains of chain_len problems)."""
    assert lib.i2lqr_dry_run(2, None, 0) == 0
    cfg = _abi.default_config(system, N, dtype, dt=0.25, layout=0)
    h = P()
    assert lib.i2lqr_create(C.byref(cfg), C.byref(h)) == 0, lib.i2lqr_last_error()
    for name, v in options.items():
        assert lib.i2lqr_set_option(h, name.encode(), v) == 0, lib.i2lqr_last_error()
    item, n, m, P_ = (8 if dtype == "f64" else 4), cfg.n, cfg.m, B * chain_len
    arena = Arena()
    X, U = arena.take(P_ * n * (N + 1) * item), arena.take(P_ * m * N * item)
    xt, lamb, cost = arena.take(P_ * n * item), arena.take(P_ * item), arena.take(P_ * item)
    obs = arena.take(P_ * max(options.get("obstacles", 1), 1) * 6 * item)
    wsb = int(lib.i2lqr_workspace_bytes(h, B)) if workspace else 0
    if wsb > 0:
        assert lib.i2lqr_set_workspace(h, arena.take(wsb), wsb) == 0
    tail = (X, U, xt, lamb, obs, cost, None, None, None, None, STREAM)
    rc = {"iterate": lambda: lib.i2lqr_iterate(h, B, 5, *tail), "solve": lambda: lib.i2lqr_solve(h, B, *tail),
          "chained": lambda: lib.i2lqr_solve_chained(h, B, chain_len, *tail)}[entry]()
    why = "" if rc == 0 else ": " + lib.i2lqr_last_error().decode()
    bad, text = report(f"column case {system} N={N} {dtype} {options} B={B} {entry} workspace {wsb} rc {rc}{why}")
    assert bad == 0, text[:400]
    note(f"iterate on {lib.i2lqr_iterate_kernel(h, B).decode()}, solve on {lib.i2lqr_solve_kernel(h, B).decode()}")
    assert lib.i2lqr_destroy(h) == 0
    return rc, text


# Every kernel, wavefront count and form the problem-major launcher chooses between, once each (the
# random configurations below reach most of them, not reliably all)
for opts in ({}, {"group_fixed_horizon": 0}, {"group_overlap": 0}, {"group_chains": 0}):
    for B0 in (1024, 1025, 2048, 2049):  # sixteen-lane kernel: 3 / 2 / 1 wavefronts, both forms
        assert column_case("bicycle6", opts, B0, "iterate")[0] == 0
for B0, ws in ((2048, True), (2049, True), (4161, True), (4161, False)):  # eight-lane: 3 / 1, workspace form
    assert column_case("bicycle4", {"group_lanes": 8}, B0, "iterate", workspace=ws, dtype="f32")[0] == 0
for opts in ({}, {"group_lanes": 8, "speculate": 1}):  # speculative kernel: 3 / 2 wavefronts, sixteen and eight lanes
    for B0 in (512, 513):
        assert column_case("bicycle6", opts, B0, "solve")[0] == 0
assert column_case("bicycle6", {"group_workspace": 1}, 4161, "iterate", workspace=False)[0] != 0
for opts in ({"group_lanes": 64}, {"group_lanes": 64, "per_step_jacobians": 0}, {"line_search": 4},
             {"line_search": 4, "group_lanes": 16}):
    column_case("bicycle6", opts, 64, "iterate")
for ws in (True, False):  # quad12: the sixteen-lane kernel with its workspace, else one problem per wavefront
    assert column_case("quad12", {}, 64, "iterate", workspace=ws)[0] == 0
for opts, B0 in (({}, 512), ({}, 513), ({"wave_chain": 1}, 513), ({"wave_chain": 1, "obstacles": 2}, 8)):
    column_case("bicycle6", opts, B0, "chained", chain_len=2)
assert column_case("quad12", {}, 8, "chained", chain_len=2)[0] != 0
print("column cases: every kernel, wavefront count and chain form of the problem-major launcher recorded")

stats = {"configs": 0, "calls": 0, "ok": 0, "refused": 0, "launches": 0, "schedules": 0}
for it in range(args.configs):
    system = rng.choice(["bicycle4", "bicycle6", "quad12"], p=[0.35, 0.45, 0.2])
    N = int(rng.choice([2, 3, 6, 10, 20, 31, 50, 64]))
    dtype = rng.choice(["f64", "f32"])
    layout = int(rng.choice([0, 1, 2]))
    cfg = _abi.default_config(system, N, dtype, dt=0.25, layout=layout)
    if rng.random() < 0.2:
        cfg.set_matrix("R", np.eye(cfg.m) * 0.1)
    if rng.random() < 0.1:
        cfg.set_matrix("Q", np.eye(cfg.n) * 0.05)
    cfg.max_iter = int(rng.choice([1, 4, 8, 17, 150]))
    B = int(rng.choice([1, 3, 64, 200, 1024, 2048, 4096, 5000, 8192, 12288, 16384, 20000, 32768, 65536, 200000]))
    if layout == 2:
        B = max(64, B // 64 * 64)
    assert lib.i2lqr_dry_run(2, None, 0) == 0  # reset ranges and records
    h = P()
    rc = lib.i2lqr_create(C.byref(cfg), C.byref(h))
    stats["configs"] += 1
    if rc != 0:
        stats["refused"] += 1
        note(f"configuration {it} create rc {rc}: {lib.i2lqr_last_error().decode()}")
        continue
    n_obs = 1  # records per problem: obs[B][n_obs][6] once "obstacles" is accepted
    accepted = {}
    for name in rng.choice(list(OPTIONS), size=int(rng.integers(0, 5)), replace=False):
        value = int(rng.choice(OPTIONS[name]))
        if lib.i2lqr_set_option(h, name.encode(), value) == 0:
            accepted[str(name)] = value
            if name == "obstacles":
                n_obs = max(value, 1)
    note(f"configuration {it}: {system} N={N} {dtype} layout={layout} B={B} max_iter={cfg.max_iter} "
         f"options {accepted}")
    if rng.random() < 0.2:
        lib.i2lqr_set_compaction(h, int(rng.choice([0, 64, 4096])))
    item = 8 if dtype == "f64" else 4
    n, m = cfg.n, cfg.m
    arena = Arena()
    X, U = arena.take(B * n * (N + 1) * item), arena.take(B * m * N * item)
    xt, lamb, obs = arena.take(B * n * item), arena.take(B * item), arena.take(B * n_obs * 6 * item)
    cost, K, k = arena.take(B * item), arena.take(B * m * n * N * item), arena.take(B * m * N * item)
    iters, status = arena.take(B * 4), arena.take(B * 4)
    X2, U2, c2 = arena.take(B * n * (N + 1) * item), arena.take(B * m * N * item), arena.take(B * item)
    qfun, cost_it = arena.take(B * 4), arena.take(B * item)
    best_idx, best_cost = arena.take(8), arena.take(item)
    pick_bytes = int(lib.i2lqr_argmin_workspace_bytes(B))
    pick_ws = arena.take(pick_bytes)
    want_gains = rng.random() < 0.5
    Kp, kp = (K, k) if want_gains else (P(None), P(None))
    obs_p = obs if rng.random() < 0.8 else P(None)
    if rng.random() < 0.9:  # the workspace the handle asks for (sometimes none: calls must refuse)
        wsb = int(lib.i2lqr_workspace_bytes(h, B))
        if wsb > 0:
            ws = arena.take(wsb)
            assert lib.i2lqr_set_workspace(h, ws, wsb) == 0
    calls = [
        lambda: lib.i2lqr_rollout(h, B, X, U, xt, cost, STREAM),
        lambda: lib.i2lqr_backward(h, B, X, U, xt, lamb, obs_p, K, k, STREAM),
        lambda: lib.i2lqr_forward(h, B, X, U, xt, K, k, X2, U2, c2, STREAM),
        lambda: lib.i2lqr_iterate(h, B, int(rng.integers(0, 12)), X, U, xt, lamb, obs_p, cost, Kp, kp,
                                  iters, status, STREAM),
        lambda: lib.i2lqr_solve(h, B, X, U, xt, lamb, obs_p, cost, Kp, kp, iters, status, STREAM),
        lambda: lib.i2lqr_iterate_pick(h, B, int(rng.integers(0, 12)), X, U, xt, lamb, obs_p, cost, Kp,
                                       kp, iters, status, qfun, 0, 55, cost_it, best_idx, best_cost,
                                       pick_ws, pick_bytes, STREAM),
        lambda: lib.i2lqr_relax_cost(h, B, X, xt, qfun, 0, 55, cost_it, STREAM),
        lambda: lib.i2lqr_argmin(h, B, cost_it, best_idx, best_cost, pick_ws, pick_bytes, STREAM),
        lambda: lib.i2lqr_pack_problem(h, B, X, U, best_idx, arena.take((m * N + n * (N + 1)) * item), STREAM),
    ]
    for k_chain in (1, 2, 4, 8):  # chains: B problems as B / k chains of k (where k divides B)
        if B % k_chain == 0 and B // k_chain <= 4096:
            calls.append(lambda k_chain=k_chain: lib.i2lqr_solve_chained(
                h, B // k_chain, k_chain, X, U, xt, lamb, obs_p, cost, Kp, kp, iters, status, STREAM))
            break

    def sharded():
        world = int(rng.choice([1, 2, 3, 8]))
        rank = int(rng.integers(0, world))
        base = int(rng.integers(0, 3))
        total = B * world + (int(rng.integers(0, world)) if base == 0 else 0)
        lo = rank * (total // world) + min(rank, total % world)
        mine = total // world + (1 if rank < total % world else 0)
        if mine != B:  # keep this rank's shard at B: choose a total that gives it exactly B
            total = B * world
        width = (total + world - 1) // world
        PK = m * N + n * (N + 1)
        r = _abi.I2lqrRound()
        r.struct_size = C.sizeof(r)
        r.n_iters = int(rng.choice([-1, 0, 3, 10]))
        r.B, r.total, r.world, r.rank = B, total, world, rank
        r.outer_iter, r.max_relax_iter, r.guard_previous = 0, 55, int(rng.integers(0, 2))
        r.loopback = 1 if world > 1 else int(rng.integers(0, 2))
        r.X, r.U, r.x_term, r.lamb, r.obs, r.cost = X.value, U.value, xt.value, lamb.value, obs_p.value, cost.value
        r.K, r.k, r.iters, r.status, r.qfun = Kp.value, kp.value, iters.value, status.value, qfun.value
        r.cost_it, r.local_best, r.local_best_cost = cost_it.value, best_idx.value, best_cost.value
        r.pick_ws, r.pick_ws_bytes = pick_ws.value, pick_bytes
        r.pack_local = arena.take(PK * item).value
        r.cost_padded = arena.take(width * item).value
        r.cost_all = arena.take(world * width * item).value
        r.pack_all = arena.take(world * PK * item).value
        sb = int(lib.i2lqr_argmin_workspace_bytes(world * width)) + 16
        r.side_ws, r.side_ws_bytes = arena.take(sb).value, sb
        r.best_cost, r.winner, r.best_global = arena.take(item).value, arena.take(PK * item).value, arena.take(16).value
        return lib.i2lqr_sharded_round_flat(h, None, C.byref(r), SIDE if rng.random() < 0.5 else P(None), STREAM)

    calls.append(sharded)
    for ci in rng.choice(len(calls), size=4, replace=False):
        rc = calls[ci]()
        stats["calls"] += 1
        stats["ok" if rc == 0 else "refused"] += 1
        why = "" if rc == 0 else ": " + lib.i2lqr_last_error().decode()  # (the refusal's text)
        bad, text = report(f"configuration {it} call {ci} rc {rc}{why}")
        if bad:
            print(f"VIOLATION in configuration {it}: {system} N={N} {dtype} layout={layout} B={B} "
                  f"call {ci} rc={rc}\n{text}")
            sys.exit(1)
        gap = schedule_gap(text) if rc == 0 else None
        if gap:
            print(f"SCHEDULE GAP in configuration {it}: {system} N={N} {dtype} layout={layout} "
                  f"B={B} call {ci}: {gap}\n{text}")
            sys.exit(1)
        stats["schedules"] += text.count("LaneArgs.early_exit=1") > 0
        stats["launches"] += text.count("\n")
        if args.verbose:
            print(it, system, N, dtype, layout, B, "call", ci, "rc", rc, lib.i2lqr_last_error().decode()[:80])
    names = lib.i2lqr_iterate_kernel(h, B), lib.i2lqr_solve_kernel(h, B)
    assert None not in names
    note(f"configuration {it} iterate on {names[0].decode()}, solve on {names[1].decode()}")
    assert lib.i2lqr_destroy(h) == 0
if trace:
    trace.close()
print(f"dry-run fuzz: {stats['configs']} configurations, {stats['calls']} calls ({stats['ok']} enqueued, "
      f"{stats['refused']} refused with an error code), {stats['launches']} recorded launches, "
      f"0 pointer-range violations, {stats['schedules']} lane solves whose schedule covers every "
      "survivor")
