"""Host-only reference of a chain of dependent solves ("wave_chain", include/i2lqr.h) and the
problem sets its tests share (test_wave_chain_host.py shows them to depend on the carry and to be
well conditioned under it; test_gpu_wave_chain.py runs them on k_chain_box).

Composed, not new arithmetic: a chain is state_box_reference.box_reference run once per chain
step on the step's problems, to termination, with lamb set to what the previous step returned
(utils/base.py:393, :414-426: `lamb` is reset per lap and carried through the candidate loop)."""
from __future__ import annotations

import numpy as np

import multi_obstacle_reference as mo
import state_box_reference as sb

OUT_KEYS = ("X", "U", "lamb", "cost", "iters", "status")


def step_index(chains, chain_len, c):
    """Problems of chain step c: problem c of chain a sits at a * chain_len + c."""
    return np.arange(chains) * chain_len + c


def step_batch(host, idx, lamb=None):
    """The problems idx of a host batch, with `lamb` in place of theirs if given."""
    out = {key: np.ascontiguousarray(np.asarray(host[key])[idx]) for key in ("X", "U", "x_term", "lamb")}
    out["obs"] = None if host.get("obs") is None else np.ascontiguousarray(np.asarray(host["obs"])[idx])
    if lamb is not None:
        out["lamb"] = np.array(lamb, dtype=np.float64)
    return out


def chain_reference(cfg, host, box, A, chains, chain_len):
    """box_reference on every chain step, the first with the host's own lamb, the others with the
    lamb the previous step returned.  host: chains * chain_len problems, chain after chain.
    Returns dict(X, U, lamb, cost, iters, status) of all of them."""
    B = chains * chain_len
    assert host["X"].shape[0] == B
    out, lamb = {}, None
    for c in range(chain_len):
        idx = step_index(chains, chain_len, c)
        ref = sb.box_reference(cfg, step_batch(host, idx, lamb), box, A, early_exit=True)
        lamb = ref["lamb"]
        for key in OUT_KEYS:
            if key not in out:
                out[key] = np.zeros((B,) + ref[key].shape[1:], ref[key].dtype)
            out[key][idx] = ref[key]
    return out


# name -> (problem set, boxed, chains, chain_len, line-search steps[, first problem]).  A boxed set is
# state_box_reference.CASES' (with its records where it has some); a plain one is
# ls_reference.CASES' with no opt-in model at all, the handle pinned to k_iterate
# ("group_lanes" 64, "per_step_jacobians" 0).  The first chains * chain_len problems of the set,
# chain after chain (from `first problem` on where the set's first ones are not well conditioned
# under the carried lamb: chosen on the CPU, test_wave_chain_host.py); a set that is too small is
# tiled.
SHAPES = {
    "b4_3x4": ("b4", True, 3, 4, 1),
    "b6_2x5": ("b6", True, 2, 5, 1),
    "b4_N1_2x3": ("b4_N1", True, 2, 3, 1),          # horizon 1
    "b4_N64_1x2": ("b4_N64", True, 1, 2, 1),        # the largest LDS
    "quad12_2x2": ("quad12", True, 2, 2, 1),
    "b4_weights_2x3": ("b4_weights", True, 2, 3, 1, 12),
    "b6_K2_A4_2x3": ("b6_K2", True, 2, 3, 4),       # two records and the line search
    "b6_1x1": ("b6", True, 1, 1, 1),
    "b4_5x1": ("b4", False, 5, 1, 1),               # chain_len 1, several chains; no opt-in model
    "b4_K2_3x4": ("b4_K2", True, 3, 4, 1),
    "b4_513x2": ("b4", False, 513, 2, 1),           # more chains than the speculative kernel takes
}
# what test_gpu_wave_chain.py compares with box_reference step by step
REFERENCE_SHAPES = ("b4_3x4", "b6_2x5", "b4_K2_3x4", "quad12_2x2")


def make_shape(name, dtype="f64"):
    """(cfg, host batch of chains * chain_len problems, Box or None, A, chains, chain_len)."""
    case, boxed, chains, chain_len, A = SHAPES[name][:5]
    first = SHAPES[name][5] if len(SHAPES[name]) > 5 else 0
    if boxed:
        cfg, host, box = sb.make_case(case, dtype)
    else:
        (cfg, host), box = mo.ls_case(case, dtype), None
    B, have = chains * chain_len, host["X"].shape[0]
    idx = (first + np.arange(B)) % have
    out = step_batch(host, idx)
    return cfg, out, box, A, chains, chain_len
