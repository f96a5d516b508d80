"""Host-only reference of the "barrier_cost" option (include/i2lqr.h) and what the tests of it
share (test_barrier_cost_host.py ties the penalty to the oracle's dumped barrier derivatives and the
loop to state_box_reference.box_reference; test_gpu_barrier_cost.py runs the sets on the kernel).

The reference's accept / reject cost does not contain the barriers (control/iterative_ilqr.py:43-48),
so there is no parity with it.  What pins the option: the penalty

    P(X, U) = sum_{t<N} sum_{a<m}  ctrl_q1 (e^{ctrl_q2 (u_t[a] - u_max[a])} + e^{ctrl_q2 (-u_max[a] - u_t[a])})
            + sum_{t<=N} sum_{records r, r[5] >= 0}  obs_q1 e^{obs_q2 h_r(x_t, t)}
            + sum_{t<=N} sum_{i bounded}  box.q1 (e_hi + e_lo)

is the function whose first derivatives the backward pass already uses (the oracle's dumped l_u,
l_x, V_x and state_box_reference.barrier_terms' d1), and the loop is box_reference's with the merit
J = c + P in the line search, the accept test and the convergence test (relative to the barrier-free
cost c of the nominal being replaced)."""
from __future__ import annotations

import numpy as np

import multi_obstacle_reference as mo
import state_box_reference as sb

MARGIN = 1e-7  # a problem is compared on the GPU only if its smallest deciding margin is at least this


def penalty(cfg, X, U, obs=None, box=None):
    """P[B] of X[B, n, N + 1], U[B, m, N] (the clipped inputs and their rollout), obs None, [B, 6] or
    [B, K, 6], box a state_box_reference.Box or None."""
    X, U = np.asarray(X, np.float64), np.asarray(U, np.float64)
    B, N, m = X.shape[0], cfg.N, cfg.m
    u_max = np.array(cfg.u_max[:m], dtype=np.float64).reshape(1, m, 1)
    with np.errstate(over="ignore"):
        P = (cfg.ctrl_q1 * (np.exp(cfg.ctrl_q2 * (U - u_max)) +
                            np.exp(cfg.ctrl_q2 * (-u_max - U)))).sum(axis=(1, 2))
        t = np.arange(N + 1)[None, :]
        for r in range(mo.records(obs, B).shape[1]):
            rec = mo.records(obs, B)[:, r, :]
            on = rec[:, 5] >= 0
            opt = np.where(on, rec[:, 5], 0).astype(int)[:, None]
            cx = np.where(opt == 2, rec[:, 0:1] - t * rec[:, 4:5], rec[:, 0:1])
            cy = np.where(opt == 1, rec[:, 1:2] + t * rec[:, 4:5], rec[:, 1:2])
            safe = np.where(on[:, None], rec[:, 2:4], 1.0)  # (a record that is off may hold zeros)
            dz, dy = X[:, 0, :] - cx, X[:, 1, :] - cy
            h = 1.0 + cfg.safety_margin - (dz * dz / safe[:, 0:1] ** 2 + dy * dy / safe[:, 1:2] ** 2)
            P = P + np.where(on, (cfg.obs_q1 * np.exp(cfg.obs_q2 * h)).sum(axis=1), 0.0)
        if box is not None and box.active:
            fin_hi, fin_lo = np.isfinite(box.hi)[None, :, None], np.isfinite(box.lo)[None, :, None]
            hi = np.where(np.isfinite(box.hi), box.hi, 0.0)[None, :, None]
            lo = np.where(np.isfinite(box.lo), box.lo, 0.0)[None, :, None]
            e_hi = np.where(fin_hi, np.exp(box.q2 * (X - hi)), 0.0)  # an unbounded side is masked
            e_lo = np.where(fin_lo, np.exp(box.q2 * (lo - X)), 0.0)
            P = P + (box.q1 * (e_hi + e_lo)).sum(axis=(1, 2))
    return P


def merit_reference(cfg, host, box=None, A=1, max_iter=None, early_exit=True, merit=True):
    """state_box_reference.box_reference's loop with the accept block of "barrier_cost": the winner
    is argmin_j J_j, accept iff J_new is finite and J_new < J, converged iff accepted and
    |(J_new - J) / c| < eps, cost = J of the returned trajectory.  merit=False: box_reference's loop,
    bit for bit.  Returns box_reference's dict and `margin`[B]: the smallest deciding margin met -
    |J_new - J| / |J|, | |(J_new - J) / c| - eps | / eps and, with A > 1, (J_second - J_best) /
    |J_best|, over the iterations whose J_new is finite (inf where none was)."""
    from oracle import oracle as orc
    RUNNING, CONVERGED, MAX_ITER, LAMB_OVERFLOW, NONFINITE = 0, 1, 2, 3, 4
    X = np.array(host["X"], dtype=np.float64)
    U = np.array(host["U"], dtype=np.float64)
    lamb = np.array(host["lamb"], dtype=np.float64)
    x_term = np.asarray(host["x_term"], dtype=np.float64)
    B = X.shape[0]
    obs = mo.records(host.get("obs"), B)
    max_iter = int(cfg.max_iter if max_iter is None else max_iter)
    K = np.zeros((B, cfg.m, cfg.n, cfg.N))
    k = np.zeros((B, cfg.m, cfg.N))
    status = np.full(B, MAX_ITER if early_exit else RUNNING, np.int32)
    iters = np.zeros(B, np.int32)
    cost_ret = np.zeros(B)
    margin = np.full(B, np.inf)
    live = np.ones(B, bool)
    pen = (lambda Xs, Us, sel: penalty(cfg, Xs, Us, obs[sel], box)) if merit else \
        (lambda Xs, Us, sel: 0.0)
    for it in range(max_iter):
        idx = np.flatnonzero(live)
        if idx.size == 0:
            break
        Xr, Ur, cost = orc.rollout_batch(cfg, X[idx], U[idx], x_term[idx])
        J = cost + pen(Xr, Ur, idx)
        kk, KK = sb.composed_backward(cfg, Xr, Ur, x_term[idx], lamb[idx], obs[idx], box)
        cand = [orc.forward_batch(cfg, Xr, Ur, x_term[idx], KK, kk * 0.5 ** j) for j in range(A)]
        Js = np.stack([c[2] + pen(c[0], c[1], idx) for c in cand])
        masked = np.where(np.isnan(Js), np.inf, Js)
        js = np.argmin(masked, axis=0)
        rows = np.arange(idx.size)
        J_new = Js[js, rows]
        Xn = np.stack([c[0] for c in cand])[js, rows]
        Un = np.stack([c[1] for c in cand])[js, rows]
        X[idx], U[idx], K[idx], k[idx] = Xr, Ur, KK, kk
        iters[idx] = it + 1
        acc = (np.isfinite(J_new) & (J_new < J)) if merit else (J_new < J)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.abs((J_new - J) / cost)
            conv = acc & (rel < cfg.eps)
            m_it = np.minimum(np.abs(J_new - J) / np.abs(J), np.abs(rel - cfg.eps) / cfg.eps)
            if A > 1:
                second = np.sort(masked, axis=0)[1]
                m_it = np.minimum(m_it, (second - J_new) / np.abs(J_new))
        m_it = np.where(np.isfinite(J_new) & ~np.isnan(m_it), m_it, np.inf)
        margin[idx] = np.minimum(margin[idx], m_it)
        a, r = idx[acc], idx[~acc]
        X[a], U[a] = Xn[acc], Un[acc]
        lamb[a] /= cfg.lamb_factor
        lamb[r] *= cfg.lamb_factor
        cost_ret[idx] = np.where(acc, J_new, J)
        over = ~acc & (lamb[idx] > cfg.max_lamb)
        for hit, word in ((conv, CONVERGED), (over, LAMB_OVERFLOW)):
            sel = idx[hit]
            if early_exit:
                status[sel] = word
                live[sel] = False
            else:
                status[sel] = np.where(status[sel] == RUNNING, word, status[sel])
    status[~np.isfinite(cost_ret)] = NONFINITE
    return dict(X=X, U=U, lamb=lamb, cost=cost_ret, iters=iters, status=status, K=K, k=k,
                margin=margin)


# (case of state_box_reference.CASES, fixed iterations or None for a solve to termination, step
# sizes): what test_gpu_barrier_cost.py compares with merit_reference.  The fixed counts are short on
# purpose: near the optimum J_new and J agree to round-off and the branch is not decidable.
GPU_RUNS = ([(case, 3, 1) for case in ("b4", "b4_hi_only", "b4_weights", "b6", "quad12", "b4_N7",
                                       "b4_N64", "b6_B1", "b6_B5", "b4_K2")] +
            [("b6_K2", 3, 4)] +
            [(case, 2, 1) for case in ("b4_N1", "b6_N1")] +
            [("b4", None, 1), ("b6", None, 1), ("b4_K2", None, 1), ("b6_K2", None, 4)])
TERMINATION_RUNS = [run for run in GPU_RUNS if run[1] is None]
# the share of a run's problems the conditioning rule may leave out
MAX_LEFT_OUT = {True: 0.20, False: 0.0}  # keyed by "to termination"

make_case = sb.make_case


class MeritCandidateSolver:
    """HipCandidateSolver(barrier_cost=True)'s solve() on the host: merit_reference behind the
    controller (independent candidates; the controller's own loop chains lamb)."""

    def __init__(self, box=None):
        self.box = box

    def solve(self, cfg, x0, x_terms, lamb0, obs_rec, U0=None):
        x_terms = np.atleast_2d(np.asarray(x_terms, float))
        B = x_terms.shape[0]
        X = np.zeros((B, cfg.n, cfg.N + 1))
        X[:, :, 0] = np.asarray(x0, float)
        U = np.zeros((B, cfg.m, cfg.N)) if U0 is None else np.asarray(U0, float).reshape(B, cfg.m, cfg.N)
        obs = None
        if obs_rec is not None:
            rec = np.asarray(obs_rec, float)
            obs = np.broadcast_to(rec, (B,) + rec.shape)
        out = merit_reference(cfg, dict(X=X, U=U, x_term=x_terms,
                                        lamb=np.asarray(lamb0, float).reshape(B), obs=obs), self.box)
        out.pop("margin")
        return out


GOLDEN_LAPS = "barrier_cost_laps.npz"  # tests/golden/: written by `python barrier_cost_reference.py`


def golden_laps():
    """The closed loop with the barrier cost on the host (MeritCandidateSolver), config 1 with the
    static obstacle, three controlled laps: dict(steps, top: without a box; steps_box, top_box: with
    the speed limit of state_box_reference)."""
    from pathlib import Path
    return dict(np.load(Path(__file__).resolve().parent / "golden" / GOLDEN_LAPS))


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    steps, ego = sb.controlled_laps(MeritCandidateSolver())
    steps_box, ego_box = sb.controlled_laps(MeritCandidateSolver(sb.speed_limit_box()))
    out = Path(__file__).resolve().parent / "golden" / GOLDEN_LAPS
    np.savez(out, steps=np.array(steps), top=np.array(sb.top_speeds(ego)),
             steps_box=np.array(steps_box), top_box=np.array(sb.top_speeds(ego_box)))
    print(out, steps, sb.top_speeds(ego), steps_box, sb.top_speeds(ego_box))
