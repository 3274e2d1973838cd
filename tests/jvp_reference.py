"""Yardstick of btrapz_solve_jvp_device: the directional derivative of one candidate's QP from the oracle's dense
assembly -- the forward-mode mirror of tests/vjp_reference.py.

x*, y* from the oracle's exact solver and the active set from y* (vjp_reference.Adjoint: the same rule and margin);
dP, dq, dl, du the central differences of the ASSEMBLY along the direction (exact to rounding where the assembly is
linear in the inputs, which it is except at the cuboid variant's max / min); the tangent KKT system
    [ P  A_act' ] [dx ]   [-(dP x + dq)]
    [ A_act  0  ] [dmu] = [   db_act   ]
by least squares; dcost = (P x + q)' dx + x' dP x / 2 + dq' x.

The assembly is linear or bilinear in every input that P and q see, so a central difference of them is exact for any
step and only its rounding, 1e-16 |P| / step, matters.  That rounding is multiplied by x in dP x, and the s axis'
control points reach 1e2 where dP x itself is of order 1: with a step of 1e-4 it alone moved dx by 1.2e-4 of its norm
along weight directions at 64 segments (and by 5e-4 at 1e-6); it falls in proportion to the step (1.9e-5 at 1e-3, 1.2e-6
at 1e-2, 1e-7 at 1e-1, measured against the same GPU result).  So P and q are differenced with H_PQ = 1e-2 times the
direction -- the smallest weight of the test families, 0.12, stays positive under a standard normal direction -- while
the bounds l, u, which have kinks (the cuboid's max / min, the far-bound threshold), keep the step h = 1e-4.
"""
import numpy as np

from spectral_amd import layout as L
from vjp_reference import Adjoint, PARAM_NAMES, dense, one, shared_with

KEYS = ("seg", "init", "ref_end", "dl_bounds", "shared")
H_PQ = 1e-2   # the difference step of P and q (module docstring)


def zero_direction(S):
    return dict(seg=np.zeros((L.NUM_SEG_FIELDS, S)), init=np.zeros(6), ref_end=np.zeros(2), dl_bounds=np.zeros(10),
                shared=np.zeros(20))


def random_direction(rng, S, keys=KEYS):
    """A dense random direction in the named arrays (field 0 of seg, the durations, stays 0)."""
    d = zero_direction(S)
    for k in keys:
        d[k] = rng.standard_normal(d[k].shape)
    d["seg"][L.F_T] = 0.0
    return d


def moved(batch, sh, direction, h):
    """(batch, shared) of a one-candidate batch moved by h times the direction."""
    bt = one(batch, 0)
    bt.seg[:, 0, :] += h * direction["seg"]
    bt.init[0] += h * direction["init"]
    bt.ref_end[0] += h * direction["ref_end"]
    bt.dl_bounds[0] += h * direction["dl_bounds"]
    for j in range(len(PARAM_NAMES)):
        if direction["shared"][j] != 0.0:
            sh = shared_with(sh, j, h * direction["shared"][j])
    return bt, sh


class Tangent:
    """The tangent solution of candidate 0 of a one-candidate batch along a direction."""

    def __init__(self, batch, sh, direction, h=1e-4, adj=None, h_pq=H_PQ):
        adj = adj if adj is not None else Adjoint(batch, sh, np.zeros(12 * batch.S), 0.0)
        self.adj, self.strict = adj, adj.strict
        P, A, q, x = adj.P, adj.A, adj.q, adj.x
        _, _, _, _, lp, up = dense(*moved(batch, sh, direction, h))
        _, _, _, _, lm, um = dense(*moved(batch, sh, direction, -h))
        _, Pp, _, qp_, _, _ = dense(*moved(batch, sh, direction, h_pq))
        _, Pm, _, qm, _, _ = dense(*moved(batch, sh, direction, -h_pq))
        fin = lambda a, b_: np.where((np.abs(a) < 1e9) & (np.abs(b_) < 1e9), a - b_, 0.0)
        dP, dq, dl, du = (Pp - Pm) / (2 * h_pq), (qp_ - qm) / (2 * h_pq), fin(lp, lm) / (2 * h), fin(up, um) / (2 * h)
        db = np.where(adj.lower | ((adj.u - adj.l) <= 1e-12), dl, du)
        act = adj.act
        Aa = A[act]
        n, ma = P.shape[0], Aa.shape[0]
        K = np.zeros((n + ma, n + ma))
        K[:n, :n] = P; K[:n, n:] = Aa.T; K[n:, :n] = Aa
        sol = np.linalg.lstsq(K, np.concatenate([-(dP @ x + dq), db[act]]), rcond=None)[0]
        self.dx = sol[:n]
        self.dcost = float((P @ x + q) @ self.dx + 0.5 * x @ (dP @ x) + dq @ x)
        # the size of what dcost is summed from (its terms cancel): the scale a comparison of dcost is relative to
        self.dcost_scale = float(np.abs((P @ x + q) * self.dx).sum() + 0.5 * np.abs(x * (dP @ x)).sum() + np.abs(dq * x).sum())
        # the active rows' targets must be consistent where the rows are dependent (a joint stated twice): else no tangent
        self.consistent = bool(np.abs(Aa @ self.dx - db[act]).max() <= 1e-7 * max(1.0, np.abs(db[act]).max())) if ma else True


def reference_jvp(batch, sh, b, direction, h=1e-4):
    """(dx [12 S], dcost, Tangent) of candidate b of a batch along a direction (dict of seg [17][S], init [6], ref_end [2],
    dl_bounds [10], shared [20])."""
    t = Tangent(one(batch, b), sh, direction, h)
    return t.dx, t.dcost, t
