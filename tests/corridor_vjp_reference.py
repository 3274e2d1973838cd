"""Yardstick of the corridor stage's backward pass (btrapz_corridor_batch_vjp_device, btrapz_corridor_vjp_host).

The record of one candidate is built from the ORACLE's corridor (helpers.oracle_corridor) by restating in numpy what the
stage adds to the cubes: the ds walk over the final span, the x / y lines of every second, ref_end and the ten dl bounds.
Its Jacobian comes from central differences of that record, one input entry at a time, h = 1e-6; the reference gradient is
J^T applied to a cotangent.  The map is piecewise linear, so the only error of a column is rounding, and the tolerance of
entry c is computed, not tuned:  4 * sum_r |ybar_r| * 4 ulp(|y_r|) / (2 h)  (4 ulp for each of the two evaluations' own
arithmetic, times 4 for the summation of the product).  A column is SKIPPED when +-h changes a decision: seg_count, any
(beg_t, end_t), or which knot attains a ds extreme."""
import copy

import numpy as np

import helpers as H
from spectral_amd import layout as L

H_STEP = 1e-6
INPUTS = ("s_bounds", "l_bounds", "ds_bounds", "dl_bounds_knots", "s_ref", "l_ref")
_ATTR = {"dl_bounds_knots": "dl_bounds"}
_FIELDS = [(L.F_DOWN_BIAS, "down_bias"), (L.F_DOWN_SKEW, "down_skew"), (L.F_UPP_BIAS, "upp_bias"), (L.F_UPP_SKEW, "upp_skew"),
           (L.F_L_DOWN_BIAS, "l_down_bias"), (L.F_L_DOWN_SKEW, "l_down_skew"), (L.F_L_UPP_BIAS, "l_upp_bias"),
           (L.F_L_UPP_SKEW, "l_upp_skew"), (L.F_BEG_L, "beg_l"), (L.F_END_L, "end_l")]


def one_candidate(kb, b):
    """Candidate b of kb as a KnotBatch of its own (copies)."""
    out = copy.copy(kb)
    out.B = 1
    for name in ("s_bounds", "l_bounds", "ds_bounds", "dl_bounds", "s_ref", "l_ref", "init"):
        setattr(out, name, np.array(getattr(kb, name)[b:b + 1], dtype=np.float64))
    return out


def array_of(kb1, name):
    return getattr(kb1, _ATTR.get(name, name))[0]


def record(kb1, variant):
    """(decisions, y): y = the differentiated record, fields 1..16 [16, n] then ref_end [2] and dl_bounds [10], flat; decisions =
    (n, spans, knots attaining the ds extremes).  n < 1: (decisions, None)."""
    n, cubes = H.oracle_corridor(kb1, 0, variant)
    if n is None or n < 1:
        return (n if n is not None else -1, None, None), None
    N, delta = kb1.N, kb1.delta
    ds, sr, lr, dl = kb1.ds_bounds[0], kb1.s_ref[0], kb1.l_ref[0], kb1.dl_bounds[0]
    y = np.zeros((L.NUM_SEG_FIELDS, n))
    spans, attain = [], []
    for k, c in enumerate(cubes[:n]):
        for f, a in _FIELDS:
            y[f, k] = getattr(c, a)
        lo, hi, at_lo, at_hi = 0.0, 1000.0, -1, -1      # solve_3d.cc:835-841, indices clamped
        for i in range(c.beg_t, c.end_t + 1):
            ii = min(max(i, 0), N - 1)
            if ds[ii, 0] > lo:
                lo, at_lo = ds[ii, 0], ii
            if ds[ii, 1] < hi:
                hi, at_hi = ds[ii, 1], ii
        y[L.F_DS_LO, k], y[L.F_DS_HI, k] = lo, hi
        i0, i1 = min(10 * k, N - 1), min(10 * k + 1, N - 1)
        y[L.F_X_SKEW, k] = (sr[i1] - sr[i0]) / delta; y[L.F_X_BIAS, k] = sr[i0]
        y[L.F_Y_SKEW, k] = (lr[i1] - lr[i0]) / delta; y[L.F_Y_BIAS, k] = lr[i0]
        spans.append((c.beg_t, c.end_t)); attain.append((at_lo, at_hi))
    dl10 = np.array([dl[min(j >> 1, N - 1), j & 1] for j in range(10)])
    return (n, tuple(spans), tuple(attain)), np.concatenate([y[1:].ravel(), [sr[N - 1], lr[N - 1]], dl10])


def flat_cotangent(n, seg_bar, ref_end_bar, dl_bounds_bar):
    """The cotangent of y: seg_bar [NUM_SEG_FIELDS, seg_stride] restricted to fields 1.. and slots < n."""
    return np.concatenate([seg_bar[1:, :n].ravel(), ref_end_bar, dl_bounds_bar])


_cache = {}


def jacobian(kb, b, variant, key=None):
    """Central differences of candidate b's record: dict with n, y, J {input: [rows, entries]}, skipped {input: bool [entries]}.
    Computed once per `key` and shared."""
    if key is not None and key in _cache:
        return _cache[key]
    kb1 = one_candidate(kb, b)
    dec0, y0 = record(kb1, variant)
    out = dict(n=dec0[0], y=y0, J={}, skipped={})
    if y0 is not None:
        for name in INPUTS:
            arr = array_of(kb1, name)
            flat = arr.reshape(-1)
            J = np.zeros((y0.size, flat.size)); skipped = np.zeros(flat.size, dtype=bool)
            for c in range(flat.size):
                x = flat[c]
                flat[c] = x + H_STEP; dp, yp = record(kb1, variant)
                flat[c] = x - H_STEP; dm, ym = record(kb1, variant)
                flat[c] = x
                if dp != dec0 or dm != dec0 or not np.isfinite(x):
                    skipped[c] = True
                    continue
                J[:, c] = (yp - ym) / (2 * H_STEP)
            out["J"][name] = J; out["skipped"][name] = skipped
    if key is not None:
        _cache[key] = out
    return out


def reference_gradient(jac, ybar):
    """{input: (gradient [entries], tolerance [entries])} for the flat cotangent ybar."""
    ulp = np.spacing(np.abs(jac["y"]))
    tol = 4.0 * float(np.sum(np.abs(ybar) * 4.0 * ulp)) / (2 * H_STEP)
    return {name: (J.T @ ybar, np.full(J.shape[1], tol)) for name, J in jac["J"].items()}


def check_caps(jac):
    """The cap on skipping: at most 2 % of the candidate's columns; returns the number of s-bound columns left with a
    non-zero Jacobian (callers hold it, or its sum over the candidates they check, to the floor of 15)."""
    total = sum(s.size for s in jac["skipped"].values()); skipped = sum(int(s.sum()) for s in jac["skipped"].values())
    assert skipped <= 0.02 * total, (skipped, total)
    J = jac["J"]["s_bounds"]
    return int((np.abs(J).max(axis=0) > 0).sum())


def compare(jac, grads, ybar, what=""):
    """grads {input: array shaped like the input} against the reference on every column that is not skipped."""
    ref = reference_gradient(jac, ybar)
    worst = 0.0
    for name, (g, tol) in ref.items():
        if name not in grads:
            continue
        got = np.asarray(grads[name], dtype=np.float64).reshape(-1)
        keep = ~jac["skipped"][name]
        err = np.abs(got - g)[keep]
        if err.size:
            worst = max(worst, float((err / tol[keep]).max()))
        bad = np.nonzero(err > tol[keep])[0]
        assert bad.size == 0, (what, name, np.nonzero(keep)[0][bad][:5], got[keep][bad][:5], g[keep][bad][:5], tol[0])
    return worst


def max_pieces_in_front(jac):
    """The largest h among the checked segments: d down_bias_k / d lo(i0 + 1) = h / delta."""
    n = jac["n"]
    rows = (L.F_DOWN_BIAS - 1) * n + np.arange(n)
    return float(jac["J"]["s_bounds"][rows].max())


def shared_origin(jac):
    """Whether two checked segments read the same lower s bound (pieces of one base segment do)."""
    n = jac["n"]
    rows = (L.F_DOWN_BIAS - 1) * n + np.arange(n)
    return bool(((np.abs(jac["J"]["s_bounds"][rows]) > 0).sum(axis=0) >= 2).any())
