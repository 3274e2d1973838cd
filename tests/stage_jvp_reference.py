"""Yardstick of the forward-mode derivatives of the prism and corridor stages (include/btrapz_hip_stage_jvp.h).

The reference tangent of an output row is J @ t with J from tests/corridor_vjp_reference.jacobian / tests/prism_vjp_reference.
jacobian: central differences of the oracle-based maps, independent of the product.  t is zeroed on the columns those
modules skip (a +-h move there changes a decision); their own caps on skipping (check_caps / check_cap, 2 %) stay asserted by
the callers.  The tolerance of output row r is computed, not tuned:

    tol_r = 4 * (sum over c with J[r, c] != 0 of |t_c|) * 4 ulp(m_r) / (2 h),   m_r = max(1, |y_r|, max_c |J[r, c] x_c|)

A row's central difference carries rounding only in the columns it depends on, a few ulp of the largest term the row is a sum
of (|J x|: a difference quotient of two bounds of 40 whose value is 0.3 is rounded at 40 / delta, not at 0.3); the floor of 1
covers rows whose value is 0 at the base point.  A row the yardstick says depends on nothing must come back EXACTLY 0."""
import numpy as np

import corridor_vjp_reference as CR
import prism_vjp_reference as PR
from spectral_amd import layout as L


def row_tolerance(J, y, x, t, h):
    """(tol [rows], depends [rows]) for the Jacobian J [rows, cols], base outputs y, base inputs x and tangent t [cols]."""
    dep = J != 0.0
    terms = np.abs(J * x[None, :]).max(axis=1) if J.shape[1] else np.zeros(J.shape[0])
    m = np.maximum(np.maximum(1.0, np.abs(y)), terms)
    return 4.0 * (dep @ np.abs(t)) * 4.0 * np.spacing(m) / (2 * h), dep.any(axis=1)


def compare(ref, tol, depends, got, what=""):
    """got against ref row by row; rows that depend on nothing exactly 0.  Returns the worst error / tolerance."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not got[~depends].any(), (what, "rows without a dependency", np.flatnonzero(~depends & (got != 0))[:5])
    err = np.abs(got - ref)
    live = depends & (tol > 0)
    assert not err[depends & ~live].any(), (what, "zero tangent, non-zero result")
    bad = np.flatnonzero(live & (err > tol))
    assert bad.size == 0, (what, bad[:5], got[bad][:5], ref[bad][:5], tol[bad][:5])
    return float((err[live] / tol[live]).max()) if live.any() else 0.0


# ---- corridor stage ---------------------------------------------------------------------------------------------------
def corridor_inputs(kb, b):
    kb1 = CR.one_candidate(kb, b)
    return {name: CR.array_of(kb1, name).copy() for name in CR.INPUTS}


def corridor_tangents(kb, T, seed=0):
    """Random tangents of the six input arrays of every candidate: {input: [T, B, ...]}."""
    rng = np.random.default_rng(seed)
    like = dict(s_bounds=kb.s_bounds, l_bounds=kb.l_bounds, ds_bounds=kb.ds_bounds, dl_bounds_knots=kb.dl_bounds, s_ref=kb.s_ref,
                l_ref=kb.l_ref)
    return {k: rng.standard_normal((T,) + np.asarray(v).shape) for k, v in like.items()}


def corridor_flat(n, seg_dot, ref_end_dot, dl_dot):
    """One direction's outputs of one candidate (seg_dot [NUM_SEG_FIELDS, seg_stride]) in the yardstick's row order."""
    return np.concatenate([seg_dot[1:, :n].ravel(), ref_end_dot, dl_dot])


def corridor_compare(jac, x, tan, got_flat, what=""):
    """jac: corridor_vjp_reference.jacobian's dict; x, tan: {input: array} of ONE candidate and ONE direction."""
    J = np.concatenate([jac["J"][name] for name in CR.INPUTS], axis=1)
    skipped = np.concatenate([jac["skipped"][name] for name in CR.INPUTS])
    xs = np.concatenate([np.asarray(x[name], dtype=np.float64).reshape(-1) for name in CR.INPUTS])
    t = np.concatenate([(np.zeros(jac["J"][name].shape[1]) if tan.get(name) is None else np.asarray(tan[name], dtype=np.float64).reshape(-1))
                        for name in CR.INPUTS])
    t = np.where(skipped, 0.0, t)
    tol, dep = row_tolerance(J, jac["y"], xs, t, CR.H_STEP)
    return compare(J @ t, tol, dep, got_flat, what)


def zero_skipped_corridor(jac, tan):
    """The tangents of one candidate and one direction with the yardstick's skipped columns zeroed (what the product is given)."""
    out = {}
    for name in CR.INPUTS:
        if tan.get(name) is None:
            continue
        a = np.array(tan[name], dtype=np.float64)
        flat = a.reshape(-1)
        flat[jac["skipped"][name]] = 0.0
        out[name] = a
    return out


# ---- prism stage ------------------------------------------------------------------------------------------------------
def prism_tangents(pr, T, seed=0):
    """Random prisms_dot [T, B, P, 8]; entries 6, 7 and inactive slots hold NaN: they must not be read."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((T,) + pr.shape)
    t[..., 6:] = np.nan
    t[:, pr[:, :, 6] == 0.0] = np.nan
    return t


def zero_skipped_prism(jac, tdot):
    """tdot [P, 8] of one scene and one direction with the yardstick's skipped columns zeroed."""
    out = np.array(tdot, dtype=np.float64)
    out[:, :6][jac["skipped"].reshape(-1, 6)] = 0.0
    return out


def prism_compare(jac, pr, tdot, s_dot, l_dot, O, what=""):
    """jac: prism_vjp_reference.jacobian's dict of the scene pr [P, 8]; tdot [P, 8] (skipped columns zeroed by the caller);
    s_dot, l_dot [O, N, 2] (None: not checked).  Padding strips and overflowing scenes must be exactly 0."""
    n = jac["strips"]
    for a in (s_dot, l_dot):
        if a is not None:
            assert not a[(n if n <= O else 0):].any(), (what, "padding or overflow")
    if n > O:
        return 0.0
    t = np.nan_to_num(np.asarray(tdot, dtype=np.float64)[:, :6].reshape(-1), nan=0.0)
    t = np.where(jac["skipped"], 0.0, t)
    J, y, x = jac["J"], jac["y"], np.asarray(pr, dtype=np.float64)[:, :6].reshape(-1)
    tol, dep = row_tolerance(J, y, x, t, PR.H_STEP)
    ref = J @ t
    half = y.size // 2
    worst = 0.0
    if s_dot is not None:
        worst = max(worst, compare(ref[:half], tol[:half], dep[:half], s_dot[:n], (what, "s")))
    if l_dot is not None:
        worst = max(worst, compare(ref[half:], tol[half:], dep[half:], l_dot[:n], (what, "l")))
    return worst
