"""The yardstick of the row audit (btrapz_check_rows_device): margins, worst rows, equality residuals and the
objective of given control points, from the oracle's assembled QP (helpers.oracle_qp_from_batch -> orc_assemble, the
restatement of solve_3d.cc:779-1129 / cuboid_3d.cc:632-988) in numpy and scipy.sparse.  A is used as the CSC arrays the
oracle returns, never dense (at 256 segments the dense A is 260 MB).

Rows are classified by INDEX.  Per axis: the rows 18 k + r of all S segments (r = 0..5 position, 6..10 velocity, 11..14
acceleration, 15..17 jerk), then 3 initial-state rows, then 3 continuity rows per joint; the l axis follows at 21 S
(row_order_identities() holds orc_assemble to that).  A side of a row whose bound is at least 1e9 in size is dropped; a NaN
margin counts as -inf, a NaN residual as +inf.

Tolerances come from magnitudes, never from an observed error: for a class of an axis
    64 * 2^-53 * max(1, max_r (sum_j |a_rj x_j| + the absolute values of the terms the row's bound is summed from)),
the same rule for the equality rows, every magnitude divided by the row's norm for unit = 1; for the objective the project's
bound for objectives, 1e-6 (1 + |obj|) (tests/test_gpu_bench_batch.py:71)."""
import numpy as np
import scipy.sparse as sp

EPS64 = 64.0 * 2.0 ** -53
FAR = 1e9
CLASS_OF_R = np.array([0] * 6 + [1] * 5 + [2] * 4 + [3] * 3)
CLASS_NNZ = (1, 2, 3, 4)
NAMES = ("position", "velocity", "acceleration", "jerk")


def csc(qp):
    return sp.csc_matrix((qp.A_x, qp.A_i, qp.A_p), shape=(qp.m, qp.n))


def row_order_identities(qp):
    """Asserts of an AssembledQp that its rows come in the order the audit numbers them, and that every inequality row has
    the coefficient pattern of its class."""
    S = qp.S
    A = csc(qp).tocsr()
    assert qp.m == 42 * S and qp.n == 12 * S
    t = np.array([qp.cubes[k].t for k in range(S)])
    pat = {1: None, 2: (-5.0, 5.0), 3: (20.0, -40.0, 20.0), 4: (-60.0, 180.0, -180.0, 60.0)}
    for axis in (0, 1):
        base, col0 = axis * 21 * S, axis * 6 * S
        for k in range(S):
            for r in range(18):
                row = A.getrow(base + 18 * k + r)
                cls = CLASS_OF_R[r]
                first = col0 + 6 * k + (r, r - 6, r - 11, r - 15)[cls]
                assert row.nnz == CLASS_NNZ[cls] and np.array_equal(np.sort(row.indices), first + np.arange(CLASS_NNZ[cls])), (axis, k, r)
                vals = row.toarray()[0, first:first + CLASS_NNZ[cls]]
                assert np.array_equal(vals, [t[k]] if cls == 0 else pat[CLASS_NNZ[cls]]), (axis, k, r, vals)
        ini = base + 18 * S
        assert [A.getrow(ini + i).nnz for i in range(3)] == [1, 2, 3]
        assert all(np.array_equal(np.sort(A.getrow(ini + i).indices), col0 + np.arange(i + 1)) for i in range(3))
        eq = np.arange(ini, base + 21 * S)
        assert np.array_equal(qp.l[eq], qp.u[eq]) and len(eq) == 3 + 3 * (S - 1)
        for k in range(S - 1):
            j = ini + 3 + 3 * k
            assert [A.getrow(j + i).nnz for i in range(3)] == [2, 4, 6]
            for i, lo in enumerate((5, 4, 3)):
                assert np.array_equal(np.sort(A.getrow(j + i).indices), col0 + 6 * k + np.arange(lo, 11 - lo + 1) if i else col0 + 6 * k + np.array([5, 6])), (axis, k, i)
            assert np.all(qp.l[j:j + 3] == 0.0)


def _bound_terms(qp, variant):
    """Per inequality row: the sum of the absolute values of the terms its bound is summed from -- the larger of its two
    sides; a side that is dropped adds nothing.  Position rows: |bias| + |skew (r / 5) t| of the row's line (the cuboid's
    inscribed s interval is the extreme of its lines over r = 0..5: the largest of them; its l rows are beg_l / end_l
    themselves); every other row's bound is one product, its own magnitude."""
    S = qp.S
    kept = lambda v: not (abs(v) >= FAR)
    terms = np.zeros(qp.m)
    for axis in (0, 1):
        base = axis * 21 * S
        for k in range(S):
            c = qp.cubes[k]
            lines = ((c.down_bias, c.down_skew), (c.upp_bias, c.upp_skew)) if axis == 0 else \
                ((c.l_down_bias, c.l_down_skew), (c.l_upp_bias, c.l_upp_skew))
            at = lambda side, r: abs(lines[side][0]) + abs(lines[side][1] * (r / 5.0) * c.t)
            for r in range(18):
                i = base + 18 * k + r
                best = 0.0
                for side, v in enumerate((qp.l[i], qp.u[i])):
                    if not kept(v):
                        continue
                    m = abs(v)
                    if r < 6 and not (variant == 1 and axis == 1):
                        m = max(m, max(at(side, rr) for rr in range(6)) if variant == 1 else at(side, r))
                    best = max(best, m)
                terms[i] = best
    return terms


def reference(qp, x, variant, unit=0):
    """The audit of x against AssembledQp qp (assembled for `variant`).  Returns a dict: margin [2, 4], worst [2, 4] (-1: none),
    eq_res [2, 2], obj;
    row_margin [m] (inequality rows: the margin of every row in `unit`, +inf where no side is left; nan elsewhere);
    tol_margin [2, 4], tol_eq [2, 2], tol_obj: the computed tolerances; rows [2][4]: the row indices (18 k + r) of a class."""
    S = qp.S
    x = np.asarray(x, dtype=np.float64)
    A = csc(qp)
    with np.errstate(invalid="ignore", over="ignore"):
        Ax = A @ x
        mag = abs(A) @ np.abs(x)
        norm = np.sqrt(np.asarray(A.multiply(A).sum(axis=1)).ravel())
        lo_kept, up_kept = ~(np.abs(qp.l) >= FAR), ~(np.abs(qp.u) >= FAR)
        m_lo = np.where(lo_kept, Ax - qp.l, np.inf)
        m_up = np.where(up_kept, qp.u - Ax, np.inf)
        m_lo = np.where(np.isnan(m_lo), -np.inf, m_lo); m_up = np.where(np.isnan(m_up), -np.inf, m_up)
        row_m = np.minimum(m_lo, m_up)
        scale = 1.0 / norm if unit == 1 else np.ones(qp.m)
        if getattr(qp, "_row_check_terms", None) is None:     # (Python loops over the rows: once per QP, both units share it)
            qp._row_check_terms = np.nan_to_num(_bound_terms(qp, variant), nan=0.0, posinf=0.0)
        terms = qp._row_check_terms
    margin = np.full((2, 4), np.inf); worst = np.full((2, 4), -1, dtype=np.int64)
    tol_m = np.zeros((2, 4)); eq = np.zeros((2, 2)); tol_e = np.zeros((2, 2))
    row_margin = np.full(qp.m, np.nan)
    rows = [[None] * 4 for _ in range(2)]
    for axis in (0, 1):
        base = axis * 21 * S
        local = np.arange(18 * S)
        for cls in range(4):
            loc = local[CLASS_OF_R[local % 18] == cls]
            idx = base + loc
            with np.errstate(invalid="ignore"):
                mm = row_m[idx] * scale[idx]
            mm = np.where(np.isnan(mm), -np.inf, mm)
            row_margin[idx] = mm
            rows[axis][cls] = loc
            j = int(np.argmin(mm))                      # (the first of equal minima: the lowest row)
            margin[axis, cls] = mm[j]
            worst[axis, cls] = loc[j] if mm[j] < np.inf else -1
            tol_m[axis, cls] = EPS64 * max(1.0, float(((mag[idx] + terms[idx]) * scale[idx]).max()))
        ini = base + 18 * S
        for part, idx in enumerate((np.arange(ini, ini + 3), np.arange(ini + 3, base + 21 * S))):
            if len(idx):
                with np.errstate(invalid="ignore"):
                    res = np.abs(Ax[idx] - qp.l[idx])
                eq[axis, part] = np.where(np.isnan(res), np.inf, res).max()
                tol_e[axis, part] = EPS64 * max(1.0, float((mag[idx] + np.abs(qp.l[idx])).max()))
            else:
                tol_e[axis, part] = EPS64
    Pu = sp.csc_matrix((qp.P_x, qp.P_i, qp.P_p), shape=(qp.n, qp.n))
    Px = Pu @ x + Pu.T @ x - Pu.diagonal() * x
    obj = float(0.5 * x @ Px + qp.q @ x)
    return dict(margin=margin, worst=worst, eq_res=eq, obj=obj, row_margin=row_margin, tol_margin=tol_m, tol_eq=tol_e,
                tol_obj=1e-6 * (1.0 + abs(obj)), rows=rows, base=(0, 21 * S))


def compare(got, ref, what, obj=True):
    """Holds one candidate's audit (dict of numpy: margin [2, 4], worst [2, 4], eq_res [2, 2], obj) to reference()'s result.
    Raises AssertionError; returns the largest ratio of an error to its tolerance."""
    worst_ratio = 0.0
    for axis in (0, 1):
        for cls in range(4):
            g, r, tol = got["margin"][axis, cls], ref["margin"][axis, cls], ref["tol_margin"][axis, cls]
            w = int(got["worst"][axis, cls])
            if not np.isfinite(r):
                assert g == r and w == ref["worst"][axis, cls], (what, axis, NAMES[cls], g, r, w)
                continue
            ratio = abs(g - r) / tol
            assert ratio <= 1.0, (what, axis, NAMES[cls], g, r, tol)
            worst_ratio = max(worst_ratio, ratio)
            # the reported row: of this axis and class, and the yardstick's margin AT it within twice the tolerance of the minimum
            assert w in ref["rows"][axis][cls], (what, axis, NAMES[cls], w)
            at = ref["row_margin"][ref["base"][axis] + w]
            assert at - r <= 2.0 * tol, (what, axis, NAMES[cls], w, at, r, tol)
        for part in (0, 1):
            g, r, tol = got["eq_res"][axis, part], ref["eq_res"][axis, part], ref["tol_eq"][axis, part]
            if not np.isfinite(r):
                assert g == r, (what, axis, part, g, r)
                continue
            ratio = abs(g - r) / tol
            assert ratio <= 1.0, (what, axis, "equality", part, g, r, tol)
            worst_ratio = max(worst_ratio, ratio)
    if obj:
        ratio = abs(got["obj"] - ref["obj"]) / ref["tol_obj"]
        assert ratio <= 1.0, (what, "obj", got["obj"], ref["obj"])
        worst_ratio = max(worst_ratio, ratio)
    return worst_ratio


def constant_velocity_ctrl(batch, b, n=None):
    """The control points of the initial state of candidate b propagated at constant velocity: position p0 + v0 tau at the six
    Bernstein abscissae of every segment, over the segment's duration (a position row reads t c_i).  [12 n], the solve's layout."""
    n = batch.S if n is None else n
    t = np.asarray(batch.seg[0, b, :n], dtype=np.float64)
    start = np.concatenate([[0.0], np.cumsum(t)[:-1]])
    out = np.zeros(12 * n)
    for axis in (0, 1):
        p0, v0 = batch.init[b, 3 * axis], batch.init[b, 3 * axis + 1]
        tau = start[:, None] + t[:, None] * (np.arange(6) / 5.0)[None, :]
        out[6 * n * axis:6 * n * (axis + 1)] = ((p0 + v0 * tau) / t[:, None]).ravel()
    return out
