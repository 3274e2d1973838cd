"""Candidates whose optimum sits on velocity, acceleration or jerk rows: the cases of tests/test_gpu_active_rows.py, made on the
CPU by the oracle alone (helpers.oracle_qp_from_batch -> orc_assemble, AssembledQp.solve_exact: its dense interior-point method).

Twelve cases: {velocity, acceleration, jerk} x {s, l} x {lower, upper}.  Per width S a batch of B candidates of the generic
family (synth.make_batch(B, S, config=3)) is solved under the family's own limits; the extreme value the class's rows attain at
x* (A x*, the rows 18 k + r of that class and axis: tests/row_check_reference.py) says where a limit would bite, and the limit is
moved there:

    acceleration, jerk   Shared.dds / ddds / ddl / dddl, batch-wide: 0.6 x the median, over the solved candidates, of the attained
                         extremes that have the side's sign (upper: the largest row value where it is > 0; lower: the smallest
                         where it is < 0)
    s velocity           F_DS_LO / F_DS_HI, per candidate, every segment: 2 % of the attained range inside the range (at 10 % the
                         oracle rejects 6 and 7 of 8 candidates at 64 segments: the corridor's margins, 3 .. 10 m, are used up
                         by a speed capped for a minute); a candidate whose initial velocity -- the first velocity row, fixed
                         by an equality row -- lies beyond the moved limit keeps the family's limit
    l velocity           dl_bounds, per candidate, all five rows: 0.6 x the attained extreme where it has the side's sign

A candidate without a base solution, or whose extreme has the other sign, keeps the family's limit (it stays in the batch).  The
tightened batch is solved again, and the oracle's multipliers name the active rows: |y_i| > 1e-6 max |y| (the rule of
tests/golden/make_long_grad_goldens.py), upper where y_i > 0.  A candidate is strictly complementary when every inequality row is
either active by that rule or has a slack above 1e-6 (1 + |bound|).  Candidates the oracle rejects under the tightened limit
stay in the batch: the product must reject them too.

A case COUNTS at a width when at least MIN_COUNT candidates are solved (status 1), strictly complementary and have an active row
of the tightened class, axis and side.  assert_census() holds a width to the conditions of DESIGN.md 7 ("What is held at which
widths"); tests/test_active_row_cases.py asserts them without a GPU."""
import copy
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from helpers import oracle_qp_from_batch
from spectral_amd import layout as L
from spectral_amd import synth

CLASSES = ("vel", "acc", "jrk")
AXES = ("s", "l")
SIDES = ("lo", "hi")
CASES = [(c, a, s) for c in CLASSES for a in AXES for s in SIDES]
CLASS_R = {"pos": np.arange(0, 6), "vel": np.arange(6, 11), "acc": np.arange(11, 15), "jrk": np.arange(15, 18)}
ROW_L1 = {"vel": 10.0, "acc": 80.0, "jrk": 480.0}          # |g|_1 of a row: (-5, 5), (20, -40, 20), (-60, 180, -180, 60)
SHARED_FIELD = {("acc", "s"): "dds", ("jrk", "s"): "ddds", ("acc", "l"): "ddl", ("jrk", "l"): "dddl"}
FACTOR = 0.6
VEL_S_INSET = 0.02
ACTIVE_REL = 1e-6
BAND = (1e-9, 1e-4)
MASKS = ("act_lo", "act_hi", "strong_lo", "strong_hi", "band")
MIN_COUNT = 2
THREADS = 8


def case_id(case):
    return "%s_%s_%s" % case


def family(S, B=8, variant=0):
    return synth.make_batch(B, S, config=3, variant=variant)


def class_rows(S, cls, axis):
    """The row indices of a class of an axis in the assembled QP: axis base 21 S, then 18 k + r."""
    base = AXES.index(axis) * 21 * S
    return (base + 18 * np.arange(S)[:, None] + CLASS_R[cls][None, :]).ravel()


def row_segment(S, row):
    return (np.asarray(row) % (21 * S)) // 18


def _csr(qp):
    import scipy.sparse as sp
    return sp.csc_matrix((qp.A_x, qp.A_i, qp.A_p), shape=(qp.m, qp.n)).tocsr()


def _solve_one(args):
    batch, sh, b = args
    qp = oracle_qp_from_batch(batch, sh, b)
    x, y, info = qp.solve_exact()
    Ax = _csr(qp) @ x
    ineq = (qp.u - qp.l) > 1e-12
    ymax = max(float(np.abs(y).max()), 1e-300)
    act = ineq & (np.abs(y) > ACTIVE_REL * ymax)
    far = lambda v: np.where(np.abs(v) < 1e9, v, 0.0)
    slack = np.minimum(Ax - qp.l, qp.u - Ax)
    scale = 1.0 + np.maximum(np.abs(far(qp.l)), np.abs(far(qp.u)))
    strict = bool(np.all(~ineq | act | (slack > ACTIVE_REL * scale)))
    # for comparisons with multipliers an interior-point solve keeps (lam = y + mu / slack, inequality rows only): a row is
    # strongly active when its multiplier is above 1e-4 of the largest INEQUALITY multiplier and it has no slack left (the
    # strictness margin); a multiplier below 1e-9 of the largest is none; a row in between says nothing either way -- the rows
    # at the ends of an active arc, slack 1e-4 .. 1e-3, where the oracle's own y is mu / slack (21 segments, acc_l_lo,
    # candidate 7: |y| = 1.8e-4 of the largest on a row 3.4e-4 off its bound).  The band tests/test_gpu_long_warm.py leaves out,
    # one decade wider and taken row by row.
    rho = np.where(ineq, np.abs(y), 0.0) / max(float(np.abs(y[ineq]).max()) if ineq.any() else 0.0, 1e-300)
    strong = (rho > BAND[1]) & (slack <= ACTIVE_REL * scale)
    return dict(x=x, y=y, Ax=Ax, l=qp.l.copy(), u=qp.u.copy(), status=int(info.status), obj=float(info.obj_val),
                act_lo=act & (y < 0), act_hi=act & (y > 0), strict=strict, strong_lo=strong & (y < 0), strong_hi=strong & (y > 0),
                band=(rho >= BAND[0]) & ~strong)


def solve_batch(batch, sh, threads=THREADS):
    """The oracle's exact solve of every candidate (the C library runs outside the interpreter's lock: a pool of threads)."""
    with ThreadPoolExecutor(max(1, min(threads, batch.B))) as pool:
        res = list(pool.map(_solve_one, [(batch, sh, b) for b in range(batch.B)]))
    stack = lambda k: np.stack([r[k] for r in res])
    out = {k: stack(k) for k in ("x", "y", "Ax", "l", "u") + MASKS}
    out["status"] = np.array([r["status"] for r in res], dtype=np.int32)
    out["obj"] = np.array([r["obj"] for r in res])
    out["strict"] = np.array([r["strict"] for r in res])
    return out


def attained(base, S, cls, axis):
    """[B, 2]: the smallest and largest value the class's rows of the axis attain at each candidate's x*."""
    v = base["Ax"][:, class_rows(S, cls, axis)]
    return np.stack([v.min(axis=1), v.max(axis=1)], axis=1)


def limit_of(batch, base, case, factor=FACTOR, stat="median"):
    """The case's moved limit, from the base solution's rows: one batch-wide value (acceleration, jerk; nan when no candidate
    attains the side's sign) or [B] per-candidate values (velocity; nan where the family's limit is kept).  stat "least": the
    batch-wide value from the attained extreme of least size instead of the median -- with two candidates the median is their
    mean, and 0.6 of it leaves the candidate with the smaller extreme without an active row (256 segments)."""
    cls, axis, side = case
    S, B = batch.S, batch.B
    hi = side == "hi"
    ok = base["status"] == 1
    ext = attained(base, S, cls, axis)
    e = ext[:, 1] if hi else ext[:, 0]
    right = ok & ((e > 0) if hi else (e < 0))
    if cls != "vel":
        if not right.any():
            return float("nan")
        return factor * float(np.median(e[right]) if stat == "median" else e[right][np.argmin(np.abs(e[right]))])
    limit = np.full(B, np.nan)
    if axis == "s":
        rng_ = ext[:, 1] - ext[:, 0]
        moved = ext[:, 1] - VEL_S_INSET * rng_ if hi else ext[:, 0] + VEL_S_INSET * rng_
        # the first velocity row of the first segment is the initial velocity, which an equality row fixes: a limit moved past
        # it leaves no feasible point whatever the solve does, so such a candidate keeps the family's limit
        pinned = base["Ax"][:, class_rows(S, "vel", "s")[0]]
        who = ok & (rng_ > 0) & ((pinned < moved) if hi else (pinned > moved))
        limit[who] = moved[who]
    else:
        limit[right] = factor * e[right]
    return limit


def apply_limit(batch, sh, case, limit):
    """(batch', sh'): the family's batch under the case's limit (limit_of; nan: the family's own stays)."""
    cls, axis, side = case
    B = batch.B
    hi = side == "hi"
    nb = batch.slice(0, B)
    nsh = copy.deepcopy(sh)
    if cls != "vel":
        if np.isfinite(limit):
            f = SHARED_FIELD[(cls, axis)]
            old = getattr(nsh, f)
            setattr(nsh, f, (old[0], float(limit)) if hi else (float(limit), old[1]))
        return nb, nsh
    who = np.isfinite(limit)
    if axis == "s":
        seg = nb.seg.copy()
        seg[L.F_DS_HI if hi else L.F_DS_LO, who, :] = limit[who][:, None]
        nb.seg = seg
    else:
        dlb = nb.dl_bounds.copy().reshape(B, 5, 2)
        dlb[who, :, 1 if hi else 0] = limit[who][:, None]
        nb.dl_bounds = dlb.reshape(B, 10)
    return nb, nsh


def tightened_bound(case, limit, b):
    """The bound the oracle's rows of the case carry for candidate b (what an active row's value is compared with)."""
    return float(limit) if case[0] != "vel" else float(limit[b])


def summarise(S, case, sol):
    """What the oracle's second solve says of a case: per candidate solved / strict / active on the tightened class, the mask
    of those active rows, and where they lie."""
    cls, axis, side = case
    rows = class_rows(S, cls, axis)
    act = (sol["act_hi"] if side == "hi" else sol["act_lo"])[:, rows]
    solved = sol["status"] == 1
    good = solved & sol["strict"] & act.any(axis=1)
    segs = row_segment(S, rows)
    hit = act[good].any(axis=0) if good.any() else np.zeros(len(rows), dtype=bool)
    return dict(solved=solved, good=good, class_rows=rows, class_act=act, n_solved=int(solved.sum()), n_good=int(good.sum()),
                first=bool(hit[segs == 0].any()), interior=bool(hit[(segs > 0) & (segs < S - 1)].any()),
                last=bool(hit[segs == S - 1].any()), counts=int(good.sum()) >= MIN_COUNT)


def build_case(batch, sh, base, case, factor=FACTOR, threads=THREADS, stat="median"):
    limit = limit_of(batch, base, case, factor, stat)
    return with_solution(batch, sh, case, limit, None, threads)


def with_solution(batch, sh, case, limit, sol=None, threads=THREADS):
    """One case as the tests use it: the tightened batch and Shared, the oracle's solution of it (solved here unless given: the
    stored answers of the slow widths) and its summary."""
    nb, nsh = apply_limit(batch, sh, case, limit)
    if sol is None:
        sol = solve_batch(nb, nsh, threads)
    return dict(case=case, batch=nb, sh=nsh, limit=limit, sol=sol, **summarise(batch.S, case, sol))


_widths = {}


def width(S, B=8, variant=0, cases=None, threads=THREADS):
    """Every case of one width, computed once per process: {"batch", "sh", "base", "cases": {case: build_case(...)}}."""
    key = (S, B, variant, None if cases is None else tuple(cases))
    if key not in _widths:
        batch, sh = family(S, B, variant)
        base = solve_batch(batch, sh, threads)
        _widths[key] = dict(batch=batch, sh=sh, base=base,
                            cases={c: build_case(batch, sh, base, c, threads=threads) for c in (CASES if cases is None else cases)})
    return _widths[key]


def census_line(S, c):
    where = "".join(ch if f else "-" for ch, f in zip("fil", (c["first"], c["interior"], c["last"])))
    return "S %3d  %-10s solved %d  class-active %d  segments %s%s" % (S, case_id(c["case"]), c["n_solved"], c["n_good"], where,
                                                                     "" if c["counts"] else "  (does not count)")


def assert_census(S, w):
    """The conditions of DESIGN.md 7 on one width of twelve cases."""
    cs = w["cases"]
    B = w["batch"].B
    counting = [c for c in CASES if cs[c]["counts"]]
    if S >= 20:
        assert len(counting) == 12, (S, [case_id(c) for c in CASES if c not in counting])
    else:
        assert len(counting) >= 9, (S, [case_id(c) for c in counting])
        for cls in CLASSES:
            for axis in AXES:
                assert any(cs[(cls, axis, side)]["counts"] for side in SIDES), (S, cls, axis)
    for c in counting:
        assert 2 * cs[c]["n_solved"] > B, (S, case_id(c), cs[c]["n_solved"])
    return counting


# ---- the stored answers of the slow widths (tests/golden/make_active_row_goldens.py writes them) ---------------------------
# width -> (B, class x axis pairs, limit_of's stat).  64: the whole matrix; beyond a wavefront the oracle's dense solve takes
# seconds to minutes a candidate, so a few pairs on the side pick_side() names, 3 or 2 candidates each.
GOLDEN = "active_rows_yardstick.npz"
PAIRS = [(c, a) for c in CLASSES for a in AXES]
STORED = {64: (8, None, "median"),
          65: (3, PAIRS, "median"),
          130: (3, [("jrk", "s"), ("jrk", "l"), ("acc", "s"), ("vel", "s")], "median"),
          256: (2, [("jrk", "s"), ("acc", "l")], "least")}


def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def pick_side(batch, base, cls, axis):
    """The sides of a pair, the one first on which more solved candidates would get a moved limit (a tie: the lower side)."""
    n = {s: int(np.isfinite(np.atleast_1d(limit_of(batch, base, (cls, axis, s)))).sum()) if cls == "vel" else
         int(((base["status"] == 1) & ((attained(base, batch.S, cls, axis)[:, 1] > 0) if s == "hi" else
                                       (attained(base, batch.S, cls, axis)[:, 0] < 0))).sum()) for s in SIDES}
    return ("hi", "lo") if n["hi"] > n["lo"] else ("lo", "hi")


def generate_stored(S, threads=THREADS, log=None):
    """The arrays of one stored width, {key: array} with keys "S<S>/...": the chosen cases, their limits and the oracle's
    answers.  Deterministic: the same bits on every run (tests/test_active_row_cases.py regenerates the 64-segment slice)."""
    B, pairs, stat = STORED[S]
    batch, sh = family(S, B)
    base = solve_batch(batch, sh, threads)
    if pairs is None:
        built = [build_case(batch, sh, base, c, threads=threads) for c in CASES]
    else:
        built = []
        for cls, axis in pairs:
            for side in pick_side(batch, base, cls, axis):
                c = build_case(batch, sh, base, (cls, axis, side), threads=threads, stat=stat)
                if c["counts"]:
                    break
            built.append(c)
    out = {"S%d/B" % S: np.array(B), "S%d/cases" % S: np.array([case_id(c["case"]) for c in built]),
           "S%d/base_status" % S: base["status"]}
    for c in built:
        if log:
            log(census_line(S, c))
        p = "S%d/%s/" % (S, case_id(c["case"]))
        out[p + "limit"] = np.asarray(c["limit"], dtype=np.float64)
        sol = c["sol"]
        solved = sol["status"] > 0
        out[p + "x"] = np.where(solved[:, None], sol["x"], 0.0)        # (a rejected candidate has no optimum: zeros)
        out[p + "obj"] = np.where(solved, sol["obj"], 0.0)
        out[p + "status"] = sol["status"]
        out[p + "strict"] = sol["strict"]
        for k in MASKS:
            out[p + k] = np.packbits(sol[k], axis=1)
    return out


_stored = {}


def stored(S, data=None):
    """A stored width in the shape width() returns (no "base"): batches regenerated from synth, limits and answers from the file."""
    if S not in _stored or data is not None:
        g = np.load(golden_path()) if data is None else data
        B = int(g["S%d/B" % S])
        batch, sh = family(S, B)
        cases = {}
        for cid in [str(c) for c in g["S%d/cases" % S]]:
            case = tuple(cid.split("_"))
            p = "S%d/%s/" % (S, cid)
            m = 42 * S
            sol = dict(x=g[p + "x"], obj=g[p + "obj"], status=g[p + "status"], strict=g[p + "strict"],
                       **{k: np.unpackbits(g[p + k], axis=1)[:, :m].astype(bool) for k in MASKS})
            limit = g[p + "limit"]
            cases[case] = with_solution(batch, sh, case, float(limit) if limit.ndim == 0 else limit, sol)
        w = dict(batch=batch, sh=sh, cases=cases)
        if data is not None:
            return w
        _stored[S] = w
    return _stored[S]


def cases_of(S, B=8):
    """width() where the oracle runs live (up to 33 segments), stored() beyond."""
    return stored(S) if S in STORED else width(S, B)


def row_values(x, S, cls, axis):
    """The values of a class's rows of an axis at control points x [..., 12 S], in class_rows() order, from the rows' own
    patterns (-5, 5), (20, -40, 20), (-60, 180, -180, 60) -- no assembled matrix (test_active_row_cases holds it to A x)."""
    x = np.asarray(x, dtype=np.float64)
    a = AXES.index(axis)
    c = x[..., 6 * S * a:6 * S * (a + 1)].reshape(x.shape[:-1] + (S, 6))
    if cls == "vel":
        v = 5.0 * (c[..., 1:] - c[..., :-1])
    elif cls == "acc":
        v = 20.0 * (c[..., 2:] - 2.0 * c[..., 1:-1] + c[..., :-2])
    else:
        v = 60.0 * (c[..., 3:] - 3.0 * c[..., 2:-1] + 3.0 * c[..., 1:-2] - c[..., :-3])
    return v.reshape(x.shape[:-1] + (-1,))


def oracle_support(sol, b, S, axis):
    """(strong, unclear), each [2 sides][18 rows][S], of candidate b: where the oracle has an inequality row of the axis strongly
    active, lower / upper, and where its multiplier lies in the band that decides nothing (_solve_one); the first row of a
    joint folded onto the last row of the segment before (include/btrapz_hip.h: a joint's bound is ONE row)."""
    base = AXES.index(axis) * 21 * S
    idx = base + 18 * np.arange(S)[None, :] + np.arange(18)[:, None]
    strong = fold_joints(np.stack([sol["strong_lo"][b][idx], sol["strong_hi"][b][idx]]))
    unclear = fold_joints(np.stack([sol["band"][b][idx]] * 2))
    return strong, unclear & ~strong


def fold_joints(sup):
    sup = sup.copy()
    for r, twin in ((0, 5), (6, 10), (11, 14)):
        sup[:, twin, :-1] |= sup[:, r, 1:]
        sup[:, r, 1:] = False
    return sup
