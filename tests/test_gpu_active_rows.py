"""Every form of the forward solve held to the oracle on candidates whose optimum sits on velocity, acceleration or jerk rows
(tests/active_row_cases.py: twelve cases, {velocity, acceleration, jerk} x {s, l} x {lower, upper}, made by tightening one
limit to where the base solution's rows reach).  Every other comparison of a solve kernel with x* runs on candidates whose
optimum sits on position rows alone: a row that is never active contributes a barrier term that vanishes as the solve
converges, so a wrong coefficient, limit, sign or missing row of these three classes passes there.

Per form and case, for every candidate of the batch:
    the oracle's accept decision (a candidate it rejects under the tightened limit stays in the batch);
    |ctrl - x*|_inf <= 1e-5 |x*|_inf and |cost - obj(x*)| <= 1e-6 |cost| (the project's bounds);
    on every row of the tightened class the oracle names active, the row's value at the GPU's control points lies within
    |g|_1 1e-5 |x*|_inf of the tightened bound (g the row's coefficients: what the control-point bound allows a row);
    check_rows on the GPU's own control points: the smallest margin of the tightened class is 0 within that bound, and the row
    it reports is one the oracle has active -- the audit's numbering of these classes tied to a solve that depends on them.
Where multipliers are kept, their support on the tightened class's rows equals the oracle's on strictly complementary candidates
(the pattern only, as tests/test_gpu_warm_edges.py).

Lane-mapping seams are held elsewhere on position-bound candidates and are not repeated: rows are lane-local, the smallest widths
suffice.  Widths up to 33 are solved by the oracle live, once per module; 64, 65, 130 and 256 come from
tests/golden/active_rows_yardstick.npz.  Every test prints its worst ratio of an error to its bound (DESIGN.md 7 records one run)."""
import ctypes as C
import os

import numpy as np
import pytest

import active_row_cases as A
from helpers import O
from spectral_amd import layout as L

pytestmark = pytest.mark.gpu
RTOL = 1e-5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASE_IDS = [A.case_id(c) for c in A.CASES]
PIN = dict(cap_iter=-1, compact=-1)


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def host(o):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in o.items()}


def case_of(S, cid, variant=0):
    """(width, case `cid` of it), from the module-wide cache inside active_row_cases."""
    w = A.width(S, variant=variant) if variant else A.cases_of(S)
    return w, w["cases"].get(tuple(cid.split("_")))


def hold(solver, what, c, r, audit=True):
    """One case's results r (numpy: ctrl [B, 12 S], cost, status) against the oracle's answers c["sol"].  Returns the worst ratios
    (ctrl, cost, rows, margin) to their bounds."""
    import torch
    sol, batch = c["sol"], c["batch"]
    cls, axis, side = c["case"]
    S, B = batch.S, batch.B
    assert np.array_equal(sol["status"] > 0, r["status"] > 0), (what, "accept decision", sol["status"], r["status"])
    ok = np.nonzero(sol["status"] == 1)[0]
    assert len(ok), what
    xs = sol["x"]
    scale = np.abs(xs).max(axis=1)
    worst = dict(ctrl=0.0, cost=0.0, rows=0.0, margin=0.0)
    for b in ok:
        e = np.abs(r["ctrl"][b, :12 * S] - xs[b]).max() / (RTOL * scale[b])
        print("%s b=%d ctrl error / bound %.3g" % (what, b, e))
        assert e <= 1.0, (what, b, "ctrl", e)
        ec = abs(r["cost"][b] - sol["obj"][b]) / (1e-6 * abs(r["cost"][b]))
        assert ec <= 1.0, (what, b, "cost", r["cost"][b], sol["obj"][b])
        worst["ctrl"], worst["cost"] = max(worst["ctrl"], e), max(worst["cost"], ec)
    good = np.nonzero(c["good"])[0]
    got = None
    if audit and len(good):
        got = host(solver.check_rows(solver.upload(batch), c["sh"], torch.from_numpy(np.nan_to_num(r["ctrl"][:, :12 * S])).to(solver.device),
                                     want=("margin", "worst")))
    ai, ci = A.AXES.index(axis), 1 + A.CLASSES.index(cls)
    either = sol["act_lo"] | sol["act_hi"]
    for b in good:
        bound = A.ROW_L1[cls] * RTOL * scale[b]
        limit = A.tightened_bound(c["case"], c["limit"], b)
        vals = A.row_values(r["ctrl"][b, :12 * S], S, cls, axis)[c["class_act"][b]]
        er = np.abs(vals - limit).max() / bound
        print("%s b=%d: %d active %s rows at %.6g, row value error / bound %.3g" % (what, b, len(vals), A.case_id(c["case"]), limit, er))
        assert er <= 1.0, (what, b, "active rows", vals, limit, bound)
        worst["rows"] = max(worst["rows"], er)
        if got is not None:
            m, w = got["margin"][b, ai, ci], int(got["worst"][b, ai, ci])
            assert abs(m) <= bound, (what, b, "check_rows margin", m, bound)
            assert w >= 0 and w % 18 in A.CLASS_R[cls] and either[b, ai * 21 * S + w], (what, b, "check_rows row", w)
            worst["margin"] = max(worst["margin"], abs(m) / bound)
    print("%s: %d solved, %d class-active; worst error / bound: ctrl %.3g cost %.3g rows %.3g margin %.3g"
          % (what, len(ok), len(good), worst["ctrl"], worst["cost"], worst["rows"], worst["margin"]))
    return worst


def support_matches(what, c, lam, status):
    """lam [2][36][B][S] of a solve with kept multipliers against the oracle's support, on the tightened class's rows of the
    strictly complementary, class-active candidates: an entry is above 1e-6 of the candidate's largest multiplier exactly where
    the oracle has the row strongly active on that side.  Rows whose oracle multiplier lies in the band that decides nothing
    (active_row_cases._solve_one: the ends of an active arc) are left out, row by row; a candidate is compared when a strongly
    active row of the tightened class and side remains."""
    cls, axis, side = c["case"]
    S = c["batch"].S
    ai = A.AXES.index(axis)
    compared = 0
    for b in np.nonzero(c["good"])[0]:
        assert status[b] > 0
        want, unclear = (m[:, A.CLASS_R[cls]] for m in A.oracle_support(c["sol"], b, S, axis))
        if not want[A.SIDES.index(side)].any():
            continue
        lb = lam[:, :, b, :]
        got = A.fold_joints(np.stack([lb[ai, :18], lb[ai, 18:]]) > 1e-6 * lb.max())[:, A.CLASS_R[cls]]
        differ = (got != want) & ~unclear
        print("%s b=%d: %d strongly active %s rows, %d in the band, %d entries differ" % (what, b, want.sum(), cls, unclear.sum(), differ.sum()))
        assert not differ.any(), (what, b, np.argwhere(differ)[:8])
        compared += 1
    print("%s: support of the kept multipliers on %s rows compared on %d candidates" % (what, cls, compared))
    return compared


def joint_times(batch):
    import torch
    return torch.from_numpy(np.cumsum(batch.seg[L.F_T], axis=1))


# ---- cold solves, one form at a time ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
@pytest.mark.parametrize("S", [1, 3, 21, 33, 64])
def test_packed(solver, S, cid):
    w, c = case_of(S, cid)
    r = host(solver.solve(solver.upload(c["batch"]), c["sh"], lean=-1, split=-1, **PIN))
    assert solver.ctx.last_solve_form() == 0
    hold(solver, "packed S=%d %s" % (S, cid), c, r)


@pytest.mark.parametrize("cid", CASE_IDS)
@pytest.mark.parametrize("S", [3, 21, 33, 64])
def test_lean_in_one_launch_and_in_two(solver, S, cid):
    w, c = case_of(S, cid)
    db = solver.upload(c["batch"])
    one = host(solver.solve(db, c["sh"], lean=1, split=-1, cap_iter=-1))
    assert solver.ctx.last_solve_form() == 8
    hold(solver, "lean S=%d %s" % (S, cid), c, one)
    two = host(solver.solve(db, c["sh"], lean=1, split=-1, cap_iter=6))
    assert solver.ctx.last_solve_form() == 11
    hold(solver, "lean, two launches S=%d %s" % (S, cid), c, two, audit=False)


@pytest.mark.parametrize("cid", CASE_IDS)
@pytest.mark.parametrize("S", [1, 5, 21])
def test_split(solver, S, cid):
    w, c = case_of(S, cid)
    r = host(solver.solve(solver.upload(c["batch"]), c["sh"], split=1, lean=-1, **PIN))
    assert solver.ctx.last_solve_form() == 1
    hold(solver, "split S=%d %s" % (S, cid), c, r)


@pytest.mark.parametrize("cid", CASE_IDS)
@pytest.mark.parametrize("lean", [-1, 1], ids=["packed", "lean"])
def test_cuboid_variant(solver, lean, cid):
    w, c = case_of(21, cid, variant=1)
    assert c["counts"], A.census_line(21, c)
    r = host(solver.solve(solver.upload(c["batch"]), c["sh"], lean=lean, split=-1, **PIN))
    assert solver.ctx.last_solve_form() == (8 if lean > 0 else 0)
    hold(solver, "cuboid %s S=21 %s" % ("lean" if lean > 0 else "packed", cid), c, r)


@pytest.mark.parametrize("S", [65, 130, 256])
def test_long_cold(solver, S):
    w = A.stored(S)
    for case, c in w["cases"].items():
        assert c["counts"], A.census_line(S, c)
        r = host(solver.solve(solver.upload(c["batch"]), c["sh"]))
        assert solver.ctx.last_solve_form() == 2
        hold(solver, "long S=%d %s" % (S, A.case_id(case)), c, r)


# ---- warm starts: from the solve under the family's own limits, whose optimum lies on other rows -------------------------
def warm_from_the_family(solver, w, c, solve, **kw):
    base_db = solver.upload(w["batch"])
    o = solve(base_db, w["sh"], keep_multipliers=True, **kw)
    x0 = solver.eval_states(base_db, o["ctrl"].clone(), joint_times(w["batch"]))
    lam = o["lam"].clone()
    o2 = solve(solver.upload(c["batch"]), c["sh"], warm=dict(x0=x0, lam=lam), keep_multipliers=True, **kw)
    return host(o2)


@pytest.mark.parametrize("cid", CASE_IDS)
@pytest.mark.parametrize("lean", [-1, 1], ids=["packed", "lean"])
@pytest.mark.parametrize("S", [3, 21, 64])
def test_warm(solver, S, lean, cid):
    w, c = case_of(S, cid)
    r = warm_from_the_family(solver, w, c, solver.solve, lean=lean)
    assert solver.ctx.last_solve_form() == (8 if lean > 0 else 0)
    hold(solver, "warm %s S=%d %s" % ("lean" if lean > 0 else "packed", S, cid), c, r)


def test_solve_long_warm(solver):
    w = A.stored(130)
    for case, c in w["cases"].items():
        r = warm_from_the_family(solver, w, c, solver.solve_long)
        assert solver.ctx.last_solve_form() == 16
        what = "solve_long warm S=130 %s" % A.case_id(case)
        hold(solver, what, c, r)
        assert support_matches(what, c, r["lam"], r["status"]) >= 2


# ---- kept multipliers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
@pytest.mark.parametrize("lean", [-1, 1], ids=["packed", "lean"])
@pytest.mark.parametrize("S", [21, 64])
def test_kept_multipliers(solver, S, lean, cid):
    w, c = case_of(S, cid)
    r = host(solver.solve(solver.upload(c["batch"]), c["sh"], keep_multipliers=True, lean=lean))
    assert solver.ctx.last_solve_form() == (8 if lean > 0 else 0)
    what = "kept multipliers %s S=%d %s" % ("lean" if lean > 0 else "packed", S, cid)
    hold(solver, what, c, r, audit=False)
    assert support_matches(what, c, r["lam"], r["status"]) >= (2 if c["counts"] else 0)


def test_kept_multipliers_long(solver):
    w = A.stored(130)
    for case, c in w["cases"].items():
        r = host(solver.solve_long(solver.upload(c["batch"]), c["sh"], keep_multipliers=True))
        assert solver.ctx.last_solve_form() == 16
        what = "kept multipliers long S=130 %s" % A.case_id(case)
        hold(solver, what, c, r, audit=False)
        assert support_matches(what, c, r["lam"], r["status"]) >= 2


# ---- a ragged record: the 1-, 3-, 21- and 33-segment candidates of one case under one batch-wide limit --------------------
RAGGED_WIDTHS = (1, 3, 21, 33)
_ragged = {}


def ragged_case(case):
    """Per width the case under the limit of the 21-segment width (one Shared for the record), solved by the oracle once."""
    if case not in _ragged:
        limit = A.width(21)["cases"][case]["limit"]
        parts = []
        for S in RAGGED_WIDTHS:
            batch, sh = A.family(S)
            parts.append(A.with_solution(batch, sh, case, limit))
            assert parts[-1]["counts"], A.census_line(S, parts[-1])
        _ragged[case] = parts
    return _ragged[case]


@pytest.mark.parametrize("lean", [-1, 1], ids=["packed", "lean"])
@pytest.mark.parametrize("cid", ["jrk_s_hi", "acc_l_lo"])
def test_solve_ragged(solver, cid, lean):
    import torch
    parts = ragged_case(tuple(cid.split("_")))
    stride = max(RAGGED_WIDTHS)
    B = sum(p["batch"].B for p in parts)
    seg = np.full((L.NUM_SEG_FIELDS, B, stride), np.nan)           # NaN in every slot beyond a candidate's count
    cnt = np.zeros(B, dtype=np.int32); init = np.zeros((B, 6)); ref_end = np.zeros((B, 2)); dlb = np.zeros((B, 10))
    where = []
    perm = np.random.default_rng(5).permutation(B)                  # the widths interleaved
    src = [(i, b) for i, p in enumerate(parts) for b in range(p["batch"].B)]
    for dst, j in enumerate(perm):
        i, b = src[j]
        pb = parts[i]["batch"]
        seg[:, dst, :pb.S] = pb.seg[:, b]; cnt[dst] = pb.S
        init[dst], ref_end[dst], dlb[dst] = pb.init[b], pb.ref_end[b], pb.dl_bounds[b]
        where.append((i, b))
    t = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(solver.device)
    rec = dict(B=B, seg_stride=stride, seg=t(seg), seg_count=t(cnt, np.int32), init=t(init), ref_end=t(ref_end), dl_bounds=t(dlb))
    r = host(solver.solve_ragged(rec, parts[0]["sh"], lean=lean, cap_iter=-1))
    assert solver.ctx.last_solve_form() == (8 if lean > 0 else 0)
    for i, p in enumerate(parts):
        rows = [dst for dst, (ii, b) in sorted(enumerate(where), key=lambda e: e[1]) if ii == i]
        hold(solver, "ragged %s, %d segments, %s" % ("lean" if lean > 0 else "packed", p["batch"].S, cid), p, {k: v[rows] for k, v in r.items()})


# ---- parameter sets: the twelve cases as twelve sets in one launch ---------------------------------------------------------
@pytest.mark.parametrize("lean", [-1, 1], ids=["packed", "lean"])
def test_solve_sets(solver, lean):
    import torch
    w = A.width(21)
    cs = [w["cases"][c] for c in A.CASES]
    B = w["batch"].B
    cat = lambda k, axis=0: np.concatenate([getattr(c["batch"], k) for c in cs], axis=axis)
    batch = L.Batch(B=12 * B, S=21, seg=np.ascontiguousarray(cat("seg", 1)), init=cat("init"), ref_end=cat("ref_end"), dl_bounds=cat("dl_bounds"))
    index = torch.from_numpy(np.repeat(np.arange(12), B).astype(np.int32)).to(solver.device)
    o = host(solver.solve_sets(solver.upload(batch), [c["sh"] for c in cs], index, lean=lean, split=-1, **PIN))
    assert solver.ctx.last_solve_form() == (8 if lean > 0 else 0)
    for g, c in enumerate(cs):
        mine = {k: v[g * B:(g + 1) * B] for k, v in o.items()}
        alone = host(solver.solve(solver.upload(c["batch"]), c["sh"], lean=lean, split=-1, **PIN))
        for k in ("ctrl", "cost", "status", "iters"):
            assert mine[k].tobytes() == alone[k].tobytes(), (A.case_id(c["case"]), k)
        hold(solver, "sets %s S=21 %s" % ("lean" if lean > 0 else "packed", A.case_id(c["case"])), c, mine, audit=False)


# ---- find_traj: the single-candidate kernels, through the header's limits --------------------------------------------------
FIELD_CLASS = {"dds": ("acc", "s"), "ddds": ("jrk", "s"), "ddl": ("acc", "l"), "dddl": ("jrk", "l")}
_traj = {}


def oracle_find_traj(path, variant, params):
    """(status, x*, cubes, input) of a corridor file by the oracle: its corridor stage, its assembly, its exact solve."""
    inp = O.ParsedInput(path)
    n, cubes = O.pipeline(variant, inp)
    assert n >= 1
    x, _, info = O.AssembledQp(variant, cubes, params, inp).solve_exact()
    return int(info.status), x, cubes, inp


def find_traj_cases(name, variant, tmp):
    """Per header field and side: the input `name` with that limit at 0.6 of what the oracle's find_traj attains on the
    class's rows, written to a file of its own and solved by the oracle.  Once per (name, variant)."""
    from spectral_amd import knots
    if (name, variant) not in _traj:
        W = np.loadtxt(os.path.join(GOLD, "inputs", "weights.txt"))
        p = O.params_from_weights(W)
        src = os.path.join(GOLD, "inputs", name + ".txt")
        st, x, cubes, _ = oracle_find_traj(src, variant, p)
        assert st == 1
        S = len(cubes)
        out = []
        kb0 = knots.parse_corridor_file(src)
        for field, (cls, axis) in FIELD_CLASS.items():
            v = A.row_values(x, S, cls, axis)
            for side, e in ((0, v.min()), (1, v.max())):
                # (an extreme below 1e-6 of the file's own limit is rounding about 0 -- c2 keeps its lane --, not a value to tighten to)
                if abs(e) > 1e-6 * abs(kb0.header[field][side]) and ((e < 0) if side == 0 else (e > 0)):
                    kb = knots.parse_corridor_file(src)
                    lim = list(kb.header[field]); lim[side] = A.FACTOR * float(e)
                    kb.header = dict(kb.header); kb.header[field] = tuple(lim)
                    path = os.path.join(tmp, "%s_%d_%s_%d.txt" % (name, variant, field, side))
                    knots.write_corridor_file(path, kb)
                    st2, x2, cubes2, inp2 = oracle_find_traj(path, variant, p)
                    out.append(dict(field=field, side=side, limit=lim[side], kb=kb, status=st2, x=x2, cubes=cubes2, inp=inp2, path=path))
        _traj[(name, variant)] = (W, p, out)
    return _traj[(name, variant)]


@pytest.mark.parametrize("variant", [0, 1], ids=["trapezoid", "cuboid"])
@pytest.mark.parametrize("name", ["c1", "c2"])
@pytest.mark.parametrize("kernel", ["split", "packed"])
def test_find_traj(name, variant, kernel, tmp_path_factory, monkeypatch):
    """find_traj's single launch runs the split form up to 21 segments and the packed one beyond or with BTRAPZ_SPLIT=0
    (tests/test_gpu_split.py): both kernels, both variants.  In the strict mode (BTRAPZ_ACCEPT=reference): by default find_traj
    hands a stalled solve to the rescue pass, whose relaxed problem is another one (tests/test_gpu_acceptance.py) -- c2, cuboid,
    under dds[0] = 0.6 of the attained value is infeasible (the oracle's tight ADMM says so too) with a least violation of
    0.0014 |g|, inside the rescue's tolerance."""
    from spectral_amd import native
    W, p, cases = find_traj_cases(name, variant, str(tmp_path_factory.mktemp("active_rows")))
    params = native.CParams(*[float(v) for v in W], 7)
    monkeypatch.setenv("BTRAPZ_ACCEPT", "reference")
    if kernel == "packed":
        monkeypatch.setenv("BTRAPZ_SPLIT", "0")
    else:
        monkeypatch.delenv("BTRAPZ_SPLIT", raising=False)
    solved = active = 0
    for c in cases:
        what = "find_traj (%s) %s variant %d %s[%d] = %.6g" % (kernel, name, variant, c["field"], c["side"], c["limit"])
        cost, traj, ctrl = native.find_traj_mem(variant, params, c["kb"])
        assert (c["status"] > 0) == (cost != O.FAIL_SENTINEL), (what, c["status"], cost)
        if c["status"] != 1:
            print("%s: rejected by both" % what)
            continue
        x, S = c["x"], len(c["cubes"])
        scale = np.abs(x).max()
        e = np.abs(ctrl - x).max() / (RTOL * scale)
        assert e <= 1.0, (what, "ctrl", e)
        rc, samp = O.sample(c["cubes"], c["inp"].delta, x, c["inp"].init_s, c["inp"].init_l)
        assert rc == 0
        ref_cost = O.lib().orc_acost(variant, C.byref(p), C.byref(c["inp"].raw), len(samp[0]),
                                     *[np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_double)) for a in samp])
        ec = abs(cost - ref_cost) / (1e-6 * abs(ref_cost))
        assert ec <= 1.0, (what, "cost", cost, ref_cost)
        cls, axis = FIELD_CLASS[c["field"]]
        bound = A.ROW_L1[cls] * RTOL * scale
        ref_rows, got_rows = A.row_values(x, S, cls, axis), A.row_values(ctrl, S, cls, axis)
        at = np.abs(ref_rows - c["limit"]) <= 1e-7 * (1.0 + abs(c["limit"]))          # the rows the oracle's x* has on the limit
        er = np.abs(got_rows[at] - c["limit"]).max() / bound if at.any() else 0.0
        assert er <= 1.0, (what, "rows", er)
        solved += 1; active += bool(at.any())
        print("%s: %d rows on the limit; error / bound: ctrl %.3g cost %.3g rows %.3g" % (what, int(at.sum()), e, ec, er))
    assert solved >= 2 and active >= 2, (name, variant, solved, active)
