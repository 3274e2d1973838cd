"""btrapz_check_rows_device (BatchSolver.check_rows) held to the yardstick of tests/row_check_reference.py, row by row, at
every edge of its lane mapping: groups of seg_stride lanes (floor(64 / seg_stride) candidates per wavefront, a partial last
wavefront), one candidate per wavefront with strided lanes beyond 64 slots, ragged records, parameter sets, the defined
cases of the header, and the solve's own results.

Control points, per candidate b: b % 3 == 0 the initial state propagated at constant velocity plus N(0, 1e-3) noise;
b % 3 == 1 the same plus N(0, 1) noise (far outside its rows); b % 3 == 2 the solve's own output where the
candidate was solved (status 1 or 2), else the first kind.  No candidate of a compared batch is skipped.

Worst observed ratios of an error to its computed tolerance (printed by every test; one run on one MI355X): 0.071 at the lane
edges, 0.052 at 65 .. 256 segments, 0.030 on the ragged record of stride 130, 0.022 with bounds at 1e10."""
import itertools
import json
import os

import numpy as np
import pytest

from helpers import oracle_qp_from_batch
from spectral_amd import layout as L
from spectral_amd import synth
import row_check_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_SIZES = (1, 2, 3, 21, 22, 32, 33, 63, 64)
OUTPUTS = ("margin", "worst", "eq_res", "obj")


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def make(family, B, S, variant, seed):
    if family == "generic":
        return synth.make_batch(B, S, config=2, variant=variant, seed=seed)
    return synth.make_scenario1_batch(B, S, variant=variant, seed=seed)


def head(batch, B):
    """The first B candidates of a batch, as a batch of their own."""
    return L.Batch(B=B, S=batch.S, seg=batch.seg[:, :B].copy(), init=batch.init[:B].copy(), ref_end=batch.ref_end[:B].copy(),
                   dl_bounds=batch.dl_bounds[:B].copy())


def one(batch, b, n=None):
    """Candidate b alone, cut to its first n segments: the uniform problem a ragged record states for it."""
    n = batch.S if n is None else n
    return L.Batch(B=1, S=n, seg=np.ascontiguousarray(batch.seg[:, b:b + 1, :n]), init=batch.init[b:b + 1].copy(),
                   ref_end=batch.ref_end[b:b + 1].copy(), dl_bounds=batch.dl_bounds[b:b + 1].copy())


def to_np(o):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in o.items()}


def choose_ctrl(batch, solved, seed, counts=None):
    """[B, 12 S] by b % 3 (module docstring).  solved: the solve's result as numpy (ctrl, status), or None."""
    rng = np.random.default_rng(seed)
    B, S = batch.B, batch.S
    ctrl = np.zeros((B, 12 * S))
    for b in range(B):
        n = S if counts is None else int(counts[b])
        x = R.constant_velocity_ctrl(batch, b, n)
        kind = b % 3
        if kind == 2 and solved is not None and solved["status"][b] in (1, 2):
            x = solved["ctrl"][b, :12 * n].copy()
        else:
            x = x + rng.normal(0.0, 1.0 if kind == 1 else 1e-3, 12 * n)
        ctrl[b, :12 * n] = x
    return ctrl


def audit(solver, rec, sets, ctrl, unit=0, set_index=None, want=OUTPUTS):
    import torch
    c = torch.from_numpy(np.ascontiguousarray(ctrl)).to(solver.device)
    return to_np(solver.check_rows(rec, sets, c, set_index=set_index, unit=unit, want=want))


def of(got, b):
    return {k: v[b] for k, v in got.items()}


def same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    for k in a:
        x, y = np.ascontiguousarray(a[k][rows_a]), np.ascontiguousarray(b[k][rows_b])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def held_to_the_yardstick(batch, sh, got_by_unit, ctrl, what, counts=None, candidates=None):
    """Every candidate (or the listed ones) of got_by_unit = {unit: audit} against reference(); returns the worst ratio."""
    worst = 0.0
    for b in (range(batch.B) if candidates is None else candidates):
        n = batch.S if counts is None else int(counts[b])
        qp = oracle_qp_from_batch(one(batch, b, n), sh, 0)
        for unit, got in got_by_unit.items():
            worst = max(worst, R.compare(of(got, b), R.reference(qp, ctrl[b, :12 * n], sh.variant, unit), (what, "b", b, "unit", unit)))
    return worst


# ---- 1. lane edges --------------------------------------------------------------------------------------------------------
_edge = {}


def edge_case(solver, S, variant):
    """253 candidates of S segments (the first 253 of a batch of 256), their control points and both units' audits, once."""
    key = (S, variant)
    if key not in _edge:
        family = ("generic", "scenario1")[(EDGE_SIZES.index(S) + variant) % 2]
        big, sh = make(family, 256, S, variant, seed=900 + S)
        batch = head(big, 253)
        solved = to_np(solver.solve(solver.upload(batch), sh))
        ctrl = choose_ctrl(batch, solved, seed=S)
        got = {u: audit(solver, solver.upload(batch), sh, ctrl, unit=u) for u in (0, 1)}
        _edge[key] = (family, big, batch, sh, ctrl, got, int((np.isin(solved["status"], (1, 2)) & (np.arange(253) % 3 == 2)).sum()))
    return _edge[key]


@pytest.mark.parametrize("variant", [0, 1], ids=["trapezoid", "cuboid"])
@pytest.mark.parametrize("S", EDGE_SIZES)
def test_every_candidate_at_every_lane_edge(solver, S, variant):
    family, big, batch, sh, ctrl, got, n_solved = edge_case(solver, S, variant)
    worst = held_to_the_yardstick(batch, sh, got, ctrl, (family, S, variant))
    print("S = %d, %s, variant %d: 253 candidates (%d at the solve's own output), worst error / tolerance %.3f" % (S, family, variant, n_solved, worst))
    # unit 1 is no other set of rows: the same equality residuals and objective, bit for bit
    assert got[0]["eq_res"].tobytes() == got[1]["eq_res"].tobytes() and got[0]["obj"].tobytes() == got[1]["obj"].tobytes()


@pytest.mark.parametrize("variant", [0, 1], ids=["trapezoid", "cuboid"])
@pytest.mark.parametrize("S", EDGE_SIZES)
def test_a_neighbours_figures_fail_the_comparison(solver, S, variant):
    """The comparison is no formality: candidate b - 1's outputs held against candidate b's yardstick are refused, at the last
    group of the first wavefront, the first of the second and the partial last wavefront."""
    family, big, batch, sh, ctrl, got, _ = edge_case(solver, S, variant)
    gpw = 64 // S
    for b in sorted({gpw - 1, gpw, 252} - {0}):
        ref = R.reference(oracle_qp_from_batch(one(batch, b), sh, 0), ctrl[b], variant, 0)
        R.compare(of(got[0], b), ref, (S, b))
        with pytest.raises(AssertionError):
            R.compare(of(got[0], b - 1), ref, (S, b, "shifted"))


@pytest.mark.parametrize("variant", [0, 1], ids=["trapezoid", "cuboid"])
@pytest.mark.parametrize("S", EDGE_SIZES)
def test_a_candidates_bits_do_not_depend_on_the_batch_around_it(solver, S, variant):
    family, big, batch, sh, ctrl, got, _ = edge_case(solver, S, variant)
    ctrl256 = np.concatenate([ctrl, np.stack([R.constant_velocity_ctrl(big, b) for b in range(253, 256)])])
    for u in (0, 1):
        same_bits(got[u], audit(solver, solver.upload(big), sh, ctrl256, unit=u), slice(0, 253), slice(0, 253))


# ---- 2. beyond a wavefront ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,family,variant", [(65, "generic", 0), (65, "scenario1", 1), (130, "scenario1", 0), (130, "generic", 1),
                                              (256, "generic", 0), (256, "scenario1", 1)])
def test_more_segments_than_lanes(solver, S, family, variant):
    batch, sh = make(family, 5, S, variant, seed=900 + S)
    solved = to_np(solver.solve(solver.upload(batch), sh))
    ctrl = choose_ctrl(batch, solved, seed=S)
    got = {u: audit(solver, solver.upload(batch), sh, ctrl, unit=u) for u in (0, 1)}
    worst = held_to_the_yardstick(batch, sh, got, ctrl, (family, S, variant))
    print("S = %d, %s, variant %d: 5 candidates, status %s, worst error / tolerance %.3f" % (S, family, variant, solved["status"], worst))


# ---- 3. ragged ------------------------------------------------------------------------------------------------------------
def ragged(solver, batch, counts):
    """The ragged record of `batch` with the given counts (a candidate's unused slots read 0), on the device."""
    import torch
    seg = batch.seg.copy()
    seg[:, np.arange(batch.S)[None, :] >= np.asarray(counts)[:, None]] = 0.0
    t = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(solver.device)
    return dict(B=batch.B, seg_stride=batch.S, seg=t(seg), seg_count=t(counts, np.int32), init=t(batch.init), ref_end=t(batch.ref_end),
                dl_bounds=t(batch.dl_bounds))


@pytest.mark.parametrize("stride,family,variant", [(21, "generic", 0), (21, "scenario1", 1), (33, "scenario1", 0), (33, "generic", 1)])
def test_a_ragged_record_gives_the_uniform_calls_bits(solver, stride, family, variant):
    B = 2 * stride + 3
    batch, sh = make(family, B, stride, variant, seed=700 + stride)
    counts = 1 + np.arange(B) % stride
    rec = ragged(solver, batch, counts)
    solved = to_np(solver.solve_ragged(rec, sh))
    ctrl = choose_ctrl(batch, solved, seed=stride, counts=counts)
    for u in (0, 1):
        got = audit(solver, rec, sh, ctrl, unit=u)
        for n in range(1, stride + 1):
            idx = np.nonzero(counts == n)[0]
            sub = L.Batch(B=len(idx), S=n, seg=np.ascontiguousarray(batch.seg[:, idx, :n]), init=batch.init[idx], ref_end=batch.ref_end[idx],
                          dl_bounds=batch.dl_bounds[idx])
            same_bits(of(got, idx), audit(solver, solver.upload(sub), sh, ctrl[idx, :12 * n], unit=u))
    # (and the uniform call is the yardstick's: the lane-edge tests; here two candidates of the record itself)
    held_to_the_yardstick(batch, sh, {1: got}, ctrl, ("ragged", stride), counts=counts, candidates=(stride - 1, B - 1))


@pytest.mark.parametrize("family,variant", [("generic", 0), ("scenario1", 1)])
def test_a_ragged_record_beyond_a_wavefront(solver, family, variant):
    batch, sh = make(family, 5, 130, variant, seed=830)
    counts = np.array([1, 64, 65, 129, 130])
    rec = ragged(solver, batch, counts)
    solved = to_np(solver.solve_ragged(rec, sh))
    ctrl = choose_ctrl(batch, solved, seed=130, counts=counts)
    got = {u: audit(solver, rec, sh, ctrl, unit=u) for u in (0, 1)}
    worst = held_to_the_yardstick(batch, sh, got, ctrl, ("ragged", 130, family), counts=counts)
    print("stride 130, counts %s, %s: status %s, worst error / tolerance %.3f" % (counts, family, solved["status"], worst))


# ---- 4. sets --------------------------------------------------------------------------------------------------------------
def test_three_sets_in_one_call_are_three_calls(solver):
    import copy
    import torch
    B, S = 67, 21
    batch, sh = make("generic", B, S, 0, seed=41)
    sets = [sh, copy.deepcopy(sh), copy.deepcopy(sh)]
    sets[1].w_s = tuple(2.0 * v for v in sh.w_s); sets[1].dds = (-1.0, 1.5); sets[1].ddds = (-7.0, 9.0); sets[1].weight_end_l = 3.0
    sets[2].w_l = tuple(0.5 * v for v in sh.w_l); sets[2].ddl = (-0.3, 0.4); sets[2].dddl = (-4.0, 1e10); sets[2].ds_ref = 5.0
    index = (np.arange(B) % 3).astype(np.int32)
    ctrl = choose_ctrl(batch, None, seed=5)
    db = solver.upload(batch)
    t = lambda a: torch.from_numpy(a).to(solver.device)
    for u in (0, 1):
        got = audit(solver, db, sets, ctrl, unit=u, set_index=t(index))
        for j in range(3):
            alone = audit(solver, db, [sets[j]], ctrl, unit=u)
            same_bits(of(got, index == j), of(alone, index == j))
        assert not np.array_equal(got["margin"][index == 1][:, 0, 2], audit(solver, db, [sets[0]], ctrl, unit=u)["margin"][index == 1][:, 0, 2])
    # a set that is none: the defined values, and the neighbours' bits as before
    out = index.copy(); out[[0, 22, 66]] = (-1, 3, 1 << 20)
    bad = audit(solver, db, sets, ctrl, unit=0, set_index=t(out))
    good = audit(solver, db, sets, ctrl, unit=0, set_index=t(index))
    keep = np.ones(B, dtype=bool); keep[[0, 22, 66]] = False
    same_bits(of(bad, keep), of(good, keep))
    defined_as_no_candidate(of(bad, ~keep))
    qp = oracle_qp_from_batch(one(batch, 1), sets[1], 0)       # (and a candidate of another set than the first is the yardstick's)
    R.compare(of(good, 1), R.reference(qp, ctrl[1], 0, 0), "set 1")


# ---- 5. defined cases -----------------------------------------------------------------------------------------------------
def defined_as_no_candidate(got):
    assert np.isneginf(got["margin"]).all() and (got["worst"] == -1).all() and np.isposinf(got["eq_res"]).all() and np.isposinf(got["obj"]).all()


def test_limits_that_are_none_and_a_line_with_one_far_end(solver):
    B, S = 13, 5
    for variant in (0, 1):
        batch, sh = make("generic", B, S, variant, seed=77)
        sh.ddds = (-1e10, 1e10); sh.dddl = (-1e10, 1e10)
        # the upper s line of segment 2 of every second candidate: 1e10 at its start, the old value at its end
        end = batch.seg[L.F_UPP_BIAS, ::2, 2] + batch.seg[L.F_UPP_SKEW, ::2, 2] * batch.seg[L.F_T, ::2, 2]
        batch.seg[L.F_UPP_BIAS, ::2, 2] = 1e10
        batch.seg[L.F_UPP_SKEW, ::2, 2] = -(1e10 - end) / batch.seg[L.F_T, ::2, 2]
        ctrl = choose_ctrl(batch, None, seed=9)
        got = {u: audit(solver, solver.upload(batch), sh, ctrl, unit=u) for u in (0, 1)}
        for u in (0, 1):
            assert np.isposinf(got[u]["margin"][:, :, 3]).all() and (got[u]["worst"][:, :, 3] == -1).all()
        worst = held_to_the_yardstick(batch, sh, got, ctrl, ("far", variant))
        qp = oracle_qp_from_batch(one(batch, 0), sh, 0)
        assert variant == 1 or (qp.u[36] >= 1e9 and abs(qp.u[41] - end[0]) < 1e-4)     # (rows 36 .. 41: the line's two ends)
        print("variant %d: jerk limits and one end of a line at 1e10, worst error / tolerance %.3f" % (variant, worst))


def test_what_is_no_candidate(solver):
    import torch
    B, S = 11, 6
    batch, sh = make("scenario1", B, S, 0, seed=78)
    ctrl = choose_ctrl(batch, None, seed=10)
    db = solver.upload(batch)
    clean = audit(solver, db, sh, ctrl)
    # one NaN, one +inf control point (the last of the l axis, the first of the s axis)
    damaged = ctrl.copy(); damaged[3, 12 * S - 1] = np.nan; damaged[7, 0] = np.inf
    got = audit(solver, db, sh, damaged)
    keep = np.ones(B, dtype=bool); keep[[3, 7]] = False
    defined_as_no_candidate(of(got, ~keep)); same_bits(of(got, keep), of(clean, keep))
    assert not solver.admissible({k: torch.from_numpy(v) for k, v in got.items()}, 1e300, 1e300)[[3, 7]].any()
    # a duration that is none, in a used segment
    b2 = head(batch, B); b2.seg[L.F_T, 2, S - 1] = 0.0; b2.seg[L.F_T, 5, 0] = -1.0; b2.seg[L.F_T, 10, 3] = np.nan
    got = audit(solver, solver.upload(b2), sh, ctrl)
    keep = np.ones(B, dtype=bool); keep[[2, 5, 10]] = False
    defined_as_no_candidate(of(got, ~keep)); same_bits(of(got, keep), of(clean, keep))
    # counts outside 1 .. stride; the others as the uniform call has them
    counts = np.full(B, S); counts[[1, 4, 9]] = (0, S + 1, -3)
    got = audit(solver, ragged(solver, batch, np.clip(counts, 0, S)) | dict(seg_count=torch.from_numpy(counts.astype(np.int32)).to(solver.device)), sh, ctrl)
    keep = np.ones(B, dtype=bool); keep[[1, 4, 9]] = False
    defined_as_no_candidate(of(got, ~keep)); same_bits(of(got, keep), of(clean, keep))


def test_every_subset_of_outputs_leaves_the_others_bits(solver):
    batch, sh = make("generic", 37, 7, 1, seed=79)
    ctrl = choose_ctrl(batch, None, seed=11)
    db = solver.upload(batch)
    for u in (0, 1):
        full = audit(solver, db, sh, ctrl, unit=u)
        for r in range(1, 4):
            for want in itertools.combinations(OUTPUTS, r):
                part = audit(solver, db, sh, ctrl, unit=u, want=want)
                assert set(part) == set(want)
                same_bits(part, {k: full[k] for k in want})


def test_refusals(solver):
    import copy
    import torch
    from spectral_amd.native import BtrapzError
    batch, sh = make("generic", 4, 3, 0, seed=80)
    db = solver.upload(batch)
    cub = copy.deepcopy(sh); cub.variant = 1
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=solver.device)
    outs = lambda B: dict(margin=z(B, 2, 4), worst=z(B, 2, 4, dt=torch.int32), eq_res=z(B, 2, 2), obj=z(B))

    def call(B=4, stride=3, sets=(sh,), ctrl=None, **o):
        solver.ctx.check_rows_device(B, stride, list(sets), None, db.seg, None, db.init, db.ref_end, db.dl_bounds,
                                     z(4, 12 * 3) if ctrl is None else ctrl, **o)
    for kw, word in ((dict(stride=0), "seg_stride"), (dict(stride=257), "seg_stride"), (dict(B=-1), "B >= 0"),
                     (dict(sets=(sh, cub)), "variant"), (dict(sets=()), "n_sets")):
        with pytest.raises(BtrapzError, match=word):
            call(**kw, **outs(4))
    with pytest.raises(BtrapzError, match="at least one output"):
        call()
    with pytest.raises(BtrapzError, match="unit"):
        call(unit=2, **outs(4))
    call(B=0, **outs(4))                                            # nothing to audit: no error, nothing written
    o = outs(4); o["obj"] += 7.0
    call(B=0, **o); torch.cuda.synchronize()
    assert (o["obj"] == 7.0).all()
    with pytest.raises(ValueError):
        solver.check_rows(db, sh, z(4, 12 * 3), want=("margin", "slack"))
    with pytest.raises(ValueError):
        solver.check_rows(db, sh, z(4, 12 * 4))


# ---- 6. against the solve -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1], ids=["config 3 (trapezoid)", "config 4 (cuboid)"])
def test_the_solves_own_results_are_admissible(solver, variant):
    """253 x 20 scenario_1 candidates -- the first 253 of the batch tools/check_rows_bench.py audits --, cold solve.  The
    tolerances of `admissible` are the figures that tool reported for the solve's accepted results on the whole batch
    (profiles/check_rows_bench.json: worst margin over the classes in unit 1, worst equality residual)."""
    import torch
    import bench
    big, sh = bench.make_workload("scenario1", 65536, 20, variant, 0)
    batch = head(big, 253)
    db = solver.upload(batch)
    o = solver.solve(db, sh)
    solved = to_np(o)
    ok = np.isin(solved["status"], (1, 2))
    assert ok.sum() >= 150 and np.isfinite(solved["ctrl"][ok]).all()
    got = solver.check_rows(db, sh, o["ctrl"], unit=1)
    g = to_np(got)
    err = np.abs(g["obj"][ok] - solved["cost"][ok]) / (1e-6 * (1.0 + np.abs(solved["cost"][ok])))
    rep = json.load(open(os.path.join(ROOT, "profiles", "check_rows_bench.json")))["accepted_results"][str(variant)]
    tol_rows, tol_eq = rep["tol_rows_unit1"], rep["tol_eq"]
    print("variant %d: %d of 253 solved; |obj - cost| / tolerance %.3g; worst margin (unit 1) %.3g against -%.3g, worst equality residual %.3g against %.3g"
          % (variant, ok.sum(), err.max(), g["margin"][ok].min(), tol_rows, g["eq_res"][ok].max(), tol_eq))
    assert (err <= 1.0).all()
    adm = solver.admissible(got, tol_rows, tol_eq).cpu().numpy()
    assert adm[ok].all(), np.nonzero(ok & ~adm)[0][:8]
    # the same plans with N(0, 1) noise on them are not
    rng = np.random.default_rng(6)
    noisy = np.stack([R.constant_velocity_ctrl(batch, b) for b in range(253)]) + rng.normal(0.0, 1.0, (253, 240))
    bad = solver.check_rows(db, sh, torch.from_numpy(noisy).to(solver.device), unit=1)
    assert not solver.admissible(bad, tol_rows, tol_eq).cpu().numpy().any()
