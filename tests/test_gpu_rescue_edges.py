"""The rescue pass (btrapz_options.elastic = 1) and the all-elastic solve (elastic = 2) at every edge of the lane mapping,
held to the oracle's relaxed solve (AssembledQp.solve_elastic): one segment per group, the last lane of a group next to
another group's first, idle tail lanes (S = 5, 21), one group per wavefront (S >= 33), a group ending on lane 62 / 63, and the
three wavefronts per problem of the long form's rescue kernel (130 segments).  Elsewhere the relaxed problem is compared at 10
and 20 segments, the bundled c7 family and two fuzz finds of 65 and 76 segments (test_gpu_forms.py, test_gpu_acceptance.py,
test_gpu_long.py).

Candidates: copies of feasible candidates of synth.make_batch(..., config=2, seed=500 + S), damaged in one of two ways.
  initial state outside   init l0 = the first segment's lower l line at its start, minus `gap`: the position row of the first
                          control point (which the initial-state equality fixes) is violated by `gap`, |g| = t = 1.
  last joint, s axis      (S >= 5) the last segment's lower s line starts `gap` above the end of the previous segment's upper
                          line; continuity makes both rows speak of one point, so each is violated by gap / 2.
Gaps are chosen on both sides of the product's default tolerance (elastic_tol of tests/golden/acceptance_table.json, 0.0125):
0.004 / 0.030 and 0.008 / 0.060 give least violations of 0.004 and 0.030.  The oracle alone decides what every compared
candidate is (exact solve: feasible or not; relaxed solve: least violation), and the test asserts of its own inputs that
every S holds a candidate of each kind with a clear margin.  Replaces the acceptance test of src/solve_3d.cc:1251-1277 for
candidate sets."""
import copy
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from helpers import O, oracle_qp_from_batch
from spectral_amd import layout as L
from spectral_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = json.load(open(os.path.join(GOLD, "acceptance_table.json")))["elastic_tol"]
SIZES = (1, 2, 3, 5, 21, 32, 33, 63, 64)
GAPS_INIT = (0.004, 0.030)
GAPS_JOINT = (0.008, 0.060)
BAND = 1e-4     # a least violation this close to the tolerance decides nothing (the violation itself is held to 1e-5)


def batch_size(S):
    """Several wavefronts, the last one partial (64 // S groups per wavefront up to 32 segments, one beyond)."""
    return 3 * (64 // S) + 1 if S <= 32 else 7


def outside_initial_state(batch, b, gap):
    batch.init[b, 3] = batch.seg[L.F_L_DOWN_BIAS, b, 0] - gap


def conflict_at_last_joint(batch, b, gap):
    s = batch.seg
    k = batch.S - 1
    t = s[L.F_T, b, k]
    s[L.F_DOWN_BIAS, b, k] = s[L.F_UPP_BIAS, b, k - 1] + s[L.F_UPP_SKEW, b, k - 1] * s[L.F_T, b, k - 1] + gap
    room = s[L.F_DOWN_BIAS, b, k] + 5.0 + max(0.0, (s[L.F_DOWN_SKEW, b, k] - s[L.F_UPP_SKEW, b, k]) * t)
    s[L.F_UPP_BIAS, b, k] = max(s[L.F_UPP_BIAS, b, k], room)


def damaged_batch(S, B):
    """(batch, sh, damaged): the generic batch with the constructions applied at positions spread over the wavefronts -- among
    them the last candidate (the partial wavefront) and the last group of the first wavefront."""
    batch, sh = synth.make_batch(B, S, config=2, seed=500 + S)
    batch = L.Batch(B=B, S=S, seg=batch.seg.copy(), init=batch.init.copy(), ref_end=batch.ref_end.copy(), dl_bounds=batch.dl_bounds.copy())
    gpw = 64 // S if S <= 32 else 1
    kinds = [(outside_initial_state, g) for g in GAPS_INIT] + ([(conflict_at_last_joint, g) for g in GAPS_JOINT] if S >= 5 else [])
    places = [gpw - 1, B - 1, gpw + 1, 2 * gpw] if B > 7 else [0, B - 1, 2, 4]
    assert len(set(places)) == 4 and max(places) < B
    damaged = {}
    for (fn, gap), b in zip(kinds, places):
        fn(batch, b, gap)
        damaged[b] = (fn.__name__, gap)
    return batch, sh, damaged


def row_violation(qp, A, x):
    """Largest violation of an inequality row by x in the row's own norm |g|, as test_gpu_acceptance.py computes it."""
    Ax = A @ x
    ineq = (qp.u - qp.l) > 1e-12
    return float((np.abs(Ax - np.clip(Ax, qp.l, qp.u))[ineq] / np.linalg.norm(A[ineq], axis=1)).max())


def relaxed(batch, sh, b):
    qp = oracle_qp_from_batch(batch, sh, b)
    x, _, info, viol = qp.solve_elastic()
    return dict(x=x, viol=viol, status=int(info.status), qp=qp)


_verdicts = {}


def verdicts(S):
    """The oracle's word on the compared candidates of damaged_batch(S): every damaged one and two untouched ones.  b -> dict
    (feasible: the exact solve's x*; else the relaxed solve's x, its least violation and the QP).  Once per S."""
    if S not in _verdicts:
        B = batch_size(S)
        batch, sh, damaged = damaged_batch(S, B)
        clean = [b for b in range(B) if b not in damaged][:2]
        out = {}

        def verdict(b):
            # a damaged candidate: the relaxed solve's least violation says whether it has a solution (the exact solve
            # spends its whole iteration budget on one that has none: 10 s at 64 segments); a clean one must have one
            if b in damaged:
                r = relaxed(batch, sh, b)
                assert r["status"] in (1, 2), (S, b, r["status"])
                if r["viol"] > 1e-7:
                    return dict(feasible=False, **r)
            x, _, info = oracle_qp_from_batch(batch, sh, b).solve_exact()
            assert info.status == 1, (S, b, info.status)
            return dict(feasible=True, x=x)
        pick = clean + sorted(damaged)
        with ThreadPoolExecutor(max_workers=len(pick)) as pool:          # (the C solver runs outside the interpreter's lock)
            out = dict(zip(pick, pool.map(verdict, pick)))
        # the batch checks something only if it holds all three kinds, each clear of the tolerance
        viols = [v["viol"] for v in out.values() if not v["feasible"]]
        assert any(v <= TOL - 0.002 for v in viols) and any(v >= TOL + 0.005 for v in viols), (S, viols)
        assert sum(v["feasible"] for v in out.values()) >= 1
        _verdicts[S] = (batch, sh, damaged, out)
    return _verdicts[S]


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def run(solver, db, sh, **kw):
    import torch
    o = solver.solve(db, sh, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in o.items()}, solver.ctx.last_solve_form()


def check_decisions(S, r, out, relaxed_x):
    """Rescued: status 2 (elastic = 2: accepted), the oracle's relaxed x to 1e-4 and its least violation to 1e-5 where
    relaxed_x; rejected: a negative status and an infinite cost."""
    for b, v in out.items():
        if v["feasible"]:
            continue
        if v["viol"] <= TOL - BAND:
            assert r["status"][b] == 2 and np.isfinite(r["cost"][b]), (S, b, r["status"][b], v["viol"])
            if relaxed_x:
                got = r["ctrl"][b]
                err = np.abs(got - v["x"]).max() / np.abs(v["x"]).max()
                A = v["qp"].dense()[1]
                dv = abs(row_violation(v["qp"], A, got) - v["viol"])
                print("S=%d b=%d least violation %.6f: |ctrl - x| / |x| = %.2e, violation differs by %.2e" % (S, b, v["viol"], err, dv))
                assert err <= 1e-4, (S, b, err)
                assert dv <= 1e-5, (S, b, dv)
        elif v["viol"] >= TOL + BAND:
            assert r["status"][b] < 0 and np.isposinf(r["cost"][b]), (S, b, r["status"][b], r["cost"][b], v["viol"])


@pytest.mark.parametrize("lean", [-1, 1])
@pytest.mark.parametrize("S", SIZES)
def test_rescue_pass_and_elastic_solve_at_every_width(solver, S, lean):
    batch, sh, damaged, out = verdicts(S)
    db = solver.upload(batch)
    kw = dict(lean=lean, cap_iter=-1, split=-1)
    plain, form = run(solver, db, sh, **kw)
    assert form == (8 if lean > 0 and S >= 3 else 0)
    ok = plain["status"] > 0
    for b, v in out.items():          # the plain solve and the oracle's exact solve agree on what has a solution ...
        assert ok[b] == v["feasible"], (S, b, plain["status"][b])
        if v["feasible"]:             # ... and on the solution
            assert np.abs(plain["ctrl"][b] - v["x"]).max() <= 1e-5 * np.abs(v["x"]).max(), (S, b)
    assert ok.sum() >= batch.B - len(damaged)
    resc, form1 = run(solver, db, sh, elastic=1, **kw)
    assert form1 == form
    # candidates the plain solve answered are not touched
    assert np.array_equal(resc["status"][ok], plain["status"][ok])
    assert np.array_equal(resc["ctrl"][ok], plain["ctrl"][ok]) and np.array_equal(resc["cost"][ok], plain["cost"][ok])
    check_decisions(S, resc, out, relaxed_x=True)
    every, _ = run(solver, db, sh, elastic=2, **kw)
    check_decisions(S, every, out, relaxed_x=False)
    assert (every["status"][ok] > 0).all()
    scale = np.abs(plain["ctrl"][ok]).max(axis=1, keepdims=True)
    assert (np.abs(every["ctrl"][ok] - plain["ctrl"][ok]) <= 1e-4 * scale).all(), (S, (np.abs(every["ctrl"][ok] - plain["ctrl"][ok]) / scale).max())


def test_rescue_pass_of_the_long_form_in_its_third_wavefront(solver):
    """130 segments: three wavefronts per problem in ipm_solve_long_elastic_kernel, and the damaged joint is the last one --
    lanes 0 / 1 of the third wavefront.  The oracle's exact solve of an infeasible problem of this size takes minutes, so
    "no solution" is the plain GPU solve's status; the relaxed solve is the oracle's."""
    S = 130
    batch, sh = synth.make_batch(3, S, config=2, seed=500 + S)
    batch = L.Batch(B=3, S=S, seg=batch.seg.copy(), init=batch.init.copy(), ref_end=batch.ref_end.copy(), dl_bounds=batch.dl_bounds.copy())
    conflict_at_last_joint(batch, 1, GAPS_JOINT[0])
    conflict_at_last_joint(batch, 2, GAPS_JOINT[1])
    db = solver.upload(batch)
    plain, form = run(solver, db, sh)
    assert form == 2
    assert plain["status"][0] > 0 and (plain["status"][1:] < 0).all(), plain["status"]
    resc, form = run(solver, db, sh, elastic=1)
    assert form == 2
    assert resc["status"][0] == plain["status"][0] and resc["cost"][0] == plain["cost"][0] and np.array_equal(resc["ctrl"][0], plain["ctrl"][0])
    with ThreadPoolExecutor(max_workers=2) as pool:
        out = dict(zip((1, 2), pool.map(lambda b: relaxed(batch, sh, b), (1, 2))))
    assert out[1]["viol"] <= TOL - 0.002 and out[2]["viol"] >= TOL + 0.005, (out[1]["viol"], out[2]["viol"])
    check_decisions(S, resc, {b: dict(feasible=False, **v) for b, v in out.items()}, relaxed_x=True)
