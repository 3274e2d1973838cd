"""The yardstick of the row audit (tests/row_check_reference.py) held to the oracle, without a GPU: on bundled inputs its
violations per class are AssembledQp.class_violations' (which classifies rows by their number of coefficients on the dense
A, where the yardstick goes by index on the sparse one), an exact solution passes the audit, and orc_assemble's rows come in
the order the audit numbers them."""
import os

import numpy as np
import pytest

from helpers import O, oracle_qp_from_batch
from spectral_amd import synth
import row_check_reference as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
W = np.loadtxt(os.path.join(GOLD, "inputs", "weights.txt"))
CASES = [("c1", 0), ("c1", 1), ("c2", 0), ("c2", 1), ("c_road_s1_3", 0), ("c_road_s1_3", 1), ("c7", 0)]


def solved(name, variant):
    """(qp, x, exact): the bundled input's QP and the oracle's exact solution, or -- where it has none -- the point its relaxed
    solve returns (c7 / trapezoid: the least-violation solution; c_road_s1_3 / cuboid, whose rows contradict each other by
    23 m: the point the relaxed solve hands back with status -3).  The exact solve runs to eps = 1e-13: the audit's tolerance
    is 64 units in the last place of the rows' magnitudes, and an interior-point iterate stopped at the default 1e-9 is not a
    solution to that precision (c2 / cuboid: a position row 65 tolerances outside, 0.7 at 1e-13)."""
    inp = O.ParsedInput(os.path.join(GOLD, "inputs", name + ".txt"))
    n, cubes = O.pipeline(variant, inp)
    assert n >= 1
    qp = O.AssembledQp(variant, cubes, O.params_from_weights(W), inp)
    x, _, info = qp.solve_exact(eps=1e-13, max_iter=200)
    if info.status == 1:
        return qp, x, True
    x, _, info, _ = qp.solve_elastic()
    assert np.isfinite(x).all()
    return qp, x, False


@pytest.mark.parametrize("name,variant", CASES)
def test_violations_per_class_are_the_oracles(name, variant):
    qp, x, exact = solved(name, variant)
    assert exact == ((name, variant) not in (("c7", 0), ("c_road_s1_3", 1)))      # (both kinds of solution are compared)
    ref = R.reference(qp, x, variant, unit=0)
    want = np.array(qp.class_violations(x))
    got = np.maximum(0.0, -ref["margin"]).max(axis=0)
    tol = ref["tol_margin"].max(axis=0)
    ratio = np.abs(got - want) / tol
    print("%s variant %d (%s solution): violations %s, |difference| / tolerance %s" % (name, variant, "exact" if exact else "relaxed", want, ratio))
    assert (ratio <= 1.0).all(), (got, want, tol)
    if not exact:
        assert want.max() > 1e-4              # (a relaxed solution that violates nothing would compare zeros)
    # the objective the yardstick computes from the sparse P is the dense one
    P, _ = qp.dense()
    assert abs(ref["obj"] - (0.5 * x @ P @ x + qp.q @ x)) <= ref["tol_obj"]
    for unit in (0, 1):                       # the worst row attains the margin, in either unit
        r = R.reference(qp, x, variant, unit=unit)
        for axis in (0, 1):
            for cls in range(4):
                w = r["worst"][axis, cls]
                assert w in r["rows"][axis][cls] and r["row_margin"][r["base"][axis] + w] == r["margin"][axis, cls]
    # unit 1 is unit 0 over the norms t, sqrt(50), sqrt(2400), sqrt(72000) of the worst row
    r1 = R.reference(qp, x, variant, unit=1)
    t = np.array([qp.cubes[k].t for k in range(qp.S)])
    for axis in (0, 1):
        for cls, nrm in enumerate((None, np.sqrt(50.0), np.sqrt(2400.0), np.sqrt(72000.0))):
            w = r1["worst"][axis, cls]
            n_ = t[w // 18] if cls == 0 else nrm
            assert abs(r1["margin"][axis, cls] - ref["row_margin"][ref["base"][axis] + w] / n_) <= 4 * 2.0 ** -53 * abs(r1["margin"][axis, cls])


@pytest.mark.parametrize("name,variant", [c for c in CASES if c not in (("c7", 0), ("c_road_s1_3", 1))])
def test_an_exact_solution_passes_the_audit(name, variant):
    qp, x, exact = solved(name, variant)
    assert exact
    ref = R.reference(qp, x, variant, unit=0)
    print("%s variant %d: smallest margin / tolerance %s, equality residuals / tolerance %s" % (
        name, variant, (ref["margin"] / ref["tol_margin"]).min(), (ref["eq_res"] / ref["tol_eq"]).ravel()))
    assert (ref["margin"] >= -ref["tol_margin"]).all(), (ref["margin"], ref["tol_margin"])
    assert (ref["eq_res"] <= ref["tol_eq"]).all(), (ref["eq_res"], ref["tol_eq"])


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 5, 65])
def test_rows_come_in_the_order_the_audit_numbers_them(S, variant):
    for make in (lambda: synth.make_batch(2, S, config=2, variant=variant, seed=40 + S), lambda: synth.make_scenario1_batch(2, S, variant=variant, seed=40 + S)):
        batch, sh = make()
        R.row_order_identities(oracle_qp_from_batch(batch, sh, 1))


def test_defined_cases_of_the_yardstick():
    """A side at 1e9 or beyond is dropped row by row; a class without a side left has margin +inf and no worst row; a NaN
    counts against the candidate."""
    batch, sh = synth.make_batch(2, 3, config=2, variant=0, seed=7)
    sh.ddds = (-1e10, 1e10)
    batch.seg[3, 0, 1] = 1e10                              # F_UPP_BIAS of segment 1: its upper line has one end at 1e10 ...
    batch.seg[4, 0, 1] = -(1e10 - 30.0)                    # ... and comes down to 30 at the other (F_UPP_SKEW, t = 1)
    qp = oracle_qp_from_batch(batch, sh, 0)
    x = R.constant_velocity_ctrl(batch, 0)
    ref = R.reference(qp, x, 0)
    assert np.isposinf(ref["margin"][0, 3]) and ref["worst"][0, 3] == -1 and np.isfinite(ref["margin"][1, 3])
    up = qp.u[18:24]
    assert up[0] >= 1e9 and abs(up[5] - 30.0) < 1e-5       # rows 18 .. 23: some sides dropped, the real end kept
    assert np.isfinite(ref["row_margin"][18 + 5]) and ref["row_margin"][18 + 5] == min(x[6 + 5] - qp.l[23], qp.u[23] - x[6 + 5])
    x[4] = np.nan
    bad = R.reference(qp, x, 0)
    assert np.isneginf(bad["margin"][0, :3]).all() and np.isposinf(bad["margin"][0, 3]) and np.isfinite(bad["margin"][1]).all()
