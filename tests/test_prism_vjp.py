"""The backward pass of the prism stage on the host (btrapz_prism_bounds_vjp_host, the twin of the device kernel: same
statements, same order of the sums) against the yardstick of tests/prism_vjp_reference.py, the yardstick's own map against
the oracle, and the defined cases against hand-computed expectations (tests/prism_vjp_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import prism_vjp_cases as K
import prism_vjp_reference as R
from oracle import prism_oracle as PO
from spectral_amd import native

SETS = K.scene_sets()


def jacobians(name):
    pr, N, O = SETS[name]
    return [R.jacobian(pr[b], N, key=(name, b)) for b in range(pr.shape[0])]


@pytest.mark.parametrize("name", sorted(SETS))
def test_the_yardsticks_map_is_the_forwards(name):
    """Unrounded s bounds within 0.005 (+ 1 ulp) of the oracle's rounded ones, l edges bit-equal, on every scene used; and the
    yardstick alone stays inside the cap on skipped columns."""
    pr, N, O = SETS[name]
    jacs = jacobians(name)
    for b, jac in enumerate(jacs):
        want = PO.prism_bounds(R.active_cars(pr[b]), N)
        assert jac["strips"] == len(want) <= O, (b, jac["strips"], len(want))
        for j, (ws, wl) in enumerate(want):
            assert np.array_equal(jac["l"][j], np.array(wl)), (b, j)
            ws = np.array(ws)
            assert (np.abs(jac["s"][j] - ws) <= 0.005 + np.spacing(np.abs(ws))).all(), (b, j, np.abs(jac["s"][j] - ws).max())
    print("skipped columns / columns:", R.check_cap(jacs))


@pytest.mark.parametrize("name", sorted(SETS))
def test_host_twin_against_yardstick(name):
    pr, N, O = SETS[name]
    jacs = jacobians(name)
    R.check_cap(jacs)
    sbar, lbar = K.cotangents(pr.shape[0], O, N)
    got = native.prism_bounds_vjp_host(pr, N, O, sbar, lbar)
    assert not np.isnan(got).any()
    worst, nonzero = 0.0, 0
    for b, jac in enumerate(jacs):
        worst = max(worst, R.compare(jac, got[b], sbar[b], lbar[b], O, (name, b)))
        nonzero += int((got[b] != 0).sum())
    assert nonzero >= 3 * pr.shape[0]
    print("worst error / tolerance:", worst)


def test_host_twin_sixteen_cars():
    """33 strips: O = 33 and O = 34 (one padding strip) against the yardstick, O = 32 zeros."""
    pr = K.pack(K.sixteen_cars(), 16)
    N = 65
    jacs = [R.jacobian(pr[b], N, key=("sixteen", b)) for b in range(pr.shape[0])]
    assert all(j["strips"] == 33 for j in jacs)
    R.check_cap(jacs)
    for O in (33, 34):
        sbar, lbar = K.cotangents(pr.shape[0], O, N, seed=O)
        got = native.prism_bounds_vjp_host(pr, N, O, sbar, lbar)
        print("O", O, "worst error / tolerance:", max(R.compare(jac, got[b], sbar[b], lbar[b], O, (O, b)) for b, jac in enumerate(jacs)))
        assert (got[:, :, 1] != 0).all()
    sbar, lbar = K.cotangents(pr.shape[0], 32, N)
    assert not native.prism_bounds_vjp_host(pr, N, 32, sbar, lbar).any()


@pytest.mark.parametrize("case", K.defined_cases(), ids=lambda c: c[0])
def test_defined_cases(case):
    name, pr, N, O, sbar, lbar, expected = case
    K.check_defined(name, native.prism_bounds_vjp_host(pr, N, O, sbar, lbar), expected)


def test_host_refusals():
    pr = K.pack(K.random_scenes(2, 1), 4)
    sbar, lbar = K.cotangents(2, 9, 71)
    ok = native.prism_bounds_vjp_host(pr, 71, 9, sbar, lbar)
    assert ok.shape == (2, 4, 8)
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_vjp_host(pr, 71, 9, None, None)
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_vjp_host(np.zeros((1, 17, 8)), 71, 9, np.zeros((1, 9, 71, 2)), None)
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_vjp_host(np.zeros((0, 4, 8)), 71, 9, np.zeros((0, 9, 71, 2)), None)
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_vjp_host(np.zeros((1, 0, 8)), 71, 9, np.zeros((1, 9, 71, 2)), None)
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_vjp_host(pr, 0, 9, np.zeros((2, 9, 0, 2)), None)
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_vjp_host(pr, 71, 0, np.zeros((2, 0, 71, 2)), None)
    road = native.CRoad.reference(); road.knots_per_second = 0.0
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_vjp_host(pr, 71, 9, sbar, lbar, road=road)
    # null prisms, road, prisms_bar: straight at the C-ABI
    f = native.lib().btrapz_prism_bounds_vjp_host
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros((2, 4, 8)); road = native.CRoad.reference()
    assert f(2, 4, 71, C.byref(road), p(pr), 9, p(sbar), p(lbar), p(out)) == 0
    assert f(2, 4, 71, None, p(pr), 9, p(sbar), p(lbar), p(out)) == -1
    assert f(2, 4, 71, C.byref(road), None, 9, p(sbar), p(lbar), p(out)) == -1
    assert f(2, 4, 71, C.byref(road), p(pr), 9, p(sbar), p(lbar), None) == -1
