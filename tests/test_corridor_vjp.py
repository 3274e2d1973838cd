"""The backward pass of the corridor stage on the host (btrapz_corridor_vjp_host, the twin of the device kernel: same
decisions, same per-segment adjoint) against the yardstick of tests/corridor_vjp_reference.py, and its defined cases."""
import numpy as np
import pytest

import corridor_vjp_cases as K
import corridor_vjp_reference as R
from spectral_amd import layout as L, native


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", ["scenario", "c1"])
def test_host_twin_against_yardstick(name, variant):
    kb = K.scenario(2) if name == "scenario" else K.c1(2)
    b = 0 if name == "scenario" else 1
    jac = R.jacobian(kb, b, variant, key=(name, 2, b, variant))
    assert jac["n"] >= 1 and R.check_caps(jac) >= 15
    sb, rb, db = K.cotangents(kb.B)
    g, count = K.host_grads(kb, b, variant, sb, rb, db)
    assert count == jac["n"]
    worst = R.compare(jac, g, R.flat_cotangent(jac["n"], sb[:, b], rb[b], db[b]), (name, variant))
    print("worst error / tolerance:", worst)


def test_host_twin_beyond_16_segments_with_a_moved_span():
    """Provenance through std::sort's order beyond 16 segments (the introsort branch), reorder and overlap."""
    kb = K.tied(K.TIED_SEED)
    jac = R.jacobian(kb, 0, 0, key=("tied", K.TIED_SEED, 0, 0))
    (n, spans, _), _ = R.record(R.one_candidate(kb, 0), 0)
    assert 16 < n <= 26 and R.check_caps(jac) >= 15 and K.moved_spans(jac, spans, kb.N, kb.delta)
    sb, rb, db = K.cotangents(kb.B, seed=7, seg_stride=K.TIED_STRIDE)
    g, count = K.host_grads(kb, 0, 0, sb, rb, db, seg_stride=K.TIED_STRIDE)
    assert count == n
    print("worst error / tolerance:", R.compare(jac, g, R.flat_cotangent(n, sb[:, 0], rb[0], db[0]), "tied"))


def test_ds_tie_and_default_rules():
    kb = K.scenario(1)
    dec, _ = R.record(R.one_candidate(kb, 0), 0)
    n, spans, _ = dec
    sb = np.zeros((L.NUM_SEG_FIELDS, 1, K.SEG_STRIDE)); sb[L.F_DS_LO, 0, :n] = 1.0 + np.arange(n); sb[L.F_DS_HI, 0, :n] = -1.0 - np.arange(n)
    # a plateau: every knot of a span attains the extreme -> the earliest knot of the span gets it
    kb.ds_bounds[0, :, 0] = 0.5; kb.ds_bounds[0, :, 1] = 7.0
    g, count = K.host_grads(kb, 0, 0, sb, None, None, want=("ds_bounds",))
    assert count == n
    want = np.zeros((kb.N, 2))
    for k, (bt, et) in enumerate(spans):
        want[min(max(bt, 0), kb.N - 1), 0] += 1.0 + k; want[min(max(bt, 0), kb.N - 1), 1] += -1.0 - k
    assert np.array_equal(g["ds_bounds"], want)
    # the defaults attain the extremes (no lower bound above 0, no upper bound below 1000): nobody gets the gradient
    kb.ds_bounds[0, :, 0] = 0.0; kb.ds_bounds[0, :, 1] = 1000.0
    g, _ = K.host_grads(kb, 0, 0, sb, None, None, want=("ds_bounds",))
    assert not g["ds_bounds"].any()
    kb.ds_bounds[0, :, 0] = -1.0; kb.ds_bounds[0, :, 1] = 2000.0
    g, _ = K.host_grads(kb, 0, 0, sb, None, None, want=("ds_bounds",))
    assert not g["ds_bounds"].any()


def test_cuboid_l_lines_get_no_gradient():
    kb = K.scenario(1)
    sb = np.zeros((L.NUM_SEG_FIELDS, 1, K.SEG_STRIDE))
    for f in (L.F_L_DOWN_BIAS, L.F_L_DOWN_SKEW, L.F_L_UPP_BIAS, L.F_L_UPP_SKEW):
        sb[f] = 1.0
    g1, n1 = K.host_grads(kb, 0, 1, sb, None, None)
    assert n1 >= 1 and all(not v.any() for v in g1.values())
    g0, n0 = K.host_grads(kb, 0, 0, sb, None, None)
    assert n0 >= 1 and g0["l_bounds"].any()


def test_slots_beyond_count_and_field_0_are_ignored():
    kb = K.c1(1)
    sb, rb, db = K.cotangents(1)
    g, n = K.host_grads(kb, 0, 0, sb, rb, db)
    sb2 = sb.copy(); sb2[:, :, n:] = 1e30; sb2[0] = -1e30
    g2, _ = K.host_grads(kb, 0, 0, sb2, rb, db)
    assert 1 <= n < K.SEG_STRIDE and all(np.array_equal(g[k], g2[k]) for k in g)


def test_host_refusals():
    kb = K.scenario(1)
    sb, rb, db = K.cotangents(1)
    with pytest.raises(native.BtrapzError):
        K.host_grads(kb, 0, 0, None, None, None)
    with pytest.raises(native.BtrapzError):
        K.host_grads(kb, 0, 0, sb, rb, db, want=())
