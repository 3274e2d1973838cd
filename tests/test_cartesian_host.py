"""btrapz_cartesian_host, _vjp_host and _jvp_host (include/btrapz_hip_cartesian.h) through ctypes, without a GPU: held to
the yardstick (tests/cartesian_reference.py) within its bound on values and on both derivatives, to the adjoint identity
between the two derivatives, to every defined case of the header bit by bit (outputs prefilled with a sentinel where
nothing may be written), and to NumPy reductions of their own cart for the audit."""
import math

import numpy as np
import pytest

import cartesian_cases as cc
import cartesian_reference as cr
from spectral_amd import native, synth
from spectral_amd.native import FRENET_SAMPLES, FRENET_STATES


@pytest.fixture(scope="module", autouse=True)
def built():
    native.build()
    return native.lib()


def shaped(f, layout):
    return f if layout == FRENET_SAMPLES else cc.to_states(f)


def unshaped(x, layout):
    return x if layout == FRENET_SAMPLES else cc.from_states(x)


# (R, n, M, lines, count kind): the kernel's edges too, so that host and device are held to the same cases
CASES = [(1, 1, 2, 1, None), (3, 63, 3, 1, None), (2, 65, 65, 2, "mixed"), (3, 130, 1000, 3, "mixed")]


def options(R, n, n_lines, kind, seed):
    rng = np.random.default_rng(seed)
    count = None if kind is None else np.array([[n, n // 2, 0, n + 7, 1][r % 5] for r in range(R)], dtype=np.int32)
    index = None if n_lines == 1 else np.array([r % n_lines for r in range(R)], dtype=np.int32)
    return rng, count, index


@pytest.mark.parametrize("layout", [FRENET_SAMPLES, FRENET_STATES])
@pytest.mark.parametrize("R,n,M,n_lines,kind", CASES)
def test_values_and_both_derivatives_within_the_bound_of_the_yardstick(R, n, M, n_lines, kind, layout):
    rl = cc.make_lines(M, n_lines)
    rng, count, index = options(R, n, n_lines, kind, 11)
    f, planted = cc.make_samples(100 + R + n, R, n, rl, line_index=index, kinds=cc.KINDS + ("beyond",), count=count)
    must = cc.must_check(planted)
    assert R * n < 100 or (len(must) >= 9 and all(planted[k] for k in ("table", "first", "last")))
    before = np.full((R, 6, n), cc.SENTINEL)
    cart = native.cartesian_host(shaped(f, layout), rl, layout=layout, count=count, line_index=index, want=("cart",),
                                 cart=before.copy())["cart"]
    worst = cc.check_forward(rl, f, count, index, cart, before=before, must=must)
    T = 3
    cart_bar = rng.uniform(-1, 1, (R, 6, n))
    f_dot = rng.uniform(-1, 1, (T, R, 6, n))
    cart_bar[:, :, n - 1:][np.broadcast_to((cc.counts_of(count, R, n) < n)[:, None, None], (R, 6, 1))] = np.nan   # not read: ignored
    f_bar = unshaped(native.cartesian_vjp_host(shaped(f, layout), rl, cart_bar, layout=layout, count=count, line_index=index), layout)
    dbefore = np.full((T, R, 6, n), cc.SENTINEL)
    cart_dot = native.cartesian_jvp_host(shaped(f, layout), rl, shaped(f_dot, layout), layout=layout, count=count, line_index=index,
                                         cart_dot=dbefore.copy())
    wv = cc.check_vjp(rl, f, count, index, cart_bar, f_bar, must=must)
    wj = cc.check_jvp(rl, f, count, index, f_dot, cart_dot, before=dbefore, must=must)
    cc.check_adjoint(f, count, np.nan_to_num(cart_bar), f_bar, f_dot, np.where(dbefore == cart_dot, 0.0, cart_dot))
    print("worst error / bound: values", worst, "vjp", wv, "jvp", wj)


def test_defined_values_where_nothing_moves():
    """v == 0 exactly: theta = NormalizeAngle(rtheta), kappa = 0, a = at, and theta, kappa, v, a have zero derivative
    while x and y keep theirs."""
    rl = synth.refline_arc(40.0, 0.5, 30.0, theta0=3.0)       # (headings beyond pi: the wrap shows)
    s, l, dds, ddl = 17.0, 1.5, 0.75, -0.5
    f = np.array([s, 0.0, dds, l, 0.0, ddl]).reshape(1, 6, 1)
    cart = native.cartesian_host(f, rl, want=("cart",))["cart"][0, :, 0]
    rth = 3.0 + s / 30.0
    assert cart[cr.V] == 0.0 and cart[cr.KAPPA] == 0.0
    assert abs(cart[cr.THETA] - (rth - 2 * np.pi)) < 1e-15 and -np.pi <= cart[cr.THETA] < np.pi
    assert abs(cart[cr.A] - dds * (1.0 - l / 30.0)) < 1e-15      # at = dds omega when nothing moves
    J = np.stack([native.cartesian_jvp_host(f, rl, np.eye(6)[q].reshape(1, 1, 6, 1))[0, 0, :, 0] for q in range(6)], 1)
    assert (J[2:] == 0.0).all()
    assert J[0, 3] == -math.sin(rl.host["rtheta"][0, 34]) and J[1, 3] == math.cos(rl.host["rtheta"][0, 34]) and J[0, 0] != 0.0
    g = native.cartesian_vjp_host(f, rl, np.ones((1, 6, 1)))[0, :, 0]
    assert np.array_equal(g, J[0] + J[1])


def test_beyond_the_centre_of_curvature_the_map_is_evaluated_and_reported():
    rl = cc.make_lines(65)
    f, _ = cc.make_samples(3, 1, 8, rl, special=False)
    f[0, 3, 5] = 45.0                                           # 1 - l / 30 = -0.5
    o = native.cartesian_host(f, rl)
    assert np.isfinite(o["cart"]).all()
    assert o["audit"]["frame_min"][0] < -0.49 and o["audit"]["worst"][0, 5] == 5 and o["audit"]["n_outside"][0] == 0
    cc.check_forward(rl, f, None, None, o["cart"])


def test_rows_without_a_valid_sample_and_lines_out_of_range():
    rl = cc.make_lines(17, 2)
    f, _ = cc.make_samples(4, 4, 6, rl, special=False)
    f[1, 0, :] = [np.nan, -1.0, 50.0, np.nan, -0.001, 41.0]                       # every sample OUTSIDE
    o = native.cartesian_host(f, rl, count=np.array([6, 6, 0, 6], dtype=np.int32), line_index=np.array([0, 1, 1, 2], dtype=np.int32),
                              cart=np.full((4, 6, 6), cc.SENTINEL))
    a = o["audit"]
    assert list(a["n_outside"]) == [0, 6, 0, 6]
    for r in (1, 2, 3):
        assert a["kappa_abs_max"][r] == a["alat_abs_max"][r] == a["a_max"][r] == a["v_max"][r] == -np.inf
        assert a["a_min"][r] == a["frame_min"][r] == np.inf and (a["worst"][r] == -1).all()
    assert np.isnan(o["cart"][[1, 3]]).all() and (o["cart"][2] == cc.SENTINEL).all() and np.isfinite(o["cart"][0]).all()
    g = native.cartesian_vjp_host(f, rl, np.ones((4, 6, 6)), count=np.array([6, 6, 0, 6], dtype=np.int32),
                                  line_index=np.array([0, 1, 1, 2], dtype=np.int32))
    assert (g[1:] == 0.0).all() and (g[0] != 0.0).any()


@pytest.mark.parametrize("R,n,M,n_lines,kind", CASES[1:])
def test_the_audit_is_the_reduction_of_the_calls_own_cart(R, n, M, n_lines, kind):
    rl = cc.make_lines(M, n_lines)
    _, count, index = options(R, n, n_lines, kind, 12)
    f, _ = cc.make_samples(200 + n, R, n, rl, line_index=index, count=count)
    o = native.cartesian_host(f, rl, count=count, line_index=index)
    cc.check_audit(rl, f, count, index, o["cart"], o["audit"])
    only = native.cartesian_host(f, rl, count=count, line_index=index, want=("audit",))["audit"]
    for k in native.KIN_AUDIT:
        assert o["audit"][k].tobytes() == only[k].tobytes(), k


def test_ties_go_to_the_lowest_sample():
    rl = cc.make_lines(9)
    f, _ = cc.make_samples(5, 1, 70, rl, special=False)
    f[0, :, 66] = f[0, :, 2]; f[0, :, 40] = f[0, :, 2]
    f[0, 1, [2, 40, 66]] = 30.0                                  # the fastest three, alike
    a = native.cartesian_host(f, rl, want=("audit",))["audit"]
    assert a["worst"][0, 4] == 2


def test_refusals():
    rl = cc.make_lines(5)
    f = np.zeros((2, 6, 3)); f[:, 1] = 1.0
    with pytest.raises(ValueError):
        native.cartesian_host(np.zeros((2, 5, 3)), rl)
    with pytest.raises(ValueError):
        native.cartesian_host(f, rl, layout=FRENET_STATES)
    lib = native.lib()
    t, keep = native._refline_host(rl)
    import ctypes as C
    out = np.zeros((2, 6, 3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.btrapz_cartesian_host(C.byref(t), None, 2, 3, 0, p(f), None, p(out), None) == 0
    assert lib.btrapz_cartesian_host(C.byref(t), None, 2, 3, 0, p(f), None, None, None) == -1           # nothing wanted
    assert lib.btrapz_cartesian_host(C.byref(t), None, 2, 3, 0, p(f), None, p(out), C.byref(native.CKinAudit())) == -1
    assert lib.btrapz_cartesian_host(C.byref(t), None, 2, 3, 7, p(f), None, p(out), None) == -1           # layout
    assert lib.btrapz_cartesian_host(C.byref(t), None, 0, 3, 0, p(f), None, p(out), None) == -1
    assert lib.btrapz_cartesian_host(None, None, 2, 3, 0, p(f), None, p(out), None) == -1
    assert lib.btrapz_cartesian_jvp_host(C.byref(t), None, 2, 3, 0, p(f), None, 33, p(f), p(out)) == -1   # T
    assert lib.btrapz_cartesian_jvp_host(C.byref(t), None, 2, 3, 0, p(f), None, 0, p(f), p(out)) == -1
    assert lib.btrapz_cartesian_vjp_host(C.byref(t), None, 2, 3, 0, p(f), None, None, p(out)) == -1
    one = native.CRefLine(1, 1, *[a.ctypes.data for a in keep])
    assert lib.btrapz_cartesian_host(C.byref(one), None, 2, 3, 0, p(f), None, p(out), None) == -1         # M < 2


def test_refline_checks_its_table():
    from spectral_amd.layout import RefLine
    z = np.zeros(4)
    with pytest.raises(ValueError):
        RefLine(np.array([0.0, 1.0, 1.0, 2.0]), z, z, z, z, z)          # not strictly increasing
    with pytest.raises(ValueError):
        RefLine(np.array([0.0]), z[:1], z[:1], z[:1], z[:1], z[:1])     # one point
    with pytest.raises(ValueError):
        RefLine(np.arange(4.0), z, z[:3], z, z, z)                      # shapes
    assert RefLine(np.arange(8.0).reshape(2, 4) % 4, *[np.zeros((2, 4))] * 5).n_lines == 2
