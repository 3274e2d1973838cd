"""btrapz_clearance_host, _vjp_host and _jvp_host through ctypes (no GPU) against the yardstick of
tests/clearance_reference.py: values and `which` at every sample (nothing skipped), the derivative's four numbers by
forward mode with unit tangents and by reverse mode with a unit cotangent (samples whose margin is below TAU skipped, at
most 10 % of them), the adjoint identity over the samples read, every defined case of the header with sentinels compared
bit by bit, the audit against NumPy reductions of the call's own clear, and exact cases -- headings 0, dyadic
coordinates and extents -- in which the clearance is known to the bit and ties go to the lowest feature and obstacle.
(cos(pi / 2) is not 0 in binary64, so the exact cases keep every heading at 0.)"""
import numpy as np
import pytest

import clearance_cases as cc
from spectral_amd import layout, native

SHAPES = [(3, 65, 4), (2, 40, 16), (2, 64, 1)]


@pytest.fixture(scope="module", autouse=True)
def built():
    native.build()


def forward(case, **kw):
    return native.clearance_host(case["cart"], case["obstacles"], case["foot"], scene_index=case["scene_index"], count=case["count"], **kw)


@pytest.mark.parametrize("R,n,O", SHAPES)
def test_values_and_which_follow_the_yardstick(R, n, O):
    case = cc.make_case(R, n, O, seed=R)
    o = forward(case)
    worst = cc.check_values(case, cc.pick_samples(case, 150), o["clear"], o["which"])
    print("worst error / bound %.3g" % worst)
    assert (o["clear"] < 0).any() and (o["clear"] > 0).any()          # both branches were drawn


@pytest.mark.parametrize("R,n,O", SHAPES)
def test_jvp_and_vjp_follow_the_yardstick(R, n, O):
    case = cc.make_case(R, n, O, seed=R)
    o = forward(case, want=("which",))
    samples = cc.pick_samples(case, 150)
    cd, od = cc.unit_tangents(case)
    jd = native.clearance_jvp_host(case["cart"], case["obstacles"], case["foot"], o["which"], cd, od)
    worst, share = cc.check_grads(case, samples, {(r, j): jd[:, r, j] for r, j in samples})
    print("JVP: worst error / bound %.3g, skipped %.3g" % (worst, share))
    cb = native.clearance_vjp_host(case["cart"], case["obstacles"], case["foot"], o["which"], np.ones((R, n)))
    assert not cb[:, 3:].any()
    # reverse mode forms the same three numbers: bit for bit those of forward mode
    assert np.array_equal(cb[:, :3].transpose(1, 0, 2), jd[:3])
    # without obs_dot the obstacles stand still
    still = native.clearance_jvp_host(case["cart"], case["obstacles"], case["foot"], o["which"], cd)
    assert np.array_equal(still[:3], jd[:3]) and not still[3:].any()


def test_adjoint_identity_over_the_samples_read():
    case = cc.make_case(5, 71, 3, n_scenes=2, seed=11, counts=[71, 0, 1, 40, 99], scene_index=[0, 1, 1, 0, 1], nan_ego=[(0, 5), (3, 39)],
                        nan_obs=[(0, 1, 7), (1, 0, 0)])
    rng = np.random.default_rng(5)
    o = forward(case, want=("which",))
    cbar = rng.normal(size=(5, 71))
    cdot = rng.normal(size=(4, 5, 6, 71))
    cart_bar = native.clearance_vjp_host(case["cart"], case["obstacles"], case["foot"], o["which"], np.where(cc_read(case), cbar, np.nan),
                                         scene_index=case["scene_index"], count=case["count"])
    clear_dot = native.clearance_jvp_host(case["cart"], case["obstacles"], case["foot"], o["which"], cdot, scene_index=case["scene_index"],
                                          count=case["count"], clear_dot=np.zeros((4, 5, 71)))
    assert np.isfinite(cart_bar).all()                                 # NaN in clear_bar beyond the counts is ignored
    for t in range(4):
        lhs, rhs = (cbar * clear_dot[t]).sum(), (cart_bar * cdot[t]).sum()
        assert abs(lhs - rhs) <= 1e-13 * np.abs(cbar * clear_dot[t]).sum()


def cc_read(case):
    m = np.zeros((case["R"], case["n"]), dtype=bool)
    for r, c in cc.rows_read(case):
        m[r, :c] = True
    return m


def test_defined_cases_with_sentinels():
    R, n, O = 6, 66, 3
    case = cc.make_case(R, n, O, n_scenes=3, seed=21, counts=[66, 0, 1, 65, 80, 66], obs_count=[3, 0, 2], scene_index=[0, 1, 2, 0, 7, -1],
                        nan_ego=[(0, 0), (0, 63), (0, 64), (0, 65), (3, 64)], nan_obs=[(0, o, j) for o in range(3) for j in (1, 63)] + [(0, 0, 64)])
    clear = np.full((R, n), -7.0)
    which = np.full((R, n), -7, dtype=np.int32)
    o = forward(case, d_safe=0.5, clear=clear, which=which)
    read = cc_read(case)
    # beyond a row's count the caller's contents stay, bit by bit
    assert (clear[~read] == -7.0).all() and (which[~read] == -7).all()
    # NaN ego poses: NaN, -1, counted
    for j in (0, 63, 64, 65):
        assert np.isnan(clear[0, j]) and which[0, j] == -1
    assert o["audit"]["n_invalid"].tolist() == [4, 0, 0, 1, 66, 66]
    # a scene_index out of range: the whole row invalid, in no extreme
    assert np.isnan(clear[4]).all() and np.isnan(clear[5]).all() and (which[4:] == -1).all()
    assert o["audit"]["clear_min"][4] == np.inf and o["audit"]["worst"][4].tolist() == [-1, -1]
    # every obstacle of scene 0 absent at samples 1 and 63: +inf, -1 (63 has a NaN ego pose, which goes first)
    assert clear[0, 1] == np.inf and which[0, 1] == -1
    # obstacle 0 absent at sample 64 of scene 0: row 3 (scene 0, a NaN ego there) and row 0 alike; at sample 2 all are present
    assert (which[3, :64] >> 4).max() <= 2
    # a scene without obstacles: +inf everywhere read (row 1 reads nothing, so: nobody)
    assert o["audit"]["clear_min"][1] == np.inf and o["audit"]["n_below"][1] == 0
    # scene 2 has two obstacles: the third is never named
    assert which[2, 0] >> 4 in (0, 1)
    # the derivatives at those samples: 0, and what is beyond the count stays (clear_dot) or is 0 (cart_bar)
    cbar = np.ones((R, n))
    cart_bar = native.clearance_vjp_host(case["cart"], case["obstacles"], case["foot"], which, cbar, scene_index=case["scene_index"],
                                         count=case["count"])
    assert not cart_bar[:, :, :][~np.broadcast_to(read[:, None, :], cart_bar.shape)].any()
    assert not cart_bar[0, :, [0, 1, 63, 64, 65]].any() and not cart_bar[4].any() and not cart_bar[5].any()
    cd, od = cc.unit_tangents(case)
    dot = np.full((6, R, n), -7.0)
    native.clearance_jvp_host(case["cart"], case["obstacles"], case["foot"], which, cd, od, scene_index=case["scene_index"], count=case["count"],
                              clear_dot=dot)
    assert (dot[:, ~read] == -7.0).all() and not dot[:, 0, [0, 1, 63, 64, 65]].any() and not dot[:, 4].any()
    # the yardstick agrees on all of it
    cc.check_values(case, [(r, j) for r, c in cc.rows_read(case) for j in range(0, c, 5)], clear, which)


def test_audit_is_the_reduction_of_the_calls_own_clear():
    case = cc.make_case(7, 130, 5, n_scenes=2, seed=31, counts=[130, 129, 64, 65, 1, 0, 200], scene_index=[0, 1, 0, 1, 0, 1, 0],
                        nan_ego=[(0, 3), (1, 128)])
    d_safe = 0.75
    o = forward(case, d_safe=d_safe)
    only = forward(case, d_safe=d_safe, want=("audit",))
    for k in native.CLEAR_AUDIT:
        assert np.array_equal(o["audit"][k], only["audit"][k]), k
    for r, c in cc.rows_read(case):
        row = o["clear"][r, :c]
        finite = np.where(np.isfinite(row), row, np.inf)
        if c == 0 or not np.isfinite(row).any():
            assert o["audit"]["clear_min"][r] == np.inf and o["audit"]["worst"][r].tolist() == [-1, -1]
        else:
            j = int(np.argmin(finite))                                  # the first on a tie
            assert o["audit"]["clear_min"][r] == finite[j] and o["audit"]["worst"][r].tolist() == [j, o["which"][r, j] >> 4]
        assert o["audit"]["n_below"][r] == int((row < d_safe).sum())
        assert o["audit"]["n_invalid"][r] == int(np.isnan(row).sum())


def exact_case(obs, half, foot=(2.0, 1.0, 0.5)):
    """One ego sample at (1, -2) with heading 0 against obstacles (x, y) with heading 0."""
    cart = np.zeros((1, 6, 1))
    cart[0, 0, 0], cart[0, 1, 0] = 1.0, -2.0
    pose = np.zeros((len(obs), 3, 1))
    pose[:, :2, 0] = obs
    o = native.clearance_host(cart, layout.Obstacles(pose, np.array(half, dtype=np.float64)), foot)
    return float(o["clear"][0, 0]), int(o["which"][0, 0])


def test_exact_cases_to_the_bit():
    # the ego's centre is (1.5, -2): it spans x in [-0.5, 3.5], y in [-3, -1]
    assert exact_case([(6.5, -2.25)], [(1.0, 1.5)]) == (2.0, 4)            # face to face: the first vertex of A that attains it
    assert exact_case([(7.5, 4.0)], [(1.0, 1.0)]) == (5.0, 4)              # corner (3.5, -1) to corner (6.5, 3): 3-4-5
    assert exact_case([(1.5, -2.0)], [(0.5, 0.25)]) == (-1.25, 1)          # nested at the centre: out along n_A
    assert exact_case([(1.75, -1.5)], [(0.5, 0.25)]) == (-0.75, 1)
    # touching exactly: g = 0 is the overlap branch, clearance 0 (not -0), the face's feature
    c, w = exact_case([(4.5, -2.0)], [(1.0, 0.5)])
    assert c == 0.0 and not np.signbit(c) and w == 0
    c, w = exact_case([(4.5, -0.5)], [(1.0, 0.5)])                         # at a corner: g_0 = g_1 = 0, the lowest wins
    assert c == 0.0 and w == 0


def test_ties_go_to_the_lowest_feature_and_the_lowest_obstacle():
    # parallel boxes overlapping: g_0 = g_2 and g_1 = g_3 exactly; u_A's face (0) wins over u_B's (2)
    assert exact_case([(4.0, -2.0)], [(1.0, 0.5)]) == (-0.5, 0)
    assert exact_case([(1.5, -0.75)], [(0.5, 0.5)]) == (-0.25, 1)
    # equal extents, edge to edge in parallel: all of 4, 7 (A's right-hand vertices) and 9, 10 (B's left-hand ones) give 1
    assert exact_case([(5.5, -2.0)], [(1.0, 1.0)]) == (1.0, 4)
    # two obstacles at the same clearance, left and right: the lower index is named, whichever side it is on
    assert exact_case([(5.5, -2.0), (-2.5, -2.0)], [(1.0, 1.0), (1.0, 1.0)]) == (1.0, 4)
    assert exact_case([(-2.5, -2.0), (5.5, -2.0)], [(1.0, 1.0), (1.0, 1.0)]) == (1.0, 5)
    assert exact_case([(9.0, 9.0), (-2.5, -2.0), (5.5, -2.0)], [(1.0, 1.0)] * 3) == (1.0, 16 + 5)


def test_the_derivative_at_a_tie_is_the_winners():
    # edge to edge in parallel: one-sided in theta, the winner is A's vertex (+,+) = (3.5, -1) against B's face x = 4.5
    cart = np.zeros((1, 6, 1))
    cart[0, 0, 0], cart[0, 1, 0] = 1.0, -2.0
    ob = layout.Obstacles(np.array([[[5.5], [-2.0], [0.0]]]), np.array([[1.0, 1.0]]))
    g = native.clearance_vjp_host(cart, ob, (2.0, 1.0, 0.5), np.array([[4]], dtype=np.int32), np.ones((1, 1)))[0, :, 0]
    # n = (-1, 0); the lever of (3.5, -1) about the pose's point (1, -2): (2.5, 1) x (-1, 0) = 1
    assert g.tolist() == [-1.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def test_refusals():
    case = cc.make_case(2, 8, 2, seed=41)
    ob, cart = case["obstacles"], case["cart"]
    with pytest.raises(native.BtrapzError):
        native.clearance_host(cart, ob, (0.0, 1.0, 0.0))
    with pytest.raises(native.BtrapzError):
        native.clearance_host(cart, ob, (2.0, np.inf, 0.0))
    with pytest.raises(native.BtrapzError):
        native.clearance_host(cart, ob, (2.0, 1.0, np.nan))
    with pytest.raises(native.BtrapzError):
        native.clearance_host(cart, ob, cc.FOOT, want=())
    with pytest.raises(native.BtrapzError):
        native.clearance_host(cart[:, :, :7], ob, cc.FOOT)                 # obstacles.n != n
    with pytest.raises(native.BtrapzError):
        native.clearance_jvp_host(cart, ob, cc.FOOT, np.zeros((2, 8), dtype=np.int32), np.zeros((native.MAX_TANGENTS + 1, 2, 6, 8)))
    with pytest.raises(ValueError):
        layout.Obstacles(np.zeros((2, 3, 8)), np.array([[1.0, 0.0], [1.0, 1.0]]))
    # the C entry point itself refuses an obstacle's half extent that is not > 0 and finite
    import ctypes as C
    half = np.array([[1.0, -1.0], [1.0, 1.0]])
    pose = np.zeros((2, 3, 8))
    cob = native.CObstacles(1, 2, 8, pose.ctypes.data, half.ctypes.data, None)
    ft = native.footprint_struct(cc.FOOT)
    clear = np.zeros((2, 8))
    rc = native.lib().btrapz_clearance_host(C.byref(ft), C.byref(cob), None, 2, 8, cart.ctypes.data_as(C.c_void_p), None, 0.0,
                                            clear.ctypes.data_as(C.c_void_p), None, None)
    assert rc == -1


@pytest.mark.parametrize("name", sorted(cc.EXACT))
def test_the_shared_exact_cases_to_the_bit(name):
    """The table the device is held to as well (tests/test_gpu_clearance.py)."""
    cart, ob, clear, which = cc.exact_inputs(name)
    o = native.clearance_host(cart, ob, cc.EXACT_FOOT)
    c = float(o["clear"][0, 0])
    assert np.float64(c).tobytes() == np.float64(clear).tobytes() and int(o["which"][0, 0]) == which
    assert o["audit"]["clear_min"][0] == clear and o["audit"]["worst"][0].tolist() == [0, which >> 4]
    if name == cc.EXACT_TIE_GRADIENT[0]:
        g = native.clearance_vjp_host(cart, ob, cc.EXACT_FOOT, o["which"], np.ones((1, 1)))[0, :, 0]
        assert g.tolist() == cc.EXACT_TIE_GRADIENT[1]


def test_a_feature_that_does_not_exist_gives_zero_whatever_the_cotangent_holds():
    case = cc.make_case(2, 9, 2, seed=51)
    which = np.empty((2, 9), dtype=np.int32)
    which[:] = np.array([12, 13, 14, 15, 16 + 12, 16 + 15, 32, -1, -9])           # features 12..15 of obstacles 0 and 1, obstacle 2, nobody
    bar = np.full((2, 9), np.nan)
    bar[1] = np.inf
    g = native.clearance_vjp_host(case["cart"], case["obstacles"], case["foot"], which, bar)
    assert g.tobytes() == np.zeros((2, 6, 9)).tobytes()
    cd, od = cc.unit_tangents(case)
    d = native.clearance_jvp_host(case["cart"], case["obstacles"], case["foot"], which, np.full_like(cd, np.nan), np.full_like(od, np.inf))
    assert d.tobytes() == np.zeros((6, 2, 9)).tobytes()
