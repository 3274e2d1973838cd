"""btrapz_frenet_host, _vjp_host and _jvp_host (include/btrapz_hip_frenet.h) against the yardstick
(tests/frenet_reference.py) within its bound, against the existing host forward (round trips, K J = I), and on every
defined case with sentinels compared bit by bit.  No GPU."""
import numpy as np
import pytest

import frenet_cases as fc
import frenet_reference as fr
from spectral_amd import native, synth

S, NS = native.FRENET_SAMPLES, native.FRENET_STATES


@pytest.fixture(scope="module")
def case():
    """3 rows on 3 lines of 129 points, 40 queries each, the special ones planted; the forward's result at order 2."""
    rl = fc.make_lines(129, 3)
    li = np.array([0, 1, 2], dtype=np.int32)
    cart, f, planted = fc.make_queries(11, 3, 40, rl, line_index=li)
    o = native.frenet_host(cart, rl, line_index=li)
    return dict(rl=rl, li=li, cart=cart, f=f, planted=planted, o=o, picks=fc.picks_of(planted, 3, 40, None, 40))


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("layout", [S, NS])
def test_values_are_within_the_bound(case, order, layout):
    o = native.frenet_host(case["cart"], case["rl"], layout=layout, order=order, line_index=case["li"])
    got = o["frenet"] if layout == S else fc.from_states(o["frenet"])
    must = [p for k in ("table", "first", "last") for p in case["planted"][k]]
    worst, same = fc.check_values(case["rl"], case["cart"], got, o["interval"], case["picks"], order, case["li"], must=must)
    assert len(same) >= 30 and int(o["n_outside"].sum()) == len(case["planted"]["nan"]) + len(case["planted"]["behind"])
    print("host twin, order %d layout %d: worst ratio to the bound %.3f over %d queries" % (order, layout, worst, len(same)))


@pytest.mark.parametrize("M", [2, 3, 1100])
def test_values_on_tables_of_other_sizes(M):
    rl = fc.make_lines(M, 2)
    li = np.array([1, 0], dtype=np.int32)
    cart, f, planted = fc.make_queries(20 + M, 2, 9, rl, line_index=li)
    o = native.frenet_host(cart, rl, line_index=li)
    worst, same = fc.check_values(rl, cart, o["frenet"], o["interval"], fc.picks_of(planted, 2, 9, None, 18), 2, li)
    assert len(same) >= 6


@pytest.mark.parametrize("order", [0, 1, 2])
def test_jvp_and_vjp_are_the_yardsticks_jacobian(case, order):
    rl, li, cart = case["rl"], case["li"], case["cart"]
    o = native.frenet_host(cart, rl, order=order, line_index=li)
    _, same = fc.check_values(rl, cart, o["frenet"], o["interval"], case["picks"], order, li)
    jvp = lambda cd: native.frenet_jvp_host(cart, rl, o["frenet"], o["interval"], cd, order=order, line_index=li)
    Kj = fc.jacobian_from_jvp(jvp, cart)
    worst = fc.check_jacobian(Kj, same, order)
    # the VJP: six unit cotangents give the rows of the same Jacobian
    Kv = np.zeros_like(Kj)
    for q in range(6):
        fb = np.zeros_like(o["frenet"]); fb[:, q] = 1.0
        Kv[:, q] = native.frenet_vjp_host(cart, rl, o["frenet"], o["interval"], fb, order=order, line_index=li)
    assert fc.check_jacobian(Kv, same, order) <= 1.0
    # OUTSIDE: 0 in every derivative
    for r, j in case["planted"]["nan"] + case["planted"]["behind"]:
        assert (Kj[r, :, :, j] == 0).all() and (Kv[r, :, :, j] == 0).all()
    print("host twin's Jacobian, order %d: worst ratio to its bound %.3f over %d queries" % (order, worst, len(same)))


@pytest.mark.parametrize("layout", [S, NS])
def test_the_adjoint_identity(case, layout):
    rl, li, cart = case["rl"], case["li"], case["cart"]
    o = native.frenet_host(cart, rl, layout=layout, line_index=li)
    rng = np.random.default_rng(3)
    fb, cd = rng.normal(size=o["frenet"].shape), rng.normal(size=(3,) + cart.shape)
    cb = native.frenet_vjp_host(cart, rl, o["frenet"], o["interval"], fb, layout=layout, line_index=li)
    fd = native.frenet_jvp_host(cart, rl, o["frenet"], o["interval"], cd, layout=layout, line_index=li)
    for t in range(3):
        lhs, rhs = (cb * cd[t]).sum(), (fb * fd[t]).sum()
        assert abs(lhs - rhs) <= 1e-12 * np.abs(cb * cd[t]).sum()


def test_the_inverse_jacobian_times_the_forwards_is_the_identity():
    """K J = I with J from btrapz_cartesian_jvp_host at the inverse's result, on queries with v >= 0.5 that are not within
    1e-9 of a table point (there the forward's interval is the next one).  The bound is assembled from the two
    yardsticks' entry bounds: |dK| |J| + (|K| + |dK|) |dJ|, plus 8 * 2^-53 |K| |J| for the product itself."""
    import cartesian_reference as cr
    rl = fc.make_lines(129, 3)
    li = np.array([0, 1, 2, 0], dtype=np.int32)
    cart, f, _ = fc.make_queries(31, 4, 50, rl, line_index=li, plant=False)
    o = native.frenet_host(cart, rl, line_index=li)
    rs = rl.host["rs"][li]
    w = (o["frenet"][:, 0] - np.take_along_axis(rs, o["interval"].astype(np.int64), 1)) / (rs[:, 1] - rs[:, 0])[:, None]
    ok = (cart[:, 4] >= 0.5) & (np.minimum(w, 1 - w) > 1e-9)
    assert ok.mean() >= 0.95
    fd = np.zeros((6,) + f.shape)
    for t in range(6):
        fd[t, :, t] = 1.0
    J = native.cartesian_jvp_host(o["frenet"], rl, fd, line_index=li)                           # [column, R, row, n]
    Kfull = fc.jacobian_from_jvp(lambda cd: native.frenet_jvp_host(cart, rl, o["frenet"], o["interval"], cd, line_index=li), cart)
    KJ = native.frenet_jvp_host(cart, rl, o["frenet"], o["interval"], J, line_index=li)           # K applied to J's columns
    rng = np.random.default_rng(1)
    where = np.argwhere(ok)
    done = 0
    for r, j in where[rng.permutation(len(where))[:40]]:
        resK = fc.yard(rl, int(li[r]), cart[r, :, j], 2)
        if resK["i"] != o["interval"][r, j] or abs(resK["omega"]) < 0.2:
            continue
        fo, Jf, _ = cr.evaluate(fc.line_of(rl, int(li[r])), o["frenet"][r, :, j])
        dJ = cr.jacobian_bound(o["frenet"][r, :, j], fo, Jf)
        Kh, Jh = Kfull[r, :, :, j], J[:, r, :, j].T
        bnd = resK["jbound"] @ np.abs(Jf) + (np.abs(resK["J"]) + resK["jbound"]) @ dJ + 8 * 2.0 ** -53 * (np.abs(Kh) @ np.abs(Jh))
        assert (np.abs(Kh @ Jh - np.eye(6)) <= bnd).all(), (r, j, Kh @ Jh - np.eye(6), bnd)
        assert (np.abs(KJ[:, r, :, j].T - np.eye(6)) <= bnd).all()
        done += 1
    assert done >= 38


def test_round_trips_through_the_existing_forward():
    rl = fc.make_lines(65, 3)
    li = np.array([0, 1, 2], dtype=np.int32)
    cart, f, _ = fc.make_queries(41, 3, 60, rl, line_index=li, plant=False)
    o = native.frenet_host(cart, rl, line_index=li)
    assert (o["interval"] >= 0).all()
    # forward -> inverse returns the Frenet draw; inverse -> forward returns the query.  1e-11: the bound's size at these
    # magnitudes (64 * 2^-53 * a few hundred), the precise statement is test_values_are_within_the_bound
    assert np.abs(o["frenet"] - f).max() <= 1e-11
    back = native.cartesian_host(o["frenet"], rl, line_index=li, want=("cart",))["cart"]
    assert np.abs(back[:, :2] - cart[:, :2]).max() <= 1e-12 and np.abs(back[:, 3:] - cart[:, 3:]).max() <= 1e-11
    assert np.abs(np.angle(np.exp(1j * (back[:, 2] - cart[:, 2])))).max() <= 1e-12


def test_defined_cases_bit_by_bit(case):
    rl, cart = case["rl"], case["cart"]
    R, _, n = cart.shape
    li = np.array([0, 3, -1], dtype=np.int32)               # rows 1 and 2: line_index out of range
    count = np.array([n + 5, n, 7], dtype=np.int32)
    fr_ = np.full((R, 6, n), fc.SENTINEL); iv = np.full((R, n), fc.ISENT, dtype=np.int32)
    o = native.frenet_host(cart, rl, line_index=li, count=count, frenet=fr_, interval=iv)
    assert np.isnan(fr_[1]).all() and (iv[1] == -1).all() and o["n_outside"][1] == n
    assert np.isnan(fr_[2, :, :7]).all() and (iv[2, :7] == -1).all() and o["n_outside"][2] == 7
    assert (fr_[2, :, 7:] == fc.SENTINEL).all() and (iv[2, 7:] == fc.ISENT).all()          # beyond the count: the caller's contents
    assert not (fr_[0] == fc.SENTINEL).any()                                               # a count beyond n reads n
    # counts 0 and 1; a window that is NaN, and one with lo > hi
    count = np.array([0, 1, n], dtype=np.int32)
    li = np.array([0, 1, 2], dtype=np.int32)
    win = np.array([[0.0, 40.0], [np.nan, 40.0], [30.0, 10.0]])
    fr_ = np.full((R, 6, n), fc.SENTINEL); iv = np.full((R, n), fc.ISENT, dtype=np.int32)
    o = native.frenet_host(cart, rl, line_index=li, count=count, s_window=win, frenet=fr_, interval=iv)
    assert (fr_[0] == fc.SENTINEL).all() and (iv[0] == fc.ISENT).all() and o["n_outside"][0] == 0
    assert np.isnan(fr_[1, :, 0]).all() and iv[1, 0] == -1 and (fr_[1, :, 1:] == fc.SENTINEL).all() and o["n_outside"][1] == 1
    assert np.isnan(fr_[2]).all() and (iv[2] == -1).all() and o["n_outside"][2] == n
    # derivatives: 0 at OUTSIDE and, in the VJP, beyond the count; the JVP keeps the caller's contents there
    o = native.frenet_host(cart, rl, line_index=li)
    cnt = np.array([5, n, 0], dtype=np.int32)
    fb = np.full(o["frenet"].shape, np.nan)                   # what the cotangent holds where nothing is read is ignored
    fb[0, :, :5] = 1.0; fb[1] = 1.0
    cb = native.frenet_vjp_host(cart, rl, o["frenet"], o["interval"], fb, line_index=li, count=cnt)
    assert (cb[0, :, 5:] == 0).all() and (cb[2] == 0).all() and np.isfinite(cb).all()
    out = np.full((2,) + o["frenet"].shape, fc.SENTINEL)
    native.frenet_jvp_host(cart, rl, o["frenet"], o["interval"], np.ones((2,) + cart.shape), line_index=li, count=cnt, frenet_dot=out)
    assert (out[:, 0, :, 5:] == fc.SENTINEL).all() and (out[:, 2] == fc.SENTINEL).all() and not (out[:, 1] == fc.SENTINEL).any()
    for r, j in case["planted"]["nan"] + case["planted"]["behind"]:
        if j < cnt[r]:
            assert (out[:, r, :, j] == 0).all() and (cb[r, :, j] == 0).all()
    # v == 0 is regular: ds = dl = 0 and finite accelerations
    still = cart.copy(); still[:, 4] = 0.0
    o0 = native.frenet_host(still, rl, line_index=li)
    ins = o0["interval"] >= 0
    assert (o0["frenet"][:, 1][ins] == 0).all() and (o0["frenet"][:, 4][ins] == 0).all() and np.isfinite(o0["frenet"][:, 2][ins]).all()
    # an interval that is out of the table is OUTSIDE to the derivatives, whatever it holds
    wild = np.full_like(o["interval"], 10 ** 6)
    assert (native.frenet_vjp_host(cart, rl, o["frenet"], wild, np.ones_like(o["frenet"]), line_index=li) == 0).all()


def test_omega_zero_gives_ieee_results():
    rl = synth.refline_arc(20.0, 0.5, 8.0)                   # centre (0, 8)
    s = rl.host["rs"][0][10]
    # a table with rkappa = 1 / 8 whose query sits at l = 8 exactly would be the centre (every g is 0 there: no + -> -
    # change, OUTSIDE); omega == 0 is reached instead with a table whose rkappa disagrees with its headings
    from spectral_amd import layout
    h = {k: rl.host[k][0].copy() for k in fr.FIELDS}
    h["rkappa"][:] = 0.5
    odd = layout.RefLine(*[h[k] for k in fr.FIELDS])
    phi = s / 8.0
    cart = np.zeros((1, 6, 1))
    cart[0, :, 0] = [(8.0 - 2.0) * np.sin(phi), 8.0 - (8.0 - 2.0) * np.cos(phi), phi, 0.0, 1.0, 0.0]     # l = 2: omega = 1 - 0.5 * 2
    o = native.frenet_host(cart, odd)
    assert o["interval"][0, 0] >= 0 and abs(o["frenet"][0, 3, 0] - 2.0) <= 1e-12
    assert abs(o["frenet"][0, 1, 0]) > 1e10 or np.isinf(o["frenet"][0, 1, 0])        # ds = v cos D / omega, omega ~ 0: as it falls


def test_the_hairpin():
    rl = fc.hairpin()
    rs, M = rl.host["rs"][0], rl.M
    far = 32.0 + 4.0 * np.pi + 32.0
    q = lambda x, y: np.array([x, y, 0, 0, 0, 0], dtype=np.float64).reshape(1, 6, 1)
    one = lambda c, **kw: native.frenet_host(c, rl, order=0, **kw)
    # between the straights there are two candidates: the nearer branch wins
    lo_, hi_ = one(q(10.0, 3.0)), one(q(10.0, 5.0))
    assert fr.find_interval(fc.line_of(rl, 0), 10.0, 3.0)[2] == 2
    assert lo_["frenet"][0, 0, 0] == 10.0 and lo_["frenet"][0, 3, 0] == 3.0 and lo_["interval"][0, 0] == 20
    near = lambda got, want: abs(got - want) <= 1e-12          # (the upper straight has heading pi: sin pi is 1.2e-16, not 0)
    assert near(hi_["frenet"][0, 0, 0], far - 10.0) and near(hi_["frenet"][0, 3, 0], 3.0)
    # the exact tie at mid-height goes to the lower index; 1e-12 above it to the other branch
    tie, above = one(q(10.0, 4.0)), one(q(10.0, 4.0 + 1e-12))
    assert tie["interval"][0, 0] == 20 and tie["frenet"][0, 3, 0] == 4.0
    assert near(above["frenet"][0, 0, 0], far - 10.0) and above["interval"][0, 0] > 64
    for c, res in ((q(10.0, 4.0), tie), (q(10.0, 4.0 + 1e-12), above)):
        assert fr.find_interval(fc.line_of(rl, 0), c[0, 0, 0], c[0, 1, 0])[0] == res["interval"][0, 0]
    # windows force the far branch, and an empty window is OUTSIDE
    forced = one(q(10.0, 3.0), s_window=np.array([[50.0, far]]))
    assert near(forced["frenet"][0, 0, 0], far - 10.0) and near(forced["frenet"][0, 3, 0], 5.0)
    assert one(q(10.0, 5.0), s_window=np.array([[0.0, 30.0]]))["frenet"][0, 3, 0] == 5.0
    empty = one(q(10.0, 3.0), s_window=np.array([[35.0, 45.0]]))                       # only the bend: no candidate for this point
    assert empty["interval"][0, 0] == -1 and np.isnan(empty["frenet"]).all() and empty["n_outside"][0] == 1
    gone = one(q(10.0, 3.0), s_window=np.array([[far + 1.0, far + 2.0]]))
    assert gone["interval"][0, 0] == -1
    # the window's edges: an interval counts when rs[i + 1] >= lo and rs[i] <= hi
    assert one(q(10.2, 3.0), s_window=np.array([[10.5, 10.5]]))["interval"][0, 0] == 20     # rs[21] == lo
    assert one(q(10.2, 3.0), s_window=np.array([[10.0, 10.0]]))["interval"][0, 0] == 20     # rs[20] == hi
    assert one(q(10.2, 3.0), s_window=np.array([[10.75, 12.0]]))["interval"][0, 0] == -1
    # beyond the centre of the bend a point shows a - -> + change only: no candidate
    assert fr.find_interval(fc.line_of(rl, 0), 60.0, 4.3)[0] == one(q(60.0, 4.3))["interval"][0, 0]


def test_the_table_ends_where_g_is_exact():
    rl = synth.refline_straight(20.0, 0.5, x0=3.0, y0=-2.0, theta0=0.0)     # heading 0: g = x - rx exactly
    M = rl.M
    xs = [3.0, np.nextafter(3.0, -np.inf), np.nextafter(3.0, np.inf), 23.0, np.nextafter(23.0, -np.inf), np.nextafter(23.0, np.inf)]
    cart = np.zeros((1, 6, len(xs)))
    cart[0, 0], cart[0, 1] = xs, 1.5
    o = native.frenet_host(cart, rl, order=0)
    assert list(o["interval"][0]) == [0, -1, 0, M - 2, M - 2, -1] and o["n_outside"][0] == 2
    assert o["frenet"][0, 0, 0] == 0.0 and o["frenet"][0, 0, 3] == 20.0 and (o["frenet"][0, 3, [0, 2, 3, 4]] == 3.5).all()
    assert 0.0 < o["frenet"][0, 0, 2] < 1e-15 and 20.0 - 1e-14 < o["frenet"][0, 0, 4] < 20.0
    assert np.isnan(o["frenet"][0, :, 1]).all() and np.isnan(o["frenet"][0, :, 5]).all()
    for j, x in enumerate(xs):
        assert fr.find_interval(fc.line_of(rl, 0), x, 1.5)[0] == o["interval"][0, j]
    # an interior table point belongs to the interval it opens, as in the forward's lookup
    cart[0, 0, 0] = 8.0
    assert native.frenet_host(cart, rl, order=0)["interval"][0, 0] == 10


def test_refusals():
    rl = fc.make_lines(3, 1)
    cart = np.zeros((1, 6, 2))
    with pytest.raises(native.BtrapzError):
        native.frenet_host(cart, rl, order=3)
    with pytest.raises(native.BtrapzError):
        native.frenet_host(cart, rl, order=-1)
    with pytest.raises(ValueError):
        native.frenet_host(cart, rl, layout=2)
    o = native.frenet_host(cart, rl)
    with pytest.raises(native.BtrapzError):
        native.frenet_jvp_host(cart, rl, o["frenet"], o["interval"], np.zeros((33, 1, 6, 2)))
