"""The forward-mode derivatives of the prism and corridor stages on the host (btrapz_prism_bounds_jvp_host,
btrapz_corridor_jvp_host: the twins of the device kernels) against the yardstick of tests/stage_jvp_reference.py, against the
host twins of the backward passes through the adjoint identity, and their defined cases and refusals."""
import ctypes as C

import numpy as np
import pytest

import corridor_vjp_cases as CK
import corridor_vjp_reference as CR
import prism_vjp_cases as PK
import prism_vjp_reference as PR
import stage_jvp_reference as S
from spectral_amd import layout as L, native

T_YARD = 3


def corridor_host(kb, b, variant, tan, seg_stride=CK.SEG_STRIDE, **kw):
    """tan: {input: [T, ...]} of candidate b."""
    return native.corridor_jvp_host(variant, kb.delta, kb.s_bounds[b], kb.l_bounds[b], kb.ds_bounds[b], kb.dl_bounds[b], kb.s_ref[b],
                                    kb.l_ref[b], seg_stride, tan, **kw)


def corridor_against_yardstick(kb, b, variant, key, seg_stride=CK.SEG_STRIDE, seed=0):
    """Candidate b's host twin against J @ t for T_YARD random directions; returns (worst error / tolerance, n)."""
    jac = CR.jacobian(kb, b, variant, key=key)
    assert jac["n"] >= 1
    CR.check_caps(jac)
    tans = S.corridor_tangents(kb, T_YARD, seed=seed)
    per = [S.zero_skipped_corridor(jac, {k: v[t, b] for k, v in tans.items()}) for t in range(T_YARD)]
    out, count = corridor_host(kb, b, variant, {k: np.stack([p[k] for p in per]) for k in per[0]}, seg_stride)
    assert count == jac["n"]
    x = S.corridor_inputs(kb, b)
    worst = 0.0
    for t in range(T_YARD):
        assert not out["seg"][t, 0].any() and not out["seg"][t, :, count:].any()       # field 0, slots >= seg_count
        worst = max(worst, S.corridor_compare(jac, x, per[t], S.corridor_flat(count, out["seg"][t], out["ref_end"][t], out["dl_bounds"][t]),
                                              (key, t)))
    return worst, count


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", ["scenario", "c1"])
def test_corridor_host_twin_against_yardstick(name, variant):
    kb = CK.scenario(2) if name == "scenario" else CK.c1(2)
    b = 0 if name == "scenario" else 1
    worst, n = corridor_against_yardstick(kb, b, variant, (name, 2, b, variant))
    print(name, variant, "segments", n, "worst error / tolerance:", worst)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("seed", CK.FUZZ_SEEDS + (CK.MIXED_SEED,))
def test_corridor_host_twin_on_fuzz_batches(seed, variant):
    """Every candidate: the count is the backward twin's, no corridor gives zeros; the first two with a corridor against the
    yardstick."""
    kb = CK.fuzz(seed)
    name = "mixed" if seed == CK.MIXED_SEED else "fuzz%d" % seed
    sb, rb, db = CK.cotangents(kb.B)
    tans = S.corridor_tangents(kb, 2, seed=seed)
    counts = []
    for b in range(kb.B):
        out, count = corridor_host(kb, b, variant, {k: v[:, b] for k, v in tans.items()})
        _, vjp_count = CK.host_grads(kb, b, variant, sb, rb, db)
        assert count == vjp_count, (b, count, vjp_count)
        counts.append(count)
        if count < 1:
            assert all(not np.isnan(a).any() and not a.any() for a in out.values()), b
        else:
            assert out["seg"].any() and out["ref_end"].any() and out["dl_bounds"].any()
    if seed == CK.MIXED_SEED:
        assert 0 in counts and -1 in counts, counts
    checked = [b for b in range(kb.B) if counts[b] >= 1][:2]
    assert checked
    for b in checked:
        worst, n = corridor_against_yardstick(kb, b, variant, (name, kb.B, b, variant), seed=seed)
        print(name, b, variant, "segments", n, "worst error / tolerance:", worst)


@pytest.mark.parametrize("variant", [0, 1])
def test_corridor_host_twin_beyond_16_segments(variant):
    kb = CK.tied(CK.TIED_SEED)
    worst, n = corridor_against_yardstick(kb, 0, variant, ("tied", CK.TIED_SEED, 0, variant), seg_stride=CK.TIED_STRIDE, seed=7)
    assert n > 16
    print("tied", variant, "segments", n, "worst error / tolerance:", worst)


def adjoint_gap(lhs_terms, rhs_terms):
    """|sum lhs - sum rhs| and the linear rounding bound 8 n 2^-53 sum |terms|, n the length of the longer sum, the terms the
    products ybar_r (J t)_r and (J' ybar)_c t_c of the two sums."""
    lhs_terms, rhs_terms = np.asarray(lhs_terms).ravel(), np.asarray(rhs_terms).ravel()
    n = max(lhs_terms.size, rhs_terms.size)
    bound = 8.0 * n * 2.0 ** -53 * float(np.abs(lhs_terms).sum() + np.abs(rhs_terms).sum())
    return abs(float(lhs_terms.sum()) - float(rhs_terms.sum())), bound


@pytest.mark.parametrize("variant", [0, 1])
def test_corridor_adjoint_identity_against_the_backward_twin(variant):
    worst = 0.0
    for name, kb, stride in (("scenario", CK.scenario(2), CK.SEG_STRIDE), ("c1", CK.c1(2), CK.SEG_STRIDE),
                             ("fuzz", CK.fuzz(CK.FUZZ_SEEDS[1]), CK.SEG_STRIDE), ("tied", CK.tied(CK.TIED_SEED), CK.TIED_STRIDE)):
        sb, rb, db = CK.cotangents(kb.B, seed=11, seg_stride=stride)
        tans = S.corridor_tangents(kb, 2, seed=12)
        for b in range(min(kb.B, 2)):
            g, n = CK.host_grads(kb, b, variant, sb, rb, db, seg_stride=stride)
            out, count = corridor_host(kb, b, variant, {k: v[:, b] for k, v in tans.items()}, seg_stride=stride)
            assert n == count
            for t in range(2):
                lhs = np.concatenate([(sb[:, b] * out["seg"][t]).ravel(), rb[b] * out["ref_end"][t], db[b] * out["dl_bounds"][t]])
                rhs = np.concatenate([(g[k] * tans[k][t, b]).ravel() for k in native.KNOT_GRADS])
                gap, bound = adjoint_gap(lhs, rhs)
                assert gap <= bound, (name, b, t, gap, bound)
                worst = max(worst, gap / bound if bound else 0.0)
    print("corridor adjoint identity, worst gap / bound:", worst)


def test_corridor_many_tangents_equal_single_calls_and_null_arrays():
    kb = CK.scenario(2)
    T = 5
    tans = {k: v[:, 0] for k, v in S.corridor_tangents(kb, T, seed=4).items()}
    out, n = corridor_host(kb, 0, 0, tans)
    for t in range(T):
        one, _ = corridor_host(kb, 0, 0, {k: v[t:t + 1] for k, v in tans.items()})
        assert all(one[k][0].tobytes() == out[k][t].tobytes() for k in out), t
    # a missing tangent is zero; any subset of the outputs is the same numbers
    only_s, _ = corridor_host(kb, 0, 0, {"s_bounds": tans["s_bounds"]})
    zeros = {k: (v if k == "s_bounds" else np.zeros_like(v)) for k, v in tans.items()}
    full, _ = corridor_host(kb, 0, 0, zeros)
    assert all(np.array_equal(only_s[k], full[k]) for k in full) and not only_s["ref_end"].any() and only_s["seg"].any()
    for want in (("seg",), ("ref_end", "dl_bounds"), ("dl_bounds",)):
        part, _ = corridor_host(kb, 0, 0, tans, want=want)
        assert set(part) == set(want) and all(np.array_equal(part[k], out[k]) for k in want)
    # the rules of ref_end and dl_bounds, read off directly
    assert np.array_equal(out["ref_end"], np.stack([tans["s_ref"][:, -1], tans["l_ref"][:, -1]], axis=1))
    assert np.array_equal(out["dl_bounds"], tans["dl_bounds_knots"][:, :5].reshape(T, 10))


def test_corridor_cuboid_l_lines_and_ds_defaults():
    kb = CK.scenario(1)
    tans = {k: v[:, 0] for k, v in S.corridor_tangents(kb, 1, seed=2).items()}
    out1, n1 = corridor_host(kb, 0, 1, tans)
    assert n1 >= 1 and out1["seg"][0, L.F_BEG_L, :n1].all()
    for f in (L.F_L_DOWN_BIAS, L.F_L_DOWN_SKEW, L.F_L_UPP_BIAS, L.F_L_UPP_SKEW):
        assert not out1["seg"][0, f].any()
    # a plateau of ds_bounds: the earliest knot of the final span supplies the tangent; the defaults: nobody
    (n, spans, _), _ = CR.record(CR.one_candidate(kb, 0), 0)
    kb.ds_bounds[0, :, 0] = 0.5; kb.ds_bounds[0, :, 1] = 7.0
    out, count = corridor_host(kb, 0, 0, tans)
    first = [min(max(bt, 0), kb.N - 1) for bt, _ in spans]
    assert count == n and np.array_equal(out["seg"][0, L.F_DS_LO, :n], tans["ds_bounds"][0, first, 0])
    assert np.array_equal(out["seg"][0, L.F_DS_HI, :n], tans["ds_bounds"][0, first, 1])
    kb.ds_bounds[0, :, 0] = -1.0; kb.ds_bounds[0, :, 1] = 2000.0
    out, _ = corridor_host(kb, 0, 0, tans)
    assert not out["seg"][0, L.F_DS_LO].any() and not out["seg"][0, L.F_DS_HI].any() and out["seg"][0, L.F_DOWN_BIAS].any()


def test_corridor_host_refusals():
    kb = CK.scenario(1)
    tans = {k: v[:, 0] for k, v in S.corridor_tangents(kb, 1).items()}
    corridor_host(kb, 0, 0, tans)
    with pytest.raises(native.BtrapzError):
        corridor_host(kb, 0, 0, {})                                            # every tangent NULL (and T = 0)
    with pytest.raises(native.BtrapzError):
        corridor_host(kb, 0, 0, tans, want=())                                 # every output NULL
    with pytest.raises(native.BtrapzError):
        corridor_host(kb, 0, 0, {k: np.repeat(v, 33, axis=0) for k, v in tans.items()})   # T = 33
    with pytest.raises(native.BtrapzError):
        corridor_host(kb, 0, 0, tans, seg_stride=65)
    with pytest.raises(native.BtrapzError):
        corridor_host(kb, 0, 2, tans)
    with pytest.raises(ValueError):
        corridor_host(kb, 0, 0, {"seg": tans["s_ref"]})
    with pytest.raises(ValueError):
        corridor_host(kb, 0, 0, {"s_ref": tans["s_ref"][:, :-1]})
    # the C entry point itself: NULL tangents struct, N beyond the wave-wide kernels
    z = np.zeros(4)
    p = native._np_ptr(z)
    t = native.CKnotTangents(p, None, None, None, None, None)
    f = native.lib().btrapz_corridor_jvp_host
    assert f(0, 3, 1, 0.1, p, p, p, p, p, p, 16, 1, None, p, None, None, None) == -1
    assert f(0, 513, 1, 0.1, p, p, p, p, p, p, 16, 1, C.byref(t), p, None, None, None) == -1
    assert f(0, 3, 65, 0.1, p, p, p, p, p, p, 16, 1, C.byref(t), p, None, None, None) == -1
    assert f(0, 3, 1, 0.1, None, p, p, p, p, p, 16, 1, C.byref(t), p, None, None, None) == -1
    assert f(0, 3, 1, 0.1, p, p, p, p, p, p, 16, 0, C.byref(t), p, None, None, None) == -1


# ---- prism stage -------------------------------------------------------------------------------------------------------
def prism_against_yardstick(pr, N, O, key, T=T_YARD, seed=3):
    """Host twin against J @ t on every scene of pr [B, P, 8]; returns the worst error / tolerance."""
    B = pr.shape[0]
    jacs = [PR.jacobian(pr[b], N, key=(key, b)) for b in range(B)]
    PR.check_cap(jacs)
    tdot = S.prism_tangents(pr, T, seed=seed)
    for b, jac in enumerate(jacs):
        for t in range(T):
            tdot[t, b] = S.zero_skipped_prism(jac, tdot[t, b])
    s_dot, l_dot = native.prism_bounds_jvp_host(pr, N, O, tdot)
    assert not np.isnan(s_dot).any() and not np.isnan(l_dot).any()
    return max(S.prism_compare(jac, pr[b], tdot[t, b], s_dot[t, b], l_dot[t, b], O, (key, b, t)) for b, jac in enumerate(jacs) for t in range(T))


@pytest.mark.parametrize("name", ["golden", "nice", "plain", "tied"])
def test_prism_host_twin_against_yardstick(name):
    pr, N, O = PK.scene_sets()[name]
    print(name, "worst error / tolerance:", prism_against_yardstick(pr, N, O, name))


def test_prism_sixteen_cars_33_strips():
    pr = PK.pack(PK.sixteen_cars(), 16)
    N = 65
    for O in (33, 34):
        print("O", O, "worst error / tolerance:", prism_against_yardstick(pr, N, O, "sixteen", seed=O))
    tdot = S.prism_tangents(pr, 2)
    s_dot, l_dot = native.prism_bounds_jvp_host(pr, N, 32, tdot)       # 33 strips, O = 32: the forward's n_strips = -1
    assert not s_dot.any() and not l_dot.any() and not np.isnan(s_dot).any() and not np.isnan(l_dot).any()


def test_prism_adjoint_identity_against_the_backward_twin():
    worst = 0.0
    for name in ("golden", "plain", "nice", "tied"):
        pr, N, O = PK.scene_sets()[name]
        pr = pr[:12]
        B = pr.shape[0]
        sbar, lbar = PK.cotangents(B, O, N, seed=5)
        g = native.prism_bounds_vjp_host(pr, N, O, sbar, lbar)
        tdot = np.nan_to_num(S.prism_tangents(pr, 2, seed=6), nan=0.0)
        s_dot, l_dot = native.prism_bounds_jvp_host(pr, N, O, tdot)
        for b in range(B):
            for t in range(2):
                lhs = np.concatenate([(sbar[b] * s_dot[t, b]).ravel(), (lbar[b] * l_dot[t, b]).ravel()])
                gap, bound = adjoint_gap(lhs, g[b] * tdot[t, b])
                assert gap <= bound, (name, b, t, gap, bound)
                worst = max(worst, gap / bound if bound else 0.0)
    print("prism adjoint identity, worst gap / bound:", worst)


def test_prism_many_tangents_equal_single_calls_and_null_outputs():
    pr, N, O = PK.scene_sets()["plain"]
    pr = pr[:10]
    T = 5
    tdot = S.prism_tangents(pr, T, seed=8)
    s_dot, l_dot = native.prism_bounds_jvp_host(pr, N, O, tdot)
    assert s_dot.any() and l_dot.any()
    for t in range(T):
        s1, l1 = native.prism_bounds_jvp_host(pr, N, O, tdot[t:t + 1])
        assert s1[0].tobytes() == s_dot[t].tobytes() and l1[0].tobytes() == l_dot[t].tobytes()
    s_only, none = native.prism_bounds_jvp_host(pr, N, O, tdot, want=("s_bounds",))
    assert none is None and s_only.tobytes() == s_dot.tobytes()
    none, l_only = native.prism_bounds_jvp_host(pr, N, O, tdot, want=("l_bounds",))
    assert none is None and l_only.tobytes() == l_dot.tobytes()


def test_prism_defined_cases():
    """A lone car with l0 = 3, vel_l = 0.25, t0 = 1, T = 3 (prism_vjp_cases' behind_vel_l_positive): edges -2, 5/3, 3 + 0.75 +
    4/3, 8; the front face is the lower bound of strip 1 at knots 10..40."""
    N, O = PK.N_KNOTS, 4
    car = [12.0, 3.0, 1.0, 2.5, 0.25, 3.0, 1.0, 0.0]
    off = [33.0, 2.0, 0.0, 9.0, 0.25, 3.0, 0.0, 0.0]
    pr = np.array([[off, car]])
    d = np.array([[[[np.nan] * 8, [0.5, -1.5, 0.25, 2.0, 3.0, -0.75, np.nan, np.nan]]]])
    s_dot, l_dot = native.prism_bounds_jvp_host(pr, N, O, d)
    s_dot, l_dot = s_dot[0, 0], l_dot[0, 0]
    moving = (-1.5 + 3.0 * 3.0) + 0.25 * -0.75
    want_l = np.zeros((O, N, 2))
    want_l[0, :, 1] = -1.5; want_l[1, :, 0] = -1.5; want_l[1, :, 1] = moving; want_l[2, :, 0] = moving
    assert np.array_equal(l_dot, want_l)
    want_s = np.zeros((O, N, 2))
    i = np.arange(10, 41)
    want_s[1, 10:41, 0] = (0.5 + 2.0 * (i / 10.0 - 1.0)) - 2.5 * 0.25
    assert np.array_equal(s_dot, want_s)
    # vel_l < 0: the LOWER end moves; the padding strip stays 0
    pr[0, 1, 4] = -0.25
    _, l_dot = native.prism_bounds_jvp_host(pr, N, O, d)
    moving = (-1.5 + 3.0 * 3.0) + -0.25 * -0.75
    assert np.array_equal(l_dot[0, 0, 1, 0], [moving, -1.5]) and not l_dot[0, 0, 3].any()
    # more strips than O: zeros everywhere
    s_dot, l_dot = native.prism_bounds_jvp_host(pr, N, 2, d)
    assert not s_dot.any() and not l_dot.any()


def test_prism_host_refusals():
    pr, N, O = PK.scene_sets()["plain"]
    pr = pr[:2]
    tdot = np.zeros((1,) + pr.shape)
    native.prism_bounds_jvp_host(pr, N, O, tdot)
    for kw in (dict(N=0), dict(O=0)):
        with pytest.raises(native.BtrapzError):
            native.prism_bounds_jvp_host(pr, kw.get("N", N), kw.get("O", O), tdot)
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_jvp_host(pr, N, O, np.zeros((33,) + pr.shape))                 # T = 33
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_jvp_host(pr, N, O, np.zeros((0,) + pr.shape))                  # T = 0
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_jvp_host(pr, N, O, tdot, want=())                              # both outputs NULL
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_jvp_host(pr, N, O, None)                                       # prisms_dot NULL
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_jvp_host(np.zeros((1, 17, 8)), N, O, np.zeros((1, 1, 17, 8)))  # P > 16
    bad = native.CRoad.reference(); bad.knots_per_second = 0.0
    with pytest.raises(native.BtrapzError):
        native.prism_bounds_jvp_host(pr, N, O, tdot, road=bad)
    with pytest.raises(ValueError):
        native.prism_bounds_jvp_host(pr, N, O, tdot[:, :1])
    f = native.lib().btrapz_prism_bounds_jvp_host
    p = native._np_ptr(np.zeros(64))
    assert f(1, 1, 1, None, p, 1, 1, p, p, p) == -1 and f(1, 1, 1, C.byref(native.CRoad.reference()), None, 1, 1, p, p, p) == -1
