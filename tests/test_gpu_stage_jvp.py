"""The forward-mode derivatives of the prism and corridor stages on the GPU (btrapz_prism_bounds_jvp_device,
btrapz_corridor_batch_jvp_device): against their host twins BIT FOR BIT at every edge of the lane mapping, against the
yardstick of tests/stage_jvp_reference.py on one candidate per family, against the device backward passes through the adjoint
identity, their defined cases, determinism and refusals; then the chain prisms -> bounds -> record -> control points
(diff.scene_jacobian, diff.trajectory_spread) against autograd and against central differences of the whole pipeline."""
import copy

import numpy as np
import pytest
import torch

import corridor_vjp_cases as CK
import corridor_vjp_reference as CR
import prism_vjp_cases as PK
import prism_vjp_reference as PR
import stage_jvp_reference as S
from spectral_amd import diff, layout as L, native, synth
from spectral_amd.native import BtrapzError, KNOT_GRADS
from test_stage_jvp import adjoint_gap, corridor_host

pytestmark = pytest.mark.gpu
OUTS = ("seg", "ref_end", "dl_bounds")


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def dev(solver, a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(solver.device, dtype=torch.float64).contiguous()


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- corridor stage ------------------------------------------------------------------------------------------------------
def device_corridor(solver, kb, variant, tans, seg_stride=CK.SEG_STRIDE):
    o = solver.corridor_batch_jvp(kb, variant, {k: dev(solver, v) for k, v in tans.items()}, seg_stride=seg_stride)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in OUTS}


def host_corridor(kb, variant, tans, seg_stride=CK.SEG_STRIDE):
    """The host twin over every candidate, in the device call's shapes; and the counts."""
    T = next(iter(tans.values())).shape[0]
    out = dict(seg=np.zeros((T, L.NUM_SEG_FIELDS, kb.B, seg_stride)), ref_end=np.zeros((T, kb.B, 2)), dl_bounds=np.zeros((T, kb.B, 10)))
    counts = []
    for b in range(kb.B):
        h, n = corridor_host(kb, b, variant, {k: v[:, b] for k, v in tans.items()}, seg_stride=seg_stride)
        out["seg"][:, :, b], out["ref_end"][:, b], out["dl_bounds"][:, b] = h["seg"], h["ref_end"], h["dl_bounds"]
        counts.append(n)
    return out, np.array(counts)


def three_knots(B):
    """The first three knots of the scenario batch: the stage's minimum horizon."""
    kb = copy.copy(CK.scenario(B))
    kb.N = 3
    for name in ("s_bounds", "l_bounds"):
        setattr(kb, name, np.ascontiguousarray(getattr(kb, name)[:, :, :3]))
    for name in ("ds_bounds", "dl_bounds", "s_ref", "l_ref"):
        setattr(kb, name, np.ascontiguousarray(getattr(kb, name)[:, :3]))
    return kb


def corridor_families():
    """(name, batch, seg_stride): B = 1 and 3; N = 3, 71 x 3 obstacles (with candidates of seg_count 0 and -1), 201 at stride
    32 (more than 16 segments), 401 at stride 64 (64, 60, 63 segments and the overflow candidate)."""
    return [("scenario1", CK.scenario(1), CK.SEG_STRIDE), ("c1x3", CK.c1(3), CK.SEG_STRIDE), ("knots3", three_knots(3), CK.SEG_STRIDE),
            ("fuzz1", CK.fuzz(1), CK.SEG_STRIDE), ("mixed", CK.fuzz(CK.MIXED_SEED), CK.SEG_STRIDE),
            ("tied", CK.tied(CK.TIED_SEED), CK.TIED_STRIDE), ("full", CK.full(), 64)]


@pytest.mark.parametrize("variant", [0, 1])
def test_corridor_kernel_equals_host_twin(solver, variant):
    seen = set()
    for name, kb, stride in corridor_families():
        tans = S.corridor_tangents(kb, 2, seed=3)
        got = device_corridor(solver, kb, variant, tans, stride)
        host, counts = host_corridor(kb, variant, tans, stride)
        rec = solver.corridor_batch(kb, variant, seg_stride=stride)
        assert np.array_equal(rec["seg_count"].cpu().numpy(), counts), (name, counts)
        for k in OUTS:
            assert same_bits(got[k], host[k]), (name, k, np.argwhere(got[k] != host[k])[:5])
        for b in range(kb.B):
            if counts[b] < 1:
                assert all(not got[k][:, ..., b, :].any() for k in OUTS), (name, b)
            else:
                assert got["seg"][:, 1:, b, :counts[b]].any() and not got["seg"][:, :, b, counts[b]:].any() and not got["seg"][:, 0].any()
        seen |= set(int(c) for c in counts)
        print(name, "variant", variant, "counts", counts)
    assert {0, -1, 64, 63, 60, 1} <= seen and any(16 < c <= 26 for c in seen), sorted(seen)


@pytest.mark.parametrize("variant", [0, 1])
def test_corridor_kernel_against_yardstick(solver, variant):
    for name, kb, b, key, stride in (("scenario", CK.scenario(2), 0, ("scenario", 2, 0, variant), CK.SEG_STRIDE),
                                     ("tied", CK.tied(CK.TIED_SEED), 0, ("tied", CK.TIED_SEED, 0, variant), CK.TIED_STRIDE)):
        jac = CR.jacobian(kb, b, variant, key=key)
        CR.check_caps(jac)
        tans = S.corridor_tangents(kb, 2, seed=5)
        for t in range(2):                                  # zero the skipped columns of the checked candidate
            z = S.zero_skipped_corridor(jac, {k: v[t, b] for k, v in tans.items()})
            for k in z:
                tans[k][t, b] = z[k]
        got = device_corridor(solver, kb, variant, tans, stride)
        n = jac["n"]
        x = S.corridor_inputs(kb, b)
        worst = max(S.corridor_compare(jac, x, {k: v[t, b] for k, v in tans.items()},
                                       S.corridor_flat(n, got["seg"][t, :, b], got["ref_end"][t, b], got["dl_bounds"][t, b]), (name, t))
                    for t in range(2))
        print(name, "variant", variant, "segments", n, "worst error / tolerance:", worst)


def test_corridor_tangent_counts_determinism_and_overwrite(solver):
    kb = CK.fuzz(CK.MIXED_SEED)                              # seg_count 0, 16, 7 and -1
    B, N, O, stride = kb.B, kb.N, kb.num_obs, CK.SEG_STRIDE
    tans = S.corridor_tangents(kb, 32, seed=6)
    full = device_corridor(solver, kb, 0, tans)
    again = device_corridor(solver, kb, 0, tans)
    assert all(same_bits(full[k], again[k]) for k in OUTS) and full["seg"].any()
    for T in (1, 2):
        part = device_corridor(solver, kb, 0, {k: v[:T] for k, v in tans.items()})
        assert all(same_bits(part[k], full[k][:T]) for k in OUTS), T
    for t in (5, 31):                                        # one call of 32 against calls of one
        one = device_corridor(solver, kb, 0, {k: v[t:t + 1] for k, v in tans.items()})
        assert all(same_bits(one[k][0], full[k][t]) for k in OUTS), t
    with pytest.raises(BtrapzError, match="BTRAPZ_MAX_TANGENTS"):
        solver.corridor_batch_jvp(kb, 0, {k: dev(solver, np.repeat(v[:1], 33, axis=0)) for k, v in tans.items()})
    # NaN-prefilled outputs come back fully overwritten -- candidates without a corridor and unused slots included
    ins = [dev(solver, a) for a in (kb.s_bounds, kb.l_bounds, kb.ds_bounds, kb.dl_bounds, kb.s_ref, kb.l_ref)]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=solver.device)
    T = 3
    seg, re, dl = nan(T, L.NUM_SEG_FIELDS, B, stride), nan(T, B, 2), nan(T, B, 10)
    t3 = {k: dev(solver, v[:T]) for k, v in tans.items()}
    solver.ctx.corridor_batch_jvp_device(0, B, N, O, kb.delta, *ins, stride, T, t3, seg, re, dl)
    torch.cuda.synchronize()
    assert not torch.isnan(seg).any() and not torch.isnan(re).any() and not torch.isnan(dl).any()
    assert same_bits(seg.cpu().numpy(), full["seg"][:T]) and same_bits(re.cpu().numpy(), full["ref_end"][:T])
    # any subset of the outputs: the same numbers, the others untouched; a missing tangent is zero
    seg2, dl2 = nan(T, L.NUM_SEG_FIELDS, B, stride), nan(T, B, 10)
    solver.ctx.corridor_batch_jvp_device(0, B, N, O, kb.delta, *ins, stride, T, t3, seg2, None, None)
    solver.ctx.corridor_batch_jvp_device(0, B, N, O, kb.delta, *ins, stride, T, t3, None, None, dl2)
    torch.cuda.synchronize()
    assert torch.equal(seg2, seg) and torch.equal(dl2, dl)
    only_s = device_corridor(solver, kb, 0, {"s_bounds": tans["s_bounds"][:T]})
    zeros = {k: (v[:T] if k == "s_bounds" else np.zeros_like(v[:T])) for k, v in tans.items()}
    ref = device_corridor(solver, kb, 0, zeros)
    assert all(np.array_equal(only_s[k], ref[k]) for k in OUTS) and not only_s["ref_end"].any() and only_s["seg"].any()


def test_corridor_refusals_and_python_checks(solver):
    d = solver.device
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=d)

    def call(B=2, N=21, O=2, S=16, T=2, outs=(True, True, True), tan=("s_bounds",)):
        ins = [z(B, O, N, 2), z(B, O, N, 2), z(B, N, 2), z(B, N, 2), z(B, N), z(B, N)]
        tn = max(T, 1)
        t = {k: z(tn, *ins[KNOT_GRADS.index(k)].shape) for k in tan} if tan is not None else None
        solver.ctx.corridor_batch_jvp_device(0, B, N, O, 0.1, *ins, S, T, t, z(tn, L.NUM_SEG_FIELDS, B, S) if outs[0] else None,
                                             z(tn, B, 2) if outs[1] else None, z(tn, B, 10) if outs[2] else None)
    call(); call(outs=(False, True, False)); call(tan=("l_ref", "ds_bounds"))
    for kw, text in ((dict(N=513), "not differentiated"), (dict(O=65), "not differentiated"), (dict(S=65), "not differentiated"),
                     (dict(outs=(False, False, False)), "all null"), (dict(tan=()), "no tangent"), (dict(tan=None), "no tangent"),
                     (dict(N=2), "N >= 3"), (dict(T=0), "BTRAPZ_MAX_TANGENTS"), (dict(T=33), "BTRAPZ_MAX_TANGENTS")):
        with pytest.raises(BtrapzError, match=text):
            call(**kw)
    torch.cuda.synchronize()
    kb = CK.scenario(2)
    tans = {k: dev(solver, v) for k, v in S.corridor_tangents(kb, 2).items()}
    with pytest.raises(ValueError, match="unknown"):
        solver.corridor_batch_jvp(kb, 0, {"seg": tans["s_ref"]})
    with pytest.raises(ValueError, match="shape"):
        solver.corridor_batch_jvp(kb, 0, {"s_ref": tans["s_ref"][:, :, :-1]})
    with pytest.raises(ValueError, match="delta"):
        solver.corridor_batch_jvp([dev(solver, a) for a in (kb.s_bounds, kb.l_bounds, kb.ds_bounds, kb.dl_bounds, kb.s_ref, kb.l_ref)], 0, tans)


@pytest.mark.parametrize("variant", [0, 1])
def test_corridor_adjoint_identity_against_the_device_backward(solver, variant):
    worst = 0.0
    for name, kb, stride in corridor_families()[1:6]:
        sb, rb, db = CK.cotangents(kb.B, seed=11, seg_stride=stride)
        tans = S.corridor_tangents(kb, 2, seed=12)
        got = device_corridor(solver, kb, variant, tans, stride)
        g = solver.corridor_batch_vjp(kb, variant, dev(solver, sb), dev(solver, rb), dev(solver, db), seg_stride=stride)
        torch.cuda.synchronize()
        g = {k: g[k].cpu().numpy() for k in KNOT_GRADS}
        for b in range(kb.B):
            for t in range(2):
                lhs = np.concatenate([(sb[:, b] * got["seg"][t, :, b]).ravel(), rb[b] * got["ref_end"][t, b], db[b] * got["dl_bounds"][t, b]])
                rhs = np.concatenate([(g[k][b] * tans[k][t, b]).ravel() for k in KNOT_GRADS])
                gap, bound = adjoint_gap(lhs, rhs)
                assert gap <= bound, (name, b, t, gap, bound)
                worst = max(worst, gap / bound if bound else 0.0)
    print("corridor adjoint identity on the device, variant", variant, "worst gap / bound:", worst)


# ---- prism stage ---------------------------------------------------------------------------------------------------------
def device_prism(solver, pr, N, O, tdot):
    s, l = solver.prism_bounds_jvp(dev(solver, pr), N, O, dev(solver, tdot))
    torch.cuda.synchronize()
    return s.cpu().numpy(), l.cpu().numpy()


def prism_against_both(solver, pr, N, O, key, T=2, seed=3, yardstick=True):
    """Kernel == host twin bit for bit; kernel against the yardstick on every scene; returns the worst error / tolerance."""
    B = pr.shape[0]
    tdot = S.prism_tangents(pr, T, seed=seed)
    jacs = None
    if yardstick:
        jacs = [PR.jacobian(pr[b], N, key=(key, b)) for b in range(B)]
        PR.check_cap(jacs)
        for b, jac in enumerate(jacs):
            for t in range(T):
                tdot[t, b] = S.zero_skipped_prism(jac, tdot[t, b])
    s, l = device_prism(solver, pr, N, O, tdot)
    hs, hl = native.prism_bounds_jvp_host(pr, N, O, tdot)
    assert same_bits(s, hs) and same_bits(l, hl), (key, np.argwhere(s != hs)[:5], np.argwhere(l != hl)[:5])
    assert not np.isnan(s).any() and not np.isnan(l).any()
    if not yardstick:
        return 0.0
    return max(S.prism_compare(jac, pr[b], tdot[t, b], s[t, b], l[t, b], O, (key, b, t)) for b, jac in enumerate(jacs) for t in range(T))


@pytest.mark.parametrize("name", ["golden", "nice", "plain", "tied"])
def test_prism_kernel_against_yardstick_and_host_twin(solver, name):
    pr, N, O = PK.scene_sets()[name]
    print(name, "worst error / tolerance:", prism_against_both(solver, pr, N, O, name))


@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 71, 129])
def test_prism_lane_mapping_edges(solver, N):
    """Knot counts around the wavefront's 64 lanes, with P = 1, 2, 3; B = 1, and B = 3 with 2 / 3 / 1 active cars."""
    scenes = PK.random_scenes(40, 100 + N, max_cars=3)
    by_count = {n: [s for s in scenes if len(s) == n] for n in (1, 2, 3)}
    worst = 0.0
    for P in (1, 2, 3):
        worst = max(worst, prism_against_both(solver, PK.pack(by_count[P][:1], P), N, 2 * P + 1, ("lanes", N, P, 1)))
    mixed = [by_count[2][1], by_count[3][1], by_count[1][1]]
    worst = max(worst, prism_against_both(solver, PK.pack(mixed, 3), N, 7, ("lanes", N, 3, 3)))
    print("N", N, "worst error / tolerance:", worst)


def test_prism_sixteen_cars_33_strips(solver):
    pr = PK.pack(PK.sixteen_cars(), 16)
    N = 65
    for O in (33, 34):
        print("O", O, "worst error / tolerance:", prism_against_both(solver, pr, N, O, "sixteen", seed=O))
    tdot = S.prism_tangents(pr, 32, seed=1)                  # 16 cars x 32 directions: the largest staging area
    s, l = device_prism(solver, pr, N, 32, tdot)             # 33 strips, O = 32: the forward's n_strips = -1
    assert not s.any() and not l.any() and not np.isnan(s).any() and not np.isnan(l).any()
    prism_against_both(solver, pr, N, 33, "sixteen", T=32, seed=2, yardstick=False)


def test_prism_tangent_counts_determinism_and_overwrite(solver):
    pr, N, O = PK.scene_sets()["plain"]
    pr = pr[:40]
    B, P = pr.shape[0], pr.shape[1]
    assert (pr[:, :, 6] == 0).any()
    tdot = S.prism_tangents(pr, 32, seed=9)
    s, l = device_prism(solver, pr, N, O, tdot)
    s2, l2 = device_prism(solver, pr, N, O, tdot)
    assert same_bits(s, s2) and same_bits(l, l2) and s.any() and l.any()
    hs, hl = native.prism_bounds_jvp_host(pr, N, O, tdot)
    assert same_bits(s, hs) and same_bits(l, hl)
    for T in (1, 2):
        a, b = device_prism(solver, pr, N, O, tdot[:T])
        assert same_bits(a, s[:T]) and same_bits(b, l[:T]), T
    for t in (7, 31):
        a, b = device_prism(solver, pr, N, O, tdot[t:t + 1])
        assert same_bits(a[0], s[t]) and same_bits(b[0], l[t]), t
    # NaN-prefilled outputs come back fully overwritten: padding strips, inactive slots, overflowing scenes (O = 2)
    road = native.CRoad.reference()
    for O2 in (O, 2):
        T = 2
        so = torch.full((T, B, O2, N, 2), float("nan"), dtype=torch.float64, device=solver.device)
        lo = torch.full_like(so, float("nan"))
        solver.ctx.prism_bounds_jvp_device(B, P, N, road, dev(solver, pr), O2, T, dev(solver, tdot[:T]), so, lo)
        torch.cuda.synchronize()
        assert not torch.isnan(so).any() and not torch.isnan(lo).any()
    # either output alone: the same numbers
    so = torch.full((2, B, O, N, 2), float("nan"), dtype=torch.float64, device=solver.device)
    lo = torch.full_like(so, float("nan"))
    solver.ctx.prism_bounds_jvp_device(B, P, N, road, dev(solver, pr), O, 2, dev(solver, tdot[:2]), so, None)
    solver.ctx.prism_bounds_jvp_device(B, P, N, road, dev(solver, pr), O, 2, dev(solver, tdot[:2]), None, lo)
    torch.cuda.synchronize()
    assert same_bits(so.cpu().numpy(), s[:2]) and same_bits(lo.cpu().numpy(), l[:2])


def test_prism_refusals(solver):
    d = solver.device
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=d)
    road = native.CRoad.reference()

    def call(B=2, P=3, N=21, O=4, T=2, outs=(True, True), road=road, prisms=True, dots=True):
        b, p, n, o, t = max(B, 1), max(P, 1), max(N, 1), max(O, 1), max(T, 1)
        solver.ctx.prism_bounds_jvp_device(B, P, N, road, z(b, p, 8) if prisms else None, O, T, z(t, b, p, 8) if dots else None,
                                           z(t, b, o, n, 2) if outs[0] else None, z(t, b, o, n, 2) if outs[1] else None)
    call(); call(outs=(True, False)); call(outs=(False, True)); call(T=32)
    bad_road = native.CRoad.reference(); bad_road.knots_per_second = 0.0
    for kw, text in ((dict(B=0), ">= 1"), (dict(P=0), ">= 1"), (dict(N=0), ">= 1"), (dict(O=0), ">= 1"), (dict(P=17), "P > 16"),
                     (dict(outs=(False, False)), "both null"), (dict(road=None), "non-null"), (dict(prisms=False), "non-null"),
                     (dict(dots=False), "non-null"), (dict(road=bad_road), "knots_per_second"), (dict(T=0), "BTRAPZ_MAX_TANGENTS"),
                     (dict(T=33), "BTRAPZ_MAX_TANGENTS")):
        with pytest.raises(BtrapzError, match=text):
            call(**kw)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="prisms_dot"):
        solver.prism_bounds_jvp(z(2, 3, 8), 21, 4, z(2, 2, 2, 8))


def test_prism_adjoint_identity_against_the_device_backward(solver):
    worst = 0.0
    for name in ("golden", "plain", "nice", "tied"):
        pr, N, O = PK.scene_sets()[name]
        pr = pr[:24]
        B = pr.shape[0]
        sbar, lbar = PK.cotangents(B, O, N, seed=5)
        g = solver.prism_bounds_vjp(dev(solver, pr), N, O, dev(solver, sbar), dev(solver, lbar)).cpu().numpy()
        tdot = np.nan_to_num(S.prism_tangents(pr, 2, seed=6), nan=0.0)
        s, l = device_prism(solver, pr, N, O, tdot)
        for b in range(B):
            for t in range(2):
                lhs = np.concatenate([(sbar[b] * s[t, b]).ravel(), (lbar[b] * l[t, b]).ravel()])
                gap, bound = adjoint_gap(lhs, g[b] * tdot[t, b])
                assert gap <= bound, (name, b, t, gap, bound)
                worst = max(worst, gap / bound if bound else 0.0)
    print("prism adjoint identity on the device, worst gap / bound:", worst)


# ---- the chain: prisms -> bounds -> record -> control points ------------------------------------------------------------
LATERAL = {1: "l0", 4: "vel_l", 5: "T"}
E2E = dict(B=8, N=71, O=5, stride=24)


@pytest.fixture(scope="module")
def constellation(solver):
    """The harness constellation of tests/test_gpu_prism_vjp.py::test_prisms_to_traj_cost_against_central_differences (copied:
    that file stays as it is): 8 scenes, two cars, the car beside the ego drifting sideways in half of the scenes."""
    B, N = E2E["B"], E2E["N"]
    rng = np.random.default_rng(7)
    scenes = []
    for b in range(B):
        scenes.append([dict(centre=(float(rng.uniform(18, 30)), 1.2, 0), vel_s=float(rng.uniform(3, 5)), vel_l=0.0, time=4.0),
                       dict(centre=(float(rng.uniform(5, 15)), 4.2, 0), vel_s=float(rng.uniform(5, 7)), vel_l=(0.05 if b % 4 == 1 else -0.05) if b % 2 else 0.0, time=4.03 if b % 2 else 4.0)])
    pr = PK.pack(scenes, 2)
    tt = np.arange(N) * 0.1
    s_ref = np.tile(40.0 / 7.0 * tt, (B, 1)); l_ref = np.tile(np.clip(1.2 + 0.0825 * (np.arange(N) - 15), 1.2, 4.5), (B, 1))
    init = np.zeros((B, 6)); init[:, 1] = 6.0; init[:, 3] = 1.2
    dsb = np.tile(np.array([0.0, 20.0]), (B, N, 1)); dlb = np.tile(np.array([-3.0, 3.0]), (B, N, 1))
    sh = synth.make_scenario1_batch(1, 7, 0)[1]
    prm = torch.tensor(diff.params_from_shared(sh), device=solver.device)
    return dict(pr=pr, s_ref=s_ref, l_ref=l_ref, init=init, dsb=dsb, dlb=dlb, sh=sh, prm=prm)


def scene_args(solver, c, rows=None):
    rows = np.arange(c["pr"].shape[0]) if rows is None else np.asarray(rows)
    return [dev(solver, c[k][rows]) for k in ("dsb", "dlb", "s_ref", "l_ref", "init")] + [c["prm"]]


def jacobian_of(solver, c, pr, pdot, rows=None, **kw):
    return diff.scene_jacobian(solver, dev(solver, pr), None if pdot is None else dev(solver, pdot), *scene_args(solver, c, rows), O=E2E["O"],
                               variant=0, delta=0.1, seg_stride=E2E["stride"], **kw)


def strictly_complementary(c, J):
    """The scenes that are solved and strictly complementary (tests/vjp_reference.Adjoint, as the copied test has it)."""
    from vjp_reference import Adjoint
    rec = J["rec"]
    stn, cn, segn = J["status"].cpu().numpy(), rec.seg_count.cpu().numpy(), rec.seg.cpu().numpy()
    ren, dln = rec.ref_end.cpu().numpy(), rec.dl_bounds.cpu().numpy()
    kept = []
    for b in range(len(stn)):
        if stn[b] in (1, 2) and cn[b] >= 1:
            n = int(cn[b])
            one = L.Batch(B=1, S=n, seg=np.ascontiguousarray(segn[:, b:b + 1, :n]), init=c["init"][b:b + 1].copy(), ref_end=ren[b:b + 1].copy(),
                          dl_bounds=dln[b:b + 1].copy())
            if Adjoint(one, c["sh"], np.zeros(12 * n), 0.0).strict:
                kept.append(b)
    return kept


def test_chained_adjoint_identity_against_autograd(solver, constellation):
    """<ctrl_bar, dctrl_t> from scene_jacobian against <prisms.grad, prisms_dot_t> from autograd through diff.prism_bounds ->
    diff.corridor -> diff.solve, on the solved scenes, to 1e-4 of the sum of |terms| (DESIGN 3.10's bound for the solve)."""
    c = constellation
    B, N, O, stride = E2E["B"], E2E["N"], E2E["O"], E2E["stride"]
    rng = np.random.default_rng(21)
    T = 4
    pdot = rng.standard_normal((T, B, 2, 8)); pdot[..., 6:] = 0.0
    J = jacobian_of(solver, c, c["pr"], pdot)
    solved = np.flatnonzero(np.isin(J["status"].cpu().numpy(), (1, 2)))
    assert solved.size >= 2, J["status"]
    ctrl_bar = rng.standard_normal((B, 12 * stride))
    p = dev(solver, c["pr"]).requires_grad_(True)
    dsb, dlb, sr, lr, ini, prm = scene_args(solver, c)
    sb, lb, ns = diff.prism_bounds(solver, p, N, O)
    seg, cnt, ref_end, dl10 = diff.corridor(solver, sb, lb, dsb, dlb, sr, lr, variant=0, delta=0.1, seg_stride=stride)
    ctrl, _, st = diff.solve(solver, seg, ini, ref_end, dl10, prm, seg_count=cnt, variant=0, delta=0.1)
    assert torch.equal(ctrl, J["ctrl"]) and torch.equal(st, J["status"]) and torch.equal(cnt, J["seg_count"]) and torch.equal(ns, J["n_strips"])
    (ctrl[torch.tensor(solved, device=solver.device)] * dev(solver, ctrl_bar[solved])).sum().backward()
    grad = p.grad.cpu().numpy()
    dctrl = J["dctrl"].cpu().numpy()
    assert dctrl[:, solved].any() and grad.any()
    worst = 0.0
    for t in range(T):
        lhs = (ctrl_bar[solved] * dctrl[t, solved]).ravel(); rhs = (grad * pdot[t]).ravel()
        gap, scale = abs(lhs.sum() - rhs.sum()), np.abs(lhs).sum() + np.abs(rhs).sum()
        print("direction", t, "<ctrl_bar, dctrl>", lhs.sum(), "<grad, prisms_dot>", rhs.sum(), "gap / sum |terms|: %.3e" % (gap / scale))
        assert gap <= 1e-4 * scale, (t, gap, scale)
        worst = max(worst, gap / scale)
    print("chained adjoint identity, worst gap / sum |terms|: %.3e" % worst)


def test_dctrl_along_lateral_parameters_against_central_differences(solver, constellation):
    """dctrl along l0 of every car and vel_l, T of a drifting car against central differences of the whole GPU pipeline,
    h = 1e-4 (1 + |x|), on the entries whose move changes no decision (the copied test's filter), to 1e-3 of the norm over
    the checked entries, on solved and strictly complementary scenes."""
    c = constellation
    pr, B, N = c["pr"], E2E["B"], E2E["N"]
    columns = [(q, k) for q in range(2) for k in LATERAL]
    pdot = np.zeros((len(columns), B, 2, 8))
    for i, (q, k) in enumerate(columns):
        pdot[i, :, q, k] = 1.0
    J = jacobian_of(solver, c, pr, pdot)
    kept = strictly_complementary(c, J)
    print("solved and strictly complementary:", kept)
    assert len(kept) >= 2
    stn, cn, nsn = J["status"].cpu().numpy(), J["seg_count"].cpu().numpy(), J["n_strips"].cpu().numpy()
    segn = J["rec"].seg.cpu().numpy()
    dctrl = J["dctrl"].cpu().numpy()
    entries = [(b, q, k) for b in kept for q in range(2) for k in LATERAL if k == 1 or pr[b, q, 4] != 0.0]
    M = len(entries)
    hs = np.array([1e-4 * (1.0 + abs(pr[b, q, k])) for b, q, k in entries])
    moved = np.concatenate([pr[[b for b, _, _ in entries]]] * 2)
    for i, (b, q, k) in enumerate(entries):
        moved[i, q, k] += hs[i]; moved[M + i, q, k] -= hs[i]
    rows = [b for b, _, _ in entries] * 2
    dsb, dlb, sr, lr, ini, prm = scene_args(solver, c, rows)        # the whole pipeline at the moved prisms, forward only
    sb2, lb2, ns2 = solver.prism_bounds(dev(solver, moved), N, E2E["O"])
    rec2 = solver.corridor_batch_tensors(0, N, 0.1, sb2, lb2, dsb, dlb, sr, lr, ini, seg_stride=E2E["stride"])
    o2 = diff.solve_kept(solver, rec2["seg"], rec2["init"], rec2["ref_end"], rec2["dl_bounds"], prm, seg_count=rec2["seg_count"], variant=0, delta=0.1)
    c2, st2, cnt2, ns2 = o2["ctrl"].cpu().numpy(), o2["status"].cpu().numpy(), rec2["seg_count"].cpu().numpy(), ns2.cpu().numpy()
    seg2 = rec2["seg"].cpu().numpy()
    windows = lambda a: [[tuple(not (i < car[2] * 10 or i > (car[2] + car[5]) * 10) for i in range(N)) for car in sc] for sc in a]
    w0, w2 = windows(pr), windows(moved)
    ok = np.array([w2[i] == w0[b] and st2[i] in (1, 2) and ns2[i] == nsn[b] and cnt2[i] == cn[b] and (seg2[L.F_T, i, :cn[b]] == segn[L.F_T, b, :cn[b]]).all()
                   for i, b in enumerate(rows)])
    usable = np.flatnonzero(ok[:M] & ok[M:])
    assert usable.size >= 4, (M, usable.size)
    fd = ((c2[:M] - c2[M:]) / (2 * hs[:, None]))[usable]
    an = np.array([dctrl[columns.index((entries[i][1], entries[i][2])), entries[i][0]] for i in usable])
    norm = float(np.linalg.norm(an))
    names = [(entries[i][0], entries[i][1], LATERAL[entries[i][2]]) for i in usable]
    print("checked entries (scene, car, parameter):", names)
    print("per entry |fd - an|.max / |an|:", [float(np.abs(fd[i] - an[i]).max() / max(np.linalg.norm(an[i]), 1e-300)) for i in range(len(usable))])
    print("norm", norm, "worst error / norm: %.3e" % (np.abs(fd - an).max() / norm))
    assert norm > 0 and np.abs(fd).max() > 1e-3
    assert np.abs(fd - an).max() <= 1e-3 * norm


def test_trajectory_spread(solver, constellation):
    c = constellation
    B, N, O, stride = E2E["B"], E2E["N"], E2E["O"], E2E["stride"]
    # a ninth scene whose reference line runs outside the road: no corridor, not solved
    pr = np.concatenate([c["pr"], c["pr"][:1]])
    cc = {k: (np.concatenate([v, v[:1]]) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    cc["l_ref"] = cc["l_ref"].copy(); cc["l_ref"][B] = 50.0
    sigma = np.zeros((B + 1, 2, 6))
    sigma[:, 1, 1] = 0.3; sigma[:, 1, 3] = 0.5; sigma[1::2, 1, 4] = 0.02; sigma[:, 0, 0] = 0.4
    args = scene_args(solver, cc)
    r = diff.trajectory_spread(solver, dev(solver, pr), dev(solver, sigma), *args, O=O, variant=0, delta=0.1, seg_stride=stride)
    J = r["jac"]
    status = J["status"].cpu().numpy()
    assert r["columns"] == [(0, 0), (1, 1), (1, 3), (1, 4)] and status[B] not in (1, 2) and np.isin(status[:B], (1, 2)).sum() >= 2
    spread, traj = r["spread"].cpu().numpy(), r["traj"].cpu().numpy()
    assert spread.shape == traj.shape and np.isnan(spread[B]).all()
    solved = np.flatnonzero(np.isin(status, (1, 2)))
    assert not np.isnan(spread[solved]).any() and spread[solved].any()
    # ... assembled by hand from scene_jacobian and sample_jvp
    pdot = np.zeros((4, B + 1, 2, 8))
    for i, (q, k) in enumerate(r["columns"]):
        pdot[i, :, q, k] = 1.0
    J2 = jacobian_of(solver, cc, pr, pdot)
    assert torch.equal(J2["dctrl"], J["dctrl"]) and torch.equal(J2["ctrl"], J["ctrl"])
    dy = diff.sample_jvp(solver, J2["dctrl"], J2["rec"].seg, seg_count=J2["rec"].seg_count, delta=0.1).cpu().numpy()
    var = np.zeros_like(traj)
    for i, (q, k) in enumerate(r["columns"]):
        var += (dy[i][:, :, :traj.shape[2]] * sigma[:, q, k][:, None, None]) ** 2
    assert np.allclose(spread[solved], np.sqrt(var)[solved], rtol=1e-14, atol=0.0)
    t2, n2 = solver.sample(J["rec"], J["ctrl"], torch.arange(B + 1), 0.1)
    assert torch.equal(t2, r["traj"]) and torch.equal(n2, r["npoints"])
    # sel: a subset, in its order
    sel = torch.tensor([int(solved[1]), B, int(solved[0])])
    rs = diff.trajectory_spread(solver, dev(solver, pr), dev(solver, sigma), *args, O=O, variant=0, delta=0.1, seg_stride=stride, sel=sel)
    ss = rs["spread"].cpu().numpy()
    assert np.isnan(ss[1]).all() and same_bits(ss[0], spread[solved[1]][:, :ss.shape[2]]) and same_bits(ss[2], spread[solved[0]][:, :ss.shape[2]])
    # 40 directions (two chunks of the stage kernels) equal the two chunks run separately, bit for bit; the solve's outputs
    # are untouched by the derivative launches in between
    rng = np.random.default_rng(5)
    p40 = rng.standard_normal((40, B + 1, 2, 8))
    sb, lb, _ = solver.prism_bounds(dev(solver, pr), N, O)
    rec = solver.corridor_batch_tensors(0, N, 0.1, sb, lb, *args[:4], args[4], seg_stride=stride)
    ref = diff.solve_kept(solver, rec["seg"], rec["init"], rec["ref_end"], rec["dl_bounds"], cc["prm"], seg_count=rec["seg_count"], variant=0, delta=0.1)
    ref = {k: ref[k].clone() for k in ("ctrl", "cost", "status", "lam")}
    J40 = jacobian_of(solver, cc, pr, p40)
    a, b = jacobian_of(solver, cc, pr, p40[:32]), jacobian_of(solver, cc, pr, p40[32:])
    assert J40["dctrl"].shape[0] == 40 and J40["dctrl"][:, torch.tensor(solved, device=solver.device)].any()
    assert torch.equal(J40["dctrl"], torch.cat([a["dctrl"], b["dctrl"]])) and torch.equal(J40["dcost"], torch.cat([a["dcost"], b["dcost"]]))
    torch.cuda.synchronize()
    for k in ("ctrl", "cost", "status"):
        assert same_bits(ref[k].cpu().numpy(), J40["out"][k].cpu().numpy()), k
    cn = J40["seg_count"].cpu().numpy()
    lam0, lam1 = ref["lam"].cpu().numpy(), J40["out"]["lam"].cpu().numpy()       # [2, 36, B, S]: a solve writes the slots of its segments
    for b in solved:
        assert cn[b] >= 1 and same_bits(np.ascontiguousarray(lam0[:, :, b, :cn[b]]), np.ascontiguousarray(lam1[:, :, b, :cn[b]])), b
    with pytest.raises(ValueError, match="sigma"):
        diff.trajectory_spread(solver, dev(solver, pr), dev(solver, sigma[:, :1]), *args, O=O, seg_stride=stride)
    with pytest.raises(ValueError, match="zero"):
        diff.trajectory_spread(solver, dev(solver, pr), dev(solver, 0 * sigma), *args, O=O, seg_stride=stride)
    with pytest.raises(ValueError, match="unknown"):
        jacobian_of(solver, cc, pr, p40[:1], more={"seg": torch.zeros(1)})
