"""The backward pass of the prism stage (btrapz_prism_bounds_vjp_device) on the GPU: against the yardstick of
tests/prism_vjp_reference.py (central differences of the frozen, unrounded map, computed tolerance) and against its host twin
BIT FOR BIT (both add in the same order: a lane's knots ascending strip after strip, then the butterfly), at every edge of the
lane mapping, its defined cases, determinism, refusals, and the autograd layer diff.prism_bounds: alone, and in front of
diff.corridor, diff.solve and diff.traj_cost against central differences of the whole pipeline."""
import numpy as np
import pytest
import torch

import prism_vjp_cases as K
import prism_vjp_reference as R
from spectral_amd import diff, layout as L, native, synth
from spectral_amd.native import BtrapzError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def dev(solver, a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(solver.device, dtype=torch.float64).contiguous()


def device_grads(solver, pr, N, O, sbar, lbar):
    g = solver.prism_bounds_vjp(dev(solver, pr), N, O, dev(solver, sbar), dev(solver, lbar))
    torch.cuda.synchronize()
    return g.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def against_both(solver, pr, N, O, key, seed=3):
    """Kernel == host twin bit for bit; kernel against the yardstick on every scene; returns worst error / tolerance."""
    B = pr.shape[0]
    sbar, lbar = K.cotangents(B, O, N, seed=seed)
    got = device_grads(solver, pr, N, O, sbar, lbar)
    host = native.prism_bounds_vjp_host(pr, N, O, sbar, lbar)
    assert same_bits(got, host), (key, np.argwhere(got != host)[:5])
    jacs = [R.jacobian(pr[b], N, key=(key, b)) for b in range(B)]
    R.check_cap(jacs)
    return max(R.compare(jac, got[b], sbar[b], lbar[b], O, (key, b)) for b, jac in enumerate(jacs))


@pytest.mark.parametrize("name", ["golden", "nice", "plain", "tied"])
def test_kernel_against_yardstick_and_host_twin(solver, name):
    pr, N, O = K.scene_sets()[name]
    print(name, "worst error / tolerance:", against_both(solver, pr, N, O, name))


@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 71, 129])
def test_lane_mapping_edges(solver, N):
    """Knot counts around the wavefront's 64 lanes, with P = 1, 2, 3; B = 1, and B = 3 with a different car count per scene."""
    scenes = K.random_scenes(40, 100 + N, max_cars=3)
    by_count = {n: [s for s in scenes if len(s) == n] for n in (1, 2, 3)}
    worst = 0.0
    for P in (1, 2, 3):
        worst = max(worst, against_both(solver, K.pack(by_count[P][:1], P), N, 2 * P + 1, ("lanes", N, P, 1)))
    mixed = [by_count[2][1], by_count[3][1], by_count[1][1]]
    worst = max(worst, against_both(solver, K.pack(mixed, 3), N, 7, ("lanes", N, 3, 3)))
    print("N", N, "worst error / tolerance:", worst)


def test_sixteen_cars_33_strips(solver):
    pr = K.pack(K.sixteen_cars(), 16)
    N = 65
    for O in (33, 34):
        print("O", O, "worst error / tolerance:", against_both(solver, pr, N, O, "sixteen", seed=O))
    sbar, lbar = K.cotangents(pr.shape[0], 32, N)
    assert not device_grads(solver, pr, N, 32, sbar, lbar).any()      # 33 strips, O = 32: the forward's n_strips = -1
    _, _, n = solver.prism_bounds(dev(solver, pr), N, 33)
    assert (n.cpu().numpy() == 33).all()


@pytest.mark.parametrize("case", K.defined_cases(), ids=lambda c: c[0])
def test_defined_cases_on_the_device(solver, case):
    name, pr, N, O, sbar, lbar, expected = case
    K.check_defined(name, device_grads(solver, pr, N, O, sbar, lbar), expected)


def test_determinism_and_full_overwrite(solver):
    pr, N, O = K.scene_sets()["plain"]
    B, P = pr.shape[0], pr.shape[1]
    sbar, lbar = K.cotangents(B, O, N, seed=9)
    a = device_grads(solver, pr, N, O, sbar, lbar)
    b = device_grads(solver, pr, N, O, sbar, lbar)
    assert same_bits(a, b) and a.any()
    # outputs pre-filled with NaN come back fully overwritten -- inactive slots and overflowing scenes included
    for O2 in (O, 2):
        s2, l2 = K.cotangents(B, O2, N, seed=9)
        out = torch.full((B, P, 8), float("nan"), dtype=torch.float64, device=solver.device)
        solver.ctx.prism_bounds_vjp_device(B, P, N, native.CRoad.reference(), dev(solver, pr), O2, dev(solver, s2), dev(solver, l2), out)
        torch.cuda.synchronize()
        assert not torch.isnan(out).any()
    assert (pr[:, :, 6] == 0).any() and not a[pr[:, :, 6] == 0].any()


def test_device_refusals(solver):
    d = solver.device
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=d)
    road = native.CRoad.reference()

    def call(B=2, P=3, N=21, O=4, bars=(True, True), road=road, prisms=True, out=True):
        solver.ctx.prism_bounds_vjp_device(B, P, N, road, z(max(B, 1), max(P, 1), 8) if prisms else None, O,
                                           z(max(B, 1), max(O, 1), max(N, 1), 2) if bars[0] else None,
                                           z(max(B, 1), max(O, 1), max(N, 1), 2) if bars[1] else None, z(max(B, 1), max(P, 1), 8) if out else None)
    call(); call(bars=(True, False)); call(bars=(False, True))
    bad_road = native.CRoad.reference(); bad_road.knots_per_second = 0.0
    for kw, text in ((dict(B=0), ">= 1"), (dict(P=0), ">= 1"), (dict(N=0), ">= 1"), (dict(O=0), ">= 1"), (dict(P=17), "P > 16"),
                     (dict(bars=(False, False)), "both null"), (dict(road=None), "non-null"), (dict(prisms=False), "non-null"),
                     (dict(out=False), "non-null"), (dict(road=bad_road), "knots_per_second")):
        with pytest.raises(BtrapzError, match=text):
            call(**kw)
    torch.cuda.synchronize()


def test_diff_prism_bounds_is_the_direct_calls(solver):
    pr, N, O = K.scene_sets()["nice"]
    p = dev(solver, pr).requires_grad_(True)
    sb, lb, n = diff.prism_bounds(solver, p, N, O)
    sb0, lb0, n0 = solver.prism_bounds(dev(solver, pr), N, O)
    assert torch.equal(sb, sb0) and torch.equal(lb, lb0) and torch.equal(n, n0) and not n.requires_grad
    sbar, lbar = K.cotangents(pr.shape[0], O, N, seed=6)
    torch.autograd.backward([sb, lb], [dev(solver, sbar), dev(solver, lbar)])      # a random linear functional of both
    assert same_bits(p.grad.cpu().numpy(), device_grads(solver, pr, N, O, sbar, lbar))
    p2 = dev(solver, pr).requires_grad_(True)
    sb2, _, _ = diff.prism_bounds(solver, p2, N, O)
    (sb2 * dev(solver, sbar)).sum().backward()                                       # s alone: the l cotangent is absent or zero
    assert same_bits(p2.grad.cpu().numpy(), device_grads(solver, pr, N, O, sbar, None))


LATERAL = {1: "l0", 4: "vel_l", 5: "T"}


def test_prisms_to_traj_cost_against_central_differences(solver):
    """prisms -> diff.prism_bounds -> diff.corridor -> diff.solve -> diff.traj_cost on the harness constellation of
    test_prisms_to_arg_min_end_to_end (8 scenes, N = 71, O = 5, seg_stride 24; the car beside the ego drifts sideways in half
    of the scenes, so that vel_l and T have a derivative, for T = 4.03 s: a window that ends between two knots, where a move of T changes
    no knot's membership): the gradient of the summed score of the candidates that are solved
    and strictly complementary w.r.t. the LATERAL parameters -- l0 of every car, vel_l and T of a car with vel_l != 0 --
    against central differences of the whole GPU pipeline, h = 1e-4 (1 + |x|), to 1e-3 of the norm of the gradient over the
    checked entries.  Only parameters whose move leaves every decision of the prism and corridor stages
    unchanged count (window membership of every knot, strip count, segment count, durations; both moved pipelines solved).

    The LONGITUDINAL parameters (s0, t0, vel_s) cannot be checked this way: the faces are rounded to two decimals, so the real
    pipeline is a step function of them in units of 0.01 and its central difference is 0 or a jump.  Their check is the
    yardstick of tests/prism_vjp_reference.py (straight-through rounding), in the tests above."""
    from vjp_reference import Adjoint
    B, N, O, stride = 8, 71, 5, 24
    rng = np.random.default_rng(7)
    scenes = []
    for b in range(B):
        scenes.append([dict(centre=(float(rng.uniform(18, 30)), 1.2, 0), vel_s=float(rng.uniform(3, 5)), vel_l=0.0, time=4.0),
                       dict(centre=(float(rng.uniform(5, 15)), 4.2, 0), vel_s=float(rng.uniform(5, 7)), vel_l=(0.05 if b % 4 == 1 else -0.05) if b % 2 else 0.0, time=4.03 if b % 2 else 4.0)])
    pr = K.pack(scenes, 2)
    tt = np.arange(N) * 0.1
    s_ref = np.tile(40.0 / 7.0 * tt, (B, 1)); l_ref = np.tile(np.clip(1.2 + 0.0825 * (np.arange(N) - 15), 1.2, 4.5), (B, 1))
    init = np.zeros((B, 6)); init[:, 1] = 6.0; init[:, 3] = 1.2
    dsb = np.tile(np.array([0.0, 20.0]), (B, N, 1)); dlb = np.tile(np.array([-3.0, 3.0]), (B, N, 1))
    sh = synth.make_scenario1_batch(1, 7, 0)[1]
    d = solver.device
    prm = torch.tensor(diff.params_from_shared(sh), device=d)
    knots = [dev(solver, a) for a in (dsb, dlb, s_ref, l_ref)]
    init_d = dev(solver, init)

    def pipeline(p, rows):
        kn = [t[rows].contiguous() for t in knots]
        sb, lb, ns = diff.prism_bounds(solver, p, N, O)
        seg, cnt, ref_end, dl10 = diff.corridor(solver, sb, lb, *kn, variant=0, delta=0.1, seg_stride=stride)
        ini = init_d[rows].contiguous()
        ctrl, _, st = diff.solve(solver, seg, ini, ref_end, dl10, prm, seg_count=cnt, variant=0, delta=0.1)
        cost = diff.traj_cost(ctrl, seg, ini, kn[2], kn[3], prm, solver, seg_count=cnt, status=st, variant=0, delta=0.1)
        return cost, st, cnt, seg, ref_end, dl10, ns

    p = dev(solver, pr).requires_grad_(True)
    every = torch.arange(B, device=d)
    cost, st, cnt, seg, ref_end, dl10, ns = pipeline(p, every)
    stn, cn, segn, nsn = st.cpu().numpy(), cnt.cpu().numpy(), seg.detach().cpu().numpy(), ns.cpu().numpy()
    ren, dln = ref_end.detach().cpu().numpy(), dl10.detach().cpu().numpy()
    kept = []
    for b in range(B):
        if stn[b] in (1, 2) and cn[b] >= 1:
            n = int(cn[b])
            one = L.Batch(B=1, S=n, seg=np.ascontiguousarray(segn[:, b:b + 1, :n]), init=init[b:b + 1].copy(), ref_end=ren[b:b + 1].copy(),
                          dl_bounds=dln[b:b + 1].copy())
            if Adjoint(one, sh, np.zeros(12 * n), 0.0).strict:
                kept.append(b)
    print("solved and strictly complementary:", kept, "status", stn, "segments", cn, "strips", nsn)
    assert len(kept) >= 2
    cost[torch.tensor(kept, device=d)].sum().backward()
    grad = p.grad.cpu().numpy()
    assert not grad[[b for b in range(B) if b not in kept]].any()

    entries = [(b, q, k) for b in kept for q in range(2) for k in LATERAL if k == 1 or pr[b, q, 4] != 0.0]
    M = len(entries)
    hs = np.array([1e-4 * (1.0 + abs(pr[b, q, k])) for b, q, k in entries])
    moved = np.concatenate([pr[[b for b, _, _ in entries]]] * 2)
    for i, (b, q, k) in enumerate(entries):
        moved[i, q, k] += hs[i]; moved[M + i, q, k] -= hs[i]
    rows = [b for b, _, _ in entries] * 2
    with torch.no_grad():
        c2, st2, cnt2, seg2, _, _, ns2 = pipeline(dev(solver, moved), torch.tensor(rows, device=d))
        c2, st2, cnt2, seg2, ns2 = c2.cpu().numpy(), st2.cpu().numpy(), cnt2.cpu().numpy(), seg2.cpu().numpy(), ns2.cpu().numpy()
    windows = lambda a: [[tuple(not (i < c[2] * 10 or i > (c[2] + c[5]) * 10) for i in range(N)) for c in sc] for sc in a]
    w0, w2 = windows(pr), windows(moved)
    ok = np.array([w2[i] == w0[b] and st2[i] in (1, 2) and ns2[i] == nsn[b] and cnt2[i] == cn[b] and (seg2[L.F_T, i, :cn[b]] == segn[L.F_T, b, :cn[b]]).all()
                   for i, b in enumerate(rows)])
    usable = np.flatnonzero(ok[:M] & ok[M:])
    assert usable.size >= 4, (M, usable.size)
    with np.errstate(invalid="ignore"):
        fd = ((c2[:M] - c2[M:]) / (2 * hs))[usable]
    an = np.array([grad[entries[i]] for i in usable])
    norm = float(np.linalg.norm(an))
    names = [(entries[i][0], entries[i][1], LATERAL[entries[i][2]]) for i in usable]
    significant = [names[i] for i in np.flatnonzero(np.abs(fd) > 1e-2 * np.abs(fd).max())]
    print("checked entries (scene, car, parameter):", names)
    print("autograd", an, "central differences", fd, "score", cost.detach().cpu().numpy()[kept])
    print("significant:", significant, "worst error / norm: %.3e" % (np.abs(fd - an).max() / norm))
    # significant: a central difference above 1e-2 of the largest, and the largest far above the round-off of a score of
    # order 1e2..1e3 divided by 2 h (1e-13 * 1e3 / 2e-4 = 5e-7)
    assert len(significant) >= 2 and np.abs(fd).max() > 1e-3
    assert norm > 0 and np.abs(fd - an).max() <= 1e-3 * norm
