"""btrapz_cartesian_device, _vjp_device and _jvp_device (include/btrapz_hip_cartesian.h) on the GPU: values and both
derivatives within the bound of the yardstick (tests/cartesian_reference.py), the adjoint identity, sentinels where nothing
may be written, the audit against NumPy reductions of the call's own cart, audit-only calls and repeated calls bit for bit
-- at the shapes where the kernels take another path: one row and one sample, 63 / 64 / 65 / 130 samples (a lane's
second and third turn), 64 / 65 / 253 rows (a workgroup's last wavefronts idle), more rows than the grid has wavefronts
(a workgroup's second turn, with another line staged), tables of 2, 3, 65, 1000 and 1024 points (staged in LDS) and 1100
(searched in global memory), both layouts, counts 0, 1, n and beyond n, two and three lines with a line_index out of
range.  Then end to end on 253 solved scenario_1 candidates."""
import math

import numpy as np
import pytest
import torch

import cartesian_cases as cc
from spectral_amd import diff, synth
from spectral_amd.native import CRefLine, FRENET_SAMPLES, FRENET_STATES, KIN_AUDIT

pytestmark = pytest.mark.gpu

# name -> (R, n, M, lines, mixed counts)
SHAPES = {
    "one": (1, 1, 2, 1, False),
    "r64_n63_m3": (64, 63, 3, 1, False),
    "r65_n64_m65": (65, 64, 65, 2, True),
    "r253_n65_m1000": (253, 65, 1000, 2, True),
    "r5_n130_m1100": (5, 130, 1100, 3, True),
    "r3_n130_m1024": (3, 130, 1024, 1, False),
    "r8200_n3_m65": (8200, 3, 65, 2, True),
}
LAYOUTS = {"samples": FRENET_SAMPLES, "states": FRENET_STATES}
PICKS = 48          # samples per shape held to the yardstick BESIDE the planted ones on table points and at the table's ends,
                    # which are always compared (cartesian_cases.must_check); both layouts share the cache


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


_inputs, _runs = {}, {}


def inputs(name):
    """The shape's host arrays, once: the line, f (SAMPLES layout), count, line_index, a cotangent, 12 tangents."""
    if name not in _inputs:
        R, n, M, n_lines, mixed = SHAPES[name]
        rl = cc.make_lines(M, n_lines)
        rng = np.random.default_rng(sum(map(ord, name)))
        count = np.array([[0, 1, n, n + 7, n // 2, n][r % 6] for r in range(R)], dtype=np.int32)[::-1].copy() if mixed else None
        index = None
        if n_lines > 1:
            index = np.array([r % n_lines for r in range(R)], dtype=np.int32)
            if R >= 6:
                index[R - 1] = n_lines; index[R // 2] = -1          # out of range: the whole row is OUTSIDE
        f, planted = cc.make_samples(rng.integers(1 << 30), R, n, rl, line_index=index, count=count)
        if R * n == 1:                      # the one sample there is: at the table's end, where the interval is clamped
            f[0, 0, 0] = rl.host["rs"][0, -1]; planted["last"].append((0, 0))
        cart_bar = rng.uniform(-1, 1, (R, 6, n))
        if count is not None:
            cart_bar[np.broadcast_to((np.arange(n)[None, :] >= np.clip(count, 0, n)[:, None])[:, None, :], (R, 6, n))] = np.nan
        _inputs[name] = dict(rl=rl, f=f, count=count, index=index, planted=planted, must=cc.must_check(planted), cart_bar=cart_bar,
                             f_dot=rng.uniform(-1, 1, (12, R, 6, n)))
    return _inputs[name]


def shaped(a, layout):
    return a if layout == FRENET_SAMPLES else cc.to_states(a)


def run(solver, name, layout):
    """Every device call of one shape and layout, once: the full forward twice (into a sentinel), the audit alone, the VJP
    twice, the JVP with 1 and with 12 tangents (into a sentinel).  Host arrays; derivatives brought back to [.., 6, n]."""
    key = (name, layout)
    if key in _runs:
        return _runs[key]
    c = inputs(name)
    d = solver.device
    R, _, n = c["f"].shape
    up = lambda a, dt=torch.float64: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dt, device=d)
    f, count, index = up(shaped(c["f"], layout)), up(c["count"], torch.int32), up(c["index"], torch.int32)
    arrays = c["rl"].on(d)
    t = CRefLine(c["rl"].n_lines, c["rl"].M, *[a.data_ptr() for a in arrays])
    stream = torch.cuda.current_stream(d).cuda_stream

    def forward(with_cart):
        cart = torch.full((R, 6, n), cc.SENTINEL, dtype=torch.float64, device=d) if with_cart else None
        au = {k: torch.full((R,), cc.SENTINEL, dtype=torch.float64, device=d) for k in KIN_AUDIT[:6]}
        au["n_outside"] = torch.full((R,), -7, dtype=torch.int32, device=d)
        au["worst"] = torch.full((R, 6), -7, dtype=torch.int32, device=d)
        solver.ctx.cartesian_device(t, index, R, n, layout, f, count, cart, au, stream=stream)
        torch.cuda.synchronize()
        return (None if cart is None else cart.cpu().numpy()), {k: v.cpu().numpy() for k, v in au.items()}

    def jvp(T):
        out = torch.full((T, R, 6, n), cc.SENTINEL, dtype=torch.float64, device=d)
        solver.ctx.cartesian_jvp_device(t, index, R, n, layout, f, count, T, up(shaped(c["f_dot"][:T], layout)), out, stream=stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def vjp():
        g = solver.cartesian_vjp(f, c["rl"], up(c["cart_bar"]), layout=layout, count=count, line_index=index)
        torch.cuda.synchronize()
        g = g.cpu().numpy()
        return g if layout == FRENET_SAMPLES else cc.from_states(g)

    cart, audit = forward(True)
    cart2, audit2 = forward(True)
    _, audit_only = forward(False)
    only_cart = solver.cartesian(f, c["rl"], layout=layout, count=count, line_index=index, want=("cart",))["cart"]
    torch.cuda.synchronize()
    _runs[key] = dict(cart=cart, audit=audit, cart2=cart2, audit2=audit2, audit_only=audit_only, only_cart=only_cart.cpu().numpy(),
                      f_bar=vjp(), f_bar2=vjp(), dot1=jvp(1), dot12=jvp(12), dot12b=jvp(12))
    return _runs[key]


CASES = [(s, l) for s in SHAPES for l in LAYOUTS]
same_bits = lambda a, b: a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name,lay", CASES)
def test_values_within_the_bound_and_nothing_written_beyond_the_counts(solver, name, lay):
    c, r = inputs(name), run(solver, name, LAYOUTS[lay])
    before = np.full_like(r["cart"], cc.SENTINEL)
    worst = cc.check_forward(c["rl"], c["f"], c["count"], c["index"], r["cart"], before=before, limit=PICKS, must=c["must"])
    assert (name == "one" and c["must"] == [(0, 0)]) or (len(c["must"]) >= 9 and all(c["planted"][k] for k in ("table", "first", "last")))
    print("%s %s: worst |error| / bound (x, y, theta, kappa, v, a) %s" % (name, lay, worst))
    # the planted samples came out as the header defines them
    for kind in ("below", "above", "nan"):
        for (row, j) in c["planted"][kind]:
            if j < cc.counts_of(c["count"], *r["cart"].shape[::2])[row]:
                assert np.isnan(r["cart"][row, :, j]).all(), (kind, row, j)
    for (row, j) in c["planted"]["still"]:
        if j < cc.counts_of(c["count"], *r["cart"].shape[::2])[row] and not np.isnan(r["cart"][row, 0, j]):
            assert r["cart"][row, 4, j] == 0.0 and r["cart"][row, 3, j] == 0.0, (row, j, r["cart"][row, :, j])
    # the wrapper's own call (cart alone, NaN where nothing is written) gives the same bits where something is
    written = r["cart"] != cc.SENTINEL
    assert same_bits(r["only_cart"][written], r["cart"][written]) and np.isnan(r["only_cart"][~written]).all()


@pytest.mark.parametrize("name,lay", CASES)
def test_both_derivatives_within_the_bound_and_adjoint_to_each_other(solver, name, lay):
    c, r = inputs(name), run(solver, name, LAYOUTS[lay])
    wv = cc.check_vjp(c["rl"], c["f"], c["count"], c["index"], c["cart_bar"], r["f_bar"], limit=PICKS, must=c["must"])
    before = np.full_like(r["dot12"], cc.SENTINEL)
    w1 = cc.check_jvp(c["rl"], c["f"], c["count"], c["index"], c["f_dot"][:1], r["dot1"], before=before[:1], limit=PICKS, must=c["must"])
    w12 = cc.check_jvp(c["rl"], c["f"], c["count"], c["index"], c["f_dot"], r["dot12"], before=before, limit=PICKS, must=c["must"])
    print("%s %s: worst |error| / bound vjp %.3g jvp T=1 %.3g T=12 %.3g" % (name, lay, wv, w1, w12))
    assert same_bits(r["dot1"][0], r["dot12"][0])            # a tangent's result does not depend on how many go along
    cc.check_adjoint(c["f"], c["count"], np.nan_to_num(c["cart_bar"]), r["f_bar"], c["f_dot"], r["dot12"])


@pytest.mark.parametrize("name,lay", CASES)
def test_the_audit_is_the_reduction_of_the_calls_own_cart(solver, name, lay):
    c, r = inputs(name), run(solver, name, LAYOUTS[lay])
    cc.check_audit(c["rl"], c["f"], c["count"], c["index"], r["cart"], r["audit"])
    for k in KIN_AUDIT:
        assert same_bits(r["audit"][k], r["audit_only"][k]), ("the audit alone differs from the full call's", k)


@pytest.mark.parametrize("name,lay", CASES)
def test_two_runs_give_identical_bits(solver, name, lay):
    r = run(solver, name, LAYOUTS[lay])
    assert same_bits(r["cart"], r["cart2"]) and same_bits(r["f_bar"], r["f_bar2"]) and same_bits(r["dot12"], r["dot12b"])
    for k in KIN_AUDIT:
        assert same_bits(r["audit"][k], r["audit2"][k]), k


def test_refusals(solver):
    from spectral_amd.native import BtrapzError, CKinAudit
    import ctypes as C
    c = inputs("r65_n64_m65")
    d = solver.device
    f = torch.tensor(c["f"], device=d)
    for bad in (dict(want=()), dict(want=("speed",))):
        with pytest.raises(ValueError):
            solver.cartesian(f, c["rl"], **bad)
    with pytest.raises(ValueError):
        solver.cartesian(f[:, :5], c["rl"])
    arrays = c["rl"].on(d)
    t = CRefLine(c["rl"].n_lines, c["rl"].M, *[a.data_ptr() for a in arrays])
    cart = torch.zeros_like(f)
    with pytest.raises(BtrapzError, match="both null"):
        solver.ctx.cartesian_device(t, None, 65, 64, 0, f, None, None, None)
    with pytest.raises(BtrapzError, match="every field"):
        solver.ctx.cartesian_device(t, None, 65, 64, 0, f, None, cart, {})
    with pytest.raises(BtrapzError, match="layout"):
        solver.ctx.cartesian_device(t, None, 65, 64, 2, f, None, cart, None)
    with pytest.raises(BtrapzError, match="R"):
        solver.ctx.cartesian_device(t, None, 0, 64, 0, f, None, cart, None)
    with pytest.raises(BtrapzError, match="M"):
        solver.ctx.cartesian_device(CRefLine(1, 1, *[a.data_ptr() for a in arrays]), None, 65, 64, 0, f, None, cart, None)
    with pytest.raises(BtrapzError, match="T"):
        solver.ctx.cartesian_jvp_device(t, None, 65, 64, 0, f, None, 33, f, cart)
    with pytest.raises(BtrapzError, match="cart_bar"):
        solver.ctx.cartesian_vjp_device(t, None, 65, 64, 0, f, None, None, cart)
    torch.cuda.synchronize()
    assert (cart == 0).all()


# ---- end to end: 253 scenario_1 candidates of 20 segments solved on the GPU ------------------------------------------------
E2E_B, E2E_S = 253, 20
_e2e = {}


def e2e(solver):
    if not _e2e:
        batch, sh = synth.make_scenario1_batch(E2E_B, E2E_S, 0)
        db = solver.upload(batch)
        o = {k: v.clone() for k, v in solver.solve(db, sh, keep_multipliers=True).items()}
        traj, npts = solver.sample(db, o["ctrl"], torch.arange(E2E_B, device=solver.device), sh.delta)
        torch.cuda.synchronize()
        _e2e.update(batch=batch, sh=sh, db=db, o=o, traj=traj, npts=npts, status=o["status"].cpu().numpy())
    return _e2e


def test_on_a_straight_line_the_plan_is_placed_as_the_harness_places_it(solver):
    """x = s, y = l, v = hypot(ds, dl), theta = atan2(dl, ds).  Tolerances from the format: x is rs[i] + w h, three
    roundings of numbers of size s; y is 0 + 1 l, exact; v and theta differ from NumPy's by the rounding of a square root
    (two units in the last place); theta by the device's arc tangent (two units of at most pi / 2), NumPy's (one) and
    NormalizeAngle's sum with pi and difference from it (2^-53 of 1.5 pi and of pi / 2): below 8 2^-53 pi together."""
    e = e2e(solver)
    assert ((e["status"] == 1) | (e["status"] == 2)).sum() >= 100
    rl = synth.refline_straight(200.0, 0.5)
    cart = solver.cartesian(e["traj"], rl, count=e["npts"], want=("cart",))["cart"]
    torch.cuda.synchronize()
    c, t, npts = cart.cpu().numpy(), e["traj"].cpu().numpy(), e["npts"].cpu().numpy()
    assert npts.max() >= 190
    u = 2.0 ** -53
    for b in np.flatnonzero(npts > 0):
        k = npts[b]
        s, ds, l, dl = t[b, 0, :k], t[b, 1, :k], t[b, 3, :k], t[b, 4, :k]
        assert (np.abs(c[b, 0, :k] - s) <= 4 * u * np.abs(s)).all() and np.array_equal(c[b, 1, :k], l)
        assert (np.abs(c[b, 4, :k] - np.hypot(ds, dl)) <= 4 * u * np.hypot(ds, dl)).all()
        assert (np.abs(c[b, 2, :k] - np.arctan2(dl, ds)) <= 8 * u * np.pi).all()
        assert np.isnan(c[b, :, k:]).all()


def test_kinematic_admissible_then_topk_returns_only_admissible_winners(solver):
    e = e2e(solver)
    rl = synth.refline_arc(200.0, 0.5, 80.0)
    audit = solver.cartesian(e["traj"], rl, count=e["npts"], want=("audit",))["audit"]
    solved = torch.tensor((e["status"] == 1) | (e["status"] == 2), device=solver.device)
    # limits that split the solved candidates: the medians of two of the audit's figures
    kappa_max = float(audit["kappa_abs_max"][solved].median())
    alat_max = float(audit["alat_abs_max"][solved].median())
    mask = solver.kinematic_admissible(audit, kappa_max, alat_max, -10.0, 10.0, 0.5) & solved
    torch.cuda.synchronize()
    assert 8 <= int(mask.sum()) < int(solved.sum())
    inf = float("inf")
    cost = e["o"]["cost"].masked_fill(~solved, inf)
    idx, best = solver.topk(cost.masked_fill(~mask, inf), 8)
    torch.cuda.synchronize()
    idx, m = idx.cpu().numpy().ravel(), mask.cpu().numpy()
    assert (idx >= 0).all() and m[idx].all()
    # ... and they are the eight cheapest admissible candidates, ties to the lower index
    masked = np.where(m, cost.cpu().numpy(), np.inf)
    assert np.array_equal(idx, np.argsort(masked, kind="stable")[:8])
    # a NaN extreme, an outside sample and a row nobody attains an extreme of are inadmissible
    probe = {k: v[:4].clone() for k, v in audit.items()}
    for k in ("kappa_abs_max", "alat_abs_max", "a_max", "v_max"):
        probe[k][:] = 0.5
    for k in ("a_min", "frame_min"):
        probe[k][:] = 0.75
    probe["n_outside"][:] = 0; probe["worst"][:] = 3
    probe["kappa_abs_max"][1] = float("nan"); probe["n_outside"][2] = 1
    for k in ("kappa_abs_max", "alat_abs_max", "a_max", "v_max"):
        probe[k][3] = -inf
    for k in ("a_min", "frame_min"):
        probe[k][3] = inf
    probe["worst"][3] = -1
    assert solver.kinematic_admissible(probe, 1.0, 1.0, -1.0, 1.0, 0.0).cpu().tolist() == [True, False, False, False]
    # ... and that last row is what the device reports for samples that are inside the table but hold no number
    bad = e["traj"][:2].clone(); bad[1, 1:] = float("nan")
    ab = solver.cartesian(bad, rl, count=e["npts"][:2].clone().fill_(5), want=("audit",))["audit"]
    assert int(ab["n_outside"][1]) == 0 and (ab["worst"][1] == -1).all()
    assert not bool(solver.kinematic_admissible(ab, 1e9, 1e9, -1e9, 1e9, -1e9)[1])


def test_gradient_of_the_curvature_penalty_through_the_whole_pipeline(solver):
    """d (sum_j kappa_j^2) / d init through diff.cartesian o diff.sample o diff.solve on an arc of radius 80 m, against
    central differences of the whole GPU pipeline along one direction per candidate, within 1e-3 of the larger of the two
    (floor: 1e-3 of the largest derivative compared) -- the tolerance and the step of the solve's own difference tests
    (tests/test_gpu_vjp.py, tests/test_gpu_long_grad.py): h = 1e-3 with the differenced solves run to their floor (eps =
    1e-12) keeps the forward's round-off below 1e-6 of the quotient, and the penalty's third derivative times h^2 / 6 is
    smaller still.  The direction leaves s0 alone (scenario_1 starts ON its lower s bound: a step below it has no solve).
    Compared: of the first 24 candidates those the CPU oracle finds solved, strictly complementary and without a weakly
    active row (the rule of tests/golden/make_long_grad_goldens.py), and whose control points move affinely over the
    step (x(+h) + x(-h) - 2 x(0) vanishes on a fixed active set; where it does not, a row changed sides inside the step
    and the quotient measures no derivative)."""
    from vjp_reference import Adjoint, one
    e = e2e(solver)
    batch, sh, d = e["batch"], e["sh"], solver.device
    rl = synth.refline_arc(200.0, 0.5, 80.0)
    first = 24
    ok = np.zeros(E2E_B, dtype=bool)
    for b in range(first):
        adj = Adjoint(one(batch, b), sh, np.zeros(12 * E2E_S), 0.0)
        eq = (adj.u - adj.l) <= 1e-12
        y = np.abs(adj.y)
        active = (~eq) & (y > 1e-6 * max(y.max(), 1e-300))
        weak = bool((y[active] <= 1e-4 * y[~eq].max()).any()) if active.any() else False
        ok[b] = adj.status in (1, 2) and adj.strict and not weak and e["status"][b] in (1, 2)
    rng = np.random.default_rng(77)
    dirn = rng.standard_normal((E2E_B, 6)); dirn[:, 0] = 0.0

    def penalty(init_np, eps):
        bt = type(batch)(B=E2E_B, S=E2E_S, seg=batch.seg, init=init_np, ref_end=batch.ref_end, dl_bounds=batch.dl_bounds)
        db = solver.upload(bt)
        o = solver.solve(db, sh, eps=eps, keep_multipliers=True)
        traj, npts = solver.sample(db, o["ctrl"], torch.arange(E2E_B, device=d), sh.delta)
        cart = solver.cartesian(traj, rl, count=npts, want=("cart",))["cart"]
        torch.cuda.synchronize()
        return torch.nansum(cart[:, 3] ** 2, dim=1).cpu().numpy(), o["ctrl"].cpu().numpy().copy(), o["status"].cpu().numpy().copy()

    h = 1e-3
    lp, xp, sp = penalty(batch.init + h * dirn, 1e-12)
    lm, xm, sm = penalty(batch.init - h * dirn, 1e-12)
    l0, x0, s0 = penalty(batch.init.copy(), 1e-12)
    fd = (lp - lm) / (2 * h)
    second, moved = np.abs(xp + xm - 2 * x0).max(1), np.abs(xp - xm).max(1)
    affine = second <= 1e-3 * np.maximum(moved, 1e-300)
    same = np.isin(sp, (1, 2)) & np.isin(sm, (1, 2)) & np.isin(s0, (1, 2))
    # the analytic side: one backward through the three layers
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=d)
    init_t = T(batch.init).requires_grad_(True)
    params = torch.tensor(diff.params_from_shared(sh), dtype=torch.float64)
    seg = T(batch.seg)
    ctrl, cost, status = diff.solve(solver, seg, init_t, T(batch.ref_end), T(batch.dl_bounds), params, variant=0, delta=sh.delta)
    traj, npts = diff.sample(ctrl, seg, init_t, solver, delta=sh.delta)
    cart = diff.cartesian(traj, rl, solver, count=npts)
    loss = torch.nansum(cart[:, 3] ** 2, dim=1)
    loss.sum().backward()
    torch.cuda.synchronize()
    an = (init_t.grad.cpu().numpy() * dirn).sum(1)
    assert np.allclose(loss.detach().cpu().numpy()[ok], l0[ok], rtol=1e-4, atol=1e-12)      # (the same penalty on both sides)
    use = ok & affine & same
    assert use.sum() >= 8, (ok.sum(), (ok & affine).sum(), use.sum())
    top = np.abs(an[use]).max()
    scale = np.maximum(np.maximum(np.abs(an), np.abs(fd)), 1e-3 * top)
    err = np.abs(fd - an) / scale
    print("curvature penalty: oracle-clean %d of %d, affine over the step %d, compared %d; worst |fd - an| / scale %.2e; an %s fd %s"
          % (ok.sum(), first, (ok & affine).sum(), use.sum(), err[use].max(), an[use][:4], fd[use][:4]))
    assert top > 0 and err[use].max() <= 1e-3, (err[use], an[use], fd[use])


def test_scene_jacobian_in_the_plane(solver):
    """diff.scene_jacobian_cartesian on the eight-scene constellation of tests/test_gpu_stage_jvp.py (copied: that file stays
    as it is): its pieces are scene_jacobian, sample, sample_jvp and the Cartesian calls, bit for bit; and along the
    tangents the pipeline really produces, dcart is the derivative of the Cartesian map: central differences of
    btrapz_cartesian_device at traj +- h dtraj, h = 1e-6, on the samples whose interval of the lookup is the same at both
    ends (the frozen decision), within 1e-6 of the row's largest entry -- the map's second derivative times h^2 / 2 and the
    forward's rounding over 2 h are both below 1e-8 of it."""
    import prism_vjp_cases as PK
    B, N, O, stride = 8, 71, 5, 24
    rng = np.random.default_rng(7)
    scenes = []
    for b in range(B):
        scenes.append([dict(centre=(float(rng.uniform(18, 30)), 1.2, 0), vel_s=float(rng.uniform(3, 5)), vel_l=0.0, time=4.0),
                       dict(centre=(float(rng.uniform(5, 15)), 4.2, 0), vel_s=float(rng.uniform(5, 7)), vel_l=(0.05 if b % 4 == 1 else -0.05) if b % 2 else 0.0,
                            time=4.03 if b % 2 else 4.0)])
    pr = PK.pack(scenes, 2)
    d = solver.device
    T_ = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(d, dtype=torch.float64).contiguous()
    tt = np.arange(N) * 0.1
    s_ref = np.tile(40.0 / 7.0 * tt, (B, 1)); l_ref = np.tile(np.clip(1.2 + 0.0825 * (np.arange(N) - 15), 1.2, 4.5), (B, 1))
    init = np.zeros((B, 6)); init[:, 1] = 6.0; init[:, 3] = 1.2
    dsb = np.tile(np.array([0.0, 20.0]), (B, N, 1)); dlb = np.tile(np.array([-3.0, 3.0]), (B, N, 1))
    sh = synth.make_scenario1_batch(1, 7, 0)[1]
    prm = torch.tensor(diff.params_from_shared(sh), device=d)
    pdot = np.zeros((3, B, 2, 8)); pdot[0, :, 0, 0] = 1.0; pdot[1, :, 1, 1] = 1.0; pdot[2, :, 1, 3] = 1.0       # s0 of car 0; l0, vel_s of car 1
    rl = synth.refline_arc(80.0, 0.5, 60.0, theta0=0.2)
    args = [T_(a) for a in (dsb, dlb, s_ref, l_ref, init)] + [prm]
    r = diff.scene_jacobian_cartesian(solver, rl, T_(pr), T_(pdot), *args, O=O, variant=0, delta=0.1, seg_stride=stride)
    J = diff.scene_jacobian(solver, T_(pr), T_(pdot), *args, O=O, variant=0, delta=0.1, seg_stride=stride)
    torch.cuda.synchronize()
    status = r["status"].cpu().numpy()
    solved = np.flatnonzero(np.isin(status, (1, 2)))
    assert len(solved) >= 2 and torch.equal(r["dctrl"], J["dctrl"]) and torch.equal(r["ctrl"], J["ctrl"])
    traj, npts = solver.sample(J["rec"], J["ctrl"], torch.arange(B, device=d), 0.1)
    dtraj = diff.sample_jvp(solver, J["dctrl"], J["rec"].seg, seg_count=J["rec"].seg_count, delta=0.1)[..., :traj.shape[2]].contiguous()
    assert torch.equal(traj, r["traj"]) and torch.equal(npts, r["npoints"]) and tuple(r["dcart"].shape) == (3, B, 6, traj.shape[2])
    cart = solver.cartesian(traj, rl, count=npts, want=("cart",))["cart"]
    dcart = solver.cartesian_jvp(traj, rl, dtraj, count=npts)
    torch.cuda.synchronize()
    same = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert same(cart, r["cart"]) and same(dcart, r["dcart"])
    h = 1e-6
    rs = rl.host["rs"][0]
    checked = 0
    for t in range(3):
        cp = solver.cartesian(traj + h * dtraj[t], rl, count=npts, want=("cart",))["cart"]
        cm = solver.cartesian(traj - h * dtraj[t], rl, count=npts, want=("cart",))["cart"]
        torch.cuda.synchronize()
        fd = ((cp - cm) / (2 * h)).cpu().numpy()
        an = r["dcart"][t].cpu().numpy()
        sp, sm = (traj + h * dtraj[t])[:, 0].cpu().numpy(), (traj - h * dtraj[t])[:, 0].cpu().numpy()
        for b in solved:
            k = int(npts[b])
            keep = np.searchsorted(rs, sp[b, :k], side="right") == np.searchsorted(rs, sm[b, :k], side="right")
            assert keep.sum() >= k // 2
            for i in range(6):
                top = max(np.abs(an[b, i, :k]).max(), np.abs(cart[b, i, :k].cpu().numpy()).max() * 1e-3, 1e-12)
                gap = fd[b, i, :k][keep] - an[b, i, :k][keep]
                if i == 2:      # a heading that crossed -pi between the two ends differs by 2 pi there: compare modulo 2 pi / 2 h
                    gap = np.array([math.remainder(g, 2 * math.pi / (2 * h)) for g in gap])
                assert np.abs(gap).max() <= 1e-6 * top, (t, b, i, np.abs(gap).max(), top)
            checked += int(keep.sum())
    assert np.abs(r["dcart"][:, solved].cpu().numpy()).max() > 1e-3 and checked > 300
    unsolved = np.setdiff1d(np.arange(B), solved)
    assert (r["dcart"][:, unsolved] == 0).all() and np.isnan(r["cart"][unsolved].cpu().numpy()).all()
