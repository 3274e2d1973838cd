"""btrapz_frenet_device, _vjp_device and _jvp_device (include/btrapz_hip_frenet.h) on the GPU: values, intervals and both
derivatives within the bound of the yardstick (tests/frenet_reference.py), the interval of the host twin, sentinels where
nothing may be written, repeated calls bit for bit -- at the shapes where the kernels take another path: one row and one
query, rows of 1, 3, 63, 64, 65 and 130 queries (256 / n rows per workgroup, idle threads behind them), 300 (one row per
workgroup in slices, n_outside from the barrier), 64 / 65 / 253 rows, more row groups than the grid has workgroups (a
workgroup's second turn), tables of 2, 3, 64, 65, 129, 1000 and 1024 points (staged at once) and 1100 (staged in two
parts), up to three lines in one workgroup with a line_index out of range, windows, both layouts, the three orders, counts
0, 1, n and beyond n, NaN and OUTSIDE queries planted at samples 0, 63, 64 and the last of a row.  Then the Python layers:
init_from_cartesian and a solve from it, prisms_from_cartesian, diff.frenet composed with diff.cartesian, and a gradient
with respect to an obstacle's position in the plane against central differences."""
import numpy as np
import pytest
import torch

import frenet_cases as fc
from spectral_amd import diff, native, synth
from spectral_amd.native import CRefLine, FRENET_SAMPLES, FRENET_STATES

pytestmark = pytest.mark.gpu

# name -> (R, n, M, lines, mixed counts, windows)
SHAPES = {
    "one": (1, 1, 2, 1, False, False),
    "r3_n3_m3": (3, 3, 3, 3, False, False),
    "r64_n63_m64": (64, 63, 64, 1, False, False),
    "r65_n64_m65": (65, 64, 65, 2, True, True),
    "r253_n65_m129": (253, 65, 129, 3, True, False),
    "r253_n1_m65": (253, 1, 65, 3, True, True),
    "r3_n130_m1000": (3, 130, 1000, 1, False, True),
    "r5_n130_m1024": (5, 130, 1024, 2, True, False),
    "r3_n65_m1100": (3, 65, 1100, 3, False, False),
    "r7_n300_m65": (7, 300, 65, 2, True, False),
    "r8200_n128_m3": (8200, 128, 3, 2, True, False),
}
LAYOUTS = {"samples": FRENET_SAMPLES, "states": FRENET_STATES}
PICKS = 20          # queries per shape held to the yardstick BESIDE the planted ones; layouts and orders share the cache


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


_inputs, _runs = {}, {}


def inputs(name):
    if name not in _inputs:
        R, n, M, n_lines, mixed, windows = SHAPES[name]
        rl = fc.make_lines(M, n_lines)
        seed = sum(map(ord, name))
        count = np.array([[0, 1, n, n + 7, n // 2, n][r % 6] for r in range(R)], dtype=np.int32)[::-1].copy() if mixed else None
        index = None
        if n_lines > 1:
            index = np.array([r % n_lines for r in range(R)], dtype=np.int32)
            if R >= 5:
                index[R - 1] = n_lines; index[R // 2] = -1          # out of range: the whole row is OUTSIDE
        cart, f, planted = fc.make_queries(seed, R, n, rl, line_index=index, count=count)
        window = None
        if windows:
            window = np.array([[[0.0, 40.0], [10.0, 30.0], [np.nan, 40.0], [30.0, 10.0], [-5.0, 12.0]][r % 5] for r in range(R)])
        _inputs[name] = dict(rl=rl, cart=cart, f=f, count=count, index=index, window=window, planted=planted,
                             picks=fc.picks_of(planted, R, n, count, PICKS, seed))
    return _inputs[name]


def run(solver, name, layout, order):
    """Every device call of one shape, layout and order, once: the forward twice (into sentinels), the JVP with six unit
    tangents, the VJP with six unit cotangents.  Host arrays in the SAMPLES order."""
    key = (name, layout, order)
    if key in _runs:
        return _runs[key]
    c = inputs(name)
    d = solver.device
    R, _, n = c["cart"].shape
    up = lambda a, dt=torch.float64: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dt, device=d)
    cart, count, index, window = up(c["cart"]), up(c["count"], torch.int32), up(c["index"], torch.int32), up(c["window"])
    arrays = c["rl"].on(d)
    t = CRefLine(c["rl"].n_lines, c["rl"].M, *[a.data_ptr() for a in arrays])
    stream = torch.cuda.current_stream(d).cuda_stream
    shape = (R, 6, n) if layout == FRENET_SAMPLES else (R, 2, n, 3)
    back = lambda a: a if layout == FRENET_SAMPLES else fc.from_states(a)

    def forward():
        fr = torch.full(shape, fc.SENTINEL, dtype=torch.float64, device=d)
        iv = torch.full((R, n), fc.ISENT, dtype=torch.int32, device=d)
        no = torch.full((R,), fc.ISENT, dtype=torch.int32, device=d)
        solver.ctx.frenet_device(t, index, R, n, layout, order, cart, count, window, fr, iv, no, stream=stream)
        torch.cuda.synchronize()
        return fr, iv, no

    fr, iv, no = forward()
    fr2, iv2, no2 = forward()
    out = dict(frenet=back(fr.cpu().numpy()), interval=iv.cpu().numpy(), n_outside=no.cpu().numpy(),
               again=(back(fr2.cpu().numpy()), iv2.cpu().numpy(), no2.cpu().numpy()))
    if R * n <= 40000:
        cd = torch.zeros((6, R, 6, n), dtype=torch.float64, device=d)
        for q in range(6):
            cd[q, :, q] = 1.0
        fd = torch.full((6,) + shape, fc.SENTINEL, dtype=torch.float64, device=d)
        solver.ctx.frenet_jvp_device(t, index, R, n, layout, order, cart, fr, iv, count, 6, cd, fd, stream=stream)
        torch.cuda.synchronize()
        out["Kj"] = np.moveaxis(back(fd.cpu().numpy()), 0, 2)                 # [R, row, column, n]
        Kv = np.zeros((R, 6, 6, n))
        for q in range(6):
            fb = np.full((R, 6, n), np.nan)                                     # NaN where nothing may be read
            fb[:, [k for k in range(6) if k % 3 <= order]] = 0.0
            if q % 3 <= order:
                fb[:, q] = 1.0
            fb = fb if layout == FRENET_SAMPLES else fc.to_states(fb)
            cb = solver.frenet_vjp(cart, c["rl"], fr, iv, up(fb), layout=layout, order=order, count=count, line_index=index)
            torch.cuda.synchronize()
            Kv[:, q] = cb.cpu().numpy()
        out["Kv"] = Kv
    _runs[key] = out
    return out


CASES = [(name, lay, 2) for name in SHAPES for lay in LAYOUTS] + \
        [(name, "samples", order) for name in ("r65_n64_m65", "r253_n65_m129") for order in (0, 1)] + \
        [("r5_n130_m1024", "states", 1), ("r3_n3_m3", "states", 0)]
IDS = ["%s-%s-order%d" % c for c in CASES]


def host(name, order):
    c = inputs(name)
    return native.frenet_host(c["cart"], c["rl"], order=order, count=c["count"], line_index=c["index"], s_window=c["window"])


@pytest.mark.parametrize("name,lay,order", CASES, ids=IDS)
def test_values_and_intervals_within_the_bound_and_nothing_written_beyond_the_counts(solver, name, lay, order):
    c = inputs(name)
    o = run(solver, name, LAYOUTS[lay], order)
    R, _, n = c["cart"].shape
    must = [p for k in ("table", "first", "last") for p in c["planted"][k]]
    worst, same = fc.check_values(c["rl"], c["cart"], o["frenet"], o["interval"], c["picks"], order, c["index"], c["window"], must=must)
    read = np.arange(n)[None, :] < fc.counts_of(c["count"], R, n)[:, None]
    assert (o["frenet"][np.broadcast_to(~read[:, None, :], (R, 6, n))] == fc.SENTINEL).all() and (o["interval"][~read] == fc.ISENT).all()
    assert not (o["frenet"][np.broadcast_to(read[:, None, :], (R, 6, n))] == fc.SENTINEL).any()
    outside = read & (o["interval"] == -1)
    assert ((o["interval"] >= 0) | (o["interval"] == -1))[read].all() and (o["interval"][read] <= c["rl"].M - 2).all()
    assert np.array_equal(o["n_outside"], outside.sum(1)) and np.isnan(o["frenet"][:, 0][outside]).all()
    # the host twin's interval at every query; on the normal of a table point rounding may pick the neighbour
    h = host(name, order)
    differ = read & (h["interval"] != o["interval"])
    assert differ.sum() <= 0.02 * read.sum() + 4, differ.sum()
    for r, j in np.argwhere(differ):
        li = 0 if c["index"] is None else int(c["index"][r])
        rs = c["rl"].host["rs"][li]
        a, b = sorted((int(h["interval"][r, j]), int(o["interval"][r, j])))
        assert a >= 0 and b == a + 1 and abs(o["frenet"][r, 0, j] - rs[b]) <= 1e-9 * (rs[b + 1] - rs[b]), (r, j, a, b)
    print("%s %s order %d: worst ratio to the bound %.3f over %d queries" % (name, lay, order, worst, len(same)))


@pytest.mark.parametrize("name,lay,order", [c for c in CASES if c[0] != "r8200_n128_m3"], ids=[i for i in IDS if "r8200" not in i])
def test_both_derivatives_within_the_bound(solver, name, lay, order):
    c = inputs(name)
    o = run(solver, name, LAYOUTS[lay], order)
    R, _, n = c["cart"].shape
    _, same = fc.check_values(c["rl"], c["cart"], o["frenet"], o["interval"], c["picks"], order, c["index"], c["window"],
                              must=[p for k in ("table", "first", "last") for p in c["planted"][k]])
    wj, wv = fc.check_jacobian(o["Kj"], same, order), fc.check_jacobian(o["Kv"], same, order)
    read = np.arange(n)[None, :] < fc.counts_of(c["count"], R, n)[:, None]
    where = lambda m: np.broadcast_to(m[:, None, None, :], (R, 6, 6, n))
    outside = read & (o["interval"] == -1)
    assert (o["Kj"][where(~read)] == fc.SENTINEL).all() and (o["Kj"][where(outside)] == 0).all()
    assert (o["Kv"][where(~read | outside)] == 0).all() and np.isfinite(o["Kv"][where(read & ~outside)]).all()
    print("%s %s order %d: Jacobian's worst ratio, JVP %.3f, VJP %.3f over %d queries" % (name, lay, order, wj, wv, len(same)))


@pytest.mark.parametrize("name", list(SHAPES))
def test_two_runs_give_identical_bits(solver, name):
    o = run(solver, name, FRENET_SAMPLES, 2)
    for a, b in zip((o["frenet"], o["interval"], o["n_outside"]), o["again"]):
        assert a.tobytes() == b.tobytes()


def test_the_hairpin_and_the_table_ends_on_the_device(solver):
    rl = fc.hairpin()
    far = 64.0 + 4.0 * np.pi
    pts = [(10.0, 3.0), (10.0, 5.0), (10.0, 4.0), (10.0, 4.0 + 1e-12), (60.0, 4.3)]
    cart = np.zeros((3, 6, len(pts)))
    cart[:, 0], cart[:, 1] = [p[0] for p in pts], [p[1] for p in pts]
    win = np.array([[0.0, far], [50.0, far], [35.0, 45.0]])
    o = solver.frenet(torch.tensor(cart, device=solver.device), rl, order=0, s_window=torch.tensor(win, device=solver.device))
    h = native.frenet_host(cart, rl, order=0, s_window=win)
    torch.cuda.synchronize()
    iv, f = o["interval"].cpu().numpy(), o["frenet"].cpu().numpy()
    assert np.array_equal(iv, h["interval"]) and list(iv[0, :4]) == [20, iv[1, 0], 20, iv[1, 2]] and (iv[1, :4] > 64).all() and (iv[2, :4] == -1).all()
    assert f[0, 0, 0] == 10.0 and f[0, 3, 2] == 4.0 and abs(f[1, 3, 0] - 5.0) <= 1e-12
    assert np.array_equal(o["n_outside"].cpu().numpy(), h["n_outside"]) and h["n_outside"][2] >= 4
    ends = synth.refline_straight(20.0, 0.5, x0=3.0, y0=-2.0, theta0=0.0)
    xs = [3.0, np.nextafter(3.0, -np.inf), np.nextafter(3.0, np.inf), 23.0, np.nextafter(23.0, -np.inf), np.nextafter(23.0, np.inf)]
    c2 = np.zeros((1, 6, 6)); c2[0, 0], c2[0, 1] = xs, 1.5
    o2 = solver.frenet(torch.tensor(c2, device=solver.device), ends, order=0)
    torch.cuda.synchronize()
    assert list(o2["interval"].cpu().numpy()[0]) == [0, -1, 0, ends.M - 2, ends.M - 2, -1]
    s = o2["frenet"].cpu().numpy()[0, 0]
    assert s[0] == 0.0 and s[3] == 20.0 and 0.0 < s[2] < 1e-15 and 20.0 - 1e-14 < s[4] < 20.0


def test_refusals(solver):
    rl = fc.make_lines(3, 1)
    d = solver.device
    arrays = rl.on(d)
    t = CRefLine(1, 3, *[a.data_ptr() for a in arrays])
    cart = torch.zeros((1, 6, 2), dtype=torch.float64, device=d)
    fr, iv = torch.zeros_like(cart), torch.zeros((1, 2), dtype=torch.int32, device=d)
    ctx = solver.ctx
    for call in (lambda: ctx.frenet_device(t, None, 1, 2, 0, 3, cart, None, None, fr),
                 lambda: ctx.frenet_device(t, None, 1, 2, 2, 2, cart, None, None, fr),
                 lambda: ctx.frenet_device(t, None, 0, 2, 0, 2, cart, None, None, fr),
                 lambda: ctx.frenet_device(t, None, 1, 2, 0, 2, None, None, None, fr),
                 lambda: ctx.frenet_device(t, None, 1, 2, 0, 2, cart, None, None, None),
                 lambda: ctx.frenet_device(CRefLine(1, 1, *[a.data_ptr() for a in arrays]), None, 1, 2, 0, 2, cart, None, None, fr),
                 lambda: ctx.frenet_vjp_device(t, None, 1, 2, 0, 2, cart, fr, None, None, fr, cart),
                 lambda: ctx.frenet_vjp_device(t, None, 1, 2, 0, 2, cart, fr, iv, None, None, cart),
                 lambda: ctx.frenet_jvp_device(t, None, 1, 2, 0, 2, cart, fr, iv, None, 33, cart, fr),
                 lambda: ctx.frenet_jvp_device(t, None, 1, 2, 0, 2, cart, fr, iv, None, 1, None, fr)):
        with pytest.raises(native.BtrapzError, match="invalid argument"):
            call()


# ---- the Python layers -------------------------------------------------------------------------------------------------
def test_init_from_cartesian_returns_the_batchs_init_and_the_same_solve(solver):
    """253 scenario_1 candidates on an arc: their init placed in the plane by the existing forward and projected back is
    the batch's init within the yardstick's bound (at most 1e-11 at these sizes: a few hundred times 64 * 2^-53), and the
    solve from it is the solve from the original within the parity bound of smoke()."""
    B, S = 253, 20
    batch, sh = synth.make_scenario1_batch(B, S, 0)
    # scenario_1 starts at s = 0: the line begins 10 m behind it (ON the first normal of a curved line the rounding of a g
    # that is zero decides between the first interval and OUTSIDE)
    from spectral_amd.layout import RefLine, REFLINE_FIELDS
    arc = synth.refline_arc(200.0, 0.5, 80.0, theta0=0.4)
    rl = RefLine(arc.host["rs"][0] - 10.0, *[arc.host[k][0] for k in REFLINE_FIELDS[1:]])
    init = np.ascontiguousarray(batch.init, dtype=np.float64)
    states = native.cartesian_host(init.reshape(B, 2, 1, 3), rl, layout=FRENET_STATES, want=("cart",))["cart"].reshape(B, 6)
    states[7, 0] = np.nan                                                   # one candidate without a pose
    got, mask = solver.init_from_cartesian(torch.tensor(states, device=solver.device), rl)
    torch.cuda.synchronize()
    got, mask = got.cpu().numpy(), mask.cpu().numpy()
    assert not mask[7] and np.isnan(got[7]).all() and mask.sum() == B - 1
    assert np.abs(got[mask] - init[mask]).max() <= 1e-11
    o1 = {k: v.clone() for k, v in solver.solve(solver.upload(batch), sh).items()}
    batch2, _ = synth.make_scenario1_batch(B, S, 0)
    batch2.init[mask] = got[mask]
    o2 = solver.solve(solver.upload(batch2), sh)
    torch.cuda.synchronize()
    s1, s2 = o1["status"].cpu().numpy(), o2["status"].cpu().numpy()
    ok = np.isin(s1, (1, 2)) & mask
    assert ok.sum() >= 100 and np.isin(s2[ok], (1, 2)).all()
    x1, x2 = o1["ctrl"].cpu().numpy()[ok], o2["ctrl"].cpu().numpy()[ok]
    assert np.abs(x1 - x2).max() <= 1e-5 * np.abs(x1).max()


def test_prisms_from_cartesian_gives_the_prisms_of_the_yardstick(solver):
    import frenet_reference as fr
    B, P, N, O = 6, 3, 71, 5
    rl = synth.refline_arc(120.0, 0.5, 60.0, theta0=0.2)
    rng = np.random.default_rng(4)
    fr0 = np.zeros((B, 6, P))
    fr0[:, 0] = rng.uniform(5.0, 60.0, (B, P)); fr0[:, 1] = rng.uniform(3.0, 7.0, (B, P))
    fr0[:, 3] = rng.uniform(-1.0, 5.0, (B, P)); fr0[:, 4] = rng.uniform(-0.1, 0.1, (B, P))
    c = native.cartesian_host(fr0, rl, want=("cart",))["cart"]
    ob = np.zeros((B, P, 8))
    ob[:, :, 0], ob[:, :, 1], ob[:, :, 3], ob[:, :, 4] = c[:, 0], c[:, 1], c[:, 2], c[:, 4]
    ob[:, :, 2], ob[:, :, 5], ob[:, :, 6] = 0.0, 4.0, 1.0
    ob[1, 2, 6] = 0.0                                      # inactive, with a pose that is OUTSIDE: not counted
    ob[1, 2, :2] = [-500.0, 0.0]
    ob[2, 0, :2] = [-500.0, 0.0]                           # active and OUTSIDE: dropped and counted
    prisms, dropped = solver.prisms_from_cartesian(torch.tensor(ob, device=solver.device), rl)
    torch.cuda.synchronize()
    pr = prisms.cpu().numpy()
    assert list(dropped.cpu().numpy()) == [0, 0, 1, 0, 0, 0] and pr[2, 0, 6] == 0 and (pr[2, 0, [0, 1, 3, 4]] == 0).all() and pr[1, 2, 6] == 0
    want = ob.copy()
    line = {k: rl.host[k][0] for k in fr.FIELDS}
    for b in range(B):
        for p in range(P):
            if (b, p) in ((1, 2), (2, 0)):
                want[b, p, [0, 1, 3, 4, 6]] = 0.0
                continue
            res = fr.evaluate(line, [ob[b, p, 0], ob[b, p, 1], ob[b, p, 3], 0.0, ob[b, p, 4], 0.0], order=1)
            assert (np.abs(pr[b, p, [0, 3, 1, 4]] - res["out"][[0, 1, 3, 4]]) <= fr.bound([ob[b, p, 0], ob[b, p, 1], ob[b, p, 3], 0.0, ob[b, p, 4], 0.0], res, 1)[[0, 1, 3, 4]]).all()
            want[b, p, [0, 3, 1, 4]] = res["out"][[0, 1, 3, 4]]
    assert np.array_equal(pr[:, :, [2, 5, 7]], ob[:, :, [2, 5, 7]])
    # the bounds of the stage from the two sets of prisms: the faces are rounded to two decimals, so equal unless a face
    # sits within the bound of a rounding boundary
    sb, lb, ns = solver.prism_bounds(prisms, N, O)
    sb2, lb2, ns2 = solver.prism_bounds(torch.tensor(want, device=solver.device), N, O)
    torch.cuda.synchronize()
    assert torch.equal(ns, ns2)
    a, b = torch.cat([sb, lb]).cpu().numpy(), torch.cat([sb2, lb2]).cpu().numpy()
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.nanmax(np.abs(np.where(np.isfinite(a), a - b, 0.0))) <= 0.01 + 1e-9
    assert (np.abs(np.where(np.isfinite(a), a - b, 0.0)) <= 1e-9).mean() >= 0.99


def test_diff_frenet_after_diff_cartesian_has_the_identitys_gradient(solver):
    rl = fc.make_lines(129, 3)
    li = np.array([0, 1, 2], dtype=np.int32)
    _, f, _ = fc.make_queries(77, 3, 40, rl, line_index=li, plant=False)
    d = solver.device
    idx = torch.tensor(li, device=d)
    x = torch.tensor(f, device=d, requires_grad=True)
    back, iv = diff.frenet(diff.cartesian(x, rl, solver, line_index=idx), rl, solver, line_index=idx)
    w = torch.tensor(np.random.default_rng(2).normal(size=f.shape), device=d)
    (back * w).sum().backward()
    torch.cuda.synchronize()
    assert (iv.cpu().numpy() >= 0).all() and not iv.requires_grad
    rs = rl.host["rs"][li]
    ivn = iv.cpu().numpy().astype(np.int64)
    wgt = (f[:, 0] - np.take_along_axis(rs, ivn, 1)) / (rs[:, 1] - rs[:, 0])[:, None]
    ok = np.broadcast_to(((wgt > 1e-9) & (wgt < 1 - 1e-9))[:, None, :], f.shape)
    assert ok.mean() >= 0.95
    # K J = I: the gradient of <w, back> with respect to x is w.  Both Jacobians carry entries up to ~1e2 (ds ~ 10, the
    # accelerations' rows), each within 256 * 2^-53 of its scale: 1e-9 of the largest weight is far above their product
    g = x.grad.cpu().numpy()
    assert np.abs(g - w.cpu().numpy())[ok].max() <= 1e-9 * np.abs(w.cpu().numpy()).max()


def test_gradient_with_respect_to_an_obstacles_position_in_the_plane(solver):
    """loss = <weights, l_bounds> of diff.prism_bounds(prisms built from diff.frenet at order 1) against central differences
    in the obstacles' x and y, h = 1e-4 (1 + |x|), decisions frozen (matched interval, strip count and the pattern of the
    bounds unchanged by the move), to 1e-3 of the gradient's norm: the bound of tests/test_gpu_prism_vjp.py.  Only the
    lateral bounds enter: the longitudinal faces are rounded to two decimals and are a step function of the position."""
    B, P, N, O = 4, 2, 71, 5
    rl = synth.refline_arc(120.0, 0.5, 60.0, theta0=0.2)
    fr0 = np.zeros((B, 6, P))
    rng = np.random.default_rng(9)
    fr0[:, 0, 0] = rng.uniform(18.2, 29.8, B); fr0[:, 0, 1] = rng.uniform(5.2, 14.8, B)
    fr0[:, 1, 0] = rng.uniform(3, 5, B); fr0[:, 1, 1] = rng.uniform(5, 7, B)
    fr0[:, 3, 0], fr0[:, 3, 1] = 1.2, 4.2
    # both cars drift sideways: at vel_l == 0 the stage has a kink (which face of the swept prism is the outer one), and a
    # move of x or y changes vel_l = v sin(theta - rtheta(s)) through s
    fr0[:, 4, 0] = [0.03, -0.03, -0.03, 0.03]
    fr0[:, 4, 1] = [0.05, -0.05, 0.05, -0.05]
    c0 = native.cartesian_host(fr0, rl, want=("cart",))["cart"]
    d = solver.device
    wts = torch.tensor(np.random.default_rng(3).normal(size=(B, O, N, 2)), device=d)

    def pipeline(cart):
        f, iv = diff.frenet(cart, rl, solver, order=1)
        zeros, ones = torch.zeros_like(f[:, 0]), torch.ones_like(f[:, 0])
        prisms = torch.stack([f[:, 0], f[:, 3], zeros, f[:, 1], f[:, 4], 4.03 * ones, ones, zeros], dim=2)
        sb, lb, ns = diff.prism_bounds(solver, prisms, N, O)
        fin = torch.isfinite(lb)
        return (torch.where(fin, lb, torch.zeros_like(lb)) * wts).sum(), iv, ns, fin

    x = torch.tensor(c0, device=d, requires_grad=True)
    loss, iv, ns, fin = pipeline(x)
    loss.backward()
    torch.cuda.synchronize()
    grad = x.grad.cpu().numpy()
    assert (ns.cpu().numpy() >= 1).all() and (grad[:, 3] == 0).all() and (grad[:, 5] == 0).all()      # order 1: kappa and a are not read
    an, fdv = [], []
    for b in range(B):
        for p in range(P):
            for k in (0, 1):
                h = 1e-4 * (1.0 + abs(c0[b, k, p]))
                vals = []
                for sgn in (1.0, -1.0):
                    cm = c0.copy(); cm[b, k, p] += sgn * h
                    with torch.no_grad():
                        l2, iv2, ns2, fin2 = pipeline(torch.tensor(cm, device=d))
                    vals.append(float(l2) if torch.equal(iv2, iv) and torch.equal(ns2, ns) and torch.equal(fin2, fin) else None)
                if None not in vals:
                    an.append(grad[b, k, p]); fdv.append((vals[0] - vals[1]) / (2 * h))
    an, fdv = np.array(an), np.array(fdv)
    norm = float(np.linalg.norm(an))
    print("obstacle x, y: autograd", an, "central differences", fdv, "worst error / norm %.3e" % (np.abs(an - fdv).max() / norm))
    assert len(an) >= 8 and norm > 1e-3 and np.abs(an - fdv).max() <= 1e-3 * norm
