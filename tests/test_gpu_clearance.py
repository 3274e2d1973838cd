"""btrapz_clearance_device, _vjp_device and _jvp_device (include/btrapz_hip_clearance.h) on the GPU: values, `which` and both
derivatives within the bounds of the yardstick (tests/clearance_reference.py) at picked samples and within twice the
value bound of the host twin everywhere (both lie within the bound of the truth), the adjoint identity, sentinels where
nothing may be written, the audit against NumPy reductions of the call's own clear, each of the seven template forms and
repeated calls bit for bit, and the call on a side stream -- at the shapes where the mapping can go wrong: 1, 3, 4, 5 and
253 rows (wavefronts per workgroup, a partial last workgroup) and 16 500 (more rows than the grid has wavefronts: a
workgroup's second turn); 1, 63, 64, 65, 71 and 129 samples (a lane's second and third sample); 1, 2, 16 and 17 obstacles
(THE OBSTACLE LOOP HAS NO CHUNKING: one obstacle per trip, so its only edges are 0, 1 and many trips); one and three scenes
with a scene_index out of range and consecutive rows on different scenes; counts 0, 1, n and beyond n; an obs_count of 0
and ragged ones; NaN ego and obstacle poses at samples 0, 63, 64 and the last.  Then end to end on 253 solved scenario_1
candidates."""
import numpy as np
import pytest
import torch

import clearance_cases as cc
import clearance_reference as cr
from spectral_amd import diff, native, synth
from spectral_amd.native import CLEAR_AUDIT, BtrapzError

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
PICKS = 40
# name -> (R, n, O, n_scenes, mixed)
SHAPES = {
    "one": (1, 1, 1, 1, False),
    "r3_n63_o2": (3, 63, 2, 1, False),
    "r4_n64_o16": (4, 64, 16, 1, False),
    "r5_n65_o17": (5, 65, 17, 3, True),
    "r4_n129_o1": (4, 129, 1, 1, True),
    "r253_n71_o2": (253, 71, 2, 3, True),
    "r16500_n3_o1": (16500, 3, 1, 3, True),
}


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


_inputs, _runs = {}, {}


def inputs(name):
    if name not in _inputs:
        R, n, O, S, mixed = SHAPES[name]
        counts = scene_index = obs_count = None
        nan_ego, nan_obs = [], []
        if mixed:
            counts = [[n, 0, 1, n + 7, n // 2 + 1][r % 5] for r in range(R)]
            if S > 1:
                scene_index = [r % S for r in range(R)]                      # consecutive rows on different scenes
                if R >= 5:
                    scene_index[R - 1] = S; scene_index[R // 2] = -1        # out of range: the whole row is invalid
                obs_count = [O, 0, max(O // 3, 1)][:S]
            planted = sorted({0, 63, 64, n - 1} & set(range(n)))
            nan_ego = [(r, j) for r in (0, min(3, R - 1)) for j in planted]
            nan_obs = [(k, o, j) for k in range(S) for o in {0, O - 1} for j in planted]
        c = cc.make_case(R, n, O, n_scenes=S, seed=sum(map(ord, name)), counts=counts, obs_count=obs_count, scene_index=scene_index,
                         nan_ego=nan_ego, nan_obs=nan_obs)
        rng = np.random.default_rng(sum(map(ord, name)) + 1)
        read = np.zeros((R, n), dtype=bool)
        for r, k in cc.rows_read(c):
            read[r, :k] = True
        c.update(read=read, clear_bar=np.where(read, rng.uniform(-1, 1, (R, n)), np.nan), cart_dot=rng.uniform(-1, 1, (3, R, 6, n)),
                 obs_dot=rng.uniform(-1, 1, (3, S, O, 3, n)), picks=cc.pick_samples(c, PICKS))
        _inputs[name] = c
    return _inputs[name]


def run(solver, name):
    """Every device call of one shape, once.  Host arrays."""
    if name in _runs:
        return _runs[name]
    c = inputs(name)
    d = solver.device
    R, n = c["R"], c["n"]
    up = lambda a, dt=torch.float64: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dt, device=d)
    cart, count, index = up(c["cart"]), up(c["count"], torch.int32), up(c["scene_index"], torch.int32)
    ob = c["obstacles"]
    kw = dict(scene_index=index, count=count)
    d_safe = 0.5

    def forward(want):
        """Through the context, into sentinels."""
        _, _, _, ft, cob, keep = solver._clearance_args(cart, ob, c["foot"], index, count)
        clear = torch.full((R, n), SENTINEL, dtype=torch.float64, device=d) if "clear" in want else None
        which = torch.full((R, n), -7, dtype=torch.int32, device=d) if "which" in want else None
        au = None
        if "audit" in want:
            au = dict(clear_min=torch.full((R,), SENTINEL, dtype=torch.float64, device=d), worst=torch.full((R, 2), -7, dtype=torch.int32, device=d),
                      n_below=torch.full((R,), -7, dtype=torch.int32, device=d), n_invalid=torch.full((R,), -7, dtype=torch.int32, device=d))
        solver.ctx.clearance_device(ft, cob, index, R, n, cart, count, d_safe, clear, which, au, stream=torch.cuda.current_stream(d).cuda_stream)
        torch.cuda.synchronize()
        host = lambda t: None if t is None else t.cpu().numpy()
        return dict(clear=host(clear), which=host(which), audit=None if au is None else {k: host(v) for k, v in au.items()})

    full = forward(("clear", "which", "audit"))
    again = forward(("clear", "which", "audit"))
    forms = {w: forward(w) for w in (("clear", "which"), ("clear", "audit"), ("clear",), ("which", "audit"), ("which",), ("audit",))}
    which = up(full["which"], torch.int32)
    cd6, od6 = cc.unit_tangents(c)

    def jvp(cd, od):
        T = cd.shape[0]
        _, _, _, ft, cob, keep = solver._clearance_args(cart, ob, c["foot"], index, count)
        out = torch.full((T, R, n), SENTINEL, dtype=torch.float64, device=d)
        solver.ctx.clearance_jvp_device(ft, cob, index, R, n, cart, count, which, T, up(cd), up(od), out,
                                        stream=torch.cuda.current_stream(d).cuda_stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def vjp(cb):
        g = solver.clearance_vjp(cart, ob, c["foot"], which, up(cb), **kw)
        torch.cuda.synchronize()
        return g.cpu().numpy()

    _runs[name] = dict(full=full, again=again, forms=forms, unit=jvp(cd6, od6), dot3=jvp(c["cart_dot"], c["obs_dot"]), dot3b=jvp(c["cart_dot"], c["obs_dot"]),
                       dot1=jvp(c["cart_dot"][:1], None), dot3_still=jvp(c["cart_dot"], None), ones_bar=vjp(np.where(c["read"], 1.0, np.nan)),
                       cart_bar=vjp(c["clear_bar"]), cart_bar2=vjp(c["clear_bar"]),
                       host=native.clearance_host(c["cart"], ob, c["foot"], scene_index=c["scene_index"], count=c["count"], d_safe=d_safe))
    return _runs[name]


same_bits = lambda a, b: a.tobytes() == b.tobytes()


def magnitudes(c, which):
    """M of clearance_reference per sample for the obstacle `which` names (0 where it names none), in NumPy."""
    ob, (hl, hw, off) = c["obstacles"].host, c["foot"]
    R, n = which.shape
    k = np.zeros(R, dtype=np.int64) if c["scene_index"] is None else np.clip(c["scene_index"], 0, c["obstacles"].n_scenes - 1)
    o = np.clip(which >> 4, 0, c["obstacles"].O - 1)
    j = np.broadcast_to(np.arange(n), (R, n))
    K = np.broadcast_to(k[:, None], (R, n))
    x, y, th = c["cart"][:, 0], c["cart"][:, 1], c["cart"][:, 2]
    m = (np.abs(x + off * np.cos(th)) + np.abs(y + off * np.sin(th)) + np.abs(ob["pose"][K, o, 0, j]) + np.abs(ob["pose"][K, o, 1, j])
         + hl + hw + ob["half"][K, o].sum(-1) + abs(off))
    return np.where(which >= 0, m, 0.0)


@pytest.mark.parametrize("name", SHAPES)
def test_values_within_the_bound_and_nothing_written_beyond_the_counts(solver, name):
    c, o = inputs(name), run(solver, name)
    clear, which, read = o["full"]["clear"], o["full"]["which"], c["read"]
    assert (clear[~read] == SENTINEL).all() and (which[~read] == -7).all()
    worst = cc.check_values(c, c["picks"], clear, which)
    print("%s: worst error / bound over %d picked samples %.3g" % (name, len(c["picks"]), worst))
    # everywhere: the host twin.  NaN, +inf and -1 in the same places; the values within twice the bound
    hc, hw = o["host"]["clear"], o["host"]["which"]
    assert np.array_equal(np.isnan(clear[read]), np.isnan(hc[read])) and np.array_equal(clear[read] == np.inf, hc[read] == np.inf)
    assert np.array_equal(which[read] == -1, hw[read] == -1)
    fin = read & np.isfinite(hc)
    bound = 2 * cr.K_VALUE * 2.0 ** -53 * np.maximum(magnitudes(c, which), magnitudes(c, hw))
    assert (np.abs(clear[fin] - hc[fin]) <= bound[fin]).all()
    if name == "r4_n129_o1":
        for j in (0, 63, 64, 128):
            assert np.isnan(clear[0, j]) and which[0, j] == -1                 # planted NaN ego poses (row 0 reads all 129)


@pytest.mark.parametrize("name", SHAPES)
def test_both_derivatives_within_the_bound_and_adjoint_to_each_other(solver, name):
    c, o = inputs(name), run(solver, name)
    read = c["read"]
    unit = o["unit"]
    assert (unit[:, ~read] == SENTINEL).all() and (o["dot3"][:, ~read] == SENTINEL).all()
    worst, share = cc.check_grads(c, c["picks"], {(r, j): unit[:, r, j] for r, j in c["picks"]})
    # reverse mode with a unit cotangent: the same three numbers, held to the same bound
    bar = o["ones_bar"]
    worst2, _ = cc.check_grads(c, c["picks"], {(r, j): list(bar[r, :3, j]) + list(unit[3:, r, j]) for r, j in c["picks"]})
    print("%s: worst derivative error / bound %.3g (JVP) %.3g (VJP), skipped %.3g" % (name, worst, worst2, share))
    for g in (bar, o["cart_bar"]):
        assert np.isfinite(g).all() and not g[:, 3:].any() and not g[np.broadcast_to(~read[:, None, :], g.shape)].any()
    # the adjoint identity over the samples read (the obstacles standing still)
    cb = np.where(read, c["clear_bar"], 0.0)
    still = np.where(read[None], o["dot3_still"], 0.0)
    for t in range(3):
        lhs, rhs = (cb * still[t]).sum(), (o["cart_bar"] * c["cart_dot"][t]).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(np.abs(cb * still[t]).sum(), 1e-300), (t, lhs, rhs)
    # one tangent is the first of three; the obstacles' tangents change the result where there is an obstacle
    assert same_bits(o["dot1"][0], o["dot3_still"][0])
    named = read & (o["full"]["which"] >= 0)
    if named.any():
        assert (o["dot3"][0][named] != o["dot3_still"][0][named]).any()


@pytest.mark.parametrize("name", SHAPES)
def test_the_audit_is_the_reduction_of_the_calls_own_clear(solver, name):
    c, o = inputs(name), run(solver, name)
    clear, which, au = o["full"]["clear"], o["full"]["which"], o["full"]["audit"]
    for r, k in cc.rows_read(c) if c["R"] <= 300 else cc.rows_read(c)[::37]:
        row = clear[r, :k]
        finite = np.where(np.isfinite(row), row, np.inf)
        if k == 0 or not np.isfinite(row).any():
            assert au["clear_min"][r] == np.inf and au["worst"][r].tolist() == [-1, -1]
        else:
            j = int(np.argmin(finite))
            assert au["clear_min"][r] == finite[j] and au["worst"][r].tolist() == [j, which[r, j] >> 4]
        assert au["n_below"][r] == int((row < 0.5).sum()) and au["n_invalid"][r] == int(np.isnan(row).sum())


@pytest.mark.parametrize("name", SHAPES)
def test_every_form_and_every_repetition_gives_identical_bits(solver, name):
    o = run(solver, name)
    full = o["full"]
    for other in [o["again"]] + list(o["forms"].values()):
        for k in ("clear", "which"):
            assert other[k] is None or same_bits(other[k], full[k]), k
        if other["audit"] is not None:
            for k in CLEAR_AUDIT:
                assert same_bits(other["audit"][k], full["audit"][k]), k
    assert same_bits(o["dot3"], o["dot3b"]) and same_bits(o["cart_bar"], o["cart_bar2"])


def test_refusals(solver):
    c = inputs("r3_n63_o2")
    d = solver.device
    cart = torch.tensor(c["cart"], device=d)
    _, R, n, ft, cob, keep = solver._clearance_args(cart, c["obstacles"], c["foot"], None, None)
    clear = torch.zeros((R, n), dtype=torch.float64, device=d)
    which = torch.zeros((R, n), dtype=torch.int32, device=d)
    call = solver.ctx.clearance_device
    with pytest.raises(BtrapzError, match="all null"):
        call(ft, cob, None, R, n, cart, None, 0.0, None, None, None)
    with pytest.raises(BtrapzError, match="every field"):
        call(ft, cob, None, R, n, cart, None, 0.0, None, None, {})
    with pytest.raises(BtrapzError, match="R"):
        call(ft, cob, None, 0, n, cart, None, 0.0, clear, None, None)
    with pytest.raises(BtrapzError, match="obstacles.n"):
        call(ft, cob, None, R, n - 1, cart, None, 0.0, clear, None, None)
    with pytest.raises(BtrapzError, match="cart"):
        call(ft, cob, None, R, n, None, None, 0.0, clear, None, None)
    with pytest.raises(BtrapzError, match="half extent"):
        call(native.CFootprint(2.0, 0.0, 0.0), cob, None, R, n, cart, None, 0.0, clear, None, None)
    with pytest.raises(BtrapzError, match="centre_offset"):
        call(native.CFootprint(2.0, 1.0, float("inf")), cob, None, R, n, cart, None, 0.0, clear, None, None)
    bad = native.CObstacles(cob.n_scenes, 0, cob.n, cob.pose, cob.half, None)
    with pytest.raises(BtrapzError, match="obstacles.O"):
        call(ft, bad, None, R, n, cart, None, 0.0, clear, None, None)
    with pytest.raises(BtrapzError, match="which"):
        solver.ctx.clearance_vjp_device(ft, cob, None, R, n, cart, None, None, clear, cart)
    with pytest.raises(BtrapzError, match="clear_bar"):
        solver.ctx.clearance_vjp_device(ft, cob, None, R, n, cart, None, which, None, cart)
    with pytest.raises(BtrapzError, match="T "):
        solver.ctx.clearance_jvp_device(ft, cob, None, R, n, cart, None, which, native.MAX_TANGENTS + 1, cart, None, clear)
    with pytest.raises(BtrapzError, match="clear_dot"):
        solver.ctx.clearance_jvp_device(ft, cob, None, R, n, cart, None, which, 1, cart, None, None)
    torch.cuda.synchronize()
    assert not clear.any()


def test_a_which_that_names_nothing_reads_nothing_and_gives_zero(solver):
    c = inputs("r5_n65_o17")
    d = solver.device
    R, n, O = c["R"], c["n"], c["O"]
    which = np.empty((R, n), dtype=np.int32)
    which[:] = np.array([O * 16, 15, 0x7fffffff, -5, 16 * 5 + 12])[np.arange(n) % 5]     # obstacle O, features 15 and 12, nonsense
    up = lambda a, dt=torch.float64: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dt, device=d)
    kw = dict(scene_index=up(c["scene_index"], torch.int32), count=up(c["count"], torch.int32))
    bar = np.full((R, n), np.nan)
    bar[1::2] = np.inf                                     # 0 whatever the cotangent holds there
    g = solver.clearance_vjp(up(c["cart"]), c["obstacles"], c["foot"], up(which, torch.int32), up(bar), **kw)
    cd, od = cc.unit_tangents(c)
    t = solver.clearance_jvp(up(c["cart"]), c["obstacles"], c["foot"], up(which, torch.int32), up(np.full_like(cd, np.nan)),
                             obs_dot=up(np.full_like(od, np.inf)), **kw)
    torch.cuda.synchronize()
    g, t = g.cpu().numpy(), t.cpu().numpy()
    assert g.tobytes() == np.zeros_like(g).tobytes() and t.tobytes() == np.zeros_like(t).tobytes()


@pytest.mark.parametrize("name", sorted(cc.EXACT))
def test_exact_cases_to_the_bit_on_the_device(solver, name):
    """The host file's exact and tie cases through btrapz_clearance_device and _vjp_device: headings 0 and dyadic
    coordinates and extents make every operation of the statement exact, with the device's sincos (sin 0 = 0, cos 0 = 1)
    and under any contraction into fused multiply-adds, so the clearance is the known value to the bit, g = 0 takes the
    overlap branch and gives +0, the lowest feature and the lowest obstacle win a tie, and the derivative at a tie is
    the winner's."""
    cart, ob, clear, which = cc.exact_inputs(name)
    cart_t = torch.tensor(cart, device=solver.device)
    o = solver.clearance(cart_t, ob, cc.EXACT_FOOT, d_safe=0.5)
    torch.cuda.synchronize()
    got = o["clear"].cpu().numpy()
    assert got.tobytes() == np.array([[clear]]).tobytes(), (float(got[0, 0]), clear)
    assert int(o["which"][0, 0]) == which
    au = {k: v.cpu().numpy() for k, v in o["audit"].items()}
    assert au["clear_min"].tobytes() == np.array([clear]).tobytes() and au["worst"].tolist() == [[0, which >> 4]]
    assert au["n_below"].tolist() == [int(clear < 0.5)] and au["n_invalid"].tolist() == [0]
    # ... and what the host twin says, bit for bit
    h = native.clearance_host(cart, ob, cc.EXACT_FOOT, d_safe=0.5)
    assert h["clear"].tobytes() == got.tobytes() and int(h["which"][0, 0]) == which
    if name == cc.EXACT_TIE_GRADIENT[0]:
        g = solver.clearance_vjp(cart_t, ob, cc.EXACT_FOOT, o["which"], torch.ones((1, 1), dtype=torch.float64, device=solver.device))
        torch.cuda.synchronize()
        assert g[0, :, 0].cpu().tolist() == cc.EXACT_TIE_GRADIENT[1]


def test_the_call_rides_the_callers_stream(solver):
    """In the manner of tests/test_gpu_streams.py: behind a device-side delay on a side stream the working tensors are
    loaded with the inputs X and the three calls are issued; until then they hold the decoy Y (valid inputs).  Work that ran
    on another stream would run inside the delay and see Y.  The calls return while the delay is still running, and the
    outputs equal the null-stream run's bit for bit."""
    X, Y = inputs("r253_n71_o2"), cc.make_case(253, 71, 2, n_scenes=3, seed=99)
    d = solver.device
    R, n = X["R"], X["n"]
    up = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=d)
    xs = dict(cart=up(X["cart"]), pose=up(X["obstacles"].host["pose"]), cbar=up(np.where(X["read"], X["clear_bar"], 0.0)), cdot=up(X["cart_dot"]))
    ys = dict(cart=up(Y["cart"]), pose=up(Y["obstacles"].host["pose"]), cbar=up(np.ones((R, n))), cdot=up(np.ones((3, R, 6, n))))
    w = {k: v.clone() for k, v in ys.items()}
    from spectral_amd import layout
    ob = layout.Obstacles(w["pose"], up(X["obstacles"].host["half"]), up(X["obstacles"].host["obs_count"], torch.int32))
    count, index = up(X["count"], torch.int32), up(X["scene_index"], torch.int32)

    def calls():
        o = solver.clearance(w["cart"], ob, X["foot"], scene_index=index, count=count, d_safe=0.5)
        g = solver.clearance_vjp(w["cart"], ob, X["foot"], o["which"], w["cbar"], scene_index=index, count=count)
        t = solver.clearance_jvp(w["cart"], ob, X["foot"], o["which"], w["cdot"], scene_index=index, count=count)
        return [o["clear"], o["which"], g, t] + [o["audit"][k] for k in CLEAR_AUDIT]

    for k in w:
        w[k].copy_(xs[k])
    ref = [t.cpu().numpy() for t in calls()]                       # the null-stream run (and the warm-up)
    side = torch.cuda.Stream(d)
    with torch.cuda.stream(side):                                   # warm the side stream's allocator pool
        calls()
    side.synchronize()
    for k in w:
        w[k].copy_(ys[k])
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(100_000_000)                              # tens of milliseconds at any shader clock
        done.record()
        for k in w:
            w[k].copy_(xs[k], non_blocking=True)
        out = calls()
        returned_early = not done.query()
    side.synchronize()
    assert returned_early
    for a, b in zip(out, ref):
        assert same_bits(a.cpu().numpy(), b)


# ---- end to end: 253 scenario_1 candidates of 20 segments solved on the GPU ------------------------------------------------
E2E_B, E2E_S = 253, 20
FOOT = (2.4, 0.95, 1.3)
_e2e = {}


def e2e(solver):
    if not _e2e:
        batch, sh = synth.make_scenario1_batch(E2E_B, E2E_S, 0)
        db = solver.upload(batch)
        o = {k: v.clone() for k, v in solver.solve(db, sh, keep_multipliers=True).items()}
        traj, npts = solver.sample(db, o["ctrl"], torch.arange(E2E_B, device=solver.device), sh.delta)
        torch.cuda.synchronize()
        rl = synth.refline_arc(260.0, 0.5, 80.0)
        # a slow car ahead in the ego's lane (the faster candidates reach it while they change lanes), one crawling in the
        # second lane, one overtaking on the far side
        ob = synth.obstacles_on_line(rl, [22.0, 50.0, 0.0], [1.3, 4.4, -3.5], [3.0, 2.0, 9.0], n=traj.shape[2], dt=sh.delta,
                                     half=(2.3, 0.9), dtheta=[0.08, -0.12, 0.05])
        _e2e.update(batch=batch, sh=sh, db=db, o=o, traj=traj, npts=npts, status=o["status"].cpu().numpy(), rl=rl, ob=ob)
    return _e2e


def test_collision_free_and_kinematic_admissible_then_topk(solver):
    e = e2e(solver)
    c = solver.cartesian(e["traj"], e["rl"], count=e["npts"])
    solved = torch.tensor((e["status"] == 1) | (e["status"] == 2), device=solver.device)
    assert int(solved.sum()) >= 100
    first = solver.clearance(c["cart"], e["ob"], FOOT, count=e["npts"], want=("audit",))["audit"]
    lo, hi = float(first["clear_min"][solved].min()), float(first["clear_min"][solved].max())
    assert np.isfinite(lo) and lo < hi
    d_safe = float(torch.quantile(first["clear_min"][solved], 0.4))         # a limit that rejects up to 40 % of the solved candidates
    audit = solver.clearance(c["cart"], e["ob"], FOOT, count=e["npts"], d_safe=d_safe, want=("audit",))["audit"]
    # kinematic limits that reject some solved rows too: the upper quartile of the largest |kappa| and of the lateral acceleration
    kappa_max = float(torch.quantile(c["audit"]["kappa_abs_max"][solved], 0.75))
    alat_max = float(torch.quantile(c["audit"]["alat_abs_max"][solved], 0.75))
    kin = solver.kinematic_admissible(c["audit"], kappa_max, alat_max, -10.0, 10.0, 0.5)
    free = solver.collision_free(audit, d_safe)
    mask = kin & free & solved
    torch.cuda.synchronize()
    # each mask rejects solved rows the other admits: the combination is neither of them
    assert bool((solved & free & ~kin).any()) and bool((solved & kin & ~free).any()), (int((solved & kin).sum()), int((solved & free).sum()))
    assert 8 <= int(mask.sum()) < min(int((solved & kin).sum()), int((solved & free).sum())), (int(mask.sum()), int(solved.sum()), d_safe)
    inf = float("inf")
    cost = e["o"]["cost"].masked_fill(~solved, inf)
    idx, best = solver.topk(cost.masked_fill(~mask, inf), 8)
    torch.cuda.synchronize()
    idx, cm = idx.cpu().numpy().ravel(), audit["clear_min"].cpu().numpy()
    assert (idx >= 0).all() and (cm[idx] >= d_safe).all() and kin.cpu().numpy()[idx].all()
    masked = np.where(mask.cpu().numpy(), cost.cpu().numpy(), np.inf)
    assert np.array_equal(idx, np.argsort(masked, kind="stable")[:8])       # ... and the cheapest of them
    # n_below agrees with the mask; a NaN, an invalid sample and a row below the limit are not collision-free
    assert np.array_equal((audit["n_below"] == 0).cpu().numpy() & (audit["n_invalid"] == 0).cpu().numpy(), free.cpu().numpy())
    probe = dict(clear_min=torch.tensor([1.0, float("nan"), 1.0, 0.25, inf], device=solver.device),
                 n_invalid=torch.tensor([0, 0, 1, 0, 0], dtype=torch.int32, device=solver.device))
    assert solver.collision_free(probe, 0.5).cpu().tolist() == [True, False, False, False, True]


def test_gradient_of_the_soft_minimum_clearance_through_the_whole_pipeline(solver):
    """d (sum_j w_j c_j) / d init, w = softmax(-c / 0.5 m) over a candidate's samples, through diff.clearance o
    diff.cartesian o diff.sample o diff.solve, against central differences of the whole GPU pipeline along one direction per
    candidate: within 1e-3 of the larger of the two (floor: 1e-3 of the largest derivative compared), h = 1e-3 and the
    differenced solves at eps = 1e-12 -- the bound, step and floor of tests/test_gpu_cartesian.py's pipeline test.
    Compared: of the first 40 candidates those the CPU oracle finds solved, strictly complementary and without a weakly
    active row, whose control points move affinely over the step, whose `which` names the same function at -h, 0 and +h
    wherever the weight is at least 1e-6 (a change of obstacle or feature inside the step is a kink: the quotient measures
    no derivative there; a vertex against a vertex has two names for one function, between which rounding decides, and
    the yardstick says which names those are), and whose margin by the yardstick is at least TAU at the samples that carry weight (>= 1e-2).  At least 16."""
    from vjp_reference import Adjoint, one
    e = e2e(solver)
    batch, sh, d = e["batch"], e["sh"], solver.device
    first, beta = 40, 0.5
    ok = np.zeros(E2E_B, dtype=bool)
    for b in range(first):
        adj = Adjoint(one(batch, b), sh, np.zeros(12 * E2E_S), 0.0)
        eq = (adj.u - adj.l) <= 1e-12
        y = np.abs(adj.y)
        active = (~eq) & (y > 1e-6 * max(y.max(), 1e-300))
        weak = bool((y[active] <= 1e-4 * y[~eq].max()).any()) if active.any() else False
        ok[b] = adj.status in (1, 2) and adj.strict and not weak and e["status"][b] in (1, 2)
    rng = np.random.default_rng(78)
    dirn = rng.standard_normal((E2E_B, 6)); dirn[:, 0] = 0.0

    def soft_min(clear):
        m = torch.isfinite(clear)
        w = torch.softmax(torch.where(m, -clear / beta, torch.full_like(clear, -float("inf"))), dim=1)
        return (w * torch.where(m, clear, torch.zeros_like(clear))).sum(1), w

    def value(init_np, eps):
        bt = type(batch)(B=E2E_B, S=E2E_S, seg=batch.seg, init=init_np, ref_end=batch.ref_end, dl_bounds=batch.dl_bounds)
        db = solver.upload(bt)
        o = solver.solve(db, sh, eps=eps, keep_multipliers=True)
        traj, npts = solver.sample(db, o["ctrl"], torch.arange(E2E_B, device=d), sh.delta)
        traj = traj[:, :, :e["ob"].n].contiguous()
        cart = solver.cartesian(traj, e["rl"], count=npts, want=("cart",))["cart"]
        c = solver.clearance(cart, e["ob"], FOOT, count=npts, want=("clear", "which"))
        loss, w = soft_min(c["clear"])
        torch.cuda.synchronize()
        return loss.cpu().numpy(), o["ctrl"].cpu().numpy().copy(), o["status"].cpu().numpy().copy(), c["which"].cpu().numpy(), w.cpu().numpy()

    h = 1e-3
    lp, xp, sp, wp, _ = value(batch.init + h * dirn, 1e-12)
    lm, xm, sm, wm, _ = value(batch.init - h * dirn, 1e-12)
    l0, x0, s0, w0, weight = value(batch.init.copy(), 1e-12)
    fd = (lp - lm) / (2 * h)
    second, moved = np.abs(xp + xm - 2 * x0).max(1), np.abs(xp - xm).max(1)
    affine = second <= 1e-3 * np.maximum(moved, 1e-300)
    same = np.isin(sp, (1, 2)) & np.isin(sm, (1, 2)) & np.isin(s0, (1, 2))
    carried = np.nan_to_num(weight) >= 1e-6
    # the analytic side: one backward through the four layers
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=d)
    init_t = T(batch.init).requires_grad_(True)
    params = torch.tensor(diff.params_from_shared(sh), dtype=torch.float64)
    seg = T(batch.seg)
    ctrl, cost, status = diff.solve(solver, seg, init_t, T(batch.ref_end), T(batch.dl_bounds), params, variant=0, delta=sh.delta)
    traj, npts = diff.sample(ctrl, seg, init_t, solver, delta=sh.delta)
    cart = diff.cartesian(traj[:, :, :e["ob"].n], e["rl"], solver, count=npts)
    clear, which = diff.clearance(cart, e["ob"], FOOT, solver, count=npts)
    loss, _ = soft_min(clear)
    rows = torch.tensor(np.flatnonzero(ok & same), device=d)
    loss[rows].sum().backward()
    torch.cuda.synchronize()
    an = (init_t.grad.cpu().numpy() * dirn).sum(1)
    assert np.allclose(loss.detach().cpu().numpy()[ok & same], l0[ok & same], rtol=1e-4, atol=1e-9)
    cart_np = cart.detach().cpu().numpy()
    case = dict(cart=cart_np, obstacles=e["ob"], foot=FOOT, count=None, scene_index=None, key=("e2e",), R=E2E_B, n=e["ob"].n, O=e["ob"].O)
    frozen = ok & affine & same
    for b in np.flatnonzero(frozen):
        renamed = [(int(b), int(j)) for j in np.flatnonzero(carried[b] & ((wp[b] != w0[b]) | (wm[b] != w0[b])))]
        ref = cc.reference(case, renamed)
        frozen[b] = all(ref[s] is not None and {int(wp[s]), int(wm[s]), int(w0[s])} <= ref[s]["which"] for s in renamed)
    use = frozen.copy()
    # the yardstick's margin at the samples that carry weight
    for b in np.flatnonzero(use):
        heavy = [(int(b), int(j)) for j in np.flatnonzero(np.nan_to_num(weight[b]) >= 1e-2)]
        ref = cc.reference(case, heavy)
        use[b] = all(ref[s] is not None and ref[s]["margin"] >= cr.TAU for s in heavy)
    assert use.sum() >= 16, (ok.sum(), (ok & affine).sum(), frozen.sum(), use.sum())
    top = np.abs(an[use]).max()
    scale = np.maximum(np.maximum(np.abs(an), np.abs(fd)), 1e-3 * top)
    err = np.abs(fd - an) / scale
    print("soft minimum clearance: oracle-clean %d of %d, affine %d, frozen %d, compared %d; worst |fd - an| / scale %.2e; an %s fd %s"
          % (ok.sum(), first, (ok & affine).sum(), frozen.sum(), use.sum(), err[use].max(), an[use][:4], fd[use][:4]))
    assert top > 0 and err[use].max() <= 1e-3, (err[use], an[use], fd[use])
