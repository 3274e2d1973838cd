"""Gradients of sampled trajectories and evaluated states on the GPU: btrapz_sample_vjp_device and
btrapz_eval_states_vjp_device against the NumPy yardstick (tests/states_reference.py, itself checked by
tests/test_states_reference.py), the autograd layers diff.sample / diff.eval_states, the gradient through the solve, and
tune.fit_trajectory.

The bound of the yardstick comparisons is derived, not measured: both sides evaluate the same sums J^T v in float64, so
every entry is compared against tol_j = 1e-12 (|J|^T |v|)_j.  The standard bound gamma_n (|J|^T |v|)_j with
n <= 3 (samples per segment) + 25 operations per entry is below 500 * 2^-53 = 5.6e-14 for up to 150 samples per segment;
1e-12 leaves a factor of about 20 for FMA contraction and summation order."""
import os

import numpy as np
import pytest
import torch

import states_reference as R
from spectral_amd import diff, knots, layout as L, synth, tune
from spectral_amd.native import BtrapzError

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
W = np.loadtxt(os.path.join(GOLD, "inputs", "weights.txt"))
REL = 1e-12
MAX_PER_SEGMENT = 150


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def dev(solver, a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(solver.device, dtype=dtype).contiguous()


def random_layout(rng, B, S, ragged):
    """Durations [B, S] (some shorter than delta: segments without samples) and segment counts."""
    t = rng.uniform(0.35, 1.6, (B, S))
    t[rng.random((B, S)) < 0.1] = 0.07
    seg = np.zeros((L.NUM_SEG_FIELDS, B, S))
    seg[L.F_T] = t
    cnt = rng.integers(1, S + 1, B).astype(np.int32) if ragged else None
    if ragged:
        cnt[0] = S
    return seg, cnt


def record(solver, seg, cnt, init=None):
    B, S = seg.shape[1], seg.shape[2]
    rec = dict(B=B, seg_stride=S, seg=dev(solver, seg), seg_count=None if cnt is None else dev(solver, cnt, torch.int32))
    if init is not None:
        rec["init"] = dev(solver, init)
    return rec


def durations(seg, cnt, b):
    S = seg.shape[2] if cnt is None else int(cnt[b])
    return seg[L.F_T, b, :S]


def check_sample_vjp(solver, seg, cnt, sel, max_points, delta, rng):
    B, S = seg.shape[1], seg.shape[2]
    rec = record(solver, seg, cnt)
    ob = rng.standard_normal((len(sel), 6, max_points))
    g = solver.sample_vjp(rec, torch.as_tensor(sel), delta, dev(solver, ob))
    torch.cuda.synchronize()
    cb, ib = g["ctrl"].cpu().numpy(), g["init"].cpu().numpy()
    worst = 0.0
    for j, b in enumerate(sel):
        Sb = S if cnt is None else int(cnt[b]) if 0 <= b < B else 0
        if not (0 <= b < B) or Sb < 1 or Sb > S:
            assert (cb[j] == 0).all() and (ib[j] == 0).all(), (j, b)
            continue
        t = durations(seg, cnt, b)
        assert R.samples_per_segment(t, delta) <= MAX_PER_SEGMENT
        want, wi = R.sample_vjp(t, delta, ob[j])
        mag, _ = R.sample_vjp(t, delta, ob[j], absolute=True)
        err = np.abs(cb[j, :12 * Sb] - want)
        assert (err <= REL * mag).all(), (j, b, (err / np.maximum(mag, 1e-300)).max())
        worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
        assert (cb[j, 12 * Sb:] == 0).all()
        assert np.array_equal(ib[j], wi)   # sample 0 is init: its cotangent, unchanged
    print("sample_vjp S=%d ragged=%s max_points=%d: worst err / (|J|^T |v|) = %.2e" % (S, cnt is not None, max_points, worst))


@pytest.mark.parametrize("S", [1, 2, 10, 20, 64, 65, 130, 256])
@pytest.mark.parametrize("ragged", [False, True])
def test_sample_vjp_against_the_yardstick(solver, S, ragged):
    rng = np.random.default_rng(100 + S + ragged)
    B, delta = 6, 0.1
    seg, cnt = random_layout(rng, B, S, ragged)
    full = max(sum(int(tk / delta) for tk in durations(seg, cnt, b)) for b in range(B)) + 2
    sel = [3, 0, 3, 5, -1, B, 1, 3, 2, 4]   # repeats, and entries outside [0, B)
    check_sample_vjp(solver, seg, cnt, sel, full, delta, rng)
    check_sample_vjp(solver, seg, cnt, sel, max(2, full // 2), delta, rng)   # a max_points that truncates
    check_sample_vjp(solver, seg, cnt, sel, 1, delta, rng)                   # ... to the initial state alone


@pytest.mark.parametrize("variant", [0, 1])
def test_sample_vjp_on_corridor_records(solver, variant):
    """The ragged records the device corridor stage produces from the bundled inputs, both variants."""
    rng = np.random.default_rng(7 + variant)
    for name in ("c1", "c2", "c3"):
        kb = knots.parse_corridor_file(os.path.join(GOLD, "inputs", name + ".txt"))
        rec = solver.corridor_batch(kb, variant, seg_stride=64)
        torch.cuda.synchronize()
        seg, cnt = rec["seg"].cpu().numpy(), rec["seg_count"].cpu().numpy()
        if not 1 <= int(cnt[0]) <= 64:
            continue
        full = sum(int(tk / kb.delta) for tk in durations(seg, cnt, 0)) + 2
        check_sample_vjp(solver, seg, cnt, [0, 0], full, kb.delta, rng)


def state_times(rng, t):
    """Times of one candidate: off the branch points (two per segment and one beyond the horizon), not > 0, exactly on
    the joints (cumulative sums as the forward's walk subtracts them), beyond the horizon; shuffled."""
    joints = np.concatenate([[0.0], np.cumsum(t)])
    tm = []
    for k in range(len(t)):
        tm += [joints[k] + 0.137 * t[k], joints[k] + 0.61 * t[k]]
    tm += [joints[-1] + 0.5, 0.0, -1.0, joints[-1] + 3.0]
    tm += list(joints[1:])
    tm = np.array(tm)
    rng.shuffle(tm)
    return tm


def check_states_vjp(solver, seg, cnt, n_pad, rng):
    B, S = seg.shape[1], seg.shape[2]
    rec = record(solver, seg, cnt)
    ctrl = rng.standard_normal((B, 12 * S))
    per = [state_times(rng, durations(seg, cnt, b)) for b in range(B)]
    n = max(len(p) for p in per) + n_pad
    times = np.stack([np.concatenate([p, rng.uniform(0, durations(seg, cnt, b).sum(), n - len(p))]) for b, p in enumerate(per)])
    xb = rng.standard_normal((B, 2, n, 3))
    g = solver.eval_states_vjp(rec, dev(solver, ctrl), dev(solver, times), dev(solver, xb))
    torch.cuda.synchronize()
    cb, tb = g["ctrl"].cpu().numpy(), g["times"].cpu().numpy()
    worst = [0.0, 0.0]
    for b in range(B):
        t = durations(seg, cnt, b)
        Sb = len(t)
        c = np.concatenate([ctrl[b, :6 * Sb], ctrl[b, 6 * Sb:12 * Sb]])
        want_c, want_t = R.states_vjp(t, c, times[b], xb[b])
        mag_c, mag_t = R.states_vjp(t, c, times[b], xb[b], absolute=True)
        ec, et = np.abs(cb[b, :12 * Sb] - want_c), np.abs(tb[b] - want_t)
        assert (ec <= REL * mag_c).all(), (b, (ec / np.maximum(mag_c, 1e-300)).max())
        assert (et <= REL * mag_t).all(), (b, (et / np.maximum(mag_t, 1e-300)).max())
        assert (cb[b, 12 * Sb:] == 0).all()
        assert (tb[b][~(times[b] > 0)] == 0).all()
        worst = [max(worst[0], float((ec / np.maximum(mag_c, 1e-300)).max())), max(worst[1], float((et / np.maximum(mag_t, 1e-300)).max()))]
    print("eval_states_vjp S=%d ragged=%s n_times=%d: worst ctrl_bar %.2e, times_bar %.2e of the bound's scale" %
          (S, cnt is not None, n, worst[0], worst[1]))


@pytest.mark.parametrize("S", [1, 2, 10, 20, 64, 65, 130, 256])
@pytest.mark.parametrize("ragged", [False, True])
def test_eval_states_vjp_against_the_yardstick(solver, S, ragged):
    rng = np.random.default_rng(200 + S + ragged)
    seg, cnt = random_layout(rng, 5, S, ragged)
    seg[L.F_T] = np.maximum(seg[L.F_T], 0.35)
    check_states_vjp(solver, seg, cnt, 0 if S > 20 else 70, rng)   # (n_times beyond 64: more than one chunk of times)


def solved_batch(solver, B=64, S=10, seed=51):
    batch, sh = synth.make_scenario1_batch(B, S, 0, seed=seed)
    db = solver.upload(batch)
    o = solver.solve(db, sh)
    torch.cuda.synchronize()
    return batch, sh, db, o["ctrl"].clone()


def test_forwards_are_unchanged(solver):
    batch, sh, db, ctrl = solved_batch(solver)
    sel = torch.tensor([5, 0, 5, 63, 17])
    want, wn = solver.sample(db, ctrl, sel, sh.delta)
    got, gn = diff.sample(ctrl, db.seg, db.init, solver, sel=sel, delta=sh.delta)
    torch.cuda.synchronize()
    assert torch.equal(want, got) and torch.equal(wn, gn)
    times = torch.from_numpy(np.cumsum(batch.seg[L.F_T], axis=1) + 0.25)
    x = solver.eval_states(db, ctrl, times)
    y = diff.eval_states(ctrl, db.seg, times, solver)
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    # ragged records with every count equal to the stride: the same rows
    cnt = torch.full((batch.B,), batch.S, dtype=torch.int32, device=solver.device)
    got2, gn2 = diff.sample(ctrl, db.seg, db.init, solver, seg_count=cnt, sel=sel, delta=sh.delta)
    y2 = diff.eval_states(ctrl, db.seg, times, solver, seg_count=cnt)
    torch.cuda.synchronize()
    assert torch.equal(want, got2) and torch.equal(wn, gn2) and torch.equal(x, y2)


def test_gradients_are_deterministic_and_uniform_equals_ragged(solver):
    rng = np.random.default_rng(9)
    B, S, delta = 48, 20, 0.1
    seg, _ = random_layout(rng, B, S, False)
    cnt = np.full(B, S, dtype=np.int32)
    sel = torch.as_tensor(rng.integers(0, B, 96))
    mp = max(sum(int(tk / delta) for tk in seg[L.F_T, b]) for b in range(B)) + 2
    ob = dev(solver, rng.standard_normal((96, 6, mp)))
    ctrl = dev(solver, rng.standard_normal((B, 12 * S)))
    times = dev(solver, rng.uniform(-0.5, seg[L.F_T].sum(1).max() + 1.0, (B, 23)))
    xb = dev(solver, rng.standard_normal((B, 2, 23, 3)))
    runs = []
    for rec in (record(solver, seg, None), record(solver, seg, None), record(solver, seg, cnt)):
        a = solver.sample_vjp(rec, sel, delta, ob)
        b = solver.eval_states_vjp(rec, ctrl, times, xb)
        torch.cuda.synchronize()
        runs.append([a["ctrl"].clone(), a["init"].clone(), b["ctrl"].clone(), b["times"].clone()])
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert torch.equal(x, y)
    # ... and through autograd, with a selection that repeats candidates
    grads = []
    for _ in range(2):
        c = ctrl.clone().requires_grad_(True)
        i = dev(solver, np.zeros((B, 6))).requires_grad_(True)
        traj, _ = diff.sample(c, dev(solver, seg), i, solver, sel=sel, delta=delta)
        (traj * ob).sum().backward()
        grads.append((c.grad.clone(), i.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_autograd_directional_derivatives(solver):
    """diff.sample and diff.eval_states are linear in ctrl (and init): a central difference along a random direction is
    exact to rounding, so it is held to the bound of the yardstick comparison, on the scale sum |v| |J| |direction|
    (+ the rounding of the two forwards over the step)."""
    rng = np.random.default_rng(11)
    B, S, delta = 7, 10, 0.1
    seg, cnt = random_layout(rng, B, S, True)
    seg[L.F_T] = np.maximum(seg[L.F_T], 0.35)
    segd, cntd = dev(solver, seg), dev(solver, cnt, torch.int32)
    sel = torch.tensor([2, 6, 2, 0])
    ctrl0 = rng.standard_normal((B, 12 * S))
    for b in range(B):
        ctrl0[b, 12 * int(cnt[b]):] = 0.0
    init0 = rng.standard_normal((B, 6))
    dc, di = rng.standard_normal(ctrl0.shape), rng.standard_normal(init0.shape)
    c = dev(solver, ctrl0).requires_grad_(True)
    i = dev(solver, init0).requires_grad_(True)
    traj, npts = diff.sample(c, segd, i, solver, seg_count=cntd, sel=sel, delta=delta)
    v = dev(solver, rng.standard_normal(tuple(traj.shape)))
    for j in range(len(sel)):
        v[j, :, int(npts[j]):] = 0.0
    (traj * v).sum().backward()
    lhs = float((c.grad * dev(solver, dc)).sum() + (i.grad * dev(solver, di)).sum())
    f = lambda s: float((diff.sample(dev(solver, ctrl0 + s * dc), segd, dev(solver, init0 + s * di), solver, seg_count=cntd,
                                     sel=sel, delta=delta)[0] * v).sum())
    h = 1.0
    fd = (f(h) - f(-h)) / (2 * h)
    # the scale of the bound: sum |v| |J| (|ctrl| + |direction|), from the yardstick
    scale = 0.0
    for j, b in enumerate(sel.tolist()):
        t = durations(seg, cnt, b)
        Sb = len(t)
        out, _ = R.sample_forward(t, delta, np.abs(ctrl0[b, :12 * Sb]) + np.abs(dc[b, :12 * Sb]),
                                  np.abs(init0[b]) + np.abs(di[b]), traj.shape[2], absolute=True)
        scale += float((out * np.abs(v[j].cpu().numpy())).sum())
    print("diff.sample directional: autograd %.15e central %.15e scale %.3e" % (lhs, fd, scale))
    assert abs(lhs - fd) <= REL * scale
    # states: ctrl by the same argument; times against the yardstick's derivative (not linear in time)
    times0 = np.stack([np.concatenate([[-0.3, durations(seg, cnt, b).sum() + 0.4], rng.uniform(0.05, durations(seg, cnt, b).sum(), 9)])
                       for b in range(B)])
    c = dev(solver, ctrl0).requires_grad_(True)
    tm = dev(solver, times0).requires_grad_(True)
    x = diff.eval_states(c, segd, tm, solver, seg_count=cntd)
    vx = dev(solver, rng.standard_normal(tuple(x.shape)))
    (x * vx).sum().backward()
    lhs = float((c.grad * dev(solver, dc)).sum())
    g = lambda s: float((diff.eval_states(dev(solver, ctrl0 + s * dc), segd, dev(solver, times0), solver, seg_count=cntd) * vx).sum())
    fd = (g(h) - g(-h)) / (2 * h)
    scale = 0.0
    vxn = vx.cpu().numpy()
    for b in range(B):
        t = durations(seg, cnt, b)
        Sb = len(t)
        J = np.abs(R.states_matrix(t, times0[b]))
        scale += float(np.abs(vxn[b]).reshape(-1) @ (J @ (np.abs(ctrl0[b, :12 * Sb]) + np.abs(dc[b, :12 * Sb]))))
        want_t = R.states_vjp(t, ctrl0[b, :12 * Sb], times0[b], vxn[b])[1]
        mag_t = R.states_vjp(t, ctrl0[b, :12 * Sb], times0[b], vxn[b], absolute=True)[1]
        assert (np.abs(tm.grad[b].cpu().numpy() - want_t) <= REL * mag_t).all()
    print("diff.eval_states directional: autograd %.15e central %.15e scale %.3e" % (lhs, fd, scale))
    assert abs(lhs - fd) <= REL * scale


def test_gradient_through_the_solve_is_a_descent_direction(solver):
    """First-order descent identity for L(theta) = sum ((diff.sample(diff.solve(theta)) - target)^2), theta the log-factors
    of the ten weights: (L(theta - eta g) - L(theta)) / (-eta |g|^2) -> 1 as eta -> 0.  Batch: the 64 scenario_1 candidates
    of test_weight_fitting_with_adam (seed 51), restricted to the candidates that are strictly complementary at theta by
    the criterion of tests/vjp_reference.py (the oracle's multipliers, on the CPU).  With seed 51 and the signs of seed 6
    the filter drops 0 of 64 candidates (checked on the CPU with the oracle); the test caps the dropped share at 1 / 2."""
    from vjp_reference import Adjoint, one
    S = 10
    batch, sh = synth.make_scenario1_batch(64, S, 0, seed=51)
    d = solver.device
    tt = lambda a: torch.tensor(a, device=d)
    seg, init, ref_end, dl = tt(batch.seg), tt(batch.init), tt(batch.ref_end), tt(batch.dl_bounds)
    p_ref = tt(diff.params_from_shared(sh))
    theta0 = np.random.default_rng(6).choice([-1.0, 1.0], 10) * np.log(1.3)
    prm0 = diff.params_from_shared(sh).copy()
    prm0[:10] *= np.exp(theta0)
    sh0 = diff.shared_from_params(prm0, 0, sh.delta)
    strict = np.array([Adjoint(one(batch, b), sh0, np.zeros(12 * S), 0.0).strict for b in range(64)])
    print("strictly complementary: %d of 64" % strict.sum())
    assert strict.sum() >= 32
    with torch.no_grad():
        c_ref, _, st_ref = diff.solve(solver, seg, init, ref_end, dl, p_ref, variant=0, delta=sh.delta)
        target, _ = diff.sample(c_ref, seg, init, solver, delta=sh.delta)
    keep = tt(strict) & ((st_ref == 1) | (st_ref == 2))

    def loss(theta):
        prm = torch.cat([p_ref[:10] * torch.exp(theta), p_ref[10:]])
        ctrl, _, st = diff.solve(solver, seg, init, ref_end, dl, prm, variant=0, delta=sh.delta)
        traj, _ = diff.sample(ctrl, seg, init, solver, delta=sh.delta)
        m = (keep & ((st == 1) | (st == 2))).to(torch.float64)[:, None, None]
        return (((traj - target) * m) ** 2).sum(), int(m.sum())

    theta = tt(theta0).requires_grad_(True)
    L0, n0 = loss(theta)
    assert n0 >= 32
    L0.backward()
    g = theta.grad.clone()
    gg = float((g * g).sum())
    assert gg > 0 and L0.item() > 0
    eta = 1.0 / gg ** 0.5
    ratios = []
    with torch.no_grad():
        for _ in range(20):
            L1, n1 = loss(theta.detach() - eta * g)
            ratios.append((L1.item() - L0.item()) / (-eta * gg) if n1 == n0 else float("nan"))
            if 0.5 <= ratios[-1] <= 1.5:
                break
            eta *= 0.5
    print("descent ratios along the halving sequence:", ["%.4f" % r for r in ratios])
    assert 0.5 <= ratios[-1] <= 1.5, ratios


def synthetic_fit(solver, starts=16, steps=100):
    """(result of tune.fit_trajectory, known weights): the target is sampled from a solve of the bundled c1 corridor with
    the bundled weights; the starts are those weights with every log-weight moved by +-ln 1.3."""
    kb = knots.parse_corridor_file(os.path.join(GOLD, "inputs", "c1.txt"))
    rec = tune.replicated_record(solver, kb, 0, 1)
    o = solver.solve_sets_ragged(rec, [tune.shared_of(W, kb.header, kb.delta, 0)], torch.zeros(1, dtype=torch.int32, device=solver.device))
    assert int(o["status"][0]) in (1, 2)
    with torch.no_grad():
        target, npts = diff.sample(o["ctrl"], rec["seg"], rec["init"], solver, seg_count=rec["seg_count"], delta=kb.delta)
    target = target[0, :, :int(npts[0])].cpu().numpy()
    return tune.fit_trajectory(solver, kb, 0, target, W, starts=starts, steps=steps, seed=6, spread=float(np.log(1.3))), W


def test_fit_trajectory_reduces_the_loss(solver):
    """tune.fit_trajectory on a target sampled from a solve with known weights.  The reduction asserted is a third of the
    factor R measured by tools/fit_trajectory.py --synthetic (profiles/fit_trajectory.json): the kernels
    are deterministic, so the margin only has to cover library and driver versions."""
    import json
    prof = json.load(open(os.path.join(os.path.dirname(GOLD), "..", "profiles", "fit_trajectory.json")))
    R_measured = prof["synthetic"]["reduction"]
    r, _ = synthetic_fit(solver, starts=prof["synthetic"]["starts"], steps=prof["synthetic"]["steps"])
    print("fit_trajectory: mean loss %.4e -> %.4e (factor %.1f; recorded R = %.1f), best %.4e" %
          (r["start_mean"], r["final_mean"], r["start_mean"] / r["final_mean"], R_measured, r["best"]))
    assert R_measured >= 3
    assert r["final_mean"] <= r["start_mean"] / (R_measured / 3), (r["start_mean"], r["final_mean"])
    assert r["solves"] == prof["synthetic"]["starts"] * (prof["synthetic"]["steps"] + 1)
    assert r["weights"].shape == (prof["synthetic"]["starts"], 10)


def test_refusals_and_defined_cases(solver):
    d = solver.device
    ctx = solver.ctx
    rng = np.random.default_rng(13)
    B, S, delta = 4, 3, 0.1
    seg, _ = random_layout(rng, B, S, False)
    segd = dev(solver, seg)
    sel = torch.tensor([0, 1], dtype=torch.int64, device=d)
    ob = dev(solver, rng.standard_normal((2, 6, 40)))
    cb = torch.empty((2, 12 * S), dtype=torch.float64, device=d)
    ib = torch.empty((2, 6), dtype=torch.float64, device=d)
    sv = lambda **k: ctx.sample_vjp_device(**{**dict(B=B, seg_stride=S, seg_count=None, delta=delta, seg=segd, sel=sel,
                                                     max_points=40, out_bar=ob, ctrl_bar=cb, init_bar=ib), **k})
    for kw, text in ((dict(seg=None), "seg, sel and out_bar"), (dict(sel=None), "seg, sel and out_bar"),
                     (dict(out_bar=None), "seg, sel and out_bar"), (dict(B=0), "B >= 1"), (dict(max_points=0), "max_points >= 1"),
                     (dict(nsel=0), "nsel >= 1"),
                     (dict(delta=0.0), "delta must be > 0"), (dict(delta=float("nan")), "delta must be > 0"),
                     (dict(seg_stride=257), "BTRAPZ_MAX_SEGMENTS_LONG"),
                     (dict(ctrl_bar=None, init_bar=None), "both null")):
        with pytest.raises(BtrapzError, match=text) as e:
            sv(**kw)
        assert "(-1)" in str(e.value)   # BTRAPZ_EINVAL
    ctrl = dev(solver, rng.standard_normal((B, 12 * S)))
    times = dev(solver, rng.uniform(0, 2, (B, 5)))
    xb = dev(solver, rng.standard_normal((B, 2, 5, 3)))
    cb2 = torch.empty((B, 12 * S), dtype=torch.float64, device=d)
    tb2 = torch.empty((B, 5), dtype=torch.float64, device=d)
    ev = lambda **k: ctx.eval_states_vjp_device(**{**dict(B=B, seg_stride=S, seg_count=None, seg=segd, ctrl=ctrl, n_times=5,
                                                          times=times, x_bar=xb, ctrl_bar=cb2, times_bar=tb2), **k})
    for kw, text in ((dict(seg=None), "seg, times and x_bar"), (dict(times=None), "seg, times and x_bar"),
                     (dict(x_bar=None), "seg, times and x_bar"), (dict(B=0), "B >= 1"), (dict(n_times=0), "n_times >= 1"),
                     (dict(seg_stride=257), "BTRAPZ_MAX_SEGMENTS_LONG"), (dict(ctrl_bar=None, times_bar=None), "both null"),
                     (dict(ctrl=None), "times_bar needs ctrl")):
        with pytest.raises(BtrapzError, match=text) as e:
            ev(**kw)
        assert "(-1)" in str(e.value)
    # NULL outputs are skipped: the other output is what the full call gives; ctrl may be NULL without times_bar
    sv(); ev()
    torch.cuda.synchronize()
    full = [cb.clone(), ib.clone(), cb2.clone(), tb2.clone()]
    for t in (cb, ib, cb2, tb2):
        t.fill_(float("nan"))
    sv(init_bar=None); sv(ctrl_bar=None); ev(times_bar=None, ctrl=None); ev(ctrl_bar=None)
    torch.cuda.synchronize()
    for x, y in zip(full, (cb, ib, cb2, tb2)):
        assert torch.equal(x, y)
    # a selection the forward answers with npoints = 0, and a candidate with a bad segment count: zeros
    cnt = dev(solver, np.array([3, 0, 4, 2]), torch.int32)
    sel4 = torch.tensor([1, 2, -3, 9, 3], dtype=torch.int64, device=d)
    ob4 = dev(solver, rng.standard_normal((5, 6, 40)))
    g = solver.sample_vjp(dict(B=B, seg_stride=S, seg=segd, seg_count=cnt), sel4, delta, ob4)
    fwd = torch.zeros((5, 6, 40), dtype=torch.float64, device=d)
    npts = torch.zeros(5, dtype=torch.int32, device=d)
    ctx.sample_ragged_device(B, S, cnt, delta, segd, dev(solver, np.zeros((B, 6))), ctrl, sel4, 40, fwd, npts)
    torch.cuda.synchronize()
    assert npts.tolist()[:4] == [0, 0, 0, 0] and npts[4] > 0
    assert (g["ctrl"][:4] == 0).all() and (g["init"][:4] == 0).all()
    assert (g["ctrl"][4, :12] != 0).any() and torch.equal(g["init"][4], ob4[4, :, 0])
    h = solver.eval_states_vjp(dict(B=B, seg_stride=S, seg=segd, seg_count=cnt), ctrl, times, xb)
    torch.cuda.synchronize()
    assert (h["ctrl"][1:3] == 0).all() and (h["times"][1:3] == 0).all()
    assert (h["ctrl"][0] != 0).any() and (h["ctrl"][3, :24] != 0).any() and (h["ctrl"][3, 24:] == 0).all()
