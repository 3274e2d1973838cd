"""btrapz_traj_cost_device / btrapz_traj_cost_vjp_device (a_cost of sampled trajectories and its gradient) on the GPU:
against find_traj's own return value, the oracle's orc_sample + orc_acost and the NumPy yardstick
(tests/acost_reference.py); bit-for-bit equalities between layouts; candidates that are not scored; the winner by a_cost;
the VJP against the yardstick and central differences; gradients through diff.solve + diff.traj_cost; Euler's relation
of the homogeneous objective; descent on c1.txt; refusals."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from acost_reference import a_cost as ref_acost, sample_count, samples
from helpers import O
from spectral_amd import diff, knots, layout as L, native, synth
from spectral_amd.native import BtrapzError
from vjp_reference import one, reference_vjp

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
W = np.loadtxt(os.path.join(GOLD, "inputs", "weights.txt"))
INPUTS = sorted(f[:-4] for f in os.listdir(os.path.join(GOLD, "inputs")) if f.startswith("c") and f.endswith(".txt"))
# find_traj returns a trajectory on 23 of the 26 (input, variant) pairs ("Acceptance"): status 1, or
# status 2 with violations for the rescued c7 family (status 2 also ends some exact solves at their round-off floor);
# c_road_s1_2 (both variants) and c_road_s1_3 cuboid return 1e11


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def shared_of(w, header, delta, variant):
    w = [float(v) for v in w]
    return L.Shared(w_s=(w[4], w[5], w[0], w[1]), w_l=(w[6], w[7], w[2], w[3]), weight_end_s=w[8], weight_end_l=w[9],
                    ds_ref=header["ds_ref"], dl_ref=header["dl_ref"], dds=tuple(header["dds"]), ddds=tuple(header["ddds"]),
                    ddl=tuple(header["ddl"]), dddl=tuple(header["dddl"]), delta=delta, variant=variant)


def dev(solver, a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(solver.device, dtype=dtype).contiguous()


def record(solver, seg, seg_count, init):
    B, S = seg.shape[1], seg.shape[2]
    return dict(B=B, seg_stride=S, seg=dev(solver, seg), seg_count=None if seg_count is None else dev(solver, seg_count, torch.int32),
                init=dev(solver, init))


def params_row(sh):
    return sh.as_array()[:20]


def oracle_acost(variant, sh, t, delta, ctrl, init, s_ref, l_ref):
    """orc_sample + orc_acost on one candidate (None where the oracle refuses the sample count)."""
    cubes = []
    for tk in t:
        c = O.Cube(); c.t = float(tk); cubes.append(c)
    rc, smp = O.sample(cubes, delta, ctrl, init[:3], init[3:], cap=100000)
    if rc != 0:
        return None
    inp = O.Input()
    inp.N, inp.delta = len(s_ref), delta
    xr, yr = np.ascontiguousarray(s_ref, dtype=np.float64), np.ascontiguousarray(l_ref, dtype=np.float64)
    inp.x_ref, inp.y_ref = O._dp(xr), O._dp(yr)
    p = O.Params(sh.w_s[2], sh.w_s[3], sh.w_l[2], sh.w_l[3], sh.w_s[0], sh.w_s[1], sh.w_l[0], sh.w_l[1],
                 sh.weight_end_s, sh.weight_end_l, 0)
    return O.lib().orc_acost(variant, C.byref(p), C.byref(inp), len(smp[0]),
                             *[np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_double)) for a in smp])


DURATIONS = (0.5, 1.0, 1.05, 0.4, 2.0, 0.75)
# segments of 70 and 130 samples: longer than one 62-sample chunk, and spanning three
LONG_DURATIONS = DURATIONS + (7.0, 13.0)


def ragged_batch(B, smax, seed, variant=0, durations=DURATIONS):
    """Random ragged batch: durations of whole and fractional sample counts, 1..smax segments, random control points and
    reference lines (a_cost does not need a solved trajectory)."""
    rng = np.random.default_rng(seed)
    stride = max(smax, 1)
    counts = rng.integers(1, smax + 1, B)
    counts[:4] = [1, smax, max(1, smax // 2), min(smax, 65) if smax >= 65 else smax]
    seg = np.zeros((L.NUM_SEG_FIELDS, B, stride))
    seg[L.F_T] = rng.choice(durations, size=(B, stride))
    ctrl = rng.standard_normal((B, 12 * stride)) * 3 + np.linspace(0, 30, 12 * stride)[None]
    init = rng.standard_normal((B, 6))
    N = int(rng.integers(20, 40 * smax))
    s_ref = np.cumsum(rng.random((B, N)), 1)
    l_ref = rng.standard_normal((B, N))
    sh = synth.shared_params(variant)
    return seg, counts.astype(np.int32), ctrl, init, s_ref, l_ref, sh


def test_matches_find_traj(solver):
    """Every bundled input and variant where find_traj returns a trajectory, rescued (status 2) ones included."""
    checked, rescued = [], []
    for name in INPUTS:
        kb = knots.parse_corridor_file(os.path.join(GOLD, "inputs", name + ".txt"))
        for variant in (0, 1):
            cost, _, ctrl = native.find_traj_mem(variant, list(W) + [1], kb)
            if cost >= 1e10:
                continue
            st, viol = native.find_traj_last_status()
            S = len(ctrl) // 12
            rec = solver.corridor_batch(kb, variant, seg_stride=max(S, 16))
            torch.cuda.synchronize()
            assert int(rec["seg_count"][0]) == S, (name, variant)
            sh = shared_of(W, kb.header, kb.delta, variant)
            c = np.zeros((1, 12 * rec["seg_stride"])); c[0, :12 * S] = ctrl
            got, npts = solver.traj_cost(rec, sh, dev(solver, c), kb.s_ref, kb.l_ref)
            got = float(got[0])
            assert abs(got - cost) <= 1e-11 * abs(cost), (name, variant, st, got, cost)
            checked.append((name, variant))
            if st == 2 and np.any(viol != 0):   # (status 2 with violations: the rescue pass's trajectory)
                rescued.append((name, variant))
    assert len(checked) == 23, checked
    assert sorted(rescued) == sorted((n, v) for n in ("c7", "c7_7", "c7_10") for v in (0, 1)), rescued


BATCHES = {
    "config3": lambda: synth.make_batch(256, 20, config=3, variant=0, seed=3),
    "cuboid": lambda: synth.make_scenario1_batch(256, 16, 1, seed=4),
}


def solved(solver, batch, sh):
    db = solver.upload(batch)
    o = solver.solve(db, sh, out={"ctrl": torch.zeros((batch.B, 12 * batch.S), dtype=torch.float64, device=solver.device),
                                  "cost": torch.empty(batch.B, dtype=torch.float64, device=solver.device),
                                  "status": torch.empty(batch.B, dtype=torch.int32, device=solver.device),
                                  "iters": torch.empty(batch.B, dtype=torch.int32, device=solver.device)})
    return db, o


def lines(batch, seed):
    rng = np.random.default_rng(seed)
    N = 10 * batch.S + 1 - 3   # shorter than the samples: the clamps are active
    s_ref = np.cumsum(rng.random((batch.B, N)) * 1.5, 1)
    l_ref = 0.3 * rng.standard_normal((batch.B, N))
    return s_ref, l_ref


@pytest.mark.parametrize("family", list(BATCHES))
def test_solved_batches_match_the_oracle(solver, family):
    batch, sh = BATCHES[family]()
    db, o = solved(solver, batch, sh)
    s_ref, l_ref = lines(batch, 7)
    cost, npts = solver.traj_cost(db, sh, o["ctrl"], s_ref, l_ref, status=o["status"])
    torch.cuda.synchronize()
    cost, npts, st = cost.cpu().numpy(), npts.cpu().numpy(), o["status"].cpu().numpy()
    ctrl = o["ctrl"].cpu().numpy()
    ok = (st == 1) | (st == 2)
    assert ok.sum() > batch.B // 2
    assert np.isinf(cost[~ok]).all() and (npts[~ok] == 0).all()
    for b in np.flatnonzero(ok)[::9]:
        want = oracle_acost(sh.variant, sh, batch.seg[L.F_T, b], sh.delta, ctrl[b], batch.init[b], s_ref[b], l_ref[b])
        assert abs(cost[b] - want) <= 1e-11 * abs(want), (b, cost[b], want)
        assert npts[b] == sample_count(batch.seg[L.F_T, b], sh.delta)[0]


@pytest.mark.parametrize("smax,variant", [(24, 0), (160, 0), (160, 1), (256, 1)])
def test_ragged_long_batches_match_the_oracle(solver, smax, variant):
    seg, counts, ctrl, init, s_ref, l_ref, sh = ragged_batch(96, smax, smax + variant, variant)
    rec = record(solver, seg, counts, init)
    cost, npts = solver.traj_cost(rec, sh, dev(solver, ctrl), s_ref, l_ref)
    torch.cuda.synchronize()
    cost, npts = cost.cpu().numpy(), npts.cpu().numpy()
    n_long = 0
    for b in range(0, 96, 5):
        S = counts[b]
        t = seg[L.F_T, b, :S]
        c = np.concatenate([ctrl[b, :6 * S], ctrl[b, 6 * S:12 * S]])
        want = oracle_acost(variant, sh, t, sh.delta, c, init[b], s_ref[b], l_ref[b])
        npd, npi = sample_count(t, sh.delta)
        if want is None or npd != npi:
            assert np.isinf(cost[b]) and npts[b] == 0
            continue
        assert abs(cost[b] - want) <= 1e-11 * abs(want), (b, S, cost[b], want)
        assert npts[b] == npd
        n_long += S > 64
    assert smax < 65 or n_long > 0


@pytest.mark.parametrize("B,S,stride", [(256, 20, 32), (6, 70, 256)])
def test_knot_level_ragged_batches_match_the_oracle(solver, B, S, stride):
    """The knot-level pipeline: scenario_1 knots through the device corridor stage and a ragged solve (S = 70: candidates
    of 65-160 segments, the long form), scored with their own reference lines."""
    kb = synth.scenario1_knots(B, S, seed=31)
    sh = synth.shared_params(0)
    rec = solver.corridor_batch(kb, 0, seg_stride=stride)
    o = solver.solve_ragged(rec, sh)
    cost, npts = solver.traj_cost(rec, sh, o["ctrl"], kb.s_ref, kb.l_ref, status=o["status"])
    torch.cuda.synchronize()
    cost, npts, st = cost.cpu().numpy(), npts.cpu().numpy(), o["status"].cpu().numpy()
    counts, t_all, ctrl = rec["seg_count"].cpu().numpy(), rec["seg"][L.F_T].cpu().numpy(), o["ctrl"].cpu().numpy()
    ok = (st == 1) | (st == 2)
    assert ok.sum() >= B // 2
    assert np.isinf(cost[~ok]).all()
    checked = []
    for b in np.flatnonzero(ok)[::max(1, B // 24)]:
        n = counts[b]
        want = oracle_acost(0, sh, t_all[b, :n], sh.delta, ctrl[b, :12 * n], kb.init[b], kb.s_ref[b], kb.l_ref[b])
        assert want is not None and abs(cost[b] - want) <= 1e-11 * abs(want), (b, n, cost[b], want)
        checked.append(n)
    assert len(set(checked)) > 1 and (S < 65 or min(checked) > 64), checked


def test_bit_for_bit_equalities(solver):
    seg, counts, ctrl, init, s_ref, l_ref, sh = ragged_batch(128, 20, 5)
    uni_count = np.full(128, 20, dtype=np.int32)
    c = dev(solver, ctrl)
    u, _ = solver.traj_cost(record(solver, seg, None, init), sh, c, s_ref, l_ref)
    r, _ = solver.traj_cost(record(solver, seg, uni_count, init), sh, c, s_ref, l_ref)
    u2, _ = solver.traj_cost(record(solver, seg, None, init), sh, c, s_ref, l_ref)
    assert torch.equal(u, r) and torch.equal(u, u2)
    # a shared reference line = the same line broadcast to every candidate
    rec = record(solver, seg, counts, init)
    a, _ = solver.traj_cost(rec, sh, c, s_ref[0], l_ref[0])
    b, _ = solver.traj_cost(rec, sh, c, np.broadcast_to(s_ref[0], s_ref.shape), np.broadcast_to(l_ref[0], l_ref.shape))
    assert torch.equal(a, b)
    # sets = one call per set
    sets = [synth.shared_params(0, weights=tuple(np.array(synth.REFERENCE_WEIGHTS) * f)) for f in (1.0, 0.5, 2.0)]
    idx = dev(solver, np.arange(128) % 3, torch.int32)
    m, _ = solver.traj_cost(rec, sets, c, s_ref, l_ref, set_index=idx)
    for g, sg in enumerate(sets):
        single, _ = solver.traj_cost(rec, sg, c, s_ref, l_ref)
        sel = torch.arange(128, device=solver.device) % 3 == g
        assert torch.equal(m[sel], single[sel])
    # the VJP too
    abar = dev(solver, np.random.default_rng(1).standard_normal(128))
    g1 = solver.traj_cost_vjp(rec, sh, c, s_ref, l_ref, abar)
    g2 = solver.traj_cost_vjp(rec, sh, c, s_ref, l_ref, abar)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_candidates_that_are_not_scored(solver):
    seg, counts, ctrl, init, s_ref, l_ref, sh = ragged_batch(16, 8, 9)
    t = seg[L.F_T]
    t[5, :2] = [100.0, 0.3]   # np accumulated in double runs ahead of the int sum
    counts[5] = 2
    npd, npi = sample_count(t[5, :2], sh.delta)
    assert npd != npi
    t[6, 0] = 0.0             # a duration find_traj refuses
    counts[7] = 0; counts[8] = 9   # invalid segment counts
    status = np.ones(16, dtype=np.int32); status[9] = -2; status[10] = 0; status[11] = 2
    sets = [sh, synth.shared_params(0, weights=tuple(np.array(synth.REFERENCE_WEIGHTS) * 2))]
    idx = np.zeros(16, dtype=np.int32); idx[12] = -1; idx[13] = 2; idx[14] = 1
    rec = record(solver, seg, counts, init)
    c = dev(solver, ctrl)
    st, si = dev(solver, status, torch.int32), dev(solver, idx, torch.int32)
    cost, npts = solver.traj_cost(rec, sets, c, s_ref, l_ref, status=st, set_index=si)
    g = solver.traj_cost_vjp(rec, sets, c, s_ref, l_ref, torch.ones(16, dtype=torch.float64, device=solver.device),
                             status=st, set_index=si)
    cost, npts = cost.cpu().numpy(), npts.cpu().numpy()
    bad = [5, 6, 7, 8, 9, 10, 12, 13]
    for b in range(16):
        if b in bad:
            assert np.isinf(cost[b]) and cost[b] > 0 and npts[b] == 0, b
            for k, v in g.items():
                assert (v[b] == 0).all(), (b, k)
        else:
            assert np.isfinite(cost[b]) and npts[b] > 0, b
    # without status every candidate with a valid count is scored
    cost2, _ = solver.traj_cost(rec, sets, c, s_ref, l_ref, set_index=si)
    assert np.isfinite(cost2.cpu().numpy()[[9, 10]]).all()
    # a reference line that is not finite gives NaN
    s_bad = s_ref.copy(); s_bad[0, 0] = np.nan
    cost3, _ = solver.traj_cost(rec, sh, c, s_bad, l_ref)
    assert np.isnan(cost3.cpu().numpy()[0])


def test_winner_by_a_cost(solver):
    batch, sh = BATCHES["config3"]()
    db, o = solved(solver, batch, sh)
    s_ref, l_ref = lines(batch, 8)
    cost, _ = solver.traj_cost(db, sh, o["ctrl"], s_ref, l_ref, status=o["status"])
    bi, bc = solver.argmin(cost)
    torch.cuda.synchronize()
    h = cost.cpu().numpy()
    assert int(bi[0]) == int(np.argmin(h)) and float(bc[0]) == h.min()


def _yardstick_grads(variant, sh, seg, counts, ctrl, init, s_ref, l_ref, abar, b):
    S = counts[b] if counts is not None else seg.shape[2]
    t = seg[L.F_T, b, :S]
    c = np.concatenate([ctrl[b, :6 * S], ctrl[b, 6 * S:12 * S]])
    r = ref_acost(variant, params_row(sh), t, sh.delta, c, init[b], s_ref[b], l_ref[b], grad=True)
    return S, r


def _max_moves(variant, sh, seg, counts, ctrl, init, b, key, step):
    """Whether the first index of max |dds| or max |ddl| of candidate b differs at the base point and the two points of a
    central difference (the max term is then within the step of a tie: its derivative is not defined there)."""
    if variant != 1 or key not in ("ctrl", "init"):
        return False
    S = counts[b]
    t = seg[L.F_T, b, :S]
    arg = []
    for sgn in (0, 1, -1):
        c = ctrl[b, :12 * S] + (sgn * step[b, :12 * S] if key == "ctrl" else 0)
        i0 = init[b] + (sgn * step[b] if key == "init" else 0)
        smp = samples(t, sh.delta, c, i0)
        arg.append((int(np.argmax(np.abs(smp[2]))), int(np.argmax(np.abs(smp[5])))))
    return len(set(arg)) > 1


@pytest.mark.parametrize("smax,variant,durations", [(20, 0, DURATIONS), (20, 1, DURATIONS), (100, 0, DURATIONS),
                                                    (12, 0, LONG_DURATIONS), (12, 1, LONG_DURATIONS)])
def test_vjp_matches_the_yardstick_and_central_differences(solver, smax, variant, durations):
    seg, counts, ctrl, init, s_ref, l_ref, sh = ragged_batch(48, smax, 40 + smax + variant, variant, durations)
    sh = synth.shared_params(variant)
    rec = record(solver, seg, counts, init)
    rng = np.random.default_rng(2)
    abar = rng.standard_normal(48)
    c = dev(solver, ctrl)
    g = {k: v.cpu().numpy() for k, v in solver.traj_cost_vjp(rec, sh, c, s_ref, l_ref, dev(solver, abar)).items()}
    cost0 = solver.traj_cost(rec, sh, c, s_ref, l_ref)[0].cpu().numpy()
    checked = 0
    for b in range(0, 48, 3):
        S, r = _yardstick_grads(variant, sh, seg, counts, ctrl, init, s_ref, l_ref, abar, b)
        if r is None:
            assert np.isinf(cost0[b])
            continue
        val, gr = r
        assert abs(cost0[b] - val) <= 1e-11 * abs(val)
        gc = np.concatenate([g["ctrl"][b, :6 * S], g["ctrl"][b, 6 * S:12 * S]])
        assert (g["ctrl"][b, 12 * S:] == 0).all()
        for key, got in (("ctrl", gc), ("init", g["init"][b]), ("params", g["params"][b]), ("s_ref", g["s_ref"][b]),
                         ("l_ref", g["l_ref"][b])):
            want = abar[b] * gr[key]
            assert np.abs(got - want).max() <= 1e-10 * max(np.linalg.norm(want), 1e-300), (b, key)
        checked += 1
    assert checked >= 8
    if durations is LONG_DURATIONS:
        S_of = [counts[b] for b in range(48)]
        assert any((seg[L.F_T, b, :S_of[b]] >= 13.0).any() and np.isfinite(cost0[b]) for b in range(0, 48, 3))
    # central differences of the device forward, along random directions
    for key in ("ctrl", "init", "s_ref", "l_ref"):
        base = dict(ctrl=ctrl, init=init, s_ref=s_ref, l_ref=l_ref)
        d = rng.standard_normal(base[key].shape)
        h = 1e-6 * np.abs(base[key]).max()
        vals = []
        for sgn in (1, -1):
            p = dict(base); p[key] = base[key] + sgn * h * d
            rr = record(solver, seg, counts, p["init"])
            vals.append(solver.traj_cost(rr, sh, dev(solver, p["ctrl"]), p["s_ref"], p["l_ref"])[0].cpu().numpy())
        fd = (vals[0] - vals[1]) / (2 * h)
        an = (g[key] * d).reshape(48, -1).sum(1)
        fin = np.isfinite(cost0)
        # skip cuboid candidates whose max is within the step of a tie (the arg-max moves inside the difference)
        ties = np.array([fin[b] and _max_moves(variant, sh, seg, counts, ctrl, init, b, key, h * d) for b in range(48)])
        fin &= ~ties
        assert fin.sum() >= 0.8 * np.isfinite(cost0).sum(), (key, ties.sum())
        assert np.allclose(fd[fin] * abar[fin], an[fin], rtol=1e-5, atol=1e-7 * np.abs(cost0[fin]).max()), key


# ---- through the solve -----------------------------------------------------------------------------------------------
def _strict(batch, sh, b):
    _, adj = reference_vjp(one(batch, b), sh, 0, np.zeros(12 * batch.S), 1.0)
    return adj.strict


@pytest.fixture(scope="module")
def through(solver):
    """32 scenario_1 candidates, each with its own set (per-candidate parameter gradients), solved and scored with the
    same weights: gradients of a_cost w.r.t. weights, ref_end, init and corridors through diff.solve + diff.traj_cost."""
    B, S = 32, 6
    batch, sh = synth.make_scenario1_batch(B, S, 0, seed=77)
    s_ref, l_ref = lines(batch, 11)
    rows = np.tile(params_row(sh), (B, 1))
    idx = dev(solver, np.arange(B), torch.int32)

    def run(seg, init, ref_end, rows_, grad=False):
        P = torch.tensor(rows_, dtype=torch.float64, device=solver.device, requires_grad=grad)
        sg = dev(solver, seg).requires_grad_(grad); it = dev(solver, init).requires_grad_(grad)
        re = dev(solver, ref_end).requires_grad_(grad)
        ctrl, cost, st = diff.solve(solver, sg, it, re, dev(solver, batch.dl_bounds), P, set_index=idx)
        a = diff.traj_cost(ctrl, sg, it, dev(solver, s_ref), dev(solver, l_ref), P, solver, set_index=idx, status=st)
        if grad:
            a.sum().backward()
            return a.detach().cpu().numpy(), st.cpu().numpy(), dict(P=P.grad.cpu().numpy(), seg=sg.grad.cpu().numpy(),
                                                                     init=it.grad.cpu().numpy(), ref_end=re.grad.cpu().numpy())
        return a.detach().cpu().numpy(), st.cpu().numpy()

    a0, st, g = run(batch.seg, batch.init, batch.ref_end, rows, grad=True)
    strict = np.array([st[b] == 1 and _strict(batch, sh, b) for b in range(B)])
    return types.SimpleNamespace(batch=batch, sh=sh, rows=rows, run=run, a0=a0, g=g, strict=strict)


def test_gradients_through_the_solve_match_central_differences(through):
    t = through
    batch = t.batch
    assert t.strict.sum() >= 8
    cases = [("P", j) for j in range(10)] + [("init", 1), ("init", 4), ("ref_end", 0), ("ref_end", 1),
                                               ("seg", L.F_X_BIAS), ("seg", L.F_UPP_BIAS), ("seg", L.F_L_DOWN_BIAS)]
    for key, j in cases:
        outs = []
        for sgn in (1, -1):
            seg, init, ref_end, rows = batch.seg.copy(), batch.init.copy(), batch.ref_end.copy(), t.rows.copy()
            if key == "P":
                h = 1e-5 * (1 + np.abs(rows[:, j])); rows[:, j] += sgn * h
            elif key == "seg":
                h = 1e-5 * (1 + np.abs(seg[j, :, 2])); seg[j, :, 2] += sgn * h
            else:
                arr = init if key == "init" else ref_end
                h = 1e-5 * (1 + np.abs(arr[:, j])); arr[:, j] += sgn * h
            outs.append(t.run(seg, init, ref_end, rows))
        ok = t.strict & (outs[0][1] == 1) & (outs[1][1] == 1)
        fd = (outs[0][0] - outs[1][0]) / (2 * h)
        an = t.g["P"][:, j] if key == "P" else (t.g["seg"][j, :, 2] if key == "seg" else t.g[key][:, j])
        # the bar of tests/test_gpu_vjp.py: 1e-3 of the candidate's gradient array
        arr = t.g["P"][:, :10] if key == "P" else (t.g["seg"][1:].transpose(1, 0, 2).reshape(len(fd), -1) if key == "seg" else t.g[key])
        scale = np.abs(arr).max(1)
        assert (np.abs(fd - an)[ok] <= 1e-3 * scale[ok]).all(), (key, j, np.max(np.abs(fd - an)[ok] / scale[ok]))


def test_euler_relation_of_the_homogeneous_objective(through):
    """a_cost of x*(w, ref_end) scored with the same w: homogeneous of degree 1 in (w, ref_end), so
    sum_i w_i da/dw_i + sum_j ref_end_j da/dref_end_j = a_cost (explicit part and the part through the solve together)."""
    t = through
    ok = t.strict
    lhs = (t.rows[:, :10] * t.g["P"][:, :10]).sum(1) + (t.batch.ref_end * t.g["ref_end"]).sum(1)
    rel = np.abs(lhs - t.a0)[ok] / np.abs(t.a0[ok])
    assert rel.max() <= 1e-4, rel.max()


# ---- descent on c1.txt -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_adam_descends_on_c1(solver, variant):
    from spectral_amd.tune import descend
    kb = knots.parse_corridor_file(os.path.join(GOLD, "inputs", "c1.txt"))
    r = descend(solver, kb, variant, W[:10], starts=16, steps=30, seed=5)
    assert r["final_mean"] < r["start_mean"], r


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals(solver):
    seg, counts, ctrl, init, s_ref, l_ref, sh = ragged_batch(4, 4, 3)
    ctx = solver.ctx
    d = lambda a, t=torch.float64: dev(solver, a, t)
    sg, ct, it, sr, lr = d(seg), d(ctrl), d(init), d(s_ref), d(l_ref)
    out = torch.empty(4, dtype=torch.float64, device=solver.device)
    N = s_ref.shape[1]
    base = dict(B=4, seg_stride=4, sets=[sh], set_index=None, seg=sg, seg_count=None, init=it, ctrl=ct, status=None, N=N,
                s_ref=sr, l_ref=lr, ref_stride=N)
    cases = [(dict(ctrl=None), "ctrl, seg, init, s_ref and l_ref"), (dict(seg=None), "ctrl, seg, init"),
             (dict(init=None), "ctrl, seg, init"), (dict(s_ref=None), "s_ref and l_ref"), (dict(l_ref=None), "s_ref and l_ref"),
             (dict(B=0), "B >= 1"), (dict(N=0), "N >= 1"), (dict(seg_stride=257), "BTRAPZ_MAX_SEGMENTS_LONG"),
             (dict(sets=[sh, synth.shared_params(1)]), "same variant and delta"),
             (dict(sets=[sh, synth.shared_params(0, delta=0.2)]), "same variant and delta"),
             (dict(ref_stride=N - 1), "ref_stride")]
    for over, msg in cases:
        kw = dict(base); kw.update(over)
        with pytest.raises(BtrapzError, match=msg.replace("(", r"\(")):
            ctx.traj_cost_device(**kw, a_cost=out)
        with pytest.raises(BtrapzError, match=msg):
            ctx.traj_cost_vjp_device(**kw, a_cost_bar=out)
    with pytest.raises(BtrapzError, match="a_cost_bar is null"):
        ctx.traj_cost_vjp_device(**base, a_cost_bar=None)
    with pytest.raises(BtrapzError, match="(-2)|EINVAL|invalid"):
        ctx.traj_cost_device(**base, a_cost=None)
