"""A parameter set per candidate (btrapz_solve_sets_device, BatchSolver.solve_sets / solve_sets_ragged): one launch over
a batch whose candidates name their weights, ds_ref / dl_ref and limits must give every candidate, bit for bit, what a
uniform solve with its own set gives it in the same form -- and that set must really reach the kernel."""
import dataclasses
import os

import numpy as np
import pytest

from helpers import O
from spectral_amd import knots, synth
from spectral_amd import layout as L
from spectral_amd.native import BtrapzError

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")
PIN = dict(cap_iter=-1, compact=-1)   # one launch, no pre-pass, on both sides


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def weight_rows(n):
    rows = []
    for line in open(os.path.join(GOLD, "all_weights.txt")):
        try:
            v = [float(t) for t in line.split()]
        except ValueError:
            continue
        if len(v) >= 10:
            rows.append(v[:10])
    assert len(rows) >= n
    return rows[:n]


def mixed_sets(n, variant=0):
    """n sets that differ in the weights (logged weight rows), ds_ref and the limits."""
    sets = []
    for g, w in enumerate(weight_rows(n)):
        sh = synth.shared_params(variant, weights=w)
        sets.append(dataclasses.replace(sh, ds_ref=5.0 + 0.5 * (g % 7), dds=(-2.0 - 0.1 * g, 2.0 + 0.1 * g),
                                        ddl=(-0.7 + 0.02 * (g % 5), 0.7 - 0.02 * (g % 5)),
                                        ddds=(-30.0 + g, 30.0 - g), dddl=(-10.0 - g, 10.0 + g)))
    return sets


def take(batch, idx):
    return L.Batch(B=len(idx), S=batch.S, seg=np.ascontiguousarray(batch.seg[:, idx]), init=np.ascontiguousarray(batch.init[idx]),
                   ref_end=np.ascontiguousarray(batch.ref_end[idx]), dl_bounds=np.ascontiguousarray(batch.dl_bounds[idx]))


def host(o):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in o.items()}


def assert_same(got, ref, idx):
    for k in ("ctrl", "cost", "status", "iters"):
        a, b = got[k][idx], ref[k]
        assert np.array_equal(a.view(np.uint8) if a.dtype == np.float64 else a, b.view(np.uint8) if b.dtype == np.float64 else b), k


def index_tensor(set_index, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(set_index, dtype=np.int32)).to(device)


@pytest.mark.parametrize("lean", [1, -1])
def test_mixed_sets_equal_separate_solves(solver, lean):
    B, G = 3072, 14
    batch, _ = synth.make_batch(B, 10, config=2)
    sets = mixed_sets(G)
    rng = np.random.default_rng(7)
    set_index = rng.permutation(np.arange(B) % G)
    o = host(solver.solve_sets(solver.upload(batch), sets, index_tensor(set_index, solver.device), lean=lean, **PIN))
    assert solver.ctx.last_solve_form() == (8 if lean > 0 else 0)
    assert (o["status"] > 0).mean() > 0.95
    for g in range(G):
        idx = np.nonzero(set_index == g)[0]
        ref = host(solver.solve(solver.upload(take(batch, idx)), sets[g], lean=lean, split=-1, **PIN))
        assert_same(o, ref, idx)
    # strided candidates against the oracle's optimum of their own set
    for b in range(0, B, 397):
        if o["status"][b] != 1:
            continue
        xs, _, st, _ = O.batch_solve(take(batch, [b]), sets[set_index[b]], 0, 1, exact=True)
        assert st[0] == 1
        assert np.abs(o["ctrl"][b] - xs[0]).max() <= 1e-5 * np.abs(xs[0]).max(), b


@pytest.mark.parametrize("lean", [1, -1])
def test_one_set_matches_the_uniform_entry_point(solver, lean):
    import torch
    batch, sh = synth.make_scenario1_batch(2048, 20)
    db = solver.upload(batch)
    o = host(solver.solve_sets(db, [sh], torch.zeros(batch.B, dtype=torch.int32, device=solver.device), lean=lean, **PIN))
    ref = host(solver.solve(db, sh, lean=lean, split=-1, **PIN))
    assert_same(o, ref, np.arange(batch.B))


@pytest.mark.parametrize("lean", [1, -1])
def test_ragged_sets_equal_separate_solves(solver, lean):
    import torch
    kb = knots.jittered(knots.parse_corridor_file(os.path.join(GOLD, "c_road_s1_3.txt")), 1024, seed=5)
    rec = solver.corridor_batch(kb, 0, seg_stride=16)
    G = 5
    sets = mixed_sets(G)
    set_index = np.random.default_rng(3).integers(0, G, size=rec["B"])
    o = host(solver.solve_sets_ragged(rec, sets, index_tensor(set_index, solver.device), lean=lean, **PIN))
    assert (o["status"] > 0).sum() > 0
    for g in range(G):
        idx = np.nonzero(set_index == g)[0]
        it = torch.from_numpy(idx).to(solver.device)
        sub = dict(B=len(idx), seg_stride=rec["seg_stride"], seg=rec["seg"][:, it].contiguous(),
                   seg_count=rec["seg_count"][it].contiguous(), init=rec["init"][it].contiguous(),
                   ref_end=rec["ref_end"][it].contiguous(), dl_bounds=rec["dl_bounds"][it].contiguous())
        ref = host(solver.solve_ragged(sub, sets[g], lean=lean, **PIN))
        assert_same(o, ref, idx)


def test_split_form_sets_equal_separate_solves(solver):
    """Few candidates: the split form (one candidate per wavefront) reads each candidate's set itself."""
    B, G = 96, 4
    batch, _ = synth.make_batch(B, 10, config=2)
    sets = mixed_sets(G)
    set_index = np.random.default_rng(11).integers(0, G, size=B)
    set_index[5] = -1
    o = host(solver.solve_sets(solver.upload(batch), sets, index_tensor(set_index, solver.device), split=1, **PIN))
    assert solver.ctx.last_solve_form() == 1
    assert o["status"][5] == -5 and np.isinf(o["cost"][5])
    for g in range(G):
        idx = np.nonzero(set_index == g)[0]
        ref = host(solver.solve(solver.upload(take(batch, idx)), sets[g], split=1, **PIN))
        assert_same(o, ref, idx)


def test_long_form_sets_equal_separate_solves(solver):
    """S = 100: the long form (one axis problem per workgroup) reads each candidate's set itself."""
    B, G = 24, 3
    batch, sh = synth.make_batch(B, 100, config=3)
    sets = [dataclasses.replace(sh, ds_ref=6.0 + g, dds=(-2.0 - 0.2 * g, 2.0 + 0.2 * g)) for g in range(G)]
    set_index = np.arange(B) % G
    set_index[7] = G
    o = host(solver.solve_sets(solver.upload(batch), sets, index_tensor(set_index, solver.device), **PIN))
    assert solver.ctx.last_solve_form() == 2
    assert o["status"][7] == -5 and np.isinf(o["cost"][7])
    assert (o["status"][set_index < G] > 0).mean() > 0.9
    for g in range(G):
        idx = np.nonzero(set_index == g)[0]
        ref = host(solver.solve(solver.upload(take(batch, idx)), sets[g], **PIN))
        assert_same(o, ref, idx)
    # (the long form's agreement with the optimum is tests/test_gpu_long.py's; the sets differ in ds_ref, so a kernel that
    #  read another candidate's set would not give the per-set solves' bits)


def test_ragged_batch_with_long_candidates(solver):
    """Slots for 160 segments: candidates of 70..120 segments (long form, one launch per count) beside candidates of
    30 and 64 (the bucketed kernel), three sets -- every candidate as in a ragged solve with its own set alone."""
    import torch
    B, G = 24, 3
    kb = synth.scenario1_knots(B, 100)
    rec = solver.corridor_batch(kb, 0, seg_stride=160)
    sh = synth.shared_params(0)
    h = kb.header
    sh.ds_ref, sh.dl_ref, sh.dds, sh.ddds, sh.ddl, sh.dddl = h["ds_ref"], h["dl_ref"], h["dds"], h["ddds"], h["ddl"], h["dddl"]
    sets = [dataclasses.replace(sh, ds_ref=sh.ds_ref + 0.5 * g) for g in range(G)]
    torch.cuda.synchronize()
    counts = rec["seg_count"].cpu().numpy().copy()
    cut = counts.copy()
    cut[0::4] = 30; cut[1::4] = 64; cut[2::4] = np.minimum(counts[2::4], 70)
    rec["seg_count"] = torch.from_numpy(cut.astype(np.int32)).to(solver.device)
    assert (cut > 64).any() and (cut <= 64).any()
    set_index = np.arange(B) % G
    o = host(solver.solve_sets_ragged(rec, sets, index_tensor(set_index, solver.device), lean=1, **PIN))
    assert solver.ctx.last_solve_form() & 16
    assert (o["status"] > 0).sum() >= B // 2 and (o["status"][cut > 64] != -5).all()
    for g in range(G):
        idx = np.nonzero(set_index == g)[0]
        it = torch.from_numpy(idx).to(solver.device)
        sub = dict(B=len(idx), seg_stride=rec["seg_stride"], seg=rec["seg"][:, it].contiguous(),
                   seg_count=rec["seg_count"][it].contiguous(), init=rec["init"][it].contiguous(),
                   ref_end=rec["ref_end"][it].contiguous(), dl_bounds=rec["dl_bounds"][it].contiguous())
        ref = host(solver.solve_ragged(sub, sets[g], lean=1, **PIN))
        assert_same(o, ref, idx)


@pytest.mark.parametrize("hint", [False, True])
def test_warm_config5_shape_per_agent_sets(solver, hint):
    """16 agents x 96 candidates, a ds_ref and limits per agent, three warm-started steps (x0 from eval_states,
    multipliers kept): every step equals the per-agent uniform solves, and so do the per-agent winners."""
    import torch
    AG, CAND, S = 16, 96, 20
    batch, sh0 = synth.make_batch(AG * CAND, S, config=5, agents=AG)
    sets = [dataclasses.replace(sh0, ds_ref=6.0 + 0.25 * a, dds=(-2.0 - 0.05 * a, 2.0 + 0.05 * a)) for a in range(AG)]
    set_index = np.repeat(np.arange(AG), CAND)
    si = index_tensor(set_index, solver.device)
    db = solver.upload(batch)
    times = torch.from_numpy(np.cumsum(batch.seg[L.F_T], axis=1))
    warm, refs_warm = None, [None] * AG
    for step in range(3):
        w = dict(warm) if warm else {}
        if hint and step > 0:
            w["hint"] = torch.from_numpy(prev_iters).to(solver.device)
        o_d = solver.solve_sets(db, sets, si, warm=w or None, keep_multipliers=True, lean=1, **PIN)
        o = host(o_d)
        bi, bc = solver.argmin(o_d["cost"], group=CAND)
        bi = bi.cpu().numpy()
        for a in range(AG):
            idx = np.arange(a * CAND, (a + 1) * CAND)
            sub = solver.upload(take(batch, idx))
            ref = host(solver.solve(sub, sets[a], warm=refs_warm[a], keep_multipliers=True, lean=1, **PIN))
            assert_same(o, ref, idx)
            assert np.array_equal(o["lam"][:, :, idx], ref["lam"])
            assert bi[a] == a * CAND + int(np.argmin(ref["cost"]))
        assert (o["status"] > 0).mean() > 0.95
        prev_iters = o["iters"].astype(np.int32)
        x0 = solver.eval_states(db, o_d["ctrl"], times)
        lam = o_d["lam"].clone()
        warm = dict(x0=x0, lam=lam)
        refs_warm = [dict(x0=x0[a * CAND:(a + 1) * CAND].contiguous(), lam=lam[:, :, a * CAND:(a + 1) * CAND].contiguous())
                     for a in range(AG)]


def test_the_set_reaches_the_kernel(solver):
    """Copies of the same candidates under two sets that differ only in ds_ref, and two that differ only in a lateral
    acceleration limit that binds: different control points, each its own set's optimum."""
    import torch
    batch, sh = synth.make_batch(64, 10, config=2)
    idx = np.array([2, 4, 2, 4])
    pair = take(batch, idx)
    for a_, b_ in ((dataclasses.replace(sh, ds_ref=7.0), dataclasses.replace(sh, ds_ref=9.0)),
                   (dataclasses.replace(sh, ddl=(-0.7, 0.7)), dataclasses.replace(sh, ddl=(-0.15, 0.15)))):
        set_index = torch.tensor([0, 0, 1, 1], dtype=torch.int32, device=solver.device)
        for lean in (1, -1):
            o = host(solver.solve_sets(solver.upload(pair), [a_, b_], set_index, lean=lean, **PIN))
            assert (o["status"] == 1).all()
            for j in range(2):
                assert np.abs(o["ctrl"][j] - o["ctrl"][j + 2]).max() > 1e-4
            for j, s_ in enumerate((a_, a_, b_, b_)):
                xs, _, st, _ = O.batch_solve(take(pair, [j]), s_, 0, 1, exact=True)
                assert st[0] == 1
                assert np.abs(o["ctrl"][j] - xs[0]).max() <= 1e-5 * np.abs(xs[0]).max(), (j, lean)


def test_refusals_and_padding(solver):
    import torch
    batch, sh = synth.make_batch(512, 10, config=2)
    db = solver.upload(batch)
    zeros = torch.zeros(batch.B, dtype=torch.int32, device=solver.device)
    bad = [dict(sets=[]), dict(sets=[sh] * 1025), dict(sets=[sh, dataclasses.replace(sh, variant=1)]),
           dict(elastic=1), dict(cap_iter=6), dict(compact=1)]
    for kw in bad:
        sets = kw.pop("sets", [sh])
        with pytest.raises(BtrapzError, match=r"\(-1\)"):
            solver.solve_sets(db, sets, zeros, **kw)
    sets = [sh, dataclasses.replace(sh, ds_ref=8.0)]
    si = np.arange(batch.B) % 2
    full = host(solver.solve_sets(db, sets, index_tensor(si, solver.device), lean=1, **PIN))
    pad = si.copy(); pad[[3, 100]] = -1; pad[[7, 511]] = 2
    o = host(solver.solve_sets(db, sets, index_tensor(pad, solver.device), lean=1, **PIN))
    out = np.array([3, 100, 7, 511])
    assert (o["status"][out] == -5).all()   # BTRAPZ_NO_CORRIDOR
    assert np.isinf(o["cost"][out]).all()
    keep = np.setdiff1d(np.arange(batch.B), out)
    assert_same(o, {k: v[keep] for k, v in full.items()}, keep)
