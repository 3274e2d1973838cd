"""One batch record and one marshalling path in the Python layer: the autograd layer spectral_amd.diff, BatchSolver's
methods called directly, and the two shapes of a batch (DeviceBatch, record dict) make the same launches on the same
inputs, so everything here is held to exact equality.  Shapes: the smallest where a layout mix-up would show -- 6
candidates of 4 segments; a ragged record of stride 8 with counts 3..8; two parameter sets, alternating."""
import numpy as np
import pytest
import torch

from spectral_amd import diff, layout as L, synth

pytestmark = pytest.mark.gpu

B, S, W = 6, 4, 8
COUNTS = [8, 3, 5, 6, 4, 7]      # one candidate with the full stride, one with 3
LAYOUTS = ["uniform-one", "ragged-one", "uniform-sets", "ragged-sets"]


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


@pytest.fixture(scope="module")
def world(solver):
    """Per layout: the input tensors, the parameter rows and sets, the direct BatchSolver solve (cloned: uniform solves
    share their output buffers) -- computed once."""
    d = solver.device
    dev = lambda a: torch.tensor(a, device=d)
    uni, sh = synth.make_scenario1_batch(B, S, 0, seed=11)
    wide, _ = synth.make_scenario1_batch(B, W, 0, seed=12)
    row = diff.params_from_shared(sh).copy()
    row2 = row.copy(); row2[:10] *= 1.1                               # the ten weights, 10 % up
    sets = [diff.shared_from_params(r, sh.variant, sh.delta) for r in (row, row2)]
    index = dev(np.arange(B, dtype=np.int32) % 2)
    cnt = dev(np.array(COUNTS, dtype=np.int32))
    out = {}
    for name in LAYOUTS:
        ragged, many = name.startswith("ragged"), name.endswith("sets")
        b = wide if ragged else uni
        seg, init, ref_end, dlb = dev(b.seg), dev(b.init), dev(b.ref_end), dev(b.dl_bounds)
        stride = W if ragged else S
        rec = dict(B=B, seg_stride=stride, seg=seg, seg_count=cnt if ragged else None, init=init, ref_end=ref_end, dl_bounds=dlb)
        db = None if ragged else solver.upload(b)
        if name == "uniform-one":
            o = solver.solve(db, sets[0], keep_multipliers=True)
        elif name == "ragged-one":
            o = dict(ctrl=torch.zeros((B, 12 * W), dtype=torch.float64, device=d), cost=torch.empty(B, dtype=torch.float64, device=d),
                     status=torch.empty(B, dtype=torch.int32, device=d), iters=torch.empty(B, dtype=torch.int32, device=d),
                     lam=torch.empty((2, 36, B, W), dtype=torch.float64, device=d))
            solver.ctx.solve_warm_device(B, W, sets[0], seg, cnt, init, ref_end, dlb, o["ctrl"], o["cost"], o["status"], o["iters"],
                                         lam_out=o["lam"], stream=torch.cuda.current_stream(d).cuda_stream)
        elif name == "uniform-sets":
            o = solver.solve_sets(db, sets, index, keep_multipliers=True)
        else:
            o = solver.solve_sets_ragged(rec, sets, index, keep_multipliers=True)
        torch.cuda.synchronize()
        out[name] = dict(tensors=(seg, init, ref_end, dlb), rec=rec, db=db, direct={k: v.clone() for k, v in o.items()},
                         params=dev(np.stack([row, row2]) if many else row), sets=sets if many else sets[0],
                         kw=dict(seg_count=cnt if ragged else None, set_index=index if many else None, variant=sh.variant,
                                 delta=sh.delta), stride=stride)
    assert all(((w["direct"]["status"] == 1) | (w["direct"]["status"] == 2)).any() for w in out.values())
    out["sh"] = sh
    return out


@pytest.mark.parametrize("name", LAYOUTS)
def test_diff_solve_is_the_direct_solve(solver, world, name):
    w = world[name]
    ctrl, cost, status = diff.solve(solver, *w["tensors"], w["params"], **w["kw"])
    kept = diff.solve_kept(solver, *w["tensors"], w["params"], **w["kw"])
    torch.cuda.synchronize()
    for k, got in (("ctrl", ctrl), ("cost", cost), ("status", status)):
        assert torch.equal(got, w["direct"][k]), k
        assert torch.equal(kept[k], w["direct"][k]), k
    assert torch.equal(kept["iters"], w["direct"]["iters"])
    if not name.startswith("ragged"):     # (a ragged solve leaves the slots beyond a candidate's count unwritten)
        assert torch.equal(kept["lam"], w["direct"]["lam"])


@pytest.mark.parametrize("name", LAYOUTS)
def test_backward_is_the_direct_vjp(solver, world, name):
    w = world[name]
    d = solver.device
    rng = np.random.default_rng(3)
    r = torch.tensor(rng.standard_normal((B, 12 * w["stride"])), device=d)
    r2 = torch.tensor(rng.standard_normal(B), device=d)
    leaves = [t.clone().requires_grad_(True) for t in w["tensors"]] + [w["params"].clone().requires_grad_(True)]
    ctrl, cost, status = diff.solve(solver, *leaves, **w["kw"])
    ok = (status == 1) | (status == 2)
    loss = (ctrl[ok] * r[ok]).sum() + (cost[ok] * r2[ok]).sum()
    loss.backward()
    ctrl_bar = torch.where(ok[:, None], r, torch.zeros_like(r))
    cost_bar = torch.where(ok, r2, torch.zeros_like(r2))
    g = solver.solve_vjp(w["rec"], w["sets"], w["direct"], ctrl_bar, cost_bar, set_index=w["kw"]["set_index"])
    torch.cuda.synchronize()
    for leaf, k in zip(leaves, ("seg", "init", "ref_end", "dl_bounds")):
        assert torch.equal(leaf.grad, g[k]), k
    if w["kw"]["set_index"] is None:
        want = g["shared"].sum(0)
    else:   # the rows of each set added in candidate order
        want = torch.zeros((2, 20), dtype=torch.float64, device=d)
        for b, k in enumerate(w["kw"]["set_index"].tolist()):
            want[k] += g["shared"][b]
    assert torch.equal(leaves[4].grad, want)
    assert leaves[4].grad.abs().max() > 0


def test_a_device_batch_and_its_record_dict_are_one_batch(solver, world):
    w, sh = world["uniform-one"], world["sh"]
    d = solver.device
    db, rec, o = w["db"], w["rec"], w["direct"]
    assert rec["seg_count"] is None and db.seg_count is None
    rng = np.random.default_rng(5)
    t = lambda *shape: torch.tensor(rng.standard_normal(shape), device=d)
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in set(a) | set(b))

    xbar, cbar = t(B, 12 * S), t(B)
    assert same(solver.solve_vjp(db, sh, o, xbar, cbar), solver.solve_vjp(rec, sh, o, xbar, cbar))

    tan = dict(shared=t(2, B, 20), init=t(2, B, 6), seg=t(2, L.NUM_SEG_FIELDS, B, S))
    assert same(solver.solve_jvp(db, sh, o, tan), solver.solve_jvp(rec, sh, o, tan))

    N = 10 * S + 1 - 3
    s_ref = torch.cumsum(torch.tensor(rng.random((B, N)) * 1.5, device=d), 1); l_ref = 0.3 * t(B, N)
    a, b = (solver.traj_cost(x, sh, o["ctrl"], s_ref, l_ref, status=o["status"]) for x in (db, rec))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[0]).any()

    sel = torch.tensor([4, 0, 4, 2], device=d)
    out, _ = solver.sample(db, o["ctrl"], sel, sh.delta)
    obar = t(*out.shape)
    assert same(solver.sample_vjp(db, sel, sh.delta, obar), solver.sample_vjp(rec, sel, sh.delta, obar))

    times = torch.tensor(rng.random((B, 5)) * S, device=d)
    sbar = t(B, 2, 5, 3)
    assert same(solver.eval_states_vjp(db, o["ctrl"], times, sbar), solver.eval_states_vjp(rec, o["ctrl"], times, sbar))
    torch.cuda.synchronize()
