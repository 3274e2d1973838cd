"""btrapz_solve_vjp_device (gradients of a batched solve) on the GPU: against the oracle yardstick
(tests/vjp_reference.py), against central differences of the GPU solve, uniform against ragged, sets against single
sets, the autograd layer spectral_amd.diff, weight fitting, refusals."""
import numpy as np
import pytest
import torch

from grad_edge_cases import _cand, _close, _solve_and_vjp
from spectral_amd import diff, layout as L, synth
from spectral_amd.native import BtrapzError
from vjp_reference import reference_vjp

pytestmark = pytest.mark.gpu

B = 256
FAMILIES = {
    "generic": lambda S, seed: synth.make_batch(B, S, config=3, variant=0, seed=seed),
    "scenario_1": lambda S, seed: synth.make_scenario1_batch(B, S, 0, seed=seed),
    "cuboid": lambda S, seed: synth.make_scenario1_batch(B, S, 1, seed=seed),
}
KEYS = ("seg", "init", "ref_end", "dl_bounds", "shared")
# primal-side gradients: unique even where the multipliers are not
PRIMAL_SEG = [L.F_X_SKEW, L.F_X_BIAS, L.F_Y_SKEW, L.F_Y_BIAS]
PRIMAL_SHARED = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def _copy(batch):
    return L.Batch(B=batch.B, S=batch.S, seg=batch.seg.copy(), init=batch.init.copy(), ref_end=batch.ref_end.copy(),
                   dl_bounds=batch.dl_bounds.copy())


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("S", [1, 2, 10, 20, 64])
def test_vjp_against_the_yardstick(solver, family, S):
    batch, sh = FAMILIES[family](S, 100 + S)
    rng = np.random.default_rng(S)
    xbar = torch.tensor(rng.standard_normal((B, 12 * S)), device=solver.device)
    cbar = torch.tensor(rng.standard_normal(B), device=solver.device)
    results = {}
    for lean in (1, -1):
        o, g = _solve_and_vjp(solver, batch, sh, xbar, cbar, lean=lean)
        st = o["status"].cpu().numpy()
        results[lean] = (st, g)
        bad = (st != 1) & (st != 2)
        for k in KEYS:   # status outside {1, 2}: exactly 0; field 0: exactly 0
            arr = g[k] if k != "seg" else np.moveaxis(g[k], 1, 0)
            assert (arr[bad] == 0).all(), k
        assert (g["seg"][L.F_T] == 0).all()
    st, g = results[-1]
    # the two forms solve to rounding: their gradients agree
    ok = (st == 1) | (st == 2)
    for k in KEYS:
        a, r = results[1][1][k], g[k]
        assert np.abs(a - r).max() <= 1e-5 * max(np.abs(r).max(), 1.0), k
    n_cmp = {1: 4, 2: 4, 10: 3, 20: 2, 64: 1}[S]
    compared = 0
    xb, cb = xbar.cpu().numpy(), cbar.cpu().numpy()
    for b in np.flatnonzero(st == 1)[:(3 * n_cmp if S < 64 else 1)]:
        ref, adj = reference_vjp(batch, sh, b, xb[b], cb[b])
        if not adj.strict:   # (a row at its bound with a vanishing multiplier: one-sided derivatives only)
            continue
        mine = _cand(g, b)
        # primal-side gradients: unique even where the multipliers are not
        for f in PRIMAL_SEG:
            assert _close(mine["seg"][f], ref["seg"][f]), (family, S, b, f)
        assert _close(mine["ref_end"], ref["ref_end"]), (family, S, b)
        assert _close(mine["shared"][PRIMAL_SHARED], ref["shared"][PRIMAL_SHARED]), (family, S, b)
        # every array on the entries where the gradient is unique (no two fields tie at a joint), tolerance relative
        # to the array's norm for the candidate
        um = adj.unique_mask()
        for k in KEYS:
            scale = max(np.abs(ref[k]).max(), 1e-300)
            err = np.abs(mine[k] - ref[k])[um[k]]
            bad_ = np.argwhere(um[k] & (np.abs(mine[k] - ref[k]) > 1e-4 * scale))
            assert bad_.size == 0, (family, S, b, k, [(tuple(i), mine[k][tuple(i)], ref[k][tuple(i)]) for i in bad_[:6]])
        compared += 1
        if compared >= n_cmp:
            break


def test_uniform_and_ragged_give_identical_gradients(solver):
    S, W = 10, 16
    batch, sh = synth.make_scenario1_batch(B, S, 0, seed=7)
    rng = np.random.default_rng(1)
    xbar = rng.standard_normal((B, 12 * S)); cbar = rng.standard_normal(B)
    d = solver.device
    o, g = _solve_and_vjp(solver, batch, sh, torch.tensor(xbar, device=d), torch.tensor(cbar, device=d), lean=-1)
    seg = np.zeros((L.NUM_SEG_FIELDS, B, W)); seg[:, :, :S] = batch.seg
    rec = dict(B=B, seg_stride=W, seg=torch.tensor(seg, device=d), seg_count=torch.full((B,), S, dtype=torch.int32, device=d),
               init=torch.tensor(batch.init, device=d), ref_end=torch.tensor(batch.ref_end, device=d),
               dl_bounds=torch.tensor(batch.dl_bounds, device=d))
    oc = dict(ctrl=torch.zeros((B, 12 * W), dtype=torch.float64, device=d), lam=torch.empty((2, 36, B, W), dtype=torch.float64, device=d),
              cost=o["cost"], status=o["status"])
    # the same solve's control points and multipliers, laid out for the wider stride
    c = o["ctrl"].view(B, 2, S, 6); cr = torch.zeros((B, 12 * W), dtype=torch.float64, device=d)
    cr[:, :12 * S] = c.reshape(B, 12 * S)   # (ctrl: the l axis starts at 6 x count)
    oc["ctrl"] = cr
    lam = torch.zeros((2, 36, B, W), dtype=torch.float64, device=d); lam[..., :S] = o["lam"]
    oc["lam"] = lam
    xr = np.zeros((B, 12 * W)); xr[:, :12 * S] = xbar
    gr = solver.solve_vjp(rec, sh, oc, torch.tensor(xr, device=d), torch.tensor(cbar, device=d))
    torch.cuda.synchronize()
    gr = {k: v.cpu().numpy() for k, v in gr.items()}
    assert np.array_equal(gr["seg"][:, :, :S], g["seg"]) and (gr["seg"][:, :, S:] == 0).all()
    for k in ("init", "ref_end", "dl_bounds", "shared"):
        assert np.array_equal(gr[k], g[k]), k


def test_sets_match_single_set_calls_bit_for_bit(solver):
    S = 20
    batch, sh = synth.make_batch(B, S, config=3, variant=0, seed=21)
    d = solver.device
    base = sh.as_array()
    sets = []
    for j in range(3):
        row = base[:20].copy(); row[:8] *= 1.0 + 0.2 * j
        sets.append(diff.shared_from_params(row, 0, sh.delta))
    idx = np.arange(B, dtype=np.int32) % 3
    idx[5] = 7   # out of range: not solved, zero gradient
    set_index = torch.tensor(idx, device=d)
    db = solver.upload(batch)
    rng = np.random.default_rng(3)
    xbar = torch.tensor(rng.standard_normal((B, 12 * S)), device=d); cbar = torch.tensor(rng.standard_normal(B), device=d)
    o = solver.solve_sets(db, sets, set_index, keep_multipliers=True, lean=-1)
    o = {k: v.clone() for k, v in o.items()}
    g = solver.solve_vjp(db, sets, o, xbar, cbar, set_index=set_index)
    g = {k: v.cpu().numpy() for k, v in g.items()}
    for j in range(3):
        one_idx = torch.zeros(B, dtype=torch.int32, device=d)
        gj = solver.solve_vjp(db, [sets[j]], o, xbar, cbar, set_index=one_idx)
        gj = {k: v.cpu().numpy() for k, v in gj.items()}
        sel = idx == j
        for k in ("init", "ref_end", "dl_bounds", "shared"):
            assert np.array_equal(g[k][sel], gj[k][sel]), (j, k)
        assert np.array_equal(g["seg"][:, sel], gj["seg"][:, sel]), j
    for k in ("init", "ref_end", "dl_bounds", "shared"):
        assert (g[k][5] == 0).all()
    assert (g["seg"][:, 5] == 0).all()


def test_autograd_layer_matches_the_c_call(solver):
    S = 10
    batch, sh = synth.make_scenario1_batch(64, S, 0, seed=31)
    d = solver.device
    t = lambda a: torch.tensor(a, device=d, requires_grad=True)
    seg, init, ref_end, dl = t(batch.seg), t(batch.init), t(batch.ref_end), t(batch.dl_bounds)
    params = torch.tensor(diff.params_from_shared(sh), device=d, requires_grad=True)
    ctrl, cost, status = diff.solve(solver, seg, init, ref_end, dl, params, variant=0, delta=sh.delta)
    w = torch.tensor(np.random.default_rng(2).standard_normal((64, 12 * S)), device=d)
    solved = ((status == 1) | (status == 2)).to(torch.float64)
    loss = ((w * ctrl).sum(1) * solved).sum() + (torch.nan_to_num(cost, posinf=0.0) * solved).sum()
    loss.backward()
    db = solver.upload(batch)
    o = solver.solve(db, sh, keep_multipliers=True)
    g = solver.solve_vjp(db, sh, o, w * solved[:, None], solved)
    assert torch.equal(seg.grad, g["seg"]) and torch.equal(init.grad, g["init"])
    assert torch.equal(ref_end.grad, g["ref_end"]) and torch.equal(dl.grad, g["dl_bounds"])
    assert torch.allclose(params.grad, g["shared"].sum(0), rtol=1e-12, atol=0)


FD_SEG = (L.F_X_BIAS, L.F_DOWN_BIAS, L.F_L_UPP_BIAS, L.F_DS_HI)


def test_gpu_finite_differences(solver):
    S = 20
    batch, sh = synth.make_scenario1_batch(64, S, 0, seed=41)
    d = solver.device
    rng = np.random.default_rng(4)
    xbar = rng.standard_normal((64, 12 * S)); cbar = rng.standard_normal(64)
    o, g = _solve_and_vjp(solver, batch, sh, torch.tensor(xbar, device=d), torch.tensor(cbar, device=d))
    st = o["status"].cpu().numpy()
    picked = []
    for b in np.flatnonzero(st == 1):
        ref, adj = reference_vjp(batch, sh, b, xbar[b], cbar[b])
        um = adj.unique_mask()
        if adj.strict and all(um["seg"][f, 7] for f in FD_SEG) and um["init"][1] and um["dl_bounds"][1]:
            picked.append(b)
        if len(picked) >= 8:
            break
    assert len(picked) >= 4

    def loss_of(bt, shp):
        oo = solver.solve(solver.upload(bt), shp)
        torch.cuda.synchronize()
        c = oo["ctrl"].cpu().numpy(); cs = oo["cost"].cpu().numpy()
        return np.array([xbar[b] @ c[b] + cbar[b] * cs[b] for b in picked])

    h = 1e-4
    k = 7
    checks = []
    for f in FD_SEG:
        p = _copy(batch); m = _copy(batch)
        hh = h * (1 + np.abs(batch.seg[f, :64, k]))
        p.seg[f, :, k] += hh; m.seg[f, :, k] -= hh
        checks.append(((loss_of(p, sh) - loss_of(m, sh)) / (2 * hh[picked]), g["seg"][f, picked, k]))
    for attr, i in (("init", 1), ("ref_end", 1), ("dl_bounds", 1)):
        p = _copy(batch); m = _copy(batch)
        hh = h * (1 + np.abs(getattr(batch, attr)[:64, i]))
        getattr(p, attr)[:, i] += hh; getattr(m, attr)[:, i] -= hh
        checks.append(((loss_of(p, sh) - loss_of(m, sh)) / (2 * hh[picked]), g[attr][picked, i]))
    arr = diff.params_from_shared(sh)
    for j in (0, 5, 10):
        hh = h * (1 + abs(arr[j]))
        ap, am = arr.copy(), arr.copy(); ap[j] += hh; am[j] -= hh
        fd = (loss_of(_copy(batch), diff.shared_from_params(ap, 0, sh.delta)) -
              loss_of(_copy(batch), diff.shared_from_params(am, 0, sh.delta))) / (2 * hh)
        checks.append((fd, g["shared"][picked, j]))
    # (tolerance relative to the field's gradients, with a floor of 1e-6 of the largest one checked: a field whose
    #  gradient is 0 sees the forward's round-off through the difference quotient)
    top = max(max(np.abs(an).max() for _, an in checks), 1e-12)
    for i, (fd, an) in enumerate(checks):
        scale = max(np.abs(an).max(), np.abs(fd).max(), 1e-3 * top)
        assert np.abs(fd - an).max() <= 1e-3 * scale, (i, fd, an)


def test_weight_fitting_with_adam(solver):
    S = 10
    batch, sh = synth.make_scenario1_batch(64, S, 0, seed=51)
    d = solver.device
    tt = lambda a: torch.tensor(a, device=d)
    seg, init, ref_end, dl = tt(batch.seg), tt(batch.init), tt(batch.ref_end), tt(batch.dl_bounds)
    p_ref = tt(diff.params_from_shared(sh))
    with torch.no_grad():
        target, _, st = diff.solve(solver, seg, init, ref_end, dl, p_ref, variant=0, delta=sh.delta)
    mask = ((st == 1) | (st == 2)).to(torch.float64)[:, None]
    fit = torch.zeros(10, dtype=torch.float64)   # log-factors of the ten weights
    fit[:10] = torch.tensor(np.random.default_rng(6).choice([-1.0, 1.0], 10) * np.log(1.3))
    fit = fit.to(d).requires_grad_(True)
    opt = torch.optim.Adam([fit], lr=0.05)

    def mse():
        prm = torch.cat([p_ref[:10] * torch.exp(fit), p_ref[10:]])
        ctrl, _, s2 = diff.solve(solver, seg, init, ref_end, dl, prm, variant=0, delta=sh.delta)
        m = mask * ((s2 == 1) | (s2 == 2)).to(torch.float64)[:, None]
        return (((ctrl - target) * m) ** 2).sum() / m.sum().clamp(min=1)

    first = float(mse().detach())
    for _ in range(50):
        opt.zero_grad()
        loss = mse()
        loss.backward()
        opt.step()
    last = float(mse().detach())
    assert last <= first / 10, (first, last)


def test_refusals(solver):
    d = solver.device
    batch, sh = synth.make_batch(8, 4, config=3, variant=0, seed=61)
    db = solver.upload(batch)
    o = solver.solve(db, sh, keep_multipliers=True)
    ctx = solver.ctx
    z = torch.zeros(8 * 12 * 65, dtype=torch.float64, device=d)
    with pytest.raises(BtrapzError, match="BTRAPZ_MAX_SEGMENTS"):
        ctx.solve_vjp_device(8, 65, [sh], None, z, None, db.init, db.ref_end, db.dl_bounds, z, z, o["status"], z, None)
    with pytest.raises(BtrapzError, match="lam"):
        ctx.solve_vjp_device(8, 4, [sh], None, db.seg, None, db.init, db.ref_end, db.dl_bounds, o["ctrl"], None,
                             o["status"], o["ctrl"], None)
    with pytest.raises(BtrapzError, match="both NULL"):
        ctx.solve_vjp_device(8, 4, [sh], None, db.seg, None, db.init, db.ref_end, db.dl_bounds, o["ctrl"], o["lam"],
                             o["status"], None, None)
    sh1 = synth.shared_params(1)
    with pytest.raises(BtrapzError, match="variant"):
        ctx.solve_vjp_device(8, 4, [sh, sh1], None, db.seg, None, db.init, db.ref_end, db.dl_bounds, o["ctrl"], o["lam"],
                             o["status"], o["ctrl"], None)
    # every refusal is BTRAPZ_EINVAL (-1)
    with pytest.raises(BtrapzError, match=r"\(-1\)"):
        ctx.solve_vjp_device(8, 4, [sh], None, db.seg, None, db.init, db.ref_end, db.dl_bounds, o["ctrl"], o["lam"],
                             o["status"], None, None)
