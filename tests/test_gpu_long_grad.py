"""Gradients and directional derivatives of solves with 65..256 segments (btrapz_solve_long_vjp_device / _jvp_device,
include/btrapz_hip_long_grad.h: long_vjp_kernel / long_jvp_kernel of btrapz_long_grad.hip -- one axis problem per workgroup of
up to four wavefronts) on the GPU, B = 5 everywhere.

Yardstick: tests/vjp_reference.py and tests/jvp_reference.py (the oracle's dense exact solve, the adjoint / tangent KKT system by
least squares), live at 65 segments and from tests/golden/long_grad_yardstick.npz at 129 and 256.  Bound: 1e-4 of each array's
norm on the entries where the gradient is unique -- the project's bound for both derivative kernels.  Every seam of the lane
mapping (65, 127, 128, 129, 192, 193, 255, 256): the adjoint identity between the two kernels (1e-4 of sum |terms|), central
differences of the GPU's own solve (1e-3), independence of the batch size, a status that says "not solved".  A ragged record
of stride 256 against the uniform calls; parameter sets; delegation up to 64 slots; refusals; the autograd layer.

Worst ratios, one run on an MI355X: see DESIGN.md 3.16."""
import os

import numpy as np
import pytest
import torch

from grad_edge_cases import SHAPES, _cand, _dev, _directions, _ragged
from jvp_reference import KEYS, Tangent, random_direction
from spectral_amd import diff, layout as L, synth
from spectral_amd.native import MAX_TANGENTS, BtrapzError
from vjp_reference import Adjoint, one

pytestmark = pytest.mark.gpu
TOL = 1e-4
B = 5
CBAR = 0.7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_grad_yardstick.npz")
GOLDEN_CASES = [("generic", 129, 0), ("generic", 129, 1), ("scenario1", 129, 0), ("generic", 256, 0)]   # make_long_grad_goldens.CASES
LIVE_CASES = [("generic", 65, 0), ("generic", 65, 1), ("scenario1", 65, 1), ("cuboid", 65, 1)]
SEAMS = [("generic", S) for S in (65, 127, 128, 129, 192, 193, 255, 256)] + [("scenario1", 128)]


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


_problems, _solves, _yard = {}, {}, {}


def problem(gen, S):
    if (gen, S) not in _problems:
        _problems[(gen, S)] = (synth.make_scenario1_batch(B, S, 0) if gen == "scenario1" else
                               synth.make_batch(B, S, config=3, variant=1) if gen == "cuboid" else synth.make_batch(B, S, config=3))
    return _problems[(gen, S)]


def solved(solver, gen, S):
    """(device batch, result dict with the multipliers kept, status as numpy) of the cold long solve, once per shape."""
    if (gen, S) not in _solves:
        batch, sh = problem(gen, S)
        db = solver.upload(batch)
        o = {k: v.clone() for k, v in solver.solve_long(db, sh, keep_multipliers=True).items()}
        torch.cuda.synchronize()
        _solves[(gen, S)] = (db, o, o["status"].cpu().numpy().copy())
    return _solves[(gen, S)]


def is_solved(st):
    return (st == 1) | (st == 2)


def npy(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------

def live_yardstick(gen, S, b):
    """The yardstick of one candidate at 65 segments, computed once: cotangent, gradients, masks, two directions and tangents."""
    if (gen, S, b) not in _yard:
        batch, sh = problem(gen, S)
        rng = np.random.default_rng(7000 + 10 * S + b)
        xbar = rng.standard_normal(12 * S)
        bt = one(batch, b)
        adj = Adjoint(bt, sh, xbar, CBAR)
        g = adj.grads()
        assert adj.status in (1, 2) and adj.strict, (gen, S, b, adj.status, adj.strict)
        um = adj.unique_mask()
        dirs, dx, dcost, dscale = [], [], [], []
        for t in range(2):
            dr = random_direction(rng, S)
            for k in KEYS:
                dr[k] = dr[k] * um[k]
            tg = Tangent(bt, sh, dr, adj=adj)
            dirs.append(dr); dx.append(tg.dx); dcost.append(tg.dcost); dscale.append(tg.dcost_scale)
        _yard[(gen, S, b)] = dict(xbar=xbar, g=g, um=um, dirs=dirs, dx=dx, dcost=dcost, dscale=dscale, unique=adj.unique)
    return _yard[(gen, S, b)]


def golden_yardstick(i):
    z = np.load(GOLDEN)
    p = "c%d_" % i
    return dict(xbar=z[p + "xbar"], g={k: z[p + "g_" + k] for k in KEYS}, um={k: z[p + "um_" + k] for k in KEYS},
                dirs=[{k: z[p + "d%d_%s" % (t, k)] for k in KEYS} for t in range(2)], dx=[z[p + "dx%d" % t] for t in range(2)],
                dcost=[float(z[p + "dcost%d" % t]) for t in range(2)], dscale=[float(z[p + "dcost_scale%d" % t]) for t in range(2)])


def vjp_ratios(mine, y):
    """Per array: the largest error on the unique entries over the yardstick's largest entry."""
    return {k: float(np.abs(mine[k] - y["g"][k])[y["um"][k]].max(initial=0.0) / max(np.abs(y["g"][k]).max(), 1e-300)) for k in KEYS}


def against_yardstick(solver, gen, S, b, y, o, what):
    """Both kernels on the whole batch; candidate b held to its yardstick y.  Returns the worst ratio."""
    batch, sh = problem(gen, S)
    db, _, st = solved(solver, gen, S)
    assert st[b] in (1, 2), (what, gen, S, b, st)
    d = solver.device
    rng = np.random.default_rng(S + b)
    xbar = rng.standard_normal((B, 12 * S)); xbar[b] = y["xbar"]
    g = npy(solver.solve_long_vjp(db, sh, o, torch.tensor(xbar, device=d), torch.full((B,), CBAR, dtype=torch.float64, device=d)))
    r = vjp_ratios(_cand(g, b), y)
    print("%s %s S=%d b=%d vjp: %s" % (what, gen, S, b, {k: "%.2e" % v for k, v in r.items()}))
    assert max(r.values()) <= TOL, (what, gen, S, b, r)
    assert (g["seg"][L.F_T] == 0).all()
    # power: the next candidate's gradient, for the same cotangent, is no match for this yardstick
    nb = (b + 1) % B
    if st[nb] in (1, 2):
        xo = xbar.copy(); xo[nb] = y["xbar"]
        go = npy(solver.solve_long_vjp(db, sh, o, torch.tensor(xo, device=d), torch.full((B,), CBAR, dtype=torch.float64, device=d)))
        ro = vjp_ratios(_cand(go, nb), y)
        assert max(ro.values()) > TOL, (what, gen, S, b, ro)
    T = 2
    tan = _directions(rng, T, B, S)
    for t in range(T):
        tan["seg"][t, :, b, :] = y["dirs"][t]["seg"]
        for k in ("init", "ref_end", "dl_bounds", "shared"):
            tan[k][t, b] = y["dirs"][t][k]
    tan["seg"][0, :, nb, :] = y["dirs"][0]["seg"]          # (power: the next candidate along the same direction)
    for k in ("init", "ref_end", "dl_bounds", "shared"):
        tan[k][0, nb] = y["dirs"][0][k]
    j = npy(solver.solve_long_jvp(db, sh, o, _dev(solver, tan)))
    worst = max(r.values())
    for t in range(T):
        ex = np.abs(j["ctrl"][t, b] - y["dx"][t]).max() / np.abs(y["dx"][t]).max()
        ec = abs(j["cost"][t, b] - y["dcost"][t]) / y["dscale"][t]
        print("%s %s S=%d b=%d jvp tangent %d: ctrl_dot %.2e cost_dot %.2e" % (what, gen, S, b, t, ex, ec))
        assert ex <= TOL and ec <= TOL, (what, gen, S, b, t, ex, ec)
        worst = max(worst, ex, ec)
    if st[nb] in (1, 2):
        exo = np.abs(j["ctrl"][0, nb] - y["dx"][0]).max() / np.abs(y["dx"][0]).max()
        assert exo > TOL, (what, gen, S, b, exo)
    return worst


@pytest.mark.parametrize("gen,S,b", LIVE_CASES)
def test_live_yardstick_at_65_segments(solver, gen, S, b):
    _, o, _ = solved(solver, gen, S)
    against_yardstick(solver, gen, S, b, live_yardstick(gen, S, b), o, "live")


@pytest.mark.parametrize("i", range(len(GOLDEN_CASES)))
def test_golden_yardstick_at_129_and_256_segments(solver, i):
    gen, S, b = GOLDEN_CASES[i]
    _, o, _ = solved(solver, gen, S)
    against_yardstick(solver, gen, S, b, golden_yardstick(i), o, "golden")


# ---- 2. multipliers that are no numbers ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("gen,S,b", LIVE_CASES)
def test_nan_multipliers_classify_by_the_slack(solver, gen, S, b):
    """Every kept multiplier of the candidate overwritten with NaN: the rows are classified by their slack alone
    (VJP_SLACK_ACTIVE's rule), and the same bound holds."""
    _, o, _ = solved(solver, gen, S)
    o2 = dict(o); o2["lam"] = o["lam"].clone()
    o2["lam"][:, :, b, :] = float("nan")
    against_yardstick(solver, gen, S, b, live_yardstick(gen, S, b), o2, "NaN multipliers")


# ---- 3. every seam --------------------------------------------------------------------------------------------------------------

def both(solver, db, sh, o, xbar, cbar, tan, set_index=None, sets=None):
    d = solver.device
    g = solver.solve_long_vjp(db, sets or sh, o, torch.tensor(xbar, device=d), torch.tensor(cbar, device=d), set_index=set_index)
    j = solver.solve_long_jvp(db, sets or sh, o, _dev(solver, tan), set_index=set_index)
    return npy(g), npy(j)


def seam_case(solver, gen, S):
    batch, sh = problem(gen, S)
    db, o, st = solved(solver, gen, S)
    assert is_solved(st).sum() >= 4, (gen, S, st)
    rng = np.random.default_rng(100 + S)
    xbar = rng.standard_normal((B, 12 * S)); cbar = rng.standard_normal(B)
    tan = _directions(rng, 3, B, S)
    return batch, sh, db, o, st, xbar, cbar, tan


@pytest.mark.parametrize("gen,S", SEAMS)
def test_adjoint_identity_between_the_two_kernels(solver, gen, S):
    """<ctrl_bar, ctrl_dot> + <cost_bar, cost_dot> = <grad, direction> per solved candidate and tangent, within 1e-4 of
    sum |ctrl_bar| |ctrl_dot| + |cost_bar| |cost_dot| (_identity's normalisation in tests/grad_edge_cases.py)."""
    batch, sh, db, o, st, xbar, cbar, tan = seam_case(solver, gen, S)
    g, j = both(solver, db, sh, o, xbar, cbar, tan)
    ok = is_solved(st)
    worst = 0.0
    for t in range(3):
        lhs = (xbar * j["ctrl"][t]).sum(1) + cbar * j["cost"][t]
        mag = (np.abs(xbar) * np.abs(j["ctrl"][t])).sum(1) + np.abs(cbar) * np.abs(j["cost"][t])
        rhs = (np.moveaxis(g["seg"], 1, 0) * np.moveaxis(tan["seg"][t], 1, 0)).sum((1, 2))
        for k in ("init", "ref_end", "dl_bounds", "shared"):
            rhs = rhs + (g[k] * tan[k][t]).sum(1)
        assert (mag[ok] > 0).all()
        worst = max(worst, float((np.abs(lhs - rhs)[ok] / mag[ok]).max()))
    print("adjoint identity %s S=%d: worst %.3e" % (gen, S, worst))
    assert worst <= TOL, (gen, S, worst)
    bad = ~ok
    assert (j["ctrl"][:, bad] == 0).all() and (j["cost"][:, bad] == 0).all() and (g["seg"][:, bad] == 0).all() and (g["shared"][bad] == 0).all()


FD_H = 1e-3
FD_EPS = 1e-12
FD_SEG = (L.F_X_SKEW, L.F_X_BIAS, L.F_Y_SKEW, L.F_Y_BIAS)


@pytest.mark.parametrize("gen,S", SEAMS)
def test_central_differences_of_the_gpu_solve(solver, gen, S):
    """<g, d> and ctrl_dot against (f(theta + h d) - f(theta - h d)) / 2h of the GPU's own solve_long, within 1e-3, on the
    candidates that are solved and strictly complementary (by the oracle: `strict_*` of tests/golden/long_grad_yardstick.npz; a
    row at its bound with a vanishing multiplier has one-sided derivatives only, as in tests/test_gpu_vjp.py) and have no
    weakly active row (`weak_*`: an active row whose multiplier is at most 1e-4 of the candidate's largest -- see below).

    d: standard normal in the reference line's fields (x / y skew and bias) and ref_end -- inputs q is LINEAR in, so that on a
    fixed active set x is affine and the cost quadratic in the step: the central difference has no truncation error at any h,
    and h only has to stay below the slack of the inactive rows and above the forward's own round-off.  (The initial state is
    left out: scenario_1 starts ON a row of segment 0, and a millimetre outside it there is no solve to difference.)  Measured
    with h = 1e-4 and the default target (KKT score 1e-9): <g, d> missed 1e-3 by up to 1.6 at 192 .. 255 segments, on another
    candidate from run to run -- the forward's noise, which grows with the horizon; h = 1e-3, a millimetre on the reference line,
    cuts it tenfold at no cost.  Two candidates' ctrl_dot missed at either h, by the same amount in every run: generic 192,
    candidate 2 (2.8e-3 with the default target, 1.6e-4 with the solves run to their round-off floor) and generic 193, candidate
    0 (1.3e-3 with either).  The oracle finds one weakly active row in each: multipliers 1.8e-2 of 1 161 and 3.0e-3 of 456, the
    next smallest 0.84 and 1.36.  An interior-point iterate keeps a row of multiplier lambda at the slack mu / lambda (5e-4 in the
    oracle's own solution of the second), so such a row still gives way under a finite step, by about |P| mu / lambda^2 of the
    response, while the kernels differentiate the optimum, where it does not: the difference quotient of the solve is no
    measurement of the derivative there (the yardstick is: 3e-5 at 256 segments), and these candidates are left out.  The three
    solves of the difference run to the floor (eps = 1e-12: a solve whose best score is below 1e-7 is reported as solved whatever
    the target), which takes the same effect out of the rows above the band; the derivatives are those of the default solve.
    That no active set changed is checked: x(+h) + x(-h) - 2 x(0) vanishes on a fixed active set, and the solves keep their status."""
    batch, sh, db, o, st, xbar, cbar, _ = seam_case(solver, gen, S)
    strict = np.load(GOLDEN)["strict_%s_%d" % (gen, S)] & ~np.load(GOLDEN)["weak_%s_%d" % (gen, S)]
    rng = np.random.default_rng(200 + S)
    dr = {k: np.zeros(SHAPES(1, B, S)[k]) for k in KEYS}
    for f in FD_SEG:
        dr["seg"][0, f] = rng.standard_normal((B, S))
    dr["ref_end"][0] = rng.standard_normal((B, 2))
    g, j = both(solver, db, sh, o, xbar, cbar, dr)
    an = (np.moveaxis(g["seg"], 1, 0) * np.moveaxis(dr["seg"][0], 1, 0)).sum((1, 2)) + (g["ref_end"] * dr["ref_end"][0]).sum(1)
    res = {}
    for sign in (1, -1, 0):
        bt = L.Batch(B=B, S=S, seg=batch.seg + sign * FD_H * dr["seg"][0], init=batch.init.copy(),
                     ref_end=batch.ref_end + sign * FD_H * dr["ref_end"][0], dl_bounds=batch.dl_bounds.copy())
        res[sign] = npy(solver.solve_long(solver.upload(bt), sh, eps=FD_EPS))
        assert np.array_equal(is_solved(res[sign]["status"]), is_solved(st)), (gen, S, sign, res[sign]["status"], st)
    ok = is_solved(st) & strict
    assert ok.sum() >= 2, (gen, S, st, strict)
    base, cost0 = res[0]["ctrl"], res[0]["cost"]
    fd_ctrl = (res[1]["ctrl"] - res[-1]["ctrl"]) / (2 * FD_H)
    second = np.abs(res[1]["ctrl"] + res[-1]["ctrl"] - 2 * base).max(1)
    moved = np.abs(res[1]["ctrl"] - res[-1]["ctrl"]).max(1)
    loss = lambda r: (xbar * r["ctrl"]).sum(1) + cbar * r["cost"]
    fd = (loss(res[1]) - loss(res[-1])) / (2 * FD_H)
    top = np.abs(an[ok]).max()
    scale = np.maximum(np.maximum(np.abs(an), np.abs(fd)), 1e-3 * top)
    e_dir = np.abs(fd - an) / scale
    e_ctrl = np.abs(fd_ctrl - j["ctrl"][0]).max(1) / np.abs(j["ctrl"][0]).max(1).clip(1e-300)
    fd_cost = (res[1]["cost"] - res[-1]["cost"]) / (2 * FD_H)
    e_cost = np.abs(fd_cost - j["cost"][0]) / np.maximum(np.abs(fd_cost), 1e-6 * np.abs(cost0)).clip(1e-300)
    fm = lambda v: "[" + " ".join("%.1e" % x for x in v) + "]"
    print("central differences %s S=%d: compared %s; <g, d> %s ctrl_dot %s cost_dot %s; second difference / moved %s" %
          (gen, S, ok.astype(int), fm(e_dir), fm(e_ctrl), fm(e_cost), fm(second / moved.clip(1e-300))))
    print("central differences %s S=%d worst: <g, d> %.2e ctrl_dot %.2e" % (gen, S, e_dir[ok].max(), e_ctrl[ok].max()))
    assert (second[ok] <= 1e-3 * moved[ok]).all(), ("an active set changed", gen, S, second, moved)
    assert e_dir[ok].max() <= 1e-3 and e_ctrl[ok].max() <= 1e-3, (gen, S, e_dir, e_ctrl)


@pytest.mark.parametrize("gen,S", SEAMS)
def test_a_candidates_rows_do_not_depend_on_the_batch_around_it(solver, gen, S):
    """B = 4 (the first four candidates, with their own solve results) against B = 5: another B * seg_stride between rows of seg,
    lam and the tangents.  Every output row equal as numbers.  And a status that says "not solved": zeros there, nothing else moves."""
    batch, sh, db, o, st, xbar, cbar, tan = seam_case(solver, gen, S)
    g5, j5 = both(solver, db, sh, o, xbar, cbar, tan)
    sm = batch.slice(0, 4)
    sm = L.Batch(B=4, S=S, seg=sm.seg.copy(), init=sm.init.copy(), ref_end=sm.ref_end.copy(), dl_bounds=sm.dl_bounds.copy())
    o4 = dict(ctrl=o["ctrl"][:4].contiguous(), lam=o["lam"][:, :, :4].contiguous(), status=o["status"][:4].contiguous())
    t4 = {k: np.ascontiguousarray(v[:, :, :4] if k == "seg" else v[:, :4]) for k, v in tan.items()}
    g4, j4 = both(solver, solver.upload(sm), sh, o4, xbar[:4].copy(), cbar[:4].copy(), t4)
    assert np.array_equal(g5["seg"][:, :4], g4["seg"]), (gen, S)
    for k in ("init", "ref_end", "dl_bounds", "shared"):
        assert np.array_equal(g5[k][:4], g4[k]), (gen, S, k)
    assert np.array_equal(j5["ctrl"][:, :4], j4["ctrl"]) and np.array_equal(j5["cost"][:, :4], j4["cost"]), (gen, S)
    assert np.abs(g4["seg"]).max() > 0 and np.abs(j4["ctrl"]).max() > 0
    # one status set to -3
    v = int(np.flatnonzero(is_solved(st))[1])
    o3 = dict(o); o3["status"] = o["status"].clone(); o3["status"][v] = -3
    g3, j3 = both(solver, db, sh, o3, xbar, cbar, tan)
    keep = np.arange(B) != v
    assert (g3["seg"][:, v] == 0).all() and (j3["ctrl"][:, v] == 0).all() and (j3["cost"][:, v] == 0).all()
    assert np.array_equal(g3["seg"][:, keep], g5["seg"][:, keep])
    for k in ("init", "ref_end", "dl_bounds", "shared"):
        assert (g3[k][v] == 0).all() and np.array_equal(g3[k][keep], g5[k][keep]), (gen, S, k)
    assert np.array_equal(j3["ctrl"][:, keep], j5["ctrl"][:, keep]) and np.array_equal(j3["cost"][:, keep], j5["cost"][:, keep])


# ---- 4. a ragged record -----------------------------------------------------------------------------------------------------------

COUNTS = (3, 64, 65, 128, 129, 200, 256, 0, 257)
STRIDE = 256


def test_ragged_record_against_the_uniform_calls(solver):
    """Stride 256, counts 3 .. 256 and two that are no counts.  n > 64: both kernels' rows equal the uniform call at seg_stride = n
    (the same ctrl, lam, status) as numbers.  n <= 64: the EXISTING solve_vjp / solve_jvp at seg_stride = n, within 1e-7 of each
    array's norm -- the kernels differ by rounding only (the order of the per-candidate sums), the penalised system amplifies a
    rounding by rho / |P| = 1e6: 1e-16 x 1e6 x 64 sweep steps = 1e-8, times ten.  Slots beyond a count and the bad counts: exact
    zeros.  NaN in every input slot beyond a count changes no number."""
    d = solver.device
    T = 2
    nB = len(COUNTS)
    src = [problem("generic", n if 1 <= n <= STRIDE else 65) for n in COUNTS]
    sh = src[0][1]
    seg = np.zeros((L.NUM_SEG_FIELDS, nB, STRIDE)); init = np.zeros((nB, 6)); ref_end = np.zeros((nB, 2)); dlb = np.zeros((nB, 10))
    rng = np.random.default_rng(9)
    xbar = np.zeros((nB, 12 * STRIDE)); cbar = rng.standard_normal(nB)
    tan = _directions(rng, T, nB, STRIDE)
    for i, n in enumerate(COUNTS):
        pb = src[i][0]
        seg[:, i, :pb.S] = pb.seg[:, 0]; init[i], ref_end[i], dlb[i] = pb.init[0], pb.ref_end[0], pb.dl_bounds[0]
        xbar[i, :12 * pb.S] = rng.standard_normal(12 * pb.S)
    t = lambda a, **kw: torch.tensor(a, device=d, **kw)
    rec = dict(B=nB, seg_stride=STRIDE, seg=t(seg), seg_count=t(np.array(COUNTS), dtype=torch.int32), init=t(init), ref_end=t(ref_end),
               dl_bounds=t(dlb))
    o = {k: v.clone() for k, v in solver.solve_long(rec, sh, keep_multipliers=True).items()}
    torch.cuda.synchronize()
    st = o["status"].cpu().numpy()
    good = np.array([1 <= n <= STRIDE for n in COUNTS])
    assert is_solved(st[good]).all() and not is_solved(st[~good]).any(), st
    forced = dict(o); forced["status"] = torch.ones_like(o["status"])     # (even if the status claimed a solve of the bad counts)
    g, j = both(solver, rec, sh, forced, xbar, cbar, tan)
    worst = 0.0
    for i, n in enumerate(COUNTS):
        if not good[i]:
            assert (g["seg"][:, i] == 0).all() and (j["ctrl"][:, i] == 0).all() and (j["cost"][:, i] == 0).all(), n
            for k in ("init", "ref_end", "dl_bounds", "shared"):
                assert (g[k][i] == 0).all(), (n, k)
            continue
        assert (g["seg"][:, i, n:] == 0).all() and (j["ctrl"][:, i, 12 * n:] == 0).all(), n
        pb = src[i][0]
        bt = one(pb, 0)
        ou = dict(ctrl=o["ctrl"][i:i + 1, :12 * n].contiguous(), lam=o["lam"][:, :, i:i + 1, :n].contiguous(), status=o["status"][i:i + 1].contiguous())
        tu = {k: np.ascontiguousarray(v[:, :, i:i + 1, :n] if k == "seg" else v[:, i:i + 1]) for k, v in tan.items()}
        dbu = solver.upload(bt)
        xu, cu = t(xbar[i:i + 1, :12 * n].copy()), t(cbar[i:i + 1].copy())
        if n > 64:
            gu, ju = npy(solver.solve_long_vjp(dbu, sh, ou, xu, cu)), npy(solver.solve_long_jvp(dbu, sh, ou, _dev(solver, tu)))
        else:
            gu, ju = npy(solver.solve_vjp(dbu, sh, ou, xu, cu)), npy(solver.solve_jvp(dbu, sh, ou, _dev(solver, tu)))
        pairs = [(g["seg"][:, i, :n], gu["seg"][:, 0])] + [(g[k][i], gu[k][0]) for k in ("init", "ref_end", "dl_bounds", "shared")] + \
            [(j["ctrl"][:, i, :12 * n], ju["ctrl"][:, 0]), (j["cost"][:, i], ju["cost"][:, 0])]
        assert np.abs(gu["seg"]).max() > 0 and np.abs(ju["ctrl"]).max() > 0, n
        for a, r in pairs:
            if n > 64:
                assert np.array_equal(a, r), n
            else:
                err = np.abs(a - r).max() / max(np.abs(r).max(), 1e-300)
                worst = max(worst, err)
                assert err <= 1e-7, (n, err)
    print("ragged, counts <= 64 against the 64-segment kernels: worst %.3e of an array's norm" % worst)
    # NaN in every input slot beyond a count
    cnt = np.array([n if 0 <= n <= STRIDE else 0 for n in COUNTS])
    beyond = np.arange(STRIDE)[None, :] >= cnt[:, None]                                   # [B, stride]
    segn = seg.copy(); segn[:, beyond] = np.nan
    lamn = o["lam"].cpu().numpy().copy(); lamn[:, :, beyond] = np.nan
    beyond12 = np.arange(12 * STRIDE)[None, :] >= 12 * cnt[:, None]
    ctrln = o["ctrl"].cpu().numpy().copy(); ctrln[beyond12] = np.nan
    xn = xbar.copy(); xn[beyond12] = np.nan
    tann = {k: v.copy() for k, v in tan.items()}; tann["seg"][:, :, beyond] = np.nan
    recn = dict(rec); recn["seg"] = t(segn)
    on = dict(ctrl=t(ctrln), lam=t(lamn), status=forced["status"])
    gn, jn = both(solver, recn, sh, on, xn, cbar, tann)
    for k in g:
        assert np.array_equal(g[k], gn[k]), k
    for k in j:
        assert np.array_equal(j[k], jn[k]), k


# ---- 5. parameter sets --------------------------------------------------------------------------------------------------------------

def test_sets_match_single_set_calls(solver):
    S = 65
    batch, sh = problem("generic", S)
    d = solver.device
    row = sh.as_array()[:20].copy(); row[:8] *= 1.2
    sets = [sh, diff.shared_from_params(row, sh.variant, sh.delta)]
    idx = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    set_index = torch.tensor(idx, device=d)
    db = solver.upload(batch)
    outs = [{k: v.clone() for k, v in solver.solve_long(db, s, keep_multipliers=True).items()} for s in sets]
    pick = lambda k, shape: torch.where((set_index == 0).reshape(shape), outs[0][k], outs[1][k])
    o = dict(ctrl=pick("ctrl", (B, 1)), lam=pick("lam", (1, 1, B, 1)), status=pick("status", (B,)))
    assert is_solved(o["status"].cpu().numpy()).sum() >= 4
    rng = np.random.default_rng(11)
    xbar = rng.standard_normal((B, 12 * S)); cbar = rng.standard_normal(B)
    tan = _directions(rng, 2, B, S)
    g, j = both(solver, db, None, o, xbar, cbar, tan, set_index=set_index, sets=sets)
    zero = torch.zeros(B, dtype=torch.int32, device=d)
    for s in range(2):
        gs, js = both(solver, db, None, o, xbar, cbar, tan, set_index=zero, sets=[sets[s]])
        sel = idx == s
        assert np.array_equal(g["seg"][:, sel], gs["seg"][:, sel]), s
        for k in ("init", "ref_end", "dl_bounds", "shared"):
            assert np.array_equal(g[k][sel], gs[k][sel]), (s, k)
        assert np.array_equal(j["ctrl"][:, sel], js["ctrl"][:, sel]) and np.array_equal(j["cost"][:, sel], js["cost"][:, sel]), s
        other = idx != s
        assert not np.array_equal(g["shared"][other], gs["shared"][other])     # (the sets do differ)
    # a set index outside the sets: zeros
    bad = set_index.clone(); bad[2] = 2
    gb, jb = both(solver, db, None, o, xbar, cbar, tan, set_index=bad, sets=sets)
    assert (gb["seg"][:, 2] == 0).all() and (gb["shared"][2] == 0).all() and (jb["ctrl"][:, 2] == 0).all() and (jb["cost"][:, 2] == 0).all()


# ---- 6. delegation and refusals -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [21, 64])
def test_up_to_64_slots_the_calls_are_the_existing_ones(solver, S):
    batch, sh = synth.make_batch(7, S, config=2, seed=500 + S)
    d = solver.device
    rng = np.random.default_rng(S)
    cases = [(solver.upload(batch), S)]
    if S == 21:
        cases.append((_ragged(solver, synth.make_batch(7, 10, config=2, seed=510)[0], 21, 5 + np.arange(7) % 6), 21))
    for rec, W in cases:
        o = solver.solve_long(rec, sh, keep_multipliers=True)
        assert is_solved(o["status"].cpu().numpy()).sum() >= 6
        xbar = torch.tensor(rng.standard_normal((7, 12 * W)), device=d); cbar = torch.tensor(rng.standard_normal(7), device=d)
        tan = _dev(solver, _directions(rng, 2, 7, W))
        g0, g1 = solver.solve_vjp(rec, sh, o, xbar, cbar), solver.solve_long_vjp(rec, sh, o, xbar, cbar)
        j0, j1 = solver.solve_jvp(rec, sh, o, tan), solver.solve_long_jvp(rec, sh, o, tan)
        for k in g0:
            assert torch.equal(g0[k], g1[k]), (S, k)
        for k in j0:
            assert torch.equal(j0[k], j1[k]), (S, k)
        assert g0["seg"].abs().max() > 0 and j0["ctrl"].abs().max() > 0


def test_refusals(solver):
    d = solver.device
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=d)
    big, sh = synth.make_batch(2, 257, config=3)
    fake = dict(ctrl=f64(2, 12 * 257), lam=f64(2, 36, 2, 257), status=torch.ones(2, dtype=torch.int32, device=d))
    with pytest.raises(BtrapzError):
        solver.solve_long_vjp(solver.upload(big), sh, fake, f64(2, 12 * 257), f64(2))
    with pytest.raises(BtrapzError):
        solver.solve_long_jvp(solver.upload(big), sh, fake, {"init": f64(1, 2, 6)})
    S = 70
    batch, sh = synth.make_batch(2, S, config=3)
    db = solver.upload(batch)
    o = solver.solve_long(db, sh, keep_multipliers=True)
    xbar, cbar = f64(2, 12 * S), torch.ones(2, dtype=torch.float64, device=d)
    # the sibling still stops at 64
    with pytest.raises(BtrapzError):
        solver.solve_vjp(db, sh, o, xbar, cbar)
    with pytest.raises(BtrapzError):
        solver.solve_jvp(db, sh, o, {"init": f64(1, 2, 6)})
    ctx = solver.ctx
    args = [2, S, [sh], None, db.seg, None, db.init, db.ref_end, db.dl_bounds, o["ctrl"], o["lam"], o["status"]]
    gs = f64(L.NUM_SEG_FIELDS, 2, S)
    ctx.solve_long_vjp_device(*args, xbar, cbar, g_seg=gs)                          # (the complete call is taken)
    for hole in (4, 7, 8, 9, 10, 11):                                                # seg, ref_end, dl_bounds, ctrl, lam, status NULL
        a = list(args); a[hole] = None
        with pytest.raises(BtrapzError):
            ctx.solve_long_vjp_device(*a, xbar, cbar, g_seg=gs)
        with pytest.raises(BtrapzError):
            ctx.solve_long_jvp_device(*a, 1, init_dot=f64(1, 2, 6), cost_dot=f64(1, 2))
    with pytest.raises(BtrapzError):
        ctx.solve_long_vjp_device(*args, None, None, g_seg=gs)                       # both cotangents NULL
    with pytest.raises(BtrapzError):
        ctx.solve_long_jvp_device(*args, 1, cost_dot=f64(1, 2))                      # no tangent
    with pytest.raises(BtrapzError):
        ctx.solve_long_jvp_device(*args, 1, init_dot=f64(1, 2, 6))                   # both outputs NULL
    for T in (0, MAX_TANGENTS + 1):
        with pytest.raises(BtrapzError):
            ctx.solve_long_jvp_device(*args, T, init_dot=f64(max(T, 1), 2, 6), cost_dot=f64(max(T, 1), 2))
    two = [sh, diff.shared_from_params(sh.as_array()[:20], 1 - sh.variant, sh.delta)]   # sets that are not alike
    with pytest.raises(BtrapzError):
        ctx.solve_long_vjp_device(2, S, two, None, *args[4:], xbar, cbar, g_seg=gs)
    ctx.solve_long_jvp_device(*args, MAX_TANGENTS, init_dot=f64(MAX_TANGENTS, 2, 6), cost_dot=f64(MAX_TANGENTS, 2))
    torch.cuda.synchronize()


# ---- 7. the autograd layer ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [65, 129])
def test_diff_solve_long_and_its_jacobian(solver, S):
    batch, sh = problem("generic", S)
    d = solver.device
    t = lambda a: torch.tensor(a, device=d, requires_grad=True)
    seg, init, ref_end, dl = t(batch.seg), t(batch.init), t(batch.ref_end), t(batch.dl_bounds)
    params = torch.tensor(diff.params_from_shared(sh), device=d, requires_grad=True)
    ctrl, cost, status = diff.solve_long(solver, seg, init, ref_end, dl, params, variant=sh.variant, delta=sh.delta)
    assert is_solved(status.cpu().numpy()).sum() >= 4
    r = torch.tensor(np.random.default_rng(S).standard_normal((B, 12 * S)), device=d)
    loss = (ctrl * r).sum() + 0.7 * cost.sum()
    loss.backward()
    db, o, _ = solved(solver, "generic", S)
    assert torch.equal(o["ctrl"], ctrl.detach()) and torch.equal(o["status"], status)
    g = solver.solve_long_vjp(db, sh, o, r, torch.full((B,), 0.7, dtype=torch.float64, device=d))
    assert torch.equal(seg.grad, g["seg"]) and torch.equal(init.grad, g["init"])
    assert torch.equal(ref_end.grad, g["ref_end"]) and torch.equal(dl.grad, g["dl_bounds"])
    assert torch.allclose(params.grad, g["shared"].sum(0), rtol=1e-12, atol=0) and g["shared"].abs().max() > 0
    cols = [0, 5, 10]
    jac = diff.solve_long_jacobian(solver, torch.tensor(batch.seg, device=d), torch.tensor(batch.init, device=d),
                                   torch.tensor(batch.ref_end, device=d), torch.tensor(batch.dl_bounds, device=d), params.detach(), cols,
                                   variant=sh.variant, delta=sh.delta)
    unit = torch.zeros((len(cols), B, 20), dtype=torch.float64, device=d)
    for i, c in enumerate(cols):
        unit[i, :, c] = 1.0
    j = solver.solve_long_jvp(db, sh, o, {"shared": unit})
    assert torch.equal(jac["dctrl"], j["ctrl"]) and torch.equal(jac["dcost"], j["cost"]) and j["ctrl"].abs().max() > 0
    again = diff.solve_long_jacobian(solver, torch.tensor(batch.seg, device=d), torch.tensor(batch.init, device=d),
                                     torch.tensor(batch.ref_end, device=d), torch.tensor(batch.dl_bounds, device=d), params.detach(), cols,
                                     variant=sh.variant, delta=sh.delta, out=jac["out"])
    assert torch.equal(again["dctrl"], jac["dctrl"])
