"""The rescue pass for candidates of 193..256 segments and for the long candidates of ragged batches
(btrapz_solve_long_rescue_device, include/btrapz_hip_long_rescue.h; ipm_solve_long_rescue_kernel: the ELASTIC instantiation of
the long form with a fourth wavefront), held to the oracle's relaxed solve (AssembledQp.solve_elastic) with the bounds of
tests/test_gpu_rescue_edges.py: |ctrl - x|_inf <= 1e-4 |x|_inf, the row violation to 1e-5, status 2 and a finite cost where the
least violation is <= elastic_tol - 1e-4, a negative status and cost +inf where it is >= elastic_tol + 1e-4.

The relaxed solve takes one to three minutes a candidate at these widths: its answers are stored
(tests/golden/long_rescue_yardstick.npz, written by tests/golden/make_long_rescue_goldens.py; tests/test_long_rescue_goldens.py
holds the file to the generator), the inputs are rebuilt here from the synth seeds and their checksum compared.

Seams: at 193 segments the damaged last joint sits between segment 191 (lane 63 of wavefront 2) and segment 192 (lane 0 of
wavefront 3, its only lane), the damaged initial state on lane 0 of wavefront 0; 255 and 256 end the fourth wavefront on its
last lane but one and on its last."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_long_rescue_goldens as G   # noqa: E402
import test_gpu_rescue_edges as E      # noqa: E402
from helpers import oracle_qp_from_batch   # noqa: E402
from spectral_amd import layout as L   # noqa: E402
from spectral_amd import native, synth   # noqa: E402

pytestmark = pytest.mark.gpu
TOL, BAND = G.TOL, E.BAND
KEYS = ("status", "cost", "ctrl", "iters")
INORM = np.array([1.0, 50.0 ** -0.5, 2400.0 ** -0.5, 72000.0 ** -0.5])   # 1 / |g| of a position (t = 1), velocity, acceleration, jerk row


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


@pytest.fixture(scope="module")
def gold():
    return np.load(G.OUT)


def grab(solver, o):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in o.items()}, solver.ctx.last_solve_form()


_seams = {}


def seam(gold, S):
    """(batch, sh) of the stored width S, rebuilt from the seeds and held to the stored checksum."""
    if S not in _seams:
        batch, sh = G.seam_batch(S, gold["bases_%d" % S])
        assert G.batch_hash(batch, sh) == str(gold["hash_%d" % S]), S
        assert (batch.seg[L.F_T] == 1.0).all()              # (INORM's position entry)
        _seams[S] = (batch, sh)
    return _seams[S]


def row_violation(qp, x):
    """Largest violation of an inequality row by x in the row's own norm |g| (tests/test_gpu_rescue_edges.py, on the sparse A)."""
    import scipy.sparse as sp
    A = sp.csc_matrix((qp.A_x, qp.A_i, qp.A_p), shape=(qp.m, qp.n)).tocsr()
    Ax = A @ x
    ineq = (qp.u - qp.l) > 1e-12
    nrm = np.sqrt(np.asarray(A.multiply(A).sum(axis=1)).ravel())
    return float((np.abs(Ax - np.clip(Ax, qp.l, qp.u))[ineq] / nrm[ineq]).max())


def check_decisions(S, r, batch, sh, x, viol, slots, what):
    """The stored verdicts on slots of r (slot 0 is the untouched candidate)."""
    seen = [0, 0]
    for b in slots:
        if b == 0:
            continue
        if viol[b] <= TOL - BAND:
            assert r["status"][b] == 2 and np.isfinite(r["cost"][b]), (what, S, b, r["status"][b], viol[b])
            got = r["ctrl"][b][:12 * S]
            err = np.abs(got - x[b]).max() / np.abs(x[b]).max()
            dv = abs(row_violation(oracle_qp_from_batch(batch, sh, b), got) - viol[b])
            print("%s S=%d b=%d least violation %.6f: |ctrl - x| / |x| = %.2e, violation differs by %.2e" % (what, S, b, viol[b], err, dv))
            assert err <= 1e-4, (what, S, b, err)
            assert dv <= 1e-5, (what, S, b, dv)
            seen[0] += 1
        elif viol[b] >= TOL + BAND:
            assert r["status"][b] < 0 and np.isposinf(r["cost"][b]), (what, S, b, r["status"][b], r["cost"][b], viol[b])
            seen[1] += 1
    return seen


def violations(solver, B):
    import torch
    v = torch.full((B, 4), float("nan"), dtype=torch.float64, device=solver.device)
    solver.ctx.rescue_violations_device(B, v, stream=torch.cuda.current_stream(solver.device).cuda_stream)
    torch.cuda.synchronize()
    return v.cpu().numpy()


# ---- 1. seams ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", G.SIZES)
def test_rescue_pass_at_the_seams_of_the_fourth_wavefront(solver, gold, S):
    batch, sh = seam(gold, S)
    x, viol = gold["x_%d" % S], gold["viol_%d" % S]
    db = solver.upload(batch)
    plain, form = grab(solver, solver.solve_long(db, sh))
    assert form == 16
    ok = plain["status"] > 0
    assert ok[0] and not ok[1:].any(), plain["status"]       # the plain solve and the oracle agree on what has a solution ...
    assert np.abs(plain["ctrl"][0] - x[0]).max() <= 1e-5 * np.abs(x[0]).max()   # ... and on the solution
    resc, form = grab(solver, solver.solve_long_rescue(db, sh))
    assert form == 16
    v4 = violations(solver, batch.B)
    # candidates the plain solve answered are not touched
    for k in KEYS:
        assert np.array_equal(resc[k][ok], plain[k][ok]), k
    seen = check_decisions(S, resc, batch, sh, x, viol, range(batch.B), "uniform")
    assert seen[0] >= 1 and seen[1] >= 1, seen
    # btrapz_rescue_violations_device: per class in the rows' own units; the largest in control-point units is the least violation
    assert np.isfinite(v4).all() and (v4[0] == 0).all()
    for b in range(1, batch.B):
        if viol[b] <= TOL - BAND:
            vn = (v4[b] * INORM).max()
            print("S=%d b=%d rescue_violations %s -> %.6f (stored %.6f)" % (S, b, v4[b], vn, viol[b]))
            assert abs(vn - viol[b]) <= 1e-5, (S, b, v4[b], viol[b])


# ---- 2. delegation, bit for bit ------------------------------------------------------------------------------------------------

def long_damaged(S):
    """Three candidates of S segments: untouched, last joint apart by 0.008 (accepted) and by 0.060 (refused)."""
    batch, sh = synth.make_batch(3, S, config=2, seed=500 + S)
    batch = L.Batch(B=3, S=S, seg=batch.seg.copy(), init=batch.init.copy(), ref_end=batch.ref_end.copy(), dl_bounds=batch.dl_bounds.copy())
    E.conflict_at_last_joint(batch, 1, E.GAPS_JOINT[0])
    E.conflict_at_last_joint(batch, 2, E.GAPS_JOINT[1])
    return batch, sh


@pytest.mark.parametrize("S", [21, 64, 65, 130, 192])
def test_up_to_192_segments_the_call_is_the_rescue_pass_that_was_there(solver, S):
    if S <= 64:
        batch, sh, _ = E.damaged_batch(S, 7)
    else:
        batch, sh = long_damaged(S)
    db = solver.upload(batch)
    theirs, f0 = grab(solver, solver.solve(db, sh, elastic=1))
    mine, f1 = grab(solver, solver.solve_long_rescue(db, sh))
    assert f0 == f1 == (2 if S > 64 else f0)
    assert (theirs["status"] == 2).any() and (theirs["status"] < 0).any() and (theirs["status"] == 1).any(), theirs["status"]
    for k in KEYS:
        assert np.array_equal(mine[k], theirs[k]), (S, k)


def test_without_a_rescue_pass_the_call_is_the_long_warm_solve(solver, gold):
    batch, sh = seam(gold, 193)
    db = solver.upload(batch)
    theirs, f0 = grab(solver, solver.solve_long(db, sh, keep_multipliers=True))
    mine, f1 = grab(solver, solver.solve_long_rescue(db, sh, keep_multipliers=True, elastic=0))
    assert f0 == f1 == 16 and theirs["status"][0] > 0 and (theirs["status"][1:] < 0).all()
    for k in KEYS + ("lam",):
        assert np.array_equal(mine[k], theirs[k]), k


# ---- 3. ragged -----------------------------------------------------------------------------------------------------------------

COUNTS = (20, 64, 65, 130, 193, 256)


def width_batch(gold, S):
    """(batch, sh, clean slot, damaged-and-accepted slot) of one width."""
    if S in G.SIZES:
        return seam(gold, S) + (0, 3)
    return long_damaged(S) + (0, 1)


@pytest.fixture(scope="module")
def ragged(gold):
    stride = 256
    src = [(S, slot) for S in COUNTS for slot in width_batch(gold, S)[2:]]
    B = len(src)
    seg = np.zeros((L.NUM_SEG_FIELDS, B, stride)); cnt = np.zeros(B, dtype=np.int32)
    init = np.zeros((B, 6)); ref_end = np.zeros((B, 2)); dlb = np.zeros((B, 10))
    perm = np.random.default_rng(11).permutation(B)
    sh = width_batch(gold, COUNTS[0])[1]
    for dst, i in enumerate(perm):
        S, b = src[i]
        pb, psh = width_batch(gold, S)[:2]
        assert np.array_equal(psh.as_array(), sh.as_array())
        seg[:, dst, :S] = pb.seg[:, b, :]; cnt[dst] = S
        init[dst], ref_end[dst], dlb[dst] = pb.init[b], pb.ref_end[b], pb.dl_bounds[b]
    return dict(B=B, stride=stride, seg=seg, cnt=cnt, init=init, ref_end=ref_end, dlb=dlb, src=[src[i] for i in perm], sh=sh)


def test_ragged_record_every_candidate_as_the_uniform_call_of_its_width(solver, gold, ragged):
    import torch
    dev = solver.device
    t = lambda a: torch.from_numpy(a).to(dev)
    B, st, sh = ragged["B"], ragged["stride"], ragged["sh"]
    rec = dict(B=B, seg_stride=st, seg=t(ragged["seg"]), seg_count=t(ragged["cnt"]), init=t(ragged["init"]), ref_end=t(ragged["ref_end"]),
               dl_bounds=t(ragged["dlb"]))
    short = ragged["cnt"] <= 64
    # the entry point that was there: a long candidate is not solved, with the option find_traj itself uses
    before, f = grab(solver, solver.solve_ragged(rec, sh, elastic=1))
    assert not f & 16 and (before["status"][~short] == -5).all() and (before["status"][short] > 0).all(), before["status"]   # BTRAPZ_NO_CORRIDOR
    mine, f = grab(solver, solver.solve_long_rescue(rec, sh))
    assert f & 16
    v4 = violations(solver, B)
    assert (mine["status"] > 0).all(), mine["status"]
    uniform = {}
    for dst, (S, b) in enumerate(ragged["src"]):
        if S <= 64:            # (a short candidate: the stride-64 record below -- the uniform call of its width may take another form)
            continue
        if S not in uniform:
            uniform[S] = grab(solver, solver.solve_long_rescue(solver.upload(width_batch(gold, S)[0]), sh))[0]
        u = uniform[S]
        clean = b == width_batch(gold, S)[2]
        assert u["status"][b] == (1 if clean else 2), (S, b, u["status"])
        assert np.array_equal(mine["ctrl"][dst, :12 * S], u["ctrl"][b]) and (mine["ctrl"][dst, 12 * S:] == 0).all(), (S, b)
        for k in ("status", "cost", "iters"):
            assert mine[k][dst] == u[k][b], (S, b, k, mine[k][dst], u[k][b])
        assert (v4[dst] == 0).all() if clean else 0.003 < (v4[dst] * INORM).max() < 0.005, (S, b, v4[dst])
    # the stored yardstick on the rescued candidates of 193 and 256 segments
    for dst, (S, b) in enumerate(ragged["src"]):
        if S in G.SIZES and b != 0:
            batch, bsh = seam(gold, S)
            got = check_decisions(S, {k: {b: mine[k][dst]} for k in KEYS}, batch, bsh, gold["x_%d" % S], gold["viol_%d" % S], [b], "ragged")
            assert got == [1, 0]
    # at most 64 segments: what btrapz_solve_ragged_device(elastic = 1) returns for a stride-64 record of them, bit for bit
    idx = np.nonzero(short)[0]
    rec64 = dict(B=len(idx), seg_stride=64, seg=t(np.ascontiguousarray(ragged["seg"][:, idx, :64])), seg_count=t(ragged["cnt"][idx]),
                 init=t(ragged["init"][idx]), ref_end=t(ragged["ref_end"][idx]), dl_bounds=t(ragged["dlb"][idx]))
    theirs, _ = grab(solver, solver.solve_ragged(rec64, sh, elastic=1))
    assert sorted(theirs["status"]) == [1, 1, 2, 2]
    for j, dst in enumerate(idx):
        S = ragged["cnt"][dst]
        assert np.array_equal(mine["ctrl"][dst, :12 * S], theirs["ctrl"][j, :12 * S])
        for k in ("status", "cost", "iters"):
            assert mine[k][dst] == theirs[k][j], (S, k)


# ---- 4. warm starts and repeats --------------------------------------------------------------------------------------------------

def test_warm_start_with_a_rescue_pass_repeats_and_prefilled_outputs(solver, gold):
    import torch
    S = 193
    batch, sh = seam(gold, S)
    x, viol = gold["x_%d" % S], gold["viol_%d" % S]
    db = solver.upload(batch)
    first, _ = grab(solver, solver.solve_long_rescue(db, sh))
    again, _ = grab(solver, solver.solve_long_rescue(db, sh))
    for k in KEYS:
        assert np.array_equal(first[k], again[k]), k
    out = solver.new_result(batch.B, S)
    out["ctrl"].fill_(float("nan")); out["cost"].fill_(float("nan")); out["status"].fill_(-99); out["iters"].fill_(-99)
    filled, _ = grab(solver, solver.solve_long_rescue(db, sh, out=out))
    for k in KEYS:
        assert np.array_equal(filled[k], first[k]), k
    # warm: joint states and multipliers of a cold solve (a stalled candidate's are whatever its last iterate was)
    o = solver.solve_long(db, sh, keep_multipliers=True)
    lam = o["lam"].clone()
    x0 = solver.eval_states(db, o["ctrl"].clone(), torch.from_numpy(np.cumsum(batch.seg[L.F_T], axis=1)))
    wplain, f = grab(solver, solver.solve_long(db, sh, warm=dict(x0=x0, lam=lam.clone())))
    assert f == 16
    wresc, f = grab(solver, solver.solve_long_rescue(db, sh, warm=dict(x0=x0, lam=lam.clone()), keep_multipliers=True))
    assert f == 16
    ok = wplain["status"] > 0
    assert ok[0] and not ok[1:].any(), wplain["status"]
    assert wplain["iters"][0] < first["iters"][0]
    for k in KEYS:
        assert np.array_equal(wresc[k][ok], wplain[k][ok]), k
    seen = check_decisions(S, wresc, batch, sh, x, viol, range(batch.B), "warm")
    assert seen[0] >= 1 and seen[1] >= 1, seen
    assert np.array_equal(wresc["status"][1:], first["status"][1:])
    assert np.isfinite(wresc["lam"][:, :, ok]).all()


# ---- 5. find_traj ----------------------------------------------------------------------------------------------------------------

def test_find_traj_rescues_a_scene_of_more_than_192_segments(gold):
    kb = G.ft_scene(float(gold["ft_l0"]))
    assert G.knots_hash(kb) == str(gold["ft_hash"])
    n, x = int(gold["ft_n"]), gold["ft_x"]
    assert n >= 200 and float(gold["ft_viol"]) <= TOL - 0.002
    params = native.CParams(*[float(v) for v in synth.REFERENCE_WEIGHTS], 1)
    cost, traj, ctrl = native.find_traj_mem(0, params, kb, cap=4096)
    st, v = native.find_traj_last_status()
    assert cost < 1e10 and st == 2 and len(ctrl) == 12 * n, (cost, st, v)
    err = np.abs(ctrl - x).max() / np.abs(x).max()
    print("find_traj, %d segments: status %d, class violations %s, |ctrl - x| / |x| = %.2e" % (n, st, v, err))
    assert err <= 1e-4, err
    os.environ["BTRAPZ_ELASTIC"] = "0"                      # strict mode: refused
    try:
        assert native.find_traj_mem(0, params, kb, cap=4096)[0] >= 1e10
    finally:
        del os.environ["BTRAPZ_ELASTIC"]


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_argument(solver):
    batch, sh = synth.make_batch(2, 70, config=3)
    db = solver.upload(batch)
    o = solver.new_result(2, 70)
    args = (2, 70, sh, db.seg, None, db.init, db.ref_end, db.dl_bounds, o["ctrl"], o["cost"], o["status"], o["iters"])
    entry = solver.ctx.solve_long_rescue_device
    with pytest.raises(native.BtrapzError, match="elastic"):
        entry(*args, elastic=2)
    with pytest.raises(native.BtrapzError, match="seg is NULL"):
        entry(*args[:3], None, *args[4:])
    with pytest.raises(native.BtrapzError, match="status is NULL"):
        entry(*args[:10], None, args[11])
    big, bsh = synth.make_batch(2, 257, config=3)
    dbig = solver.upload(big)
    ob = solver.new_result(2, 257)
    with pytest.raises(native.BtrapzError, match="seg_stride"):
        entry(2, 257, bsh, dbig.seg, None, dbig.init, dbig.ref_end, dbig.dl_bounds, ob["ctrl"], ob["cost"], ob["status"], ob["iters"])
    entry(*args)                                             # and the arguments as they are: served
    import torch
    torch.cuda.synchronize()
    assert (o["status"].cpu().numpy() > 0).all()
