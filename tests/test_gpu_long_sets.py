"""A parameter set per candidate with warm starts beyond 64 segments and with the rescue pass at every width
(btrapz_solve_long_sets_device, include/btrapz_hip_long_sets.h; BatchSolver.solve_long_sets).

The yardstick for every value is the one-set entry point: candidate b's ctrl, cost, status, iters and lam slots must be, bit for
bit, what btrapz_solve_long_rescue_device (and what it delegates to) writes there for a batch of the same shape solved with
sets[set_index[b]], the same start and the same options (lean pinned).  That path is held to the oracle by
tests/test_gpu_long_rescue.py, test_gpu_rescue_edges.py, test_gpu_long_warm.py and test_gpu_active_rows.py: here every
comparison of a solve's outputs is array_equal, never a tolerance.  (Two bounds are stated where they are used: the oracle
anchor's stored one, and the rounding of a three-term sum taken in another order in the diff test.)

Inputs: synth.make_scenario1_batch; damage = the initial lateral position GAP below segment 0's lower line (rescued, least
violation GAP) or FAR below it (beyond elastic_tol: BTRAPZ_PRIMAL_INFEASIBLE).  Sets 0..2 differ in weights (logged rows) and
ds_ref -- the objective only, so a damaged candidate's rows are the same under each --, set 3 in the lateral acceleration limit.
Candidates name the sets round-robin; one names a set that does not exist."""
import dataclasses
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import test_gpu_long_rescue as R       # noqa: E402
import test_gpu_param_sets as P        # noqa: E402
from spectral_amd import layout as L   # noqa: E402
from spectral_amd import native, synth   # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("ctrl", "cost", "status", "iters")
FILL = -777.0                           # what every output slot holds before a call
GAP, FAR = 0.004, 0.060                 # tools/long_rescue_bench.py's damage; far beyond elastic_tol (0.0125)
NO_CORRIDOR, MAX_ITER, PRIMAL_INFEASIBLE = -5, -2, -3


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def four_sets(sh):
    sets = []
    for g, w in enumerate(P.weight_rows(3)):
        ws = synth.shared_params(sh.variant, weights=w)
        sets.append(dataclasses.replace(sh, w_s=ws.w_s, w_l=ws.w_l, weight_end_s=ws.weight_end_s, weight_end_l=ws.weight_end_l,
                                        ds_ref=sh.ds_ref + 0.5 * g))
    sets.append(dataclasses.replace(sh, ddl=(sh.ddl[0] - 0.2, sh.ddl[1] + 0.2)))
    return sets


def copy_batch(batch):
    return L.Batch(B=batch.B, S=batch.S, seg=batch.seg.copy(), init=batch.init.copy(), ref_end=batch.ref_end.copy(),
                   dl_bounds=batch.dl_bounds.copy())


def damage(batch, b, gap):
    batch.init[b, 3] = batch.seg[L.F_L_DOWN_BIAS, b, 0] - gap


def uniform_case(S, B=None, rescue=True, seed=None):
    """(batch, sets, set_index, bad): round-robin sets, candidate B - 1 names set 9; with rescue: candidates 0..7 (two per set:
    scenario_1 has candidates without a trajectory of its own making) damaged by GAP, candidate 8 by FAR."""
    B = B or (24 if rescue else 12)
    batch, sh = synth.make_scenario1_batch(B, S, 0, seed=(4000 + S) if seed is None else seed)
    batch = copy_batch(batch)
    idx = (np.arange(B) % 4).astype(np.int32)
    idx[B - 1] = 9
    if rescue:
        for b in range(8):
            damage(batch, b, GAP)
        damage(batch, 8, FAR)
    return batch, four_sets(sh), idx, B - 1


def tensor(solver, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(solver.device)


def prefilled(solver, r, keep):
    import torch
    o = solver.new_result(r.B, r.S)
    o["ctrl"].fill_(FILL); o["cost"].fill_(FILL); o["status"].fill_(-99); o["iters"].fill_(-99)
    lam = torch.full((2, 36, r.B, r.S), FILL, dtype=torch.float64, device=solver.device) if keep else None
    return o, lam


def finish(solver, o, lam, elastic, B):
    import torch
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy().copy() for k, v in o.items()}
    if lam is not None:
        h["lam"] = lam.cpu().numpy().copy()
    h["form"] = solver.ctx.last_solve_form()
    if elastic:
        h["viol"] = R.violations(solver, B)
    return h


def call_sets(solver, rec, sets, idx, x0=None, lam0=None, keep=False, elastic=0, lean=0):
    """btrapz_solve_long_sets_device on prefilled outputs (lam_out a buffer of its own, prefilled too)."""
    import torch
    r = solver._record(rec)
    o, lam = prefilled(solver, r, keep)
    solver.ctx.solve_long_sets_device(r.B, r.S, sets, tensor(solver, np.asarray(idx, dtype=np.int32)), r.seg, r.seg_count, r.init, r.ref_end,
                                      r.dl_bounds, o["ctrl"], o["cost"], o["status"], o["iters"], x0=x0, lam0=lam0, lam_out=lam,
                                      stream=torch.cuda.current_stream(solver.device).cuda_stream, elastic=elastic, lean=lean, cap_iter=-1)
    return finish(solver, o, lam, elastic, r.B)


def call_one(solver, rec, sh, x0=None, lam0=None, keep=False, elastic=0, lean=0):
    """The yardstick: btrapz_solve_long_rescue_device with one set, the same way."""
    import torch
    r = solver._record(rec)
    o, lam = prefilled(solver, r, keep)
    solver.ctx.solve_long_rescue_device(r.B, r.S, sh, r.seg, r.seg_count, r.init, r.ref_end, r.dl_bounds, o["ctrl"], o["cost"], o["status"],
                                        o["iters"], x0=x0, lam0=lam0, lam_out=lam, stream=torch.cuda.current_stream(solver.device).cuda_stream,
                                        elastic=elastic, lean=lean)
    return finish(solver, o, lam, elastic, r.B)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == np.float64 else a


def assert_rows(got, ref, rows, what, keys=KEYS):
    """got's slots of candidates `rows` are ref's, bit for bit (lam: [2, 36, B, S]; viol: [B, 4])."""
    for k in keys:
        a, b = (got[k][:, :, rows], ref[k][:, :, rows]) if k == "lam" else (got[k][rows], ref[k][rows])
        assert np.array_equal(bits(a), bits(b)), (what, k)


def assert_untouched(got, bad, what):
    assert got["status"][bad] == NO_CORRIDOR and np.isposinf(got["cost"][bad]) and got["iters"][bad] == 0, (what, got["status"][bad], got["cost"][bad])
    assert (got["ctrl"][bad] == FILL).all(), what
    if "lam" in got:
        assert (got["lam"][:, :, bad] == FILL).all(), what


def per_set(solver, rec, sets, idx, got, what, keys, **kw):
    """Every set's candidates against the one-set call on the same batch; returns the one-set results."""
    refs = []
    for g, sh in enumerate(sets):
        ref = call_one(solver, rec, sh, **kw)
        rows = np.nonzero(idx == g)[0]
        assert len(rows), g
        assert_rows(got, ref, rows, (what, "set", g), keys)
        assert ref["form"] == got["form"], (what, g, ref["form"], got["form"])
        refs.append(ref)
    return refs


def rescue_conditions(got, idx, n_sets, bad, what):
    st = got["status"]
    print("%s: statuses %s" % (what, st.tolist() if len(st) <= 64 else np.unique(st, return_counts=True)))
    for g in range(n_sets):
        assert (st[idx == g] == 2).any(), (what, "no rescued candidate in set", g, st[idx == g])
    assert (st == PRIMAL_INFEASIBLE).any(), (what, st)
    assert 2 * (st == 1).sum() >= len(st), (what, st)
    assert_untouched(got, bad, what)


def joint_times(solver, seg_T, shift=0.0):
    return tensor(solver, np.cumsum(seg_T, axis=1) + shift)


# ---- 1. warm long sets, uniform -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [65, 128, 129, 192, 193, 256])
def test_warm_long_sets_uniform(solver, S):
    import torch
    d = 0.1
    batch, sets, idx, bad = uniform_case(S, rescue=False)
    B = batch.B
    db = solver.upload(batch)
    cold = call_sets(solver, db, sets, idx, keep=True)
    assert cold["form"] == 16
    assert_untouched(cold, bad, (S, "cold"))
    per_set(solver, db, sets, idx, cold, (S, "cold"), KEYS + ("lam",), keep=True)
    # one replanning step (tools/long_warm_bench.py): every line 0.1 s later, the initial state along the previous solution, start
    # = the previous trajectory 0.1 s later and the previous multipliers.  (The candidate without a set has no solution: its start
    # is that of candidate 0, which no compared slot reads.)
    ctrl = tensor(solver, cold["ctrl"]); ctrl[bad] = ctrl[0]
    lam = tensor(solver, cold["lam"]); lam[:, :, bad] = 0.0
    x0 = solver.eval_states(db, ctrl, joint_times(solver, batch.seg[L.F_T], d))
    new_init = solver.eval_states(db, ctrl, torch.full((B, 1), d, dtype=torch.float64)).cpu().numpy()
    nb = copy_batch(batch)
    for bias, skew in ((L.F_DOWN_BIAS, L.F_DOWN_SKEW), (L.F_UPP_BIAS, L.F_UPP_SKEW), (L.F_L_DOWN_BIAS, L.F_L_DOWN_SKEW),
                       (L.F_L_UPP_BIAS, L.F_L_UPP_SKEW), (L.F_X_BIAS, L.F_X_SKEW), (L.F_Y_BIAS, L.F_Y_SKEW)):
        nb.seg[bias] = nb.seg[bias] + nb.seg[skew] * d
    nb.init = np.concatenate([new_init[:, 0, 0], new_init[:, 1, 0]], axis=1)
    ndb = solver.upload(nb)
    warm = call_sets(solver, ndb, sets, idx, x0=x0, lam0=lam, keep=True)
    assert warm["form"] == 16
    assert_untouched(warm, bad, (S, "warm"))
    per_set(solver, ndb, sets, idx, warm, (S, "warm"), KEYS + ("lam",), x0=x0, lam0=lam, keep=True)
    ok = (cold["status"] > 0) & (warm["status"] > 0)
    print("S=%d: mean iterations cold %.2f, warm %.2f over %d candidates" % (S, cold["iters"][ok].mean(), warm["iters"][ok].mean(), ok.sum()))
    assert ok.sum() >= B // 2 and warm["iters"][ok].mean() < cold["iters"][ok].mean()


# ---- 2. rescue long sets, uniform -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("start", ["cold", "warm"])
@pytest.mark.parametrize("S", [65, 192, 193, 256])
def test_rescue_long_sets_uniform(solver, S, start):
    batch, sets, idx, bad = uniform_case(S)
    db = solver.upload(batch)
    kw = dict(elastic=1)
    if start == "warm":   # from the own plain solution and its multipliers (a stalled candidate's: its last iterate)
        first = call_sets(solver, db, sets, idx, keep=True)
        ctrl = tensor(solver, first["ctrl"]); ctrl[bad] = ctrl[bad - 1]
        lam = tensor(solver, first["lam"]); lam[:, :, bad] = 0.0
        kw.update(x0=solver.eval_states(db, ctrl, joint_times(solver, batch.seg[L.F_T])), lam0=lam, keep=True)
    got = call_sets(solver, db, sets, idx, **kw)
    assert got["form"] == (2 if (S <= 192 and start == "cold") else 16)
    rescue_conditions(got, idx, 4, bad, (S, start))
    per_set(solver, db, sets, idx, got, (S, start), KEYS + ("viol",) + (("lam",) if start == "warm" else ()), **kw)
    assert (got["viol"][bad] == 0).all()


# ---- 3. packed and lean rescue with sets ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("lean", [1, -1])
@pytest.mark.parametrize("S", [1, 3, 21, 32, 33, 64])
def test_packed_rescue_with_sets(solver, S, lean):
    B = 253
    batch, sets, idx, bad = uniform_case(S, B=B, rescue=False)
    for b in range(0, B - 1, 9):                         # every ninth candidate damaged: 28 over the four sets, two of them FAR
        damage(batch, b, FAR if b in (9, 135) else GAP)
    db = solver.upload(batch)
    got = call_sets(solver, db, sets, idx, elastic=1, lean=lean)
    rescue_conditions(got, idx, 4, bad, (S, lean))
    for g, sh in enumerate(sets):
        r = solver._record(db)
        o, _ = prefilled(solver, r, False)
        solver.solve(db, sh, elastic=1, lean=lean, cap_iter=-1, out=o)
        ref = finish(solver, o, None, 1, B)
        assert_rows(got, ref, np.nonzero(idx == g)[0], (S, lean, g), KEYS + ("viol",))
        assert ref["form"] == got["form"], (S, lean, g, ref["form"], got["form"])


# ---- 4. ragged record, stride 256 -----------------------------------------------------------------------------------------------

COUNTS = (1, 20, 21, 64, 65, 130, 193, 256)
PER = 5


@pytest.fixture(scope="module")
def ragged():
    """PER candidates of every count, width after width; the first of a width damaged by GAP (widths w -> set 5 w mod 4: every
    set has two), the second of the first width by FAR; sets round-robin over the record, the last candidate names none."""
    stride = 256
    B = PER * len(COUNTS)
    seg = np.zeros((L.NUM_SEG_FIELDS, B, stride)); cnt = np.zeros(B, dtype=np.int32)
    init = np.zeros((B, 6)); ref_end = np.zeros((B, 2)); dlb = np.zeros((B, 10))
    parts, sh = {}, None
    for w, S in enumerate(COUNTS):
        pb, sh = synth.make_scenario1_batch(PER, S, 0, seed=4100 + S)
        pb = copy_batch(pb)
        damage(pb, 0, GAP)
        if w == 0:
            damage(pb, 1, FAR)
        parts[S] = pb
        rows = slice(PER * w, PER * (w + 1))
        seg[:, rows, :S] = pb.seg; cnt[rows] = S
        init[rows], ref_end[rows], dlb[rows] = pb.init, pb.ref_end, pb.dl_bounds
    idx = (np.arange(B) % 4).astype(np.int32)
    idx[B - 1] = -1
    return dict(B=B, stride=stride, seg=seg, cnt=cnt, init=init, ref_end=ref_end, dlb=dlb, idx=idx, bad=B - 1, parts=parts, sets=four_sets(sh))


@pytest.mark.parametrize("start", ["cold", "warm"])
def test_ragged_record_stride_256(solver, ragged, start):
    B, st, idx, bad, sets = ragged["B"], ragged["stride"], ragged["idx"], ragged["bad"], ragged["sets"]
    t = lambda a: tensor(solver, a)
    rec = dict(B=B, seg_stride=st, seg=t(ragged["seg"]), seg_count=t(ragged["cnt"]), init=t(ragged["init"]), ref_end=t(ragged["ref_end"]),
               dl_bounds=t(ragged["dlb"]))
    kw = dict(elastic=1, lean=-1)
    x0 = lam = None
    if start == "warm":
        first = call_sets(solver, rec, sets, idx, keep=True, lean=-1)
        assert first["form"] & 16
        ctrl = t(first["ctrl"]); ctrl[bad] = 0.0
        lam = t(first["lam"]); lam[:, :, bad] = 0.0
        x0 = solver.eval_states(rec, ctrl, joint_times(solver, ragged["seg"][L.F_T]))
        kw.update(x0=x0, lam0=lam, keep=True)
    got = call_sets(solver, rec, sets, idx, **kw)
    assert got["form"] & 16
    rescue_conditions(got, idx, 4, bad, ("ragged", start))
    # slots beyond a candidate's count keep what they held
    for b in range(B):
        assert (got["ctrl"][b, 12 * ragged["cnt"][b]:] == FILL).all(), b
        if "lam" in got and b != bad:
            assert (got["lam"][:, :, b, ragged["cnt"][b]:] == FILL).all(), b
    # the contract: the one-set call on the same record
    per_set(solver, rec, sets, idx, got, ("ragged", start), KEYS + ("viol",) + (("lam",) if start == "warm" else ()), **kw)
    # a long candidate: the uniform one-set call of its own width (and start)
    for w, S in enumerate(COUNTS):
        if S <= 64:
            continue
        rows = np.arange(PER * w, PER * (w + 1))
        ub = solver.upload(ragged["parts"][S])
        ukw = dict(elastic=1, lean=-1)
        if start == "warm":
            ukw.update(x0=x0[rows][:, :, :S].contiguous(), lam0=lam[:, :, rows][:, :, :, :S].contiguous(), keep=True)
        for g, sh in enumerate(sets):
            mine = rows[idx[rows] == g]
            if not len(mine):
                continue
            u = call_one(solver, ub, sh, **ukw)
            for b in mine:
                j = b - PER * w
                assert np.array_equal(bits(got["ctrl"][b, :12 * S]), bits(u["ctrl"][j])), (S, b, "ctrl")
                for k in ("cost", "status", "iters"):
                    assert bits(got[k][b:b + 1]).tobytes() == bits(u[k][j:j + 1]).tobytes(), (S, b, k, got[k][b], u[k][j])
                assert np.array_equal(bits(got["viol"][b]), bits(u["viol"][j])), (S, b, "viol")
                if start == "warm":
                    assert np.array_equal(bits(got["lam"][:, :, b, :S]), bits(u["lam"][:, :, j])), (S, b, "lam")


# ---- 5. the set reaches every new kernel ----------------------------------------------------------------------------------------

def paired(S, seed):
    """Candidates 2 i and 2 i + 1 alike; pair 0 damaged by GAP."""
    batch, sh = synth.make_scenario1_batch(3, S, 0, seed=seed)
    rep = np.repeat(np.arange(3), 2)
    batch = L.Batch(B=6, S=S, seg=batch.seg[:, rep].copy(), init=batch.init[rep].copy(), ref_end=batch.ref_end[rep].copy(),
                    dl_bounds=batch.dl_bounds[rep].copy())
    return batch, [sh, dataclasses.replace(sh, ds_ref=sh.ds_ref - 4.0)], (np.arange(6) % 2).astype(np.int32)


@pytest.mark.parametrize("S,kind", [(100, "warm"), (20, "rescue"), (130, "rescue"), (200, "rescue")])
def test_the_set_reaches_every_new_kernel(solver, S, kind):
    batch, sets, idx = paired(S, 4200 + S)
    if kind == "rescue":
        damage(batch, 0, GAP); damage(batch, 1, GAP)
        kw = dict(elastic=1, lean=-1)
    db = solver.upload(batch)
    if kind == "warm":
        first = call_sets(solver, db, sets, idx, keep=True)
        kw = dict(x0=solver.eval_states(db, tensor(solver, first["ctrl"]), joint_times(solver, batch.seg[L.F_T])), lam0=tensor(solver, first["lam"]),
                  keep=True)
    got = call_sets(solver, db, sets, idx, **kw)
    per_set(solver, db, sets, idx, got, (S, kind), KEYS, **kw)
    # (a status-1 solve has a KKT score below 1e-7: two solves of ONE problem differ by about that; 1e-4 is a different optimum)
    want = 2 if kind == "rescue" else 1
    pairs = [(0, 1)] if kind == "rescue" else [(b, b + 1) for b in (0, 2, 4)]
    diffs = [np.abs(got["ctrl"][a] - got["ctrl"][b]).max() for a, b in pairs if got["status"][a] == got["status"][b] == want]
    print("S=%d %s: statuses %s, the pairs' control points differ by %s" % (S, kind, got["status"].tolist(), diffs))
    assert diffs and max(diffs) > 1e-4, (got["status"], diffs)


# ---- 6. delegation --------------------------------------------------------------------------------------------------------------

def test_what_the_sets_solve_served_is_its_own(solver):
    import torch
    cur = lambda: torch.cuda.current_stream(solver.device).cuda_stream

    def old(rec, sets, idx, keep, x0=None, lam0=None):
        r = solver._record(rec)
        o, lam = prefilled(solver, r, keep)
        solver.ctx.solve_sets_device(r.B, r.S, sets, tensor(solver, idx), r.seg, r.seg_count, r.init, r.ref_end, r.dl_bounds, o["ctrl"], o["cost"],
                                     o["status"], o["iters"], x0=x0, lam0=lam0, lam_out=lam, stream=cur(), cap_iter=-1)
        return finish(solver, o, lam, 0, r.B)

    # beyond 64 segments without a warm argument: the cold long form (2), not the warm one
    batch, sets, idx, bad = uniform_case(100, rescue=False)
    db = solver.upload(batch)
    mine, theirs = call_sets(solver, db, sets, idx), old(db, sets, idx, False)
    assert mine["form"] == theirs["form"] == 2
    assert_rows(mine, theirs, np.arange(batch.B), "cold 100")
    # up to 64 segments with warm arguments, uniform and ragged
    batch, sets, idx, bad = uniform_case(20, B=40, rescue=False)
    db = solver.upload(batch)
    first = old(db, sets, idx, True)
    lam = tensor(solver, first["lam"])
    ctrl = tensor(solver, first["ctrl"]); ctrl[bad] = ctrl[0]
    x0 = solver.eval_states(db, ctrl, joint_times(solver, batch.seg[L.F_T]))
    mine, theirs = call_sets(solver, db, sets, idx, x0=x0, lam0=lam, keep=True), old(db, sets, idx, True, x0=x0, lam0=lam)
    assert mine["form"] == theirs["form"]
    assert_rows(mine, theirs, np.arange(batch.B), "warm 20", KEYS + ("lam",))
    cnt = (1 + np.arange(batch.B) % 20).astype(np.int32)
    rec = dict(B=batch.B, seg_stride=20, seg=db.seg, seg_count=tensor(solver, cnt), init=db.init, ref_end=db.ref_end, dl_bounds=db.dl_bounds)
    for keep in (False, True):
        mine, theirs = call_sets(solver, rec, sets, idx, keep=keep), old(rec, sets, idx, keep)
        assert mine["form"] == theirs["form"]
        assert_rows(mine, theirs, np.arange(batch.B), ("ragged 20", keep), KEYS + (("lam",) if keep else ()))


# ---- 7. n_sets = 1024 -----------------------------------------------------------------------------------------------------------

def test_a_thousand_sets_on_a_ragged_record(solver):
    B, st, G = 2048, 32, 1024
    batch, sh = synth.make_scenario1_batch(B, st, 0, seed=4300)
    batch = copy_batch(batch)
    hit = np.arange(5, B, 257)
    for b in hit:
        damage(batch, b, GAP)
    cnt = (8 + (np.arange(B) * 7) % 25).astype(np.int32)                  # 8..32
    sets = [dataclasses.replace(sh, ds_ref=sh.ds_ref + 0.001 * g) for g in range(G)]
    idx = (np.arange(B) % G).astype(np.int32)
    db = solver.upload(batch)
    rec = dict(B=B, seg_stride=st, seg=db.seg, seg_count=tensor(solver, cnt), init=db.init, ref_end=db.ref_end, dl_bounds=db.dl_bounds)
    got = call_sets(solver, rec, sets, idx, elastic=1, lean=-1)
    print("1024 sets: statuses", np.unique(got["status"], return_counts=True), "damaged", got["status"][hit].tolist())
    assert (got["status"][hit] == 2).any() and 2 * (got["status"] == 1).sum() >= B
    sample = list(hit) + [0, 1, 31, 1023, 1024, 2047, 700, 1500]
    for b in sample[:16]:
        ref = solver.solve_ragged(rec, sets[idx[b]], elastic=1, cap_iter=-1, lean=-1)
        ref = finish(solver, ref, None, 1, B)
        n = 12 * cnt[b]
        assert np.array_equal(bits(got["ctrl"][b, :n]), bits(ref["ctrl"][b, :n])) and (got["ctrl"][b, n:] == FILL).all(), b
        assert_rows(got, ref, np.array([b]), ("1024 sets", b), ("cost", "status", "iters", "viol"))


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_argument(solver):
    import torch
    batch, sets, idx, bad = uniform_case(70, B=4, rescue=False)
    idx[bad] = 1
    db = solver.upload(batch)
    o = solver.new_result(4, 70)
    it = tensor(solver, idx)
    args = [4, 70, sets, it, db.seg, None, db.init, db.ref_end, db.dl_bounds, o["ctrl"], o["cost"], o["status"], o["iters"]]
    entry = solver.ctx.solve_long_sets_device
    for kw, word in ((dict(elastic=2), "elastic"), (dict(elastic=-1), "elastic"), (dict(cap_iter=6), "cap_iter"), (dict(compact=1), "compact")):
        with pytest.raises(native.BtrapzError, match=word):
            entry(*args, **kw)
    l = native.lib()
    opt = native._options(); opt.queue = 1
    cs = native._sets_array(sets)
    raw = lambda o_, n_sets=len(sets), sets_=cs, B=4, S=70, seg=db.seg, index=it, status=o["status"]: l.btrapz_solve_long_sets_device(
        solver.ctx._h, sets_, n_sets, native._ptr(index), o_, None, B, S, native._ptr(seg), None, native._ptr(db.init), native._ptr(db.ref_end),
        native._ptr(db.dl_bounds), native._ptr(o["ctrl"]), native._ptr(o["cost"]), native._ptr(status), native._ptr(o["iters"]), None)
    err = lambda: l.btrapz_last_error(solver.ctx._h).decode()
    import ctypes as C
    assert raw(C.byref(opt)) == -1 and "queue" in err()
    opt = native._options(); opt.start = 1
    assert raw(C.byref(opt)) == -1 and "start" in err()
    assert raw(None, n_sets=0) == -1 and "n_sets" in err()
    assert raw(None, n_sets=1 << 20) == -1 and "n_sets" in err()
    assert raw(None, sets_=None) == -1 and "sets is NULL" in err()
    assert raw(None, index=None) == -1 and "set_index is NULL" in err()
    assert raw(None, seg=None) == -1 and "seg is NULL" in err()
    assert raw(None, status=None) == -1 and "status is NULL" in err()
    assert raw(None, B=0) == -1 and "B < 1" in err()
    assert raw(None, S=0) == -1 and "seg_stride < 1" in err()
    assert raw(None, S=257) == -1 and "seg_stride" in err()
    with pytest.raises(native.BtrapzError, match="variant and delta"):
        entry(*args[:2], [sets[0], dataclasses.replace(sets[1], delta=0.2)], *args[3:])
    # the older call refuses what it refused
    with pytest.raises(native.BtrapzError, match="elastic"):
        solver.ctx.solve_sets_device(*args, elastic=1)
    with pytest.raises(native.BtrapzError, match="more than 64 segments"):
        solver.ctx.solve_sets_device(*args, lam_out=torch.empty((2, 36, 4, 70), dtype=torch.float64, device=solver.device))
    # iters may be NULL; and the arguments as they are: served
    o["status"].fill_(-99)
    entry(*args[:12], None, elastic=1)
    torch.cuda.synchronize()
    assert (o["status"].cpu().numpy() != -99).all(), o["status"]


# ---- 9. oracle anchor -----------------------------------------------------------------------------------------------------------

def test_oracle_anchor_at_193_segments(solver):
    gold = np.load(R.G.OUT)
    S = 193
    batch, sh = R.seam(gold, S)
    sets = [dataclasses.replace(sh, ds_ref=sh.ds_ref + 1.0), sh]
    idx = np.array([1, 1, 0, 1, 1], dtype=np.int32)
    got = call_sets(solver, solver.upload(batch), sets, idx, elastic=1)
    assert got["form"] == 16
    seen = R.check_decisions(S, got, batch, sh, gold["x_%d" % S], gold["viol_%d" % S], [b for b in range(batch.B) if idx[b] == 1], "sets")
    assert seen[0] >= 1, seen


# ---- 10. diff.solve_long_sets / solve_long_sets_jacobian ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [65, 129])
def test_diff_solve_long_with_sets(solver, S):
    """diff.solve_long and diff.solve_long_jacobian keep their signatures (tests/test_long_grad_abi.py pins them without
    set_index): the sets form has names of its own, diff.solve_long_sets and diff.solve_long_sets_jacobian."""
    import torch
    from spectral_amd import diff
    B = 6
    batch, sh = synth.make_batch(B, S, config=2, seed=500 + S)
    dev = solver.device
    row = sh.as_array()[:20].copy()
    row2 = row.copy(); row2[:8] *= 1.2
    params = torch.tensor(np.stack([row, row2]), dtype=torch.float64, device=dev)
    idx = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
    set_index = torch.tensor(idx, device=dev)
    rng = np.random.default_rng(S)
    xbar = torch.tensor(rng.standard_normal((B, 12 * S)), device=dev); cbar = torch.tensor(rng.standard_normal(B), device=dev)

    def grads(p, **kw):
        seg = torch.tensor(batch.seg, device=dev, requires_grad=True); init = torch.tensor(batch.init, device=dev, requires_grad=True)
        p = p.clone().requires_grad_(True)
        fn = diff.solve_long_sets if kw else diff.solve_long       # (one parameter row: the function that was there)
        ctrl, cost, status = fn(solver, seg, init, torch.tensor(batch.ref_end, device=dev), torch.tensor(batch.dl_bounds, device=dev), p,
                                variant=sh.variant, delta=sh.delta, **kw)
        ((ctrl * xbar).sum() + (cost * cbar).sum()).backward()
        torch.cuda.synchronize()
        return (ctrl.detach().cpu().numpy(), cost.detach().cpu().numpy(), status.cpu().numpy(), seg.grad.cpu().numpy(), init.grad.cpu().numpy(),
                p.grad.cpu().numpy())

    ctrl, cost, status, gseg, ginit, gp = grads(params, set_index=set_index)
    assert (status > 0).sum() >= 4, status
    cols = [0, 5, 10, 16]
    args = [torch.tensor(a, device=dev) for a in (batch.seg, batch.init, batch.ref_end, batch.dl_bounds)]
    jac = diff.solve_long_sets_jacobian(solver, *args, params, cols, set_index=set_index, variant=sh.variant, delta=sh.delta)
    for g in range(2):
        c1, k1, s1, gs1, gi1, gp1 = grads(params[g])
        sel = idx == g
        assert np.array_equal(ctrl[sel], c1[sel]) and np.array_equal(cost[sel], k1[sel]) and np.array_equal(status[sel], s1[sel]), g
        assert np.array_equal(gseg[:, sel], gs1[:, sel]) and np.array_equal(ginit[sel], gi1[sel]), g
        # the parameter row of set g: the sum of ITS candidates' rows of the one-set backward pass.  The sum runs in another order
        # (index_add_ against sum): three terms, two roundings either way -- 2 x 2^-52 x sum |row|, the one bound here that is not 0.
        db = solver.upload(batch)
        shg = diff.shared_from_params(params[g].cpu().numpy(), sh.variant, sh.delta)
        og = {k: v.clone() for k, v in solver.solve_long(db, shg, keep_multipliers=True).items()}
        rows = solver.solve_long_vjp(db, shg, og, xbar, cbar)["shared"].cpu().numpy()
        all_rows = 5.0 * 2.0 ** -52 * np.abs(rows).sum(0)               # (without the keyword: the sum over all six, the same way)
        assert (np.abs(rows.sum(0) - gp1) <= all_rows).all(), (g, rows.sum(0), gp1)
        want, bound = rows[sel].sum(0), 2.0 * 2.0 ** -52 * np.abs(rows[sel]).sum(0)
        print("S=%d set %d: |params grad| %.3e, difference to the per-set sum %.3e (bound %.3e)" % (S, g, np.abs(want).max(), np.abs(gp[g] - want).max(), bound.max()))
        assert (np.abs(gp[g] - want) <= bound).all(), (g, gp[g], want)
        m = torch.tensor(sel, device=dev)
        j1 = diff.solve_long_jacobian(solver, *args, params[g], cols, variant=sh.variant, delta=sh.delta)
        assert np.array_equal(jac["dctrl"][:, m].cpu().numpy(), j1["dctrl"][:, m].cpu().numpy()), g
        assert np.array_equal(jac["dcost"][:, m].cpu().numpy(), j1["dcost"][:, m].cpu().numpy()), g
    assert not np.array_equal(gp[0], gp[1])
