"""Warm starts and kept multipliers for candidates of 65..256 segments (btrapz_solve_long_warm_device, include/btrapz_hip_long.h:
ipm_solve_long_warm_kernel, the WARM instantiation of the long form in btrapz_kernels.hip -- one axis problem per workgroup of up
to four wavefronts), at every seam of the lane mapping: one lane in the second wavefront (65), a wavefront that ends on its last
lane but one / on its last lane / one lane into the next (127, 128, 129; 192, 193; 255, 256).

The yardstick of x* is the cold long solve of the same batch through the existing entry point (solver.solve: the code
tests/test_gpu_long.py holds to the oracle up to 256 segments); at 65 and 129 segments the oracle's dense exact solve is asked
too, on two candidates each (1 s and 8 s per candidate; 67 s at 256 -- hence not there).  Bounds: control points within 1e-5 of
|x|_inf (the project's parity bound), cost within 1e-6 (1 + |cost|).

As in tests/test_gpu_warm_edges.py a start read from the wrong slot, axis or row cannot change the optimum, only the iteration
count: every width compares cold, the start from the candidate's own solution and multipliers, and the start from the NEXT
candidate's.  The right start must beat both, strictly, on the mean over the accepted candidates.

Batches: synth.make_batch(5, S, config=3), and synth.make_scenario1_batch(5, 128, 0).

Mean iteration counts (iters[] over the accepted candidates) cold / right start / rolled start, one run on an MI355X:

    S    batch       cold   right  rolled
    65   generic      9.80   2.00   16.80
    127  generic     12.60   2.00   22.00
    128  generic     13.00   2.00   22.40
    129  generic     12.60   2.00   22.00
    192  generic     14.80   2.20   20.60
    193  generic     15.20   2.00   22.80
    255  generic     15.00   2.00   22.60
    256  generic     14.20   2.00   21.80
    128  scenario_1  10.20   2.00   10.20
(the cold column is also what the existing entry point takes on the same batch, count for count; the shifted problem: 5.40 /
5.80 / 5.60 warm against 10.00 / 13.00 / 14.20 cold at 65 / 129 / 256 segments; the ragged record: 2.00 warm against 10.89 cold
over all counts, 12.61 over the long candidates alone)
"""
import numpy as np
import pytest

from helpers import oracle_qp_from_batch
from spectral_amd import layout as L
from spectral_amd import native, synth

pytestmark = pytest.mark.gpu
RTOL = 1e-5
SEAMS = [("generic", S) for S in (65, 127, 128, 129, 192, 193, 255, 256)] + [("scenario1", 128)]
ORACLE_WIDTHS = (65, 129)


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


_problems, _oracle, _yard = {}, {}, {}


def problem(S, gen="generic"):
    if (gen, S) not in _problems:
        _problems[(gen, S)] = synth.make_scenario1_batch(5, S, 0) if gen == "scenario1" else synth.make_batch(5, S, config=3)
    return _problems[(gen, S)]


def oracle_x(batch, sh, key, b):
    """(accepted, x*) of candidate b by the oracle's dense exact solve, computed once per key."""
    if (key, b) not in _oracle:
        x, _, info = oracle_qp_from_batch(batch, sh, b).solve_exact(max_iter=120)
        _oracle[(key, b)] = (info.status in (1, 2), x)
    return _oracle[(key, b)]


def grab(solver, o):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in o.items()}, solver.ctx.last_solve_form()


def yardstick(solver, S, gen="generic"):
    """The cold long solve of the batch through the entry point that was there before (form 2), once per shape."""
    if (gen, S) not in _yard:
        batch, sh = problem(S, gen)
        r, f = grab(solver, solver.solve(solver.upload(batch), sh))
        assert f == 2
        _yard[(gen, S)] = r
    return _yard[(gen, S)]


def joint_times(batch, shift=0.0):
    import torch
    return torch.from_numpy(np.cumsum(batch.seg[L.F_T], axis=1) + shift)


def rel_err(ctrl, xs):
    return np.abs(ctrl - xs).max(axis=1) / np.abs(xs).max(axis=1)


def assert_same_optimum(r, yard, ok, what):
    assert (r["status"][ok] > 0).all(), (what, r["status"], yard["status"])
    err = rel_err(r["ctrl"][ok], yard["ctrl"][ok])
    assert err.max() <= RTOL, (what, err)
    assert (np.abs(r["cost"][ok] - yard["cost"][ok]) <= 1e-6 * (1 + np.abs(yard["cost"][ok]))).all(), (what, r["cost"], yard["cost"])


def assert_oracle(r, batch, sh, key, what, n=2):
    checked = 0
    for b in range(n):
        accepted, x = oracle_x(batch, sh, key, b)
        assert accepted == (r["status"][b] > 0), (what, b, r["status"][b])
        if accepted:
            assert np.abs(r["ctrl"][b] - x).max() <= RTOL * np.abs(x).max(), (what, b, np.abs(r["ctrl"][b] - x).max() / np.abs(x).max())
            checked += 1
    assert checked >= 1, what


@pytest.mark.parametrize("gen,S", SEAMS)
def test_warm_start_at_every_seam_same_optimum_fewer_iterations(solver, gen, S):
    batch, sh = problem(S, gen)
    yard = yardstick(solver, S, gen)
    db = solver.upload(batch)
    o = solver.solve_long(db, sh, keep_multipliers=True)
    lam = o["lam"].clone()
    cold, f = grab(solver, o)
    assert f == 16
    x0 = solver.eval_states(db, o["ctrl"].clone(), joint_times(batch))
    warm, f = grab(solver, solver.solve_long(db, sh, warm=dict(x0=x0, lam=lam.clone())))
    assert f == 16
    rolled, f = grab(solver, solver.solve_long(db, sh, warm=dict(x0=x0.roll(1, 0).contiguous(), lam=lam.roll(1, 2).contiguous())))
    assert f == 16
    ok = yard["status"] > 0
    assert ok.sum() >= 4, yard["status"]
    for what, r in (("cold", cold), ("warm", warm), ("rolled", rolled)):
        assert_same_optimum(r, yard, ok, (gen, S, what))
        if gen == "generic" and S in ORACLE_WIDTHS:
            assert_oracle(r, batch, sh, S, (S, what))
    it_cold, it_right, it_rolled = (float(r["iters"][ok].mean()) for r in (cold, warm, rolled))
    print("iterations S=%d %s: cold %.2f right %.2f rolled %.2f (cold, existing entry point: %.2f)" %
          (S, gen, it_cold, it_right, it_rolled, float(yard["iters"][ok].mean())))
    assert it_right < it_cold, (it_right, it_cold, it_rolled)
    assert it_right < it_rolled, (it_right, it_cold, it_rolled)


@pytest.mark.parametrize("S", [65, 129, 256])
def test_warm_start_on_the_shifted_problem(solver, S):
    """One replanning step, built as tests/test_gpu_warm_edges.py::test_warm_start_on_the_shifted_problem_at_the_edges builds it:
    every line is evaluated 0.1 s later, the initial state advances along the previous solution; start = the previous trajectory
    0.1 s later and the previous multipliers."""
    import torch
    d = 0.1
    batch, sh = problem(S)
    B = batch.B
    db = solver.upload(batch)
    prev = solver.solve_long(db, sh, keep_multipliers=True)
    p_ctrl, lam = prev["ctrl"].clone(), prev["lam"].clone()
    x0 = solver.eval_states(db, p_ctrl, joint_times(batch, d))
    new_init = solver.eval_states(db, p_ctrl, torch.full((B, 1), d, dtype=torch.float64)).cpu().numpy()   # [B, 2, 1, 3]
    nb = batch.slice(0, B)
    seg = nb.seg.copy()
    for bias, skew in ((L.F_DOWN_BIAS, L.F_DOWN_SKEW), (L.F_UPP_BIAS, L.F_UPP_SKEW), (L.F_L_DOWN_BIAS, L.F_L_DOWN_SKEW),
                       (L.F_L_UPP_BIAS, L.F_L_UPP_SKEW), (L.F_X_BIAS, L.F_X_SKEW), (L.F_Y_BIAS, L.F_Y_SKEW)):
        seg[bias] = seg[bias] + seg[skew] * d
    nb.seg = seg
    nb.init = np.concatenate([new_init[:, 0, 0], new_init[:, 1, 0]], axis=1)
    ndb = solver.upload(nb)
    cold, f = grab(solver, solver.solve(ndb, sh))
    assert f == 2
    o = solver.solve_long(ndb, sh, warm=dict(x0=x0, lam=lam), keep_multipliers=True)
    warm, f = grab(solver, o)
    assert f == 16
    ok = cold["status"] > 0
    assert ok.any() and np.array_equal(warm["status"] > 0, ok), (cold["status"], warm["status"])
    assert_same_optimum(warm, cold, ok, (S, "shifted, warm"))
    if S == 65:
        assert_oracle(warm, nb, sh, "shifted 65", (S, "shifted, warm"))
        assert_oracle(cold, nb, sh, "shifted 65", (S, "shifted, cold"))
    lam_new = warm["lam"][:, :, ok]
    assert np.isfinite(lam_new).all() and (lam_new >= 0).all()
    print("shifted S=%d: iterations cold %.2f warm %.2f" % (S, cold["iters"][ok].mean(), warm["iters"][ok].mean()))


@pytest.mark.parametrize("S", [65, 129])
def test_a_candidates_slot_does_not_depend_on_the_batch_around_it(solver, S):
    """The same five candidates as B = 5 and their first four as B = 4: the stride of a multiplier row (B * seg_stride) differs, so
    a wrong one shows.  Candidates 0..3: every output bit for bit, the cold call's and the warm call's."""
    batch, sh = problem(S)
    small = batch.slice(0, 4)
    small = L.Batch(B=4, S=S, seg=small.seg.copy(), init=small.init.copy(), ref_end=small.ref_end.copy(), dl_bounds=small.dl_bounds.copy())
    got = {}
    for n, bt in ((5, batch), (4, small)):
        db = solver.upload(bt)
        o = solver.solve_long(db, sh, keep_multipliers=True)
        lam = o["lam"].clone()
        cold, f = grab(solver, o)
        assert f == 16
        x0 = solver.eval_states(db, o["ctrl"].clone(), joint_times(bt))
        warm, f = grab(solver, solver.solve_long(db, sh, warm=dict(x0=x0, lam=lam), keep_multipliers=True))
        assert f == 16
        got[n] = (cold, warm)
    assert (got[5][0]["status"][:4] > 0).sum() >= 3
    for i, what in enumerate(("cold", "warm")):
        five, four = got[5][i], got[4][i]
        for k in ("ctrl", "cost", "status", "iters"):
            assert np.array_equal(five[k][:4], four[k]), (S, what, k)
        assert np.array_equal(five["lam"][:, :, :4], four["lam"]), (S, what, "lam")
        assert np.isfinite(four["lam"]).all()


# ---- support of the kept multipliers (oracle_support and merge_joint_rows: as in tests/test_gpu_warm_edges.py) --------------

ROW_OFFSET = {1: 0, 2: 6, 3: 11, 4: 15}     # coefficients per row -> first row of its class (header: 6 position, 5 velocity, 4 acceleration, 3 jerk)
JOINT_TWIN = {0: 5, 6: 10, 11: 14}          # include/btrapz_hip.h: a joint's bound stated by both segments is ONE row


def oracle_support(adj, S):
    """Boolean [2 sides][2 axes][18 rows][S]: where the oracle's y marks an inequality row active, lower / upper.  Which segment
    and which row of its 18 a row of the oracle's A is comes from A alone: the segment and control point of its first column,
    its class from the number of coefficients."""
    A, y = adj.A, adj.y
    ineq = (adj.u - adj.l) > 1e-12
    ymax = np.abs(y).max()
    out = np.zeros((2, 2, 18, S), dtype=bool)
    for i in np.nonzero(ineq)[0]:
        cols = np.nonzero(A[i])[0]
        j = cols[0]
        axis, k, cp = j // (6 * S), (j % (6 * S)) // 6, j % 6
        assert len(cols) in ROW_OFFSET and (cols == j + np.arange(len(cols))).all() and cp + len(cols) <= 6
        r = ROW_OFFSET[len(cols)] + cp
        if abs(y[i]) > 1e-6 * ymax:
            out[0 if y[i] < 0 else 1, axis, r, k] = True
    return out


def merge_joint_rows(sup):
    """The first position, velocity and acceleration row of segment k + 1 and the last of segment k bound one quantity
    (continuity); the interface counts them as one row (include/btrapz_hip.h, btrapz_solve_vjp_device).  Fold the pair."""
    sup = sup.copy()
    for r, twin in JOINT_TWIN.items():
        sup[:, :, twin, :-1] |= sup[:, :, r, 1:]
        sup[:, :, r, 1:] = False
    return sup


_adjoints = {}


@pytest.mark.parametrize("S", [65, 129])
def test_support_of_the_kept_multipliers(solver, S):
    """lam_out against the oracle's y on a strictly complementary accepted candidate that touches a row: an entry is above 1e-6 of
    the candidate's largest multiplier exactly where the oracle has the row active on that side -- the cold call's multipliers and
    those the warm call writes back.

    "Strictly complementary" with a margin the comparison can stand on.  The two sides of it do not hold the same "largest
    multiplier": the oracle's y includes the continuity rows (here 2 to 25 times the largest inequality multiplier), lam_out
    holds inequality rows only; and an interior-point multiplier of a row of slack s is y + mu / s, not y.  A row whose |y| is
    within two decades of the 1e-6 threshold -- between 1e-8 and 1e-4 of the largest inequality multiplier -- is active by one
    scale and inactive by the other: such a candidate is not compared.  make_batch(5, S, config=3), default seed, checked on
    the CPU: candidate 0 has one such row at both widths (65: s axis, segment 38, last position row, |y| = 5.7e-5 = 2.0e-6 of
    27.9 and 9.0e-8 of 636, slack 1.8e-3; 129: segment 80, |y| = 6.6e-5 = 2.1e-7 of 306, slack 1.1e-3 -- the one entry of each
    pattern on which the first run disagreed, its other 7 and 14 active rows matching), candidate 1 has none and 7 / 10 active
    rows: it is the one compared."""
    from vjp_reference import Adjoint, one
    batch, sh = problem(S)
    db = solver.upload(batch)
    o = solver.solve_long(db, sh, keep_multipliers=True)
    lam_t = o["lam"].clone()
    cold, _ = grab(solver, o)
    x0 = solver.eval_states(db, o["ctrl"].clone(), joint_times(batch))
    warm, _ = grab(solver, solver.solve_long(db, sh, warm=dict(x0=x0, lam=lam_t), keep_multipliers=True))
    compared = 0
    for b in range(batch.B):
        if cold["status"][b] <= 0:
            continue
        if (S, b) not in _adjoints:
            _adjoints[(S, b)] = Adjoint(one(batch, b), sh, np.zeros(12 * S), 0.0)
        adj = _adjoints[(S, b)]
        if not adj.strict or adj.status not in (1, 2):
            continue
        ratio = np.abs(adj.y[(adj.u - adj.l) > 1e-12])
        ratio = ratio / ratio.max()
        if ((ratio >= 1e-8) & (ratio <= 1e-4)).any():
            print("support S=%d b=%d: not compared, |y| / largest in the band: %s" % (S, b, np.sort(ratio[(ratio >= 1e-8) & (ratio <= 1e-4)])))
            continue
        want = merge_joint_rows(oracle_support(adj, S))
        if not want.any():
            continue
        for what, r in (("cold", cold), ("warm", warm)):
            lb = r["lam"][:, :, b, :]                    # [2][36][S]
            got = merge_joint_rows(np.stack([lb[:, :18], lb[:, 18:]]) > 1e-6 * lb.max())
            print("support S=%d %s b=%d: %d active rows, %d entries differ" % (S, what, b, want.sum(), (got != want).sum()))
            assert np.array_equal(got, want), (S, what, b, np.argwhere(got != want)[:8])
        compared += 1
        break                                            # (the oracle's dense solve and its adjoint: 10 s a candidate at 129)
    assert compared >= 1, (S, compared)


# ---- ragged --------------------------------------------------------------------------------------------------------------

COUNTS = (3, 33, 64, 65, 66, 128, 129, 200, 256)


@pytest.fixture(scope="module")
def ragged():
    """Every count in one record of 256-segment slots: the first three candidates of each width's batch, shuffled."""
    per, stride = 3, 256
    src = [(S, b) for S in COUNTS for b in range(per)]
    B = len(src)
    seg = np.zeros((L.NUM_SEG_FIELDS, B, stride)); cnt = np.zeros(B, dtype=np.int32)
    init = np.zeros((B, 6)); ref_end = np.zeros((B, 2)); dlb = np.zeros((B, 10))
    perm = np.random.default_rng(4).permutation(B)
    for dst, i in enumerate(perm):
        S, b = src[i]
        pb = problem(S)[0]
        seg[:, dst, :S] = pb.seg[:, b, :]; cnt[dst] = S
        init[dst], ref_end[dst], dlb[dst] = pb.init[b], pb.ref_end[b], pb.dl_bounds[b]
    return dict(B=B, stride=stride, seg=seg, cnt=cnt, init=init, ref_end=ref_end, dlb=dlb, src=[src[i] for i in perm], sh=problem(3)[1])


def test_ragged_record_with_short_and_long_candidates(solver, ragged):
    """Through the C entry point: cold with lam_out, then warm from its own joint states and multipliers -- once as they are and
    once with NaN in every x0 / lam0 slot beyond a candidate's count."""
    import torch
    dev = solver.device
    t = lambda a: torch.from_numpy(a).to(dev)
    B, st, sh = ragged["B"], ragged["stride"], ragged["sh"]
    rec = dict(B=B, seg_stride=st, seg=t(ragged["seg"]), seg_count=t(ragged["cnt"]), init=t(ragged["init"]), ref_end=t(ragged["ref_end"]),
               dl_bounds=t(ragged["dlb"]))
    ref_status = solver.solve_ragged(rec, sh)["status"].cpu().numpy().copy()
    o = dict(ctrl=torch.zeros((B, 12 * st), dtype=torch.float64, device=dev), cost=torch.empty(B, dtype=torch.float64, device=dev),
             status=torch.empty(B, dtype=torch.int32, device=dev), iters=torch.empty(B, dtype=torch.int32, device=dev))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(entry, x0, lam0, lam_out):
        o["ctrl"].zero_()
        entry(B, st, sh, rec["seg"], rec["seg_count"], rec["init"], rec["ref_end"], rec["dl_bounds"], o["ctrl"], o["cost"], o["status"],
              o["iters"], x0=x0, lam0=lam0, lam_out=lam_out, stream=stream)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in o.items()}, solver.ctx.last_solve_form()
    long_entry, short_entry = solver.ctx.solve_long_warm_device, solver.ctx.solve_warm_device
    lam = torch.zeros((2, 36, B, st), dtype=torch.float64, device=dev)
    cold, f = call(long_entry, None, None, lam)
    assert f & 16
    assert np.array_equal(cold["status"], ref_status)
    ok = cold["status"] > 0
    assert ok.sum() >= B - len(COUNTS)
    x0 = torch.empty((B, 2, st, 3), dtype=torch.float64, device=dev)
    times = torch.cumsum(rec["seg"][L.F_T], dim=1).contiguous()
    solver.ctx.eval_states_device(B, st, rec["seg_count"], rec["seg"], o["ctrl"], st, times, x0, stream=stream)
    warm, f = call(long_entry, x0, lam.clone(), None)
    assert f & 16
    assert np.array_equal(warm["status"], ref_status)
    # at most 64 segments: what btrapz_solve_warm_device returns for the same record, bit for bit (it leaves the others unsolved)
    lam_s = torch.zeros((2, 36, B, st), dtype=torch.float64, device=dev)
    s_cold, f = call(short_entry, None, None, lam_s)
    assert not f & 16
    s_warm, _ = call(short_entry, x0, lam_s.clone(), None)
    short = ragged["cnt"] <= 64
    assert short.sum() == 9 and (s_cold["status"][~short] == -5).all() and (s_warm["status"][~short] == -5).all()   # BTRAPZ_NO_CORRIDOR
    for mine, theirs in ((cold, s_cold), (warm, s_warm)):
        for k in ("ctrl", "cost", "status", "iters"):
            assert np.array_equal(mine[k][short], theirs[k][short]), k
    assert np.array_equal(lam.cpu().numpy()[:, :, short], lam_s.cpu().numpy()[:, :, short])
    # beyond: the uniform cold solve of the candidate's own batch
    seen = 0
    for dst, (S, b) in enumerate(ragged["src"]):
        if S <= 64:
            continue
        yard = yardstick(solver, S)
        assert (yard["status"][b] > 0) == (warm["status"][dst] > 0), (S, b)
        if yard["status"][b] > 0:
            for what, r in (("cold", cold), ("warm", warm)):
                x = yard["ctrl"][b]
                assert np.abs(r["ctrl"][dst, :12 * S] - x).max() <= RTOL * np.abs(x).max(), (what, S, b)
                assert abs(r["cost"][dst] - yard["cost"][b]) <= 1e-6 * (1 + abs(yard["cost"][b])), (what, S, b)
                assert (r["ctrl"][dst, 12 * S:] == 0).all()
            seen += 1
    assert seen >= 18 - 6, seen
    it_cold, it_warm = cold["iters"][ok].mean(), warm["iters"][ok].mean()
    print("ragged: iterations cold %.2f warm %.2f (long candidates alone: %.2f / %.2f)" %
          (it_cold, it_warm, cold["iters"][ok & ~short].mean(), warm["iters"][ok & ~short].mean()))
    assert it_warm < it_cold and warm["iters"][ok & ~short].mean() < cold["iters"][ok & ~short].mean()
    # slots beyond the count are nobody's: NaN there changes no bit
    beyond = torch.arange(st, device=dev)[None, :] >= rec["seg_count"][:, None].long()            # [B, st]
    x0n = x0.clone(); x0n[beyond[:, None, :].expand(B, 2, st)] = float("nan")
    lamn = lam.clone(); lamn[beyond[None, None].expand(2, 36, B, st)] = float("nan")
    assert torch.isnan(x0n).any() and torch.isnan(lamn).any()
    poisoned, _ = call(long_entry, x0n, lamn, None)
    for k in ("status", "iters", "cost", "ctrl"):
        assert np.array_equal(poisoned[k], warm[k], equal_nan=True), k


# ---- delegation and refusals -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [21, 64])
def test_up_to_64_segments_the_call_is_the_warm_solve(solver, S):
    batch, sh = synth.make_batch(7, S, config=2, seed=500 + S)
    db = solver.upload(batch)
    res = {}
    for name, fn in (("solve", solver.solve), ("solve_long", solver.solve_long)):
        o = fn(db, sh, keep_multipliers=True)
        lam = o["lam"].clone()
        cold, f_cold = grab(solver, o)
        x0 = solver.eval_states(db, o["ctrl"].clone(), joint_times(batch))
        warm, f_warm = grab(solver, fn(db, sh, warm=dict(x0=x0, lam=lam), keep_multipliers=True))
        res[name] = (cold, warm, f_cold, f_warm)
    assert res["solve"][2:] == res["solve_long"][2:] and not res["solve_long"][2] & 16
    assert (res["solve"][0]["status"] > 0).sum() >= 6
    for i in range(2):
        for k in ("ctrl", "cost", "status", "iters", "lam"):
            assert np.array_equal(res["solve"][i][k], res["solve_long"][i][k]), (S, i, k)


def test_refusals_and_the_cold_start_without_warm_arguments(solver):
    import torch
    big, sh = synth.make_batch(2, 257, config=3)
    with pytest.raises(native.BtrapzError):
        solver.solve_long(solver.upload(big), sh, keep_multipliers=True)
    batch, sh = synth.make_batch(2, 70, config=3)
    db = solver.upload(batch)
    o = solver.new_result(2, 70)
    args = (2, 70, sh, db.seg, None, db.init, db.ref_end, db.dl_bounds, o["ctrl"], o["cost"], o["status"], o["iters"])
    with pytest.raises(native.BtrapzError):
        solver.ctx.solve_long_warm_device(*args, elastic=1)
    with pytest.raises(native.BtrapzError):
        solver.ctx.solve_long_warm_device(*args[:3], None, *args[4:])       # seg NULL
    with pytest.raises(native.BtrapzError):                                # the sibling still stops at 64
        solver.ctx.solve_warm_device(*args, lam_out=torch.zeros((2, 36, 2, 70), dtype=torch.float64, device=solver.device))
    # no warm arguments at all: the cold start, the same iterates as with the multipliers kept
    plain, f = grab(solver, solver.solve_long(db, sh))
    assert f == 16
    kept, f = grab(solver, solver.solve_long(db, sh, keep_multipliers=True))
    assert f == 16 and (kept["status"] > 0).all()
    for k in ("ctrl", "cost", "status", "iters"):
        assert np.array_equal(plain[k], kept[k]), k
