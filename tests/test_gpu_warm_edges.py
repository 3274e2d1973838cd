"""Warm starts (btrapz_solve_warm_device with x0 / lam0: the packed warm kernels of btrapz_kernels.hip, the lean ones of
btrapz_lean_warm.hip) at every edge of the lane mapping -- a single segment per group, the last lane of a group next to another
group's first, idle tail lanes (S = 5, 21), one group per wavefront from S = 33, a group that ends on lane 62, a full wavefront.
The cold solve is held to the oracle at these widths by test_gpu_parity.py / test_gpu_lean.py; the warm instantiations are
other kernels with a set-up of their own (per-lane reads of x0 [B][2][S][3] and lam0 [2][36][B][S], sanitising, slacks from the
gaps, the cold restart) and were only ever run at 10 and 20 segments.

A start read from the wrong slot, axis or row cannot change the optimum -- the QP is strictly convex -- it only costs
iterations.  So beside x* every case compares the iteration counts of three solves of ONE problem: cold, from its own
solution and multipliers, and from those of the NEXT candidate (x0 and lam rolled by one along B).  The right start must beat
both, strictly, on the mean over the accepted candidates; no number is fitted.

Batches: synth.make_batch(B, S, config=2, seed=500 + S), B = 3 * (64 // S) + 1 up to 32 segments and 7 beyond: several
wavefronts, the last one partial.  The cuboid variant joins at 3, 5 and 21 segments (beyond, the generic family leaves its
0 ... 100 m clamp and the oracle itself reports the candidates infeasible).

Mean iteration counts (iters[] over the accepted candidates) cold / right start / rolled start, one run on an MI355X:

    S   variant  B    form    cold   right  rolled
    1   0        193  packed   4.00   2.00    9.15
    2   0        97   packed   5.09   2.26    9.15
    3   0        64   packed   4.89   2.00    7.78
    3   0        64   lean     4.89   2.00    7.81
    5   0        37   packed   5.46   2.00    7.86
    5   0        37   lean     5.46   2.00    7.86
    21  0        10   packed   7.10   2.00   12.40
    21  0        10   lean     7.10   2.00   12.40
    32  0        7    packed   7.57   2.00   18.43
    32  0        7    lean     7.57   2.00   18.43
    33  0        7    packed   8.57   2.00   14.57
    33  0        7    lean     8.71   2.00   14.71
    63  0        7    packed  10.00   2.00   16.71
    63  0        7    lean    10.00   2.00   16.71
    64  0        7    packed  10.43   2.00   19.71
    64  0        7    lean    10.43   2.00   19.71
    3   1        64   packed   4.84   2.05    7.69
    3   1        64   lean     4.84   2.05    7.69
    5   1        37   packed   5.32   2.00    7.16
    5   1        37   lean     5.32   2.00    7.16
    21  1        10   packed   6.20   2.00    8.80
    21  1        10   lean     6.20   2.00    8.80
(the shifted problem: 3.2 ... 4.1 warm against 4.9 ... 10.9 cold at 3, 21, 33 and 64 segments, both forms)

Replaces the reference's fresh OSQP workspace per call (src/solve_3d.cc:1246, osqp_cleanup :1256) for the replanning loop."""
import numpy as np
import pytest

from helpers import O
from spectral_amd import layout as L
from spectral_amd import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-5
SIZES = (1, 2, 3, 5, 21, 32, 33, 63, 64)
SHAPES = [(S, 0) for S in SIZES] + [(S, 1) for S in (3, 5, 21)]
# uniform batches of one or two segments take the packed form whatever btrapz_options.lean says: once
CASES = [(S, v, lean) for S, v in SHAPES for lean in ((1,) if S <= 2 else (-1, 1))]


def batch_size(S):
    return 3 * (64 // S) + 1 if S <= 32 else 7


def expected_form(S, lean):
    return 8 if lean > 0 and S >= 3 else 0


def rel_err(ctrl, xs):
    return np.abs(ctrl - xs).max(axis=1) / np.abs(xs).max(axis=1)


_problems = {}


def problem(S, variant):
    """(batch, sh, n, xs, st): the batch of one shape and the oracle's exact solve of its first n = min(B, 4) candidates (3 from
    63 segments on), computed once and shared by every test of the shape."""
    if (S, variant) not in _problems:
        B = batch_size(S)
        batch, sh = synth.make_batch(B, S, config=2, variant=variant, seed=500 + S)
        n = min(B, 4) if S < 63 else 3
        xs, obj, st, _ = O.batch_solve(batch, sh, 0, n, exact=True, threads=n)
        assert (st == 1).sum() >= n - 1, (S, variant, st)
        _problems[(S, variant)] = (batch, sh, n, xs, st)
    return _problems[(S, variant)]


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def joint_times(batch, shift=0.0):
    import torch
    return torch.from_numpy(np.cumsum(batch.seg[L.F_T], axis=1) + shift)


def grab(solver, o):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in o.items() if k != "lam"}, solver.ctx.last_solve_form()


def assert_oracle(r, n, xs, st, what):
    for b in range(n):
        assert (st[b] > 0) == (r["status"][b] > 0), (what, b, st[b], r["status"][b])
    good = st > 0
    assert rel_err(r["ctrl"][:n][good], xs[good]).max() <= RTOL, (what, rel_err(r["ctrl"][:n][good], xs[good]))


@pytest.mark.parametrize("S,variant,lean", CASES)
def test_warm_start_at_every_width_same_optimum_fewer_iterations(solver, S, variant, lean):
    batch, sh, n, xs, st = problem(S, variant)
    db = solver.upload(batch)
    form = expected_form(S, lean)
    o = solver.solve(db, sh, keep_multipliers=True, lean=lean)
    lam = o["lam"].clone()
    cold, f = grab(solver, o)
    assert f == form
    x0 = solver.eval_states(db, o["ctrl"].clone(), joint_times(batch))
    warm, f = grab(solver, solver.solve(db, sh, warm=dict(x0=x0, lam=lam.clone()), lean=lean))
    assert f == form
    rolled, f = grab(solver, solver.solve(db, sh, warm=dict(x0=x0.roll(1, 0).contiguous(), lam=lam.roll(1, 2).contiguous()), lean=lean))
    assert f == form
    ok = cold["status"] > 0
    assert ok.sum() >= batch.B - 1
    # the same optimum whatever the start: accepted by all three, the oracle's x*, the cold solve's cost
    assert (warm["status"][ok] > 0).all() and (rolled["status"][ok] > 0).all()
    for what, r in (("cold", cold), ("warm", warm), ("rolled", rolled)):
        assert_oracle(r, n, xs, st, (S, variant, lean, what))
    assert rel_err(warm["ctrl"][ok], cold["ctrl"][ok]).max() <= RTOL and rel_err(rolled["ctrl"][ok], cold["ctrl"][ok]).max() <= RTOL
    assert np.abs(warm["cost"][ok] - cold["cost"][ok]).max() <= 1e-6 * (1 + np.abs(cold["cost"][ok]).max())
    # the iteration side: the start of THIS candidate is worth something, the next candidate's is not
    it_cold, it_right, it_rolled = (float(r["iters"][ok].mean()) for r in (cold, warm, rolled))
    print("iterations S=%d variant=%d form=%d B=%d: cold %.2f right %.2f rolled %.2f" % (S, variant, form, batch.B, it_cold, it_right, it_rolled))
    assert it_right < it_cold, (it_right, it_cold, it_rolled)
    assert it_right < it_rolled, (it_right, it_cold, it_rolled)


@pytest.mark.parametrize("S", [3, 21, 33, 64])
@pytest.mark.parametrize("lean", [-1, 1])
def test_warm_start_on_the_shifted_problem_at_the_edges(solver, S, lean):
    """One replanning step, as test_gpu_warm_start.py::test_warm_start_on_shifted_problem_matches_oracle: every line is
    evaluated 0.1 s later, the initial state advances along the previous solution; start = the previous trajectory 0.1 s
    later and the previous multipliers."""
    import torch
    d = 0.1
    batch, sh, _, _, _ = problem(S, 0)
    B = batch.B
    db = solver.upload(batch)
    prev = solver.solve(db, sh, keep_multipliers=True, lean=lean)
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
    cold, _ = grab(solver, solver.solve(ndb, sh, lean=lean))
    o = solver.solve(ndb, sh, warm=dict(x0=x0, lam=lam), keep_multipliers=True, lean=lean)
    warm, f = grab(solver, o)
    assert f == expected_form(S, lean)
    ok = cold["status"] > 0
    assert ok.any() and np.array_equal(warm["status"] > 0, ok), (cold["status"], warm["status"])
    xs, obj, st, _ = O.batch_solve(nb, sh, 0, 3, exact=True, threads=3)
    assert (st > 0).any()
    assert_oracle(warm, 3, xs, st, (S, lean, "shifted, warm"))
    assert_oracle(cold, 3, xs, st, (S, lean, "shifted, cold"))
    lam_new = o["lam"].cpu().numpy()[:, :, ok]
    assert np.isfinite(lam_new).all() and (lam_new >= 0).all()
    print("shifted S=%d lean=%d: iterations cold %.2f warm %.2f" % (S, lean, cold["iters"][ok].mean(), warm["iters"][ok].mean()))


COUNTS = (1, 2, 3, 5, 21, 32, 33, 63, 64)


@pytest.fixture(scope="module")
def ragged():
    """Every count in one batch of 64-segment slots: the first six candidates of each shape's batch, shuffled."""
    per, stride = 6, 64
    src = [(S, b) for S in COUNTS for b in range(per)]
    B = len(src)
    seg = np.zeros((L.NUM_SEG_FIELDS, B, stride)); cnt = np.zeros(B, dtype=np.int32)
    init = np.zeros((B, 6)); ref_end = np.zeros((B, 2)); dlb = np.zeros((B, 10))
    perm = np.random.default_rng(4).permutation(B)
    for dst, i in enumerate(perm):
        S, b = src[i]
        pb = problem(S, 0)[0]
        seg[:, dst, :S] = pb.seg[:, b, :]; cnt[dst] = S
        init[dst], ref_end[dst], dlb[dst] = pb.init[b], pb.ref_end[b], pb.dl_bounds[b]
    return dict(B=B, stride=stride, seg=seg, cnt=cnt, init=init, ref_end=ref_end, dlb=dlb, src=[src[i] for i in perm], sh=problem(1, 0)[1])


@pytest.mark.parametrize("lean", [-1, 1])
def test_ragged_warm_start_with_every_count_in_one_batch(solver, ragged, lean):
    """Through the C entry point: cold with lam_out, then warm from its own joint states and multipliers -- once as they are and
    once with NaN in every x0 / lam0 slot beyond a candidate's count.  A correct kernel never reads those: bit-equal results."""
    import torch
    dev = solver.device
    t = lambda a: torch.from_numpy(a).to(dev)
    B, st, sh = ragged["B"], ragged["stride"], ragged["sh"]
    rec = dict(B=B, seg_stride=st, seg=t(ragged["seg"]), seg_count=t(ragged["cnt"]), init=t(ragged["init"]), ref_end=t(ragged["ref_end"]),
               dl_bounds=t(ragged["dlb"]))
    ref = solver.solve_ragged(rec, sh, lean=lean, cap_iter=-1)
    torch.cuda.synchronize()
    assert solver.ctx.last_solve_form() == (8 if lean > 0 else 0)
    ref_status = ref["status"].cpu().numpy().copy()
    o = dict(ctrl=torch.zeros((B, 12 * st), dtype=torch.float64, device=dev), cost=torch.empty(B, dtype=torch.float64, device=dev),
             status=torch.empty(B, dtype=torch.int32, device=dev), iters=torch.empty(B, dtype=torch.int32, device=dev))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(x0, lam0, lam_out):
        o["ctrl"].zero_()
        solver.ctx.solve_warm_device(B, st, sh, rec["seg"], rec["seg_count"], rec["init"], rec["ref_end"], rec["dl_bounds"], o["ctrl"],
                                     o["cost"], o["status"], o["iters"], x0=x0, lam0=lam0, lam_out=lam_out, stream=stream, lean=lean)
        torch.cuda.synchronize()
        assert solver.ctx.last_solve_form() == (8 if lean > 0 else 0)
        return {k: v.cpu().numpy().copy() for k, v in o.items()}
    lam = torch.zeros((2, 36, B, st), dtype=torch.float64, device=dev)
    cold = call(None, None, lam)
    assert np.array_equal(cold["status"], ref_status)
    ok = cold["status"] > 0
    assert ok.sum() >= B - len(COUNTS)
    x0 = torch.empty((B, 2, st, 3), dtype=torch.float64, device=dev)
    times = torch.cumsum(rec["seg"][L.F_T], dim=1).contiguous()
    solver.ctx.eval_states_device(B, st, rec["seg_count"], rec["seg"], o["ctrl"], st, times, x0, stream=stream)
    warm = call(x0, lam.clone(), None)
    assert np.array_equal(warm["status"], ref_status)
    # the oracle's x* on two candidates per count, cold and warm
    seen = {S: 0 for S in COUNTS}
    for dst, (S, b) in enumerate(ragged["src"]):
        if b >= 2:
            continue
        _, _, n, xs, ost = problem(S, 0)
        assert (ost[b] > 0) == (warm["status"][dst] > 0), (S, b)
        if ost[b] > 0:
            for what, r in (("cold", cold), ("warm", warm)):
                assert np.abs(r["ctrl"][dst, :12 * S] - xs[b]).max() <= RTOL * np.abs(xs[b]).max(), (what, S, b)
            seen[S] += 1
    assert all(v >= 1 for v in seen.values()) and sum(seen.values()) >= 2 * len(COUNTS) - 2, seen
    assert warm["iters"][ok].mean() < cold["iters"][ok].mean(), (warm["iters"][ok].mean(), cold["iters"][ok].mean())
    # slots beyond the count are nobody's: NaN there changes no bit
    beyond = torch.arange(st, device=dev)[None, :] >= rec["seg_count"][:, None].long()            # [B, st]
    x0n = x0.clone(); x0n[beyond[:, None, :].expand(B, 2, st)] = float("nan")
    lamn = lam.clone(); lamn[beyond[None, None].expand(2, 36, B, st)] = float("nan")
    assert torch.isnan(x0n).any() and torch.isnan(lamn).any()
    poisoned = call(x0n, lamn, None)
    for k in ("status", "iters", "cost", "ctrl"):
        assert np.array_equal(poisoned[k], warm[k], equal_nan=True), k


# ---- support of the kept multipliers ---------------------------------------------------------------------------------

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


@pytest.mark.parametrize("S,lean", [(2, 1), (21, -1), (21, 1), (64, -1), (64, 1)])
def test_support_of_the_kept_multipliers(solver, S, lean):
    """lam_out against the oracle's y on strictly complementary candidates: an entry is above 1e-6 of the candidate's largest
    multiplier exactly where the oracle has the row active on that side.  Only the pattern -- the kernel's row scaling is not
    part of the interface.  A multiplier stored under the wrong row, segment, axis or candidate shows here."""
    import torch
    from vjp_reference import Adjoint, one
    batch, sh, _, _, _ = problem(S, 0)
    o = solver.solve(solver.upload(batch), sh, keep_multipliers=True, lean=lean)
    torch.cuda.synchronize()
    assert solver.ctx.last_solve_form() == expected_form(S, lean)
    lam = o["lam"].cpu().numpy()                     # [2][36][B][S]
    status = o["status"].cpu().numpy()
    compared = 0
    for b in range(batch.B):
        adj = _adjoint(S, b, lambda: Adjoint(one(batch, b), sh, np.zeros(12 * S), 0.0))
        if not adj.strict or status[b] <= 0:
            continue
        want = merge_joint_rows(oracle_support(adj, S))
        if not want.any():                           # (short horizons: a candidate that touches no row says little)
            continue
        lb = lam[:, :, b, :]                         # [2][36][S]
        got = merge_joint_rows(np.stack([lb[:, :18], lb[:, 18:]]) > 1e-6 * lb.max())
        print("support S=%d lean=%d b=%d: %d active rows, %d entries differ" % (S, lean, b, want.sum(), (got != want).sum()))
        assert np.array_equal(got, want), (S, lean, b, np.argwhere(got != want)[:8])
        compared += 1
        if compared == 2:
            break
    assert compared >= 2, (S, compared)


_adjoints = {}


def _adjoint(S, b, make):
    if (S, b) not in _adjoints:
        _adjoints[(S, b)] = make()
    return _adjoints[(S, b)]
