"""The forwards of the sampling and of the state evaluation on the GPU -- sample_kernel behind btrapz_sample_device /
btrapz_sample_ragged_device (its body also samples inside find_traj's single-candidate kernels) and eval_states_kernel
behind btrapz_eval_states_device -- against the exact yardstick of tests/exact_reference.py (held to the older
yardsticks on the CPU by tests/test_exact_reference.py), at every width where a lane or slot mapping of the library has an
edge, uniform and ragged, on the batches of tests/forward_cases.py.

The entry points are called directly (BatchSolver.sample zero-fills `out` and picks max_points itself).  out, npoints
and x lie between guard zones and are prefilled with a NaN of a recognisable bit pattern: everything a call should not
have touched is compared bit by bit.  The bound is exact_reference.REL = 1e-13 of the entry's scale, derived there."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact_reference as X
import forward_cases as FC
import states_reference as R
from acost_reference import sample_count
from spectral_amd import knots, layout as L, native, synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
W = np.loadtxt(os.path.join(GOLD, "inputs", "weights.txt"))
SENT = 0x7ff8dead0000beef          # a quiet NaN no arithmetic produces
NP_SENT = -0x21524111
GUARD = 96                         # doubles in front of and behind every output
SEL = [3, 0, 3, 5, -1, 6, 1, 2, 4]   # repeats, and indices outside [0, B) for B = 6
BITS = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def dev(solver, a, dtype=torch.float64):
    return torch.from_numpy(np.array(a)).to(solver.device, dtype=dtype).contiguous()   # (a copy: the cases are read-only)


def ratio(err, scale):
    return float((err / np.maximum(scale, 1e-300)).max()) if err.size else 0.0


def guarded(solver, n, fill, dtype):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=solver.device)
    return buf, buf[GUARD:GUARD + n]


def unguard(buf, n, fill):
    a = buf.cpu().numpy()
    assert (a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all(), "a write outside the output"
    return a[GUARD:GUARD + n]


def filled(a, fill):
    """The NaN slots beyond the candidates' counts replaced (another garbage: must change no bit of any result)."""
    a = np.array(a)
    a[np.isnan(a)] = fill
    return a


def call_sample(solver, case, cnt, sel, max_points, garbage=None):
    """One call of btrapz_sample_device (cnt is None) or btrapz_sample_ragged_device on sentinel-filled outputs:
    (bits of out [nsel, 6, max_points] as int64, npoints [nsel])."""
    seg, ctrl = (case["seg"], case["ctrl"]) if garbage is None else (filled(case["seg"], garbage), filled(case["ctrl"], garbage))
    n = len(sel) * 6 * max_points
    obuf, out = guarded(solver, n, SENT, torch.int64)
    nbuf, npts = guarded(solver, len(sel), NP_SENT, torch.int32)
    args = (dev(solver, seg), dev(solver, case["init"]), dev(solver, ctrl), dev(solver, sel, torch.int64), max_points,
            out.view(torch.float64), npts)
    if cnt is None:
        solver.ctx.sample_device(case["B"], case["S"], FC.DELTA, *args)
    else:
        solver.ctx.sample_ragged_device(case["B"], case["S"], dev(solver, cnt, torch.int32), FC.DELTA, *args)
    torch.cuda.synchronize()
    return unguard(obuf, n, SENT).reshape(len(sel), 6, max_points).copy(), unguard(nbuf, len(sel), NP_SENT).copy()


def call_states(solver, case, cnt, ctrl, times):
    """One call of btrapz_eval_states_device on a sentinel-filled x: its bits [B, 2, n_times, 3] as int64."""
    B, n_times = times.shape
    xbuf, x = guarded(solver, B * 6 * n_times, SENT, torch.int64)
    solver.ctx.eval_states_device(B, case["S"], None if cnt is None else dev(solver, cnt, torch.int32), dev(solver, case["seg"]),
                                  dev(solver, ctrl), n_times, dev(solver, times), x.view(torch.float64))
    torch.cuda.synchronize()
    return unguard(xbuf, B * 6 * n_times, SENT).reshape(B, 2, n_times, 3).copy()


# ---- sampling ---------------------------------------------------------------------------------------------------------
def valid(case, cnt, b):
    return 0 <= b < case["B"] and 1 <= FC.count_of(case, b, cnt) <= case["S"]


def check_sampling(solver, case, key, cnt, sel, max_points):
    """key: (S, ragged, family) of the case, or None when cnt is not the case's own (no exact check then: the rows of
    candidates with the case's own count are compared by the caller).  Returns (bits, npoints, worst ratio)."""
    bits, npts = call_sample(solver, case, cnt, sel, max_points)
    vals = bits.view(np.float64)
    worst = 0.0
    for j, b in enumerate(sel):
        if not valid(case, cnt, b):
            assert npts[j] == 0, (j, b)
            assert (bits[j] == SENT).all(), (j, b)      # a refused selection: its row is untouched
            continue
        n = FC.count_of(case, b, cnt)
        t = case["seg"][L.F_T, b, :n]
        npd, npi = sample_count(t, FC.DELTA)
        assert npts[j] == npd, (j, b, npts[j], npd, npi)
        assert np.array_equal(bits[j, :, 0], BITS(case["init"][b])), (j, b)
        w = min(npi - 1, max_points - 1)              # written samples beyond sample 0
        assert (bits[j, :, 1 + w:] == SENT).all(), (j, b)   # the rest of the row, and 1 + total .. npoints when np runs ahead
        assert (bits[j, :, 1:1 + w] != SENT).all(), (j, b)
        if key is not None and b in FC.checked(case):
            want, scale = FC.exact_samples_of(*key, b)
            err = np.abs(vals[j, :, 1:1 + w] - want[:, :w])
            assert (err <= X.REL * scale[:, :w]).all(), (j, b, ratio(err, scale[:, :w]))
            worst = max(worst, ratio(err, scale[:, :w]))
    for j, b in enumerate(sel):                        # a selection named twice has two identical rows
        for i in range(j):
            if sel[i] == b:
                assert np.array_equal(bits[i], bits[j]) and npts[i] == npts[j], (i, j, b)
    return bits, npts, worst


def cut_inside_a_segment(case, cnt, sel, max_points):
    """Does sample index max_points (the first one not written) follow a sample of its own segment, for a selection?"""
    for b in sel:
        if valid(case, cnt, b):
            sg = X.sample_segments(FC.durations(case, b), FC.DELTA)
            if max_points - 1 < len(sg) and sg[max_points - 1][1] >= 2:
                return True
    return False


@pytest.mark.parametrize("S", FC.WIDTHS)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("family", ["a", "b"])
def test_sampling_against_the_exact_yardstick(solver, S, ragged, family):
    same, ahead = FC.coverage(S, ragged)   # (sample_count alone; over both families of this width)
    assert same >= 1 and (ahead >= 1 or S < 2), (same, ahead)
    case = FC.layout(S, ragged, family)
    key, cnt, B = (S, ragged, family), case["cnt"], case["B"]
    assert SEL[5] == B
    full = max(sample_count(FC.durations(case, b), FC.DELTA)[0] for b in range(B))
    assert full // 2 >= 2 and cut_inside_a_segment(case, cnt, SEL, full // 2)
    worst = 0.0
    for max_points in (full + 2, full // 2, 1):
        bits, npts, w = check_sampling(solver, case, key, cnt, SEL, max_points)
        worst = max(worst, w)
        again, npts2 = call_sample(solver, case, cnt, SEL, max_points)
        assert np.array_equal(bits, again) and np.array_equal(npts, npts2)   # a second call: identical bits
        if not ragged:   # the uniform entry point and the ragged one with every count at the stride: identical bits
            other, npts3 = call_sample(solver, case, np.full(B, S, dtype=np.int32), SEL, max_points)
            assert np.array_equal(bits, other) and np.array_equal(npts, npts3)
        else:            # other garbage beyond the candidates' counts: identical bits
            other, npts3 = call_sample(solver, case, cnt, SEL, max_points, garbage=-3.25e7)
            assert np.array_equal(bits, other) and np.array_equal(npts, npts3)
    # a candidate without segments and one with one more than the stride: refused, the others as before
    bad = np.array(case["cnt"] if ragged else np.full(B, S), dtype=np.int32)
    bad[2], bad[5] = 0, S + 1
    bits, npts, _ = check_sampling(solver, case, key, cnt, SEL, full + 2)
    bits_bad, npts_bad, _ = check_sampling(solver, case, None, bad, SEL, full + 2)
    for j, b in enumerate(SEL):
        if b in (2, 5):
            assert npts_bad[j] == 0 and (bits_bad[j] == SENT).all()
        else:
            assert np.array_equal(bits_bad[j], bits[j]) and npts_bad[j] == npts[j]
    print("sampling S=%d ragged=%s family %s: worst err / scale = %.2e of the bound %.0e (%.3f)" %
          (S, ragged, family, worst, X.REL, worst / X.REL))


def test_the_wrappers_max_points_never_cuts_a_trajectory(solver):
    """BatchSolver.sample sizes `out` by floor(t / delta + 1e-9), another truncation than the kernel's: on family (b) at 64
    segments -- where the kernel's count runs ahead of its own int sum -- it is at least npoints for every candidate."""
    case = FC.layout(64, False, "b")
    rec = dict(B=case["B"], seg_stride=64, seg=dev(solver, case["seg"]), seg_count=None, init=dev(solver, case["init"]))
    out, npts = solver.sample(rec, dev(solver, case["ctrl"]), torch.arange(case["B"]), FC.DELTA)
    torch.cuda.synchronize()
    npts = npts.cpu().numpy()
    ahead = 0
    for b in range(case["B"]):
        npd, npi = sample_count(FC.durations(case, b), FC.DELTA)
        assert npts[b] == npd and out.shape[2] >= npd, (b, out.shape, npd)
        ahead += npd > npi
    assert ahead >= 1
    assert tuple(out.shape[:2]) == (case["B"], 6)


# ---- state evaluation -------------------------------------------------------------------------------------------------
def check_states(solver, case, times, exact_on):
    """eval_states on the case against exact_states for the candidates `exact_on`; returns (bits, worst ratio)."""
    cnt, B = case["cnt"], case["B"]
    bits = call_states(solver, case, cnt, case["ctrl"], times)
    vals = bits.view(np.float64)
    assert np.array_equal(bits, call_states(solver, case, cnt, case["ctrl"], times))   # a second call: identical bits
    if cnt is None:
        assert np.array_equal(bits, call_states(solver, case, np.full(B, case["S"], dtype=np.int32), case["ctrl"], times))
    else:   # other garbage beyond the candidates' counts
        other = dict(case, seg=filled(case["seg"], 4.5e9))
        assert np.array_equal(bits, call_states(solver, other, cnt, filled(case["ctrl"], -7.0e11), times))
    worst = 0.0
    for b in range(B):
        n, t = FC.count_of(case, b), FC.durations(case, b)
        c = case["ctrl"][b, :12 * n]
        # a time that is not > 0, NaN included: the start of the first segment, and the same bits for each of them
        c0 = [c[6 * n * ax:6 * n * ax + 3] for ax in range(2)]
        start = np.array([[p[0] * t[0], 5.0 * (p[1] - p[0]), 20.0 * (p[2] - 2.0 * p[1] + p[0]) / t[0]] for p in c0])
        scale0 = X.scale_states(t, c, [0.0])[:, 0]
        early = np.nonzero(~(times[b] > 0))[0]
        for j in early:
            assert (np.abs(vals[b, :, j] - start) <= X.REL * scale0).all(), (b, j, times[b, j])
            assert np.array_equal(bits[b, :, j], bits[b, :, early[0]]), (b, j, times[b, j])
        assert not np.isnan(vals[b]).any(), b
        if b in exact_on:
            want, scale = X.exact_states(t, c, times[b]), X.scale_states(t, c, times[b])
            err = np.abs(vals[b] - want)
            assert (err <= X.REL * scale).all(), (b, ratio(err, scale))
            worst = max(worst, ratio(err, scale))
    return bits, worst


@pytest.mark.parametrize("S", FC.WIDTHS)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("family", ["a", "b"])
def test_eval_states_against_the_exact_yardstick(solver, S, ragged, family):
    case = FC.layout(S, ragged, family)
    B = case["B"]
    times = FC.times_of(case)
    assert np.isnan(times).sum() == B and (times == 0.0).sum() == B and (times == -1.0).sum() == B
    bits, worst = check_states(solver, case, times, FC.checked(case))
    # independently of the float walk: the segment of the exact cumulative sums is the walk's, and the walk's located time
    # is the requested one to S 2^-52 horizon (tests/test_exact_reference.py has the argument)
    for b in FC.checked(case):
        t = FC.durations(case, b)
        joints = X.exact_joints(t)
        for k_made, tm in FC.interior_times(t):
            assert (times[b] == tm).any()
            k, rem = X.exact_segment(joints, tm)
            kw, remw, over, _ = R.walk(t, float(tm))
            assert kw == k == k_made and over == 0.0
            assert abs(Fraction(remw) - rem) <= Fraction(len(t) * 2.0 ** -52 * float(t.sum()))
    # a candidate without segments and one with one more than the stride: NaN everywhere, the neighbours as before
    bad = np.array(case["cnt"] if ragged else np.full(B, S), dtype=np.int32)
    bad[2], bad[5] = 0, S + 1
    bits_bad = call_states(solver, case, bad, case["ctrl"], times)
    for b in range(B):
        if b in (2, 5):
            assert np.isnan(bits_bad[b].view(np.float64)).all() and (bits_bad[b] != SENT).all()
        else:
            assert np.array_equal(bits_bad[b], bits[b])
    print("eval_states S=%d ragged=%s family %s n_times=%d: worst err / scale = %.2e of the bound %.0e (%.3f)" %
          (S, ragged, family, times.shape[1], worst, X.REL, worst / X.REL))


@pytest.mark.parametrize("B,n_times", [(6, 1), (5, 103)])
def test_eval_states_with_one_time_and_with_a_partial_last_block(solver, B, n_times):
    """n_times = 1, and B n_times = 515 threads: a partial third block of 256."""
    case = FC.layout(10, True, "b", B=B)
    times = FC.times_of(case, n_times=n_times, seed=n_times)
    assert times.shape == (B, n_times)
    _, worst = check_states(solver, case, times, range(B))
    print("eval_states B=%d n_times=%d: worst err / scale = %.2e" % (B, n_times, worst))


# ---- across kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", FC.WIDTHS)
def test_samples_are_the_states_at_their_times(solver, S):
    """Sample l < linter of segment k against eval_states at sum_{i<k} t_i + (l / linter) t_k (formed exactly, rounded once):
    within the sum of both bounds plus (|v|, |a|, |jerk|) <= (10 m, 80 m / t, 480 m / t^2) times the time error
    S 2^-52 horizon of the walk.  (l = linter is a joint: random control points are not continuous there, and the walk may
    leave the time on either side.)"""
    case = FC.layout(S, True, "b")
    B, cnt = case["B"], case["cnt"]
    full = max(sample_count(FC.durations(case, b), FC.DELTA)[0] for b in range(B))
    bits, npts = call_sample(solver, case, cnt, list(range(B)), full + 2)
    smp = bits.view(np.float64)
    per, where = [], []
    for b in range(B):
        t = FC.durations(case, b)
        joints = X.exact_joints(t)
        sg = X.sample_segments(t, FC.DELTA)
        rows = [(r, k, l, lin) for r, (k, l, lin) in enumerate(sg) if l < lin]
        per.append(np.array([float(joints[k] + Fraction(l, lin) * Fraction(float(t[k]))) for _, k, l, lin in rows]))
        where.append(rows)
    n = max(max(len(p) for p in per), 1)
    times = np.stack([np.concatenate([p, np.zeros(n - len(p))]) for p in per])
    x = call_states(solver, case, cnt, case["ctrl"], times).view(np.float64)
    worst, compared = 0.0, 0
    for b in range(B):
        nb, t = FC.count_of(case, b), FC.durations(case, b)
        dt = nb * 2.0 ** -52 * float(t.sum())
        for j, (r, k, l, lin) in enumerate(where[b]):
            kw, _, over, _ = R.walk(t, float(times[b, j]))
            assert kw == k and over == 0.0
            for ax in range(2):
                m = float(np.abs(case["ctrl"][b, 6 * nb * ax + 6 * k:6 * nb * ax + 6 * k + 6]).max())
                scale = np.array([m * t[k], 10 * m, 80 * m / t[k]])
                tol = 2 * X.REL * scale + np.array([10 * m, 80 * m / t[k], 480 * m / t[k] ** 2]) * dt
                err = np.abs(smp[b, 3 * ax:3 * ax + 3, 1 + r] - x[b, ax, j])
                assert (err <= tol).all(), (b, k, l, ax, err, tol)
                worst = max(worst, float((err / tol).max()))
                compared += 1
    assert compared >= (1 if S > 1 else 0)
    print("sample vs state S=%d: %d entries, worst err / bound = %.3f" % (S, compared, worst))


def test_find_traj_writes_the_batched_samplers_rows(solver):
    """Rows s, l, ds, dl, dds, ddl of find_traj's trajectory come from the same sample_candidate, run by 128 threads on
    durations in LDS: against btrapz_sample_ragged_device on the control points it returned, over the record of
    corridor_batch, within the yardstick's bound; the counts are equal."""
    compared, equal_bits = [], []
    for name in ("c1", "c2", "c3"):
        kb = knots.parse_corridor_file(os.path.join(GOLD, "inputs", name + ".txt"))
        for variant in (0, 1):
            cost, traj, ctrl = native.find_traj_mem(variant, list(W) + [1], kb)
            if cost >= 1e10:
                continue
            S = len(ctrl) // 12
            rec = solver.corridor_batch(kb, variant, seg_stride=max(S, 16))
            torch.cuda.synchronize()
            assert int(rec["seg_count"][0]) == S, (name, variant)
            stride = rec["seg_stride"]
            t = rec["seg"][L.F_T, 0, :S].cpu().numpy()
            init = rec["init"].cpu().numpy()
            seg = np.array(rec["seg"].cpu().numpy())
            seg[L.F_T, 0, S:] = np.nan
            c = np.full((1, 12 * stride), np.nan); c[0, :12 * S] = ctrl
            case = dict(B=1, S=stride, seg=seg, cnt=np.array([S], dtype=np.int32), ctrl=c, init=init)
            npd, npi = sample_count(t, kb.delta)
            assert FC.DELTA == kb.delta
            bits, npts = call_sample(solver, case, case["cnt"], [0], npd + 2)
            got = bits.view(np.float64)[0]
            assert npts[0] == npd == npi == traj.shape[1], (name, variant, npts[0], npd, npi, traj.shape)
            rows = np.stack([traj[1], traj[3], traj[5], traj[2], traj[4], traj[6]])
            assert np.array_equal(BITS(rows[:, 0]), BITS(init[0])) and np.array_equal(bits[0, :, 0], BITS(init[0]))
            want, scale = X.exact_samples(t, kb.delta, ctrl, S), X.scale_samples(t, kb.delta, ctrl, S)
            for what, a in (("find_traj", rows[:, 1:]), ("sample_ragged", got[:, 1:npi])):
                err = np.abs(a - want)
                assert (err <= X.REL * scale).all(), (name, variant, what, ratio(err, scale))
            err = np.abs(rows[:, 1:] - got[:, 1:npi])
            assert (err <= X.REL * scale).all(), (name, variant, ratio(err, scale))
            assert (bits[0, :, npi:] == SENT).all()
            compared.append((name, variant))
            equal_bits.append(np.array_equal(BITS(rows), bits[0, :, :npi]))
    print("find_traj vs sample_ragged: %s; bit for bit equal: %s" % (compared, equal_bits))
    assert len(compared) >= 4, compared


@pytest.mark.parametrize("S", FC.WIDTHS)
@pytest.mark.parametrize("ragged", [False, True])
def test_traj_cost_counts_the_samplers_points(solver, S, ragged):
    """On family (a), where the double-accumulated count equals 1 + the int sum, traj_cost scores every candidate and
    reports the sampler's npoints."""
    case = FC.layout(S, ragged, "a")
    B, cnt = case["B"], case["cnt"]
    _, npts = call_sample(solver, case, cnt, list(range(B)), 1)
    rec = dict(B=B, seg_stride=S, seg=dev(solver, filled(case["seg"], 1.0)), init=dev(solver, case["init"]),
               seg_count=None if cnt is None else dev(solver, cnt, torch.int32))
    rng = np.random.default_rng(S)
    N = 50
    cost, n_points = solver.traj_cost(rec, synth.shared_params(0, delta=FC.DELTA), dev(solver, filled(case["ctrl"], 0.0)),
                                      np.cumsum(rng.random(N)), rng.standard_normal(N))
    torch.cuda.synchronize()
    for b in range(B):
        npd, npi = sample_count(FC.durations(case, b), FC.DELTA)
        assert npd == npi == npts[b] == int(n_points[b]), (b, npd, npi, npts[b], int(n_points[b]))
    assert torch.isfinite(cost).all()
