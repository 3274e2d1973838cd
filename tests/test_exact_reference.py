"""The exact yardstick of the sampling and state-evaluation forwards (tests/exact_reference.py) on the CPU, held to the
older yardsticks before anything on a GPU relies on it: the NumPy forwards of tests/states_reference.py, the oracle's
orc_sample (which restates the reference with pow()) and the Bezier closed form.  All within the bound the kernels are
held to, 1e-13 of the scale of exact_reference.py: every side but the exact one is a float64 evaluation of the same sums."""
import os
from fractions import Fraction

import numpy as np
import pytest

import exact_reference as X
import forward_cases as FC
import states_reference as R
from acost_reference import sample_count
from helpers import O
from test_gpu_warm_start import bezier_state

GOLD = os.path.join(os.path.dirname(__file__), "golden")
W = np.loadtxt(os.path.join(GOLD, "inputs", "weights.txt"))


def ratio(err, scale):
    return float((err / np.maximum(scale, 1e-300)).max()) if err.size else 0.0


@pytest.mark.parametrize("S", [1, 20, 256])
@pytest.mark.parametrize("family", ["a", "b"])
def test_exact_samples_against_the_numpy_forward(S, family):
    case = FC.layout(S, True, family)
    worst = 0.0
    for b in FC.checked(case):
        n, t = FC.count_of(case, b), FC.durations(case, b)
        want, scale = FC.exact_samples_of(S, True, family, b)
        npd, npi = sample_count(t, FC.DELTA)
        assert want.shape == (6, npi - 1)
        got, npts = R.sample_forward(t, FC.DELTA, case["ctrl"][b, :12 * n], case["init"][b], npi + 2)
        assert npts == npd and np.array_equal(got[:, 0], case["init"][b]) and (got[:, npi:] == 0).all()
        err = np.abs(got[:, 1:npi] - want)
        assert (err <= X.REL * scale).all(), (b, ratio(err, scale))
        worst = max(worst, ratio(err, scale))
    print("exact_samples vs states_reference.sample_forward S=%d family %s: worst err / scale = %.2e" % (S, family, worst))


@pytest.mark.parametrize("S", [1, 20, 256])
@pytest.mark.parametrize("family", ["a", "b"])
def test_exact_states_against_the_numpy_forward_and_the_bezier_formula(S, family):
    case = FC.layout(S, True, family)
    times = FC.times_of(case)
    worst = 0.0
    for b in FC.checked(case):
        n, t = FC.count_of(case, b), FC.durations(case, b)
        c = case["ctrl"][b, :12 * n]
        want, scale = X.exact_states(t, c, times[b]), X.scale_states(t, c, times[b])
        got = R.states_forward(t, c, times[b])
        err = np.abs(got - want)
        assert (err <= X.REL * scale).all(), (b, ratio(err, scale))
        worst = max(worst, ratio(err, scale))
        # the closed form, at the walk's own segment and local time
        for j, tm in enumerate(times[b]):
            k, rem, over, clamped = R.walk(t, float(tm))
            for ax in range(2):
                ck = c[6 * n * ax + 6 * k:6 * n * ax + 6 * k + 6]
                if over > 0.0:
                    e = bezier_state(ck, t[k], 1.0)
                    bz = np.array([e[0] + e[1] * over, e[1], 0.0])
                else:
                    bz = bezier_state(ck, t[k], rem / t[k])
                assert (np.abs(bz - want[ax, j]) <= X.REL * scale[ax, j]).all(), (b, j, ax, bz, want[ax, j])
            if clamped:   # a time that is not > 0, NaN included: the start of the first segment
                assert k == 0 and rem == 0.0
                assert np.array_equal(want[:, j], X.exact_states(t, c, [0.0])[:, 0])
    print("exact_states vs states_reference.states_forward S=%d family %s: worst err / scale = %.2e" % (S, family, worst))


@pytest.mark.parametrize("S", FC.WIDTHS)
def test_the_float_walk_finds_the_segment_of_the_exact_cumulative_sums(S):
    """Independently of the float walk: for the interior times, the segment the exact rational cumulative sums give is the
    one states_reference.walk picks, and the walk's located time differs from the requested one by at most
    S 2^-52 horizon (at most S - 1 subtractions, each rounded by at most 2^-53 of a value below the horizon)."""
    n_checked = 0
    for family in ("a", "b"):
        case = FC.layout(S, True, family)
        for b in range(case["B"]):
            t = FC.durations(case, b)
            bound = Fraction(len(t) * 2.0 ** -52 * float(t.sum()))
            joints = X.exact_joints(t)
            for k_made, tm in FC.interior_times(t):
                k, rem = X.exact_segment(joints, tm)
                kw, remw, over, clamped = R.walk(t, float(tm))
                assert kw == k == k_made and over == 0.0 and not clamped
                assert abs(Fraction(remw) - rem) <= bound
                n_checked += 1
    assert n_checked >= 2 * 2 * 2 * S   # (candidate 0 of both families has S segments)


def test_coverage_of_the_duration_families():
    """Every width >= 2 has a checked candidate whose double-accumulated count equals 1 + the int sum and one where it runs
    ahead; no segment has more than 150 samples; segments without samples lie in the middle and at the end."""
    for S in FC.WIDTHS:
        for ragged in (False, True):
            same, ahead = FC.coverage(S, ragged)
            assert same >= 1 and (ahead >= 1 or S < 2), (S, ragged, same, ahead)
    case = FC.layout(10, False, "b")
    shorts = [int(np.argmin(FC.durations(case, b))) for b in range(case["B"])]
    assert 9 in shorts and any(s < 9 for s in shorts)
    assert any(int(tk / FC.DELTA) == 149 for b in range(case["B"]) for tk in FC.durations(case, b))


@pytest.mark.parametrize("name", ["c1", "c2"])
@pytest.mark.parametrize("variant", [0, 1])
def test_exact_samples_against_the_oracle(name, variant):
    """orc_sample on the committed x* of the bundled corridors (the durations are the oracle's own corridor stage's)."""
    path = os.path.join(GOLD, "inputs", name + ".txt")
    inp = O.ParsedInput(path)
    cost, S, _, cubes, info = O.find_traj(variant, path, None, O.params_from_weights(W))
    ctrl = np.load(os.path.join(GOLD, "scenario_xstar.npz"))["%s/%d/xstar" % (name, variant)]
    assert cost < 1e10 and ctrl.shape == (12 * S,)
    t = np.array([c.t for c in cubes])
    rc, smp = O.sample(cubes, inp.delta, ctrl, inp.init_s, inp.init_l)
    assert rc == 0
    got = np.array([np.asarray(a, dtype=np.float64) for a in smp])
    want, scale = X.exact_samples(t, inp.delta, ctrl, S), X.scale_samples(t, inp.delta, ctrl, S)
    assert got.shape == (6, want.shape[1] + 1) == (6, sample_count(t, inp.delta)[0])
    assert np.array_equal(got[:, 0], np.concatenate([inp.init_s, inp.init_l]))
    err = np.abs(got[:, 1:] - want)
    assert (err <= X.REL * scale).all(), ratio(err, scale)
    print("exact_samples vs orc_sample %s variant %d (S=%d): worst err / scale = %.2e" % (name, variant, S, ratio(err, scale)))
