"""Exact restatement of the two forwards from control points to what a caller looks at -- sample_kernel
(btrapz_sample_device / btrapz_sample_ragged_device, and find_traj's own sampling) and eval_states_kernel
(btrapz_eval_states_device) -- in rational arithmetic over the inputs' float64 values.  Nothing is rounded before the
final float(): what the kernels are held to is the value itself, not another float64 evaluation of it.

What is part of the functions' DEFINITION, and therefore taken over in floating point, not recomputed:
  * linter = int(t_k / delta), the float truncation of solve_3d.cc:1351 (and the counts of acost_reference.sample_count);
  * the segment a time falls in, the time left inside it and the time beyond the horizon: the float walk
    `while k < S - 1 and rem > t[k]` of states_reference.walk.
Everything after that -- tau = l / linter or rem / t_k, the Bernstein sums, the scaling by the duration -- is exact.
Conventions are the kernels': position is the Bernstein sum TIMES the duration, velocity is unscaled, acceleration is
DIVIDED by the duration; a candidate's control points lie at [0, 6 S) (s axis) and [6 S, 12 S) (l axis).

The scale of the tolerance per written entry (scale_samples / scale_states), with m = max |c| over the six control
points of the entry's segment and axis: position m t_k (+ 10 m over beyond the horizon), velocity 10 m, acceleration
80 m / t_k -- the Bernstein bases sum to 1, so |5 dc| <= 10 m and |20 d2c| <= 80 m.  A kernel is held to
REL = 1e-13 times that scale, which is derived, not measured: an entry is at most 6 terms of at most 12 roundings each,
plus the sum and the scaling, gamma_25 = 2.8e-15; the rounding of tau, and of 1 - tau by at most 2^-53 absolute, moves a
degree-5 Bernstein sum by at most 5 * 2 * 2^-53 m each; together below 5e-15 of the scale.  1e-13 leaves a factor 20 for
FMA contraction and summation order (the margin tests/test_gpu_states.py argues for).  A wrong slot, axis offset,
binomial coefficient or segment on random control points misses by O(1) of the scale."""
from bisect import bisect_left
from fractions import Fraction
from math import comb

import numpy as np

from acost_reference import sample_count
from states_reference import walk

REL = 1e-13
BC0, BC1, BC2 = [comb(5, i) for i in range(6)], [comb(4, i) for i in range(5)], [comb(3, i) for i in range(4)]


def _sums(c, num, den):
    """The three Bernstein sums of one segment and axis at tau = num / den (integers, or a Fraction over 1) -- position
    before the factor t, velocity, acceleration before the factor 1 / t -- for c: the 6 control points as Fractions."""
    tau = Fraction(num) / Fraction(den)
    om = 1 - tau
    pw = [tau ** i for i in range(6)]
    qw = [om ** i for i in range(6)]
    p = sum(c[i] * BC0[i] * pw[i] * qw[5 - i] for i in range(6))
    v = sum(5 * (c[i + 1] - c[i]) * BC1[i] * pw[i] * qw[4 - i] for i in range(5))
    a = sum(20 * (c[i + 2] - 2 * c[i + 1] + c[i]) * BC2[i] * pw[i] * qw[3 - i] for i in range(4))
    return p, v, a


def _points(ctrl, S, ax, k):
    return [Fraction(float(v)) for v in ctrl[6 * S * ax + 6 * k:6 * S * ax + 6 * k + 6]]


def _m(ctrl, S, ax, k):
    return float(np.abs(np.asarray(ctrl[6 * S * ax + 6 * k:6 * S * ax + 6 * k + 6], dtype=np.float64)).max())


# ---- sampling ---------------------------------------------------------------------------------------------------------
def exact_samples(t, delta, ctrl, S):
    """Samples 1 .. total of one candidate, [6, total] (s, ds, dds, l, dl, ddl): t its S durations, ctrl its row (only
    [0, 12 S) is read).  total = the int sum of acost_reference.sample_count, minus sample 0 (the initial state)."""
    assert len(t) == S
    total = sample_count(t, delta)[1] - 1
    out = np.zeros((6, total))
    r = 0
    for k in range(S):
        linter = int(t[k] / delta)
        if linter < 1:
            continue
        tk = Fraction(float(t[k]))
        cs = [_points(ctrl, S, ax, k) for ax in range(2)]
        for l in range(1, linter + 1):
            for ax in range(2):
                p, v, a = _sums(cs[ax], l, linter)
                out[3 * ax + 0, r] = float(p * tk)
                out[3 * ax + 1, r] = float(v)
                out[3 * ax + 2, r] = float(a / tk)
            r += 1
    assert r == total
    return out


def scale_samples(t, delta, ctrl, S):
    """The tolerance's scale of every entry of exact_samples, [6, total]."""
    total = sample_count(t, delta)[1] - 1
    out = np.zeros((6, total))
    r = 0
    for k in range(S):
        linter = max(int(t[k] / delta), 0)
        for ax in range(2):
            m = _m(ctrl, S, ax, k)
            out[3 * ax + 0, r:r + linter] = m * t[k]
            out[3 * ax + 1, r:r + linter] = 10 * m
            out[3 * ax + 2, r:r + linter] = 80 * m / t[k]
        r += linter
    return out


def sample_segments(t, delta):
    """(k, l, linter) of samples 1 .. total, in order."""
    return [(k, l, int(t[k] / delta)) for k in range(len(t)) for l in range(1, int(t[k] / delta) + 1)]


# ---- state evaluation -------------------------------------------------------------------------------------------------
def exact_states(t, ctrl, times):
    """x [2, n_times, 3] = (p, v, a) per axis of one candidate (t: its S durations; ctrl: its row) at `times`.  The
    segment, the time left in it and the time beyond the horizon are the float walk's (states_reference.walk); the
    evaluation at tau = rem / t_k -- or 1 beyond the horizon, where p continues at the end velocity and a = 0 -- is
    exact."""
    S = len(t)
    x = np.zeros((2, len(times), 3))
    for j, tm in enumerate(times):
        k, rem, over, _ = walk(t, float(tm))
        tk = Fraction(float(t[k]))
        for ax in range(2):
            c = _points(ctrl, S, ax, k)
            if over > 0.0:
                p, v, a = _sums(c, 1, 1)
                x[ax, j] = [float(p * tk + v * Fraction(over)), float(v), 0.0]
            else:
                p, v, a = _sums(c, Fraction(rem), tk)
                x[ax, j] = [float(p * tk), float(v), float(a / tk)]
    return x


def scale_states(t, ctrl, times):
    """The tolerance's scale of every entry of exact_states, [2, n_times, 3]; 0 for the acceleration beyond the horizon,
    which is the constant 0."""
    S = len(t)
    s = np.zeros((2, len(times), 3))
    for j, tm in enumerate(times):
        k, rem, over, _ = walk(t, float(tm))
        for ax in range(2):
            m = _m(ctrl, S, ax, k)
            s[ax, j] = [m * t[k] + 10 * m * over, 10 * m, 0.0 if over > 0.0 else 80 * m / t[k]]
    return s


def exact_joints(t):
    """The exact cumulative sums 0, t_0, t_0 + t_1, ... of the durations."""
    joints = [Fraction(0)]
    for tk in t:
        joints.append(joints[-1] + Fraction(float(tk)))
    return joints


def exact_segment(joints, time):
    """The segment a time > 0 falls in by the EXACT cumulative sums of the durations (exact_joints): the first k with
    time <= t_0 + ... + t_k, the last segment beyond the horizon; and the exact time left inside it.  Independent of the
    float walk."""
    tm = Fraction(float(time))
    k = min(max(bisect_left(joints, tm) - 1, 0), len(joints) - 2)
    return k, tm - joints[k]
