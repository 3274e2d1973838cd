"""The batches on which the forwards of the sampling and of the state evaluation are held to tests/exact_reference.py:
shared by tests/test_exact_reference.py (CPU) and tests/test_gpu_sample_eval_forward.py.  NumPy only.

Widths: every segment count at which a lane or slot mapping of the library has an edge, up to seg_stride = 256.  Two
families of durations per width, at delta = 0.1:
  (a) m * delta, m in 1 .. 20 -- the way the reference forms a duration; the double-accumulated sample count np then
      equals 1 + sum (int)(t_k / delta);
  (b) family (a) mixed with literal decimals m / 10, on which (int)(t_k / delta) truncates m - 1ulp to m - 1 while the
      double accumulation rounds it back up: np runs ahead of 1 + the sum.
Both carry a 0.07 s segment (no samples; in the middle or at the end) and a 14.95 s one (149 samples: three passes of
the sampling's 64-thread block).  Slots beyond a candidate's own count hold NaN in the durations and control points."""
import functools

import numpy as np

import exact_reference as X
from acost_reference import sample_count
from spectral_amd import layout as L

DELTA = 0.1
WIDTHS = [1, 2, 10, 20, 64, 65, 130, 256]
MAX_PER_SEGMENT = 150
EXACT_ALL_BELOW = 130   # at and beyond: the exact check on the first, the last and the shortest candidate only


def family_durations(rng, n, family):
    m = rng.integers(1, 21, n)
    t = m * DELTA
    if family == "b":
        lit = rng.random(n) < 0.5
        t[lit] = m[lit] / 10
    return t


@functools.lru_cache(maxsize=None)
def layout(S, ragged, family, B=6):
    """dict(B, S, seg [NUM_SEG_FIELDS, B, S], cnt int32 [B] or None, ctrl [B, 12 S], init [B, 6])."""
    rng = np.random.default_rng(7000 + 8 * S + 2 * ragged + (family == "b") + 1000 * B)
    cnt = np.full(B, S, dtype=np.int32)
    if ragged:
        cnt = rng.integers(1, S + 1, B).astype(np.int32)
        cnt[0] = S
        cnt[B - 2] = 1
    seg = np.zeros((L.NUM_SEG_FIELDS, B, S))
    seg[L.F_T] = np.nan
    ctrl = np.full((B, 12 * S), np.nan)
    for b in range(B):
        n = int(cnt[b])
        t = family_durations(rng, n, family)
        if n == 1:
            if b % 3 != 2:
                t[0] = 14.95 if b % 3 == 0 else 0.07
        elif n == 2 and b % 3 == 2:
            if family == "b":
                t[:] = [5 * DELTA, 3 / 10]   # the shortest run-ahead: 6 + 2.9999999999999996 rounds to 9, the int sum is 8
        else:
            short = n - 1 if b % 2 == 0 else int(rng.integers(0, n - 1))   # at the end, or in front of other segments
            t[short] = 0.07
            if b % 3 != 2:
                t[(short + 1 + int(rng.integers(0, n - 1))) % n] = 14.95
        seg[L.F_T, b, :n] = t
        ctrl[b, :12 * n] = rng.standard_normal(12 * n) * 3 + np.linspace(0, 30, 12 * n)
    init = rng.standard_normal((B, 6))
    for a in (seg, cnt, ctrl, init):
        a.setflags(write=False)   # shared between tests: left unchanged
    return dict(B=B, S=S, seg=seg, cnt=cnt if ragged else None, ctrl=ctrl, init=init)


def count_of(case, b, cnt=None):
    cnt = case["cnt"] if cnt is None else cnt
    return case["S"] if cnt is None else int(cnt[b])


def durations(case, b):
    return case["seg"][L.F_T, b, :count_of(case, b)]


def checked(case):
    """The candidates held to the exact yardstick (all of them are held to the counts and the untouched entries)."""
    B, S = case["B"], case["S"]
    if S < EXACT_ALL_BELOW:
        return list(range(B))
    cnt = np.full(B, S) if case["cnt"] is None else case["cnt"]
    return sorted({0, B - 1, int(np.argmin(cnt))})


@functools.lru_cache(maxsize=None)
def exact_samples_of(S, ragged, family, b):
    """(exact samples 1 .. total [6, total], the tolerance's scale) of candidate b of layout(S, ragged, family)."""
    case = layout(S, ragged, family)
    n, t = count_of(case, b), durations(case, b)
    want, scale = X.exact_samples(t, DELTA, case["ctrl"][b], n), X.scale_samples(t, DELTA, case["ctrl"][b], n)
    want.setflags(write=False); scale.setflags(write=False)
    return want, scale


def coverage(S, ragged):
    """(checked candidates with np == 1 + total, with np > 1 + total) over both families, by sample_count alone; also
    holds every segment to MAX_PER_SEGMENT samples and family (a) to np == 1 + total throughout."""
    same, ahead = 0, 0
    for family in ("a", "b"):
        case = layout(S, ragged, family)
        for b in range(case["B"]):
            t = durations(case, b)
            assert max(int(tk / DELTA) for tk in t) <= MAX_PER_SEGMENT
            npd, npi = sample_count(t, DELTA)
            assert npd >= npi
            if family == "a":
                assert npd == npi, (S, ragged, b)
            if b in checked(case):
                same += npd == npi
                ahead += npd > npi
    return same, ahead


def state_times(rng, t):
    """Times of one candidate: two interior points per segment, every joint as np.cumsum(t) (what a warm start passes),
    0, -1 and NaN, and two beyond the horizon; shuffled."""
    joints = np.concatenate([[0.0], np.cumsum(t)])
    tm = [tm for _, tm in interior_times(t)]
    tm += list(joints[1:]) + [0.0, -1.0, np.nan, joints[-1] + 0.5, joints[-1] + 3.0]
    tm = np.array(tm)
    rng.shuffle(tm)
    return tm


def times_of(case, n_times=None, seed=0):
    """times [B, n_times]: state_times of every candidate, padded with random times inside its horizon (or cut) to a common
    n_times (default: the longest list)."""
    rng = np.random.default_rng(9000 + case["S"] + seed)
    per = [state_times(rng, durations(case, b)) for b in range(case["B"])]
    n = max(len(p) for p in per) if n_times is None else n_times
    rows = []
    for b, p in enumerate(per):
        pad = rng.uniform(0, durations(case, b).sum(), max(n - len(p), 0))
        rows.append(np.concatenate([p, pad])[:n])
    return np.stack(rows)


def interior_times(t):
    """The interior times of state_times, in segment order: [(k, time)]."""
    joints = np.concatenate([[0.0], np.cumsum(t)])
    return [(k, joints[k] + f * t[k]) for k in range(len(t)) for f in (0.137, 0.61)]
