"""Cases of the clearance stage and their comparison with the yardstick (tests/clearance_reference.py), shared by
tests/test_clearance_host.py and tests/test_gpu_clearance.py.  Poses and headings are drawn uniformly -- general position,
not lane-parallel -- in a square that grows with the obstacle count, so that both branches (overlapping, disjoint) and
every feature occur.  The yardstick of a case is computed once per (case, sample set) and kept."""
import numpy as np

import clearance_reference as cr
from spectral_amd import layout

FOOT = (2.4, 0.95, 1.3)
_cache = {}


def make_case(R, n, O, n_scenes=1, seed=0, counts=None, obs_count=None, scene_index=None, nan_ego=(), nan_obs=()):
    """-> dict(cart [R, 6, n], obstacles (layout.Obstacles), foot, count, scene_index, key).  nan_ego: (row, sample) pairs
    whose ego pose gets a NaN (in x, y or theta in turn); nan_obs: (scene, obstacle, sample) triples alike."""
    rng = np.random.default_rng(1000 + seed)
    box = 4.0 + 5.0 * np.sqrt(O)
    cart = rng.uniform(-1.0, 1.0, (R, 6, n))
    cart[:, :2] *= box
    cart[:, 2] *= np.pi
    pose = rng.uniform(-1.0, 1.0, (n_scenes, O, 3, n))
    pose[:, :, :2] *= box
    pose[:, :, 2] *= np.pi
    half = rng.uniform(0.4, 3.0, (n_scenes, O, 2))
    for i, (r, j) in enumerate(nan_ego):
        cart[r, i % 3, j] = np.nan
    for i, (k, o, j) in enumerate(nan_obs):
        pose[k, o, i % 3, j] = np.nan
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    key = (R, n, O, n_scenes, seed, tuple(counts) if counts is not None else None, tuple(obs_count) if obs_count is not None else None,
           tuple(scene_index) if scene_index is not None else None, tuple(nan_ego), tuple(nan_obs))
    return dict(cart=cart, obstacles=layout.Obstacles(pose, half, i32(obs_count)), foot=FOOT, count=i32(counts),
                scene_index=i32(scene_index), key=key, R=R, n=n, O=O)


def rows_read(case):
    """-> [(row, samples read)]"""
    n = case["n"]
    c = case["count"]
    return [(r, n if c is None else int(min(max(c[r], 0), n))) for r in range(case["R"])]


def scene_of(case, r):
    k = 0 if case["scene_index"] is None else int(case["scene_index"][r])
    return k if 0 <= k < case["obstacles"].n_scenes else -1


def pick_samples(case, at_most, seed=7):
    """The (row, sample) pairs that are compared: all that are read when there are few, else the edges of the lane mapping
    (samples 0, 63, 64, the last) of every row that has them and a random draw of the rest."""
    every = [(r, j) for r, c in rows_read(case) for j in range(c)]
    if len(every) <= at_most:
        return every
    rng = np.random.default_rng(seed)
    edge = [(r, j) for r, c in rows_read(case)[:: max(1, case["R"] // 8)] for j in {0, 63, 64, c - 1} if 0 <= j < c]
    rest = [every[i] for i in rng.choice(len(every), at_most - len(edge), replace=False)]
    return sorted(set(edge + rest))


def obstacles_at(case, k, j):
    ob = case["obstacles"]
    h = ob.host
    cnt = ob.O if h["obs_count"] is None else int(min(max(h["obs_count"][k], 0), ob.O))
    return [tuple(h["pose"][k, o, :, j]) + tuple(h["half"][k, o]) for o in range(cnt)]


def reference(case, samples, grads=False):
    """The yardstick at `samples`: dict (r, j) -> cr.sample(...) (None for an invalid pose), with "grad" (six numbers) added
    when grads and the margin allows."""
    key = (case["key"], tuple(samples))
    ref = _cache.setdefault(key, {})
    for r, j in samples:
        if (r, j) not in ref:
            k = scene_of(case, r)
            pose = case["cart"][r, :3, j]
            ref[(r, j)] = None if k < 0 or np.isnan(pose).any() else cr.sample(pose, case["foot"], obstacles_at(case, k, j))
        s = ref[(r, j)]
        if grads and s is not None and "grad" not in s:
            s["grad"] = None
            if s["obstacle"] >= 0 and s["margin"] >= cr.TAU:
                s["grad"] = cr.gradient(case["cart"][r, :3, j], case["foot"], obstacles_at(case, scene_of(case, r), j)[s["obstacle"]])
    return ref


def check_values(case, samples, clear, which):
    """Every sample: |clear - yardstick| within its bound (nothing skipped), NaN / +inf and which = -1 exactly where the
    definition says; which names the yardstick's winner wherever the margin is at least TAU.  Returns the worst ratio."""
    ref = reference(case, samples)
    worst = 0.0
    for (r, j) in samples:
        s = ref[(r, j)]
        c, w = float(clear[r, j]), int(which[r, j])
        if s is None:
            assert np.isnan(c) and w == -1, (r, j, c, w)
        elif s["obstacle"] < 0:
            assert c == np.inf and w == -1, (r, j, c, w)
        else:
            err = abs(cr.mp.mpf(c) - s["clear"])
            assert err <= s["value_bound"], (r, j, c, float(s["clear"]), float(err / s["value_bound"]))
            worst = max(worst, float(err / s["value_bound"]))
            if s["margin"] >= cr.TAU:
                assert w in s["which"], (r, j, w, s["which"])
    return worst


def check_grads(case, samples, J, cap=0.10):
    """J: dict (r, j) -> the six numbers (d clear / d x, y, theta of the ego, d / d ox, oy, otheta of the winning obstacle)
    from the product; compared with mp.diff of the yardstick at every sample whose margin is at least TAU.  Asserts that
    at most `cap` of the samples with an obstacle were skipped.  Returns (worst ratio, share skipped)."""
    ref = reference(case, samples, grads=True)
    worst, compared, skipped = 0.0, 0, 0
    for (r, j) in samples:
        s = ref[(r, j)]
        got = [float(v) for v in J[(r, j)]]
        if s is None or s["obstacle"] < 0:
            assert got == [0.0] * 6, (r, j, got)
            continue
        if s["grad"] is None:
            skipped += 1
            continue
        compared += 1
        for a, b in zip(got, s["grad"]):
            err = abs(cr.mp.mpf(a) - b)
            assert err <= s["grad_bound"], (r, j, got, [float(v) for v in s["grad"]], float(err / s["grad_bound"]))
            worst = max(worst, float(err / s["grad_bound"]))
    share = skipped / max(1, skipped + compared)
    assert share <= cap, (skipped, compared)
    return worst, share


def unit_tangents(case):
    """Six tangents: the ego's x, y, theta and every obstacle's x, y, theta -> (cart_dot [6, R, 6, n], obs_dot
    [6, n_scenes, O, 3, n])."""
    ob = case["obstacles"]
    cd = np.zeros((6, case["R"], 6, case["n"]))
    od = np.zeros((6, ob.n_scenes, ob.O, 3, case["n"]))
    for i in range(3):
        cd[i, :, i] = 1.0
        od[3 + i, :, :, i] = 1.0
    return cd, od


# ---- exact cases: headings 0, dyadic coordinates and extents, so that every operation of the statement is exact on the
#      host and on the device alike (sin 0 = 0, cos 0 = 1; a fused multiply-add of exact operands rounds nothing) ----
EXACT_FOOT = (2.0, 1.0, 0.5)     # the ego's pose is (1, -2, 0): its centre is (1.5, -2), it spans x in [-0.5, 3.5], y in [-3, -1]
# (obstacle centres, their half extents, the clearance, which): what the definition gives, to the bit
EXACT = {
    "face to face": ([(6.5, -2.25)], [(1.0, 1.5)], 2.0, 4),                 # the first vertex of A that attains it
    "corner to corner, 3-4-5": ([(7.5, 4.0)], [(1.0, 1.0)], 5.0, 4),
    "nested at the centre": ([(1.5, -2.0)], [(0.5, 0.25)], -1.25, 1),
    "nested off the centre": ([(1.75, -1.5)], [(0.5, 0.25)], -0.75, 1),
    "touching at a face: g = 0 is the overlap branch": ([(4.5, -2.0)], [(1.0, 0.5)], 0.0, 0),
    "touching at a corner: g_0 = g_1 = 0, the lowest wins": ([(4.5, -0.5)], [(1.0, 0.5)], 0.0, 0),
    "parallel, overlapping along u: g_0 = g_2": ([(4.0, -2.0)], [(1.0, 0.5)], -0.5, 0),
    "parallel, overlapping along n: g_1 = g_3": ([(1.5, -0.75)], [(0.5, 0.5)], -0.25, 1),
    "edge to edge in parallel: features 4, 7, 9, 10 tie": ([(5.5, -2.0)], [(1.0, 1.0)], 1.0, 4),
    "two obstacles tie, the right one first": ([(5.5, -2.0), (-2.5, -2.0)], [(1.0, 1.0)] * 2, 1.0, 4),
    "two obstacles tie, the left one first": ([(-2.5, -2.0), (5.5, -2.0)], [(1.0, 1.0)] * 2, 1.0, 5),
    "two obstacles tie behind a far one": ([(9.0, 9.0), (-2.5, -2.0), (5.5, -2.0)], [(1.0, 1.0)] * 3, 1.0, 16 + 5),
}
# the winner's one-sided derivative at the tie "edge to edge in parallel": A's vertex (3.5, -1) against B's face x = 4.5, so
# n = (-1, 0) and the lever of (3.5, -1) about the pose's point (1, -2) is (2.5, 1) x (-1, 0) = 1
EXACT_TIE_GRADIENT = ("edge to edge in parallel: features 4, 7, 9, 10 tie", [-1.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def exact_inputs(name):
    """-> (cart [1, 6, 1], layout.Obstacles, the clearance, which) of an EXACT case."""
    obs, half, clear, which = EXACT[name]
    cart = np.zeros((1, 6, 1))
    cart[0, 0, 0], cart[0, 1, 0] = 1.0, -2.0
    pose = np.zeros((len(obs), 3, 1))
    pose[:, :2, 0] = obs
    return cart, layout.Obstacles(pose, np.array(half, dtype=np.float64)), clear, which
