"""Scenes, cotangents and hand-computed expectations shared by tests/test_prism_vjp.py (host twin) and
tests/test_gpu_prism_vjp.py (kernel).  Not collected."""
import json
import os

import numpy as np

import helpers as H
from oracle import prism_oracle as PO

GOLD = os.path.join(os.path.dirname(__file__), "golden")
N_KNOTS, P_MAX, O_MAX = 71, 4, 9
W, LS = PO.W_SAFE, PO.L_SAFE


def pack(scenes, P_max):
    arr = np.zeros((len(scenes), P_max, 8))
    for b, cars in enumerate(scenes):
        for p, c in enumerate(cars):
            arr[b, p, :7] = [c["centre"][0], c["centre"][1], c["centre"][2], c.get("vel_s", 0.0), c.get("vel_l", 0.0), c.get("time", 3.0), 1.0]
    return arr


def random_scenes(n, seed, max_cars=4, nice=False):
    """The generator of tests/test_gpu_prism_bounds.py (copied: that file stays as it is)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cars = []
        for r in range(int(rng.integers(1, max_cars + 1))):
            ahead = rng.uniform() < 0.5
            q = (lambda v, k: round(float(v), k)) if nice else (lambda v, k: float(v))   # "nice" decimals provoke rounding ties
            cars.append(dict(centre=(q(rng.uniform(5, 40), 1), q(rng.uniform(-3.0, 9.0), 2), 0 if ahead else q(rng.uniform(0.1, 3.0), 1)),
                             vel_s=q(rng.uniform(0, 8), 1) + (0.005 if nice else 0.0), vel_l=float(rng.choice([0.0, 0.25, -0.25])),
                             time=float(rng.choice([3.0, 4.0]))))
        out.append(cars)
    return out


def golden_scenes():
    """Every well-formed scene of tests/golden/prism_goldens.json (the filter of test_reference_goldens_through_the_device)."""
    G = json.load(open(os.path.join(GOLD, "prism_goldens.json")))
    return [sc["cars"] for sc in G["scenes"]
            if not (any(r["l"][0] >= r["l"][1] for r in sc["strips"]) or
                    any(sc["strips"][i + 1]["l"][0] < sc["strips"][i]["l"][0] for i in range(len(sc["strips"]) - 1)))]


def scene_sets():
    """name -> (prisms [B, P, 8], N, O): the scenes the host twin and the kernel are held to the yardstick on."""
    tied = H.tied_prism_scenes(5, 24, N=201, max_cars=3)[0]
    return dict(golden=(pack(golden_scenes(), P_MAX), N_KNOTS, O_MAX),
                plain=(pack(random_scenes(150, 1), P_MAX), N_KNOTS, O_MAX),
                nice=(pack(random_scenes(150, 2, nice=True), P_MAX), N_KNOTS, O_MAX),
                tied=(pack(tied, 3), 201, 7))


def cotangents(B, O, N, seed=3):
    """Random s_bar, l_bar [B, O, N, 2], entries on padding strips included."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (B, O, N, 2)), rng.uniform(-1.0, 1.0, (B, O, N, 2))


def sixteen_cars(seed=0, B=2):
    """Sixteen active cars whose 32 extent ends are distinct and inside the road: 33 strips, about six cars over each.  The
    cars of a scene share one speed and their face lines lie at least 1.5 apart, so that no max / min among the many cars
    over a strip is decided by the rounding (the yardstick would skip those columns); which car wins still changes from knot
    to knot with the windows."""
    rng = np.random.default_rng(seed)
    scenes = []
    for _ in range(B):
        cars = []
        vs = float(rng.uniform(1.0, 4.0))
        order = rng.permutation(16)
        for q in range(16):
            ahead = q % 2 == 0
            t0 = 0 if ahead else float(rng.uniform(0.1, 3.0))
            s0 = 5.0 + 1.5 * float(order[q]) + float(rng.uniform(0, 0.4)) + vs * t0
            cars.append(dict(centre=(s0, -0.6 + 0.45 * q + float(rng.uniform(0, 0.01)), t0), vel_s=vs, vel_l=0.0, time=float(rng.choice([3.0, 4.0]))))
        scenes.append(cars)
    return scenes


# ---- the defined cases, each with a hand-computed expectation ----------------------------------------------------------
A_LO, A_HI, E_LO, E_HI = 2.0, 3.0, 1.0, 0.5        # the cotangent of every (s lower, s upper, l lower, l upper) entry


def _const_bars(O, N):
    s = np.zeros((1, O, N, 2)); l = np.zeros((1, O, N, 2))
    s[..., 0], s[..., 1], l[..., 0], l[..., 1] = A_LO, A_HI, E_LO, E_HI
    return s, l


def _car(s0, l0, t0, vs, vl, T, on=1.0):
    return [s0, l0, t0, vs, vl, T, on, 0.0]


def _face_row(bar, knots, t0, vs):
    """(s0_bar, t0_bar, vel_s_bar) of a face that is the bound at `knots`, every cotangent entry `bar`."""
    k = np.asarray(list(knots), dtype=np.float64)
    return bar * k.size, -vs * bar * k.size, bar * float(np.sum(k / 10.0 - t0))


def defined_cases():
    """[(name, prisms [1, P, 8], N, O, s_bar, l_bar, expected [P, 8])].  Road: s in [0, 50], l in [-2, 8], w_safe 4/3; N = 71.
    A lone car with l0 = 3 and vel_l = 0 has the extent [5/3, 13/3] strictly inside the road: edges -2, 5/3, 13/3, 8, three
    strips, the middle one covered.  With constant cotangents every inner edge collects N (E_LO + E_HI) = 106.5, the lower
    one from (strip 1 lower, strip 0 upper), and a face collects its bar once per knot of the window inside the horizon."""
    N = N_KNOTS
    inner = N * (E_LO + E_HI)
    cases = []

    def add(name, cars, O, expected, s=True, l=True, pad=None):
        sb, lb = _const_bars(O, N)
        if pad is not None:          # cotangents on padding strips: ignored
            sb[:, pad:] = 1e30; lb[:, pad:] = -1e30
        cases.append((name, np.array([cars], dtype=np.float64), N, O, sb if s else None, lb if l else None, np.array(expected, dtype=np.float64)))

    # t0 = 0 (ahead): the rear face is the UPPER bound at knots 0..40 of strip 1; vel_l = 0 takes the vel_l >= 0 branch
    s0b, t0b, vsb = _face_row(A_HI, range(0, 41), 0.0, 2.0)
    lone = _car(20.0, 3.0, 0.0, 2.0, 0.0, 4.0)
    want = [s0b, 2 * inner, t0b, vsb, 4.0 * inner, 0.0 * inner, 0, 0]
    add("ahead_vel_l_zero", [lone], 3, [want])
    add("padding_strip", [lone], 4, [want], pad=3)
    add("overflow", [lone], 2, [[0] * 8])
    add("null_l_bar", [lone], 3, [[s0b, 0, t0b, vsb, 0, 0, 0, 0]], l=False)
    add("null_s_bar", [lone], 3, [[0, 2 * inner, 0, 0, 4.0 * inner, 0, 0, 0]], s=False)
    add("inactive_slot", [_car(33.0, 2.0, 0.0, 9.0, 0.25, 3.0, on=0.0), lone], 3, [[0] * 8, want])
    # t0 > 0: the front face is the LOWER bound at knots 10..40; vel_l > 0: l_max = l0 + vel_l T + w_safe moves
    s0b, t0b, vsb = _face_row(A_LO, range(10, 41), 1.0, 2.5)
    add("behind_vel_l_positive", [_car(12.0, 3.0, 1.0, 2.5, 0.25, 3.0)], 3, [[s0b, 2 * inner, t0b, vsb, 3.0 * inner, 0.25 * inner, 0, 0]])
    # vel_l < 0: l_min = l0 + vel_l T - w_safe moves; a window that ends beyond N - 1: knots 50..70
    s0b, t0b, vsb = _face_row(A_LO, range(50, 71), 5.0, 1.5)
    add("window_beyond_horizon_vel_l_negative", [_car(12.0, 3.0, 5.0, 1.5, -0.25, 4.0)], 3,
        [[s0b, 2 * inner, t0b, vsb, 4.0 * inner, -0.25 * inner, 0, 0]])
    # two identical cars: the first supplies both edges and wins every tie
    s0b, t0b, vsb = _face_row(A_HI, range(0, 41), 0.0, 2.0)
    add("identical_cars", [lone, lone], 3, [want, [0] * 8])
    # nested extents with a coinciding lower end: A = [5/3, 3 + 1 + 4/3], B = [5/3, 13/3] -> edges -2, 5/3 (A's: the lower
    # index), 13/3 (B's), 16/3 (A's), 8; four strips.  Strip 1 is covered by A and B (equal faces: A keeps them), strip 2 by A.
    a_car = _car(20.0, 3.0, 0.0, 2.0, 0.25, 4.0); b_car = _car(20.0, 3.0, 0.0, 2.0, 0.0, 4.0)
    s0a, t0a, vsa = _face_row(A_HI, list(range(0, 41)) * 2, 0.0, 2.0)
    add("nested_coinciding_extents", [a_car, b_car], 4,
        [[s0a, 2 * inner, t0a, vsa, 4.0 * inner, 0.25 * inner, 0, 0], [0, inner, 0, 0, 4.0 * inner, 0.0, 0, 0]])
    # a face beyond the road's limit (rear face 60 - 10/3 > 50).  The FIRST covering car's face replaces the limit: B alone
    # first gets the upper bound although it is above s_hi; C (face 62 - 10/3) is not strictly tighter and gets nothing.
    s0b, t0b, vsb = _face_row(A_HI, range(0, 41), 0.0, 0.0)
    far_b = _car(60.0, 3.0, 0.0, 0.0, 0.0, 4.0); far_c = _car(62.0, 3.0, 0.0, 0.0, 0.0, 4.0)
    row_b = [s0b, 2 * inner, t0b, vsb, 4.0 * inner, 0.0, 0, 0]
    add("face_beyond_limit_first_replaces", [far_b, far_c], 3, [row_b, [0] * 8])
    # ... as the SECOND car over the strip it does not: A (t0 > 0, upper bound s_hi = 50) comes first, B's 56.67 is not < 50
    s0a, t0a, vsa = _face_row(A_LO, range(10, 41), 1.0, 2.5)
    add("face_beyond_limit_second_does_not", [_car(12.0, 3.0, 1.0, 2.5, 0.0, 3.0), far_b], 3,
        [[s0a, 2 * inner, t0a, vsa, 3.0 * inner, 0.0, 0, 0], [0] * 8])
    # strips nobody covers: cotangents of s on strips 0 and 2 only reach no face
    sb, lb = _const_bars(3, N)
    sb[:, 1] = 0.0
    cases.append(("uncovered_strips", np.array([[lone]], dtype=np.float64), N, 3, sb, None, np.zeros((1, 8))))
    return cases


def check_defined(name, got, expected):
    got = np.asarray(got).reshape(expected.shape)
    assert np.allclose(got, expected, rtol=1e-12, atol=1e-12), (name, got, expected)
    assert np.array_equal(got == 0.0, expected == 0.0), (name, got, expected)
