"""The yardstick of the Cartesian stage (tests/cartesian_reference.py) held to three things it does not come from: the
numbers the reference's own frenet_to_cartesian3D returned (tests/golden/cartesian_goldens.json) -- which also shows that
the reference's float64 function stays inside the bound every kernel is held to --, the straight-line identity the
reference's harness assumes (x = s, y = l, v = hypot, theta = atan2), and the closed form on a circular arc."""
import json
import math
import os

import numpy as np
import pytest

import cartesian_reference as cr
from spectral_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def goldens():
    g = json.load(open(os.path.join(HERE, "golden", "cartesian_goldens.json")))
    lines = {k: {f: np.array(v[f]) for f in cr.FIELDS} for k, v in g["lines"].items()}
    return lines, g["samples"]


def test_the_reference_function_stays_inside_the_bound_of_the_yardstick(goldens):
    lines, samples = goldens
    assert len(samples) >= 300 and {s["line"] for s in samples} == set(lines) and len(lines) >= 3
    worst = np.zeros(6)
    for smp in samples:
        line, f, ref = lines[smp["line"]], np.array(smp["frenet"]), np.array(smp["out"])
        assert f[0] == line["rs"][smp["i"]] and f[1] >= 0.5           # on a table point, moving
        out, J, _ = cr.evaluate(line, f)
        b = cr.bound(f, out, J)
        worst = np.maximum(worst, np.abs(ref - out) / b)
        assert (np.abs(ref - out) <= b).all(), (smp, ref, out, b)
    print("worst |reference - yardstick| / bound per output (x, y, theta, kappa, v, a):", worst)


def line_of(rl):
    return {k: rl.host[k][0] for k in cr.FIELDS}


def test_on_a_straight_line_the_map_is_what_the_harness_assumes():
    line = line_of(synth.refline_straight(50.0, 0.5))
    rng = np.random.default_rng(5)
    for _ in range(40):
        f = np.array([rng.uniform(0, 50), rng.uniform(0.5, 12), rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(-2, 2)])
        out, J, om = cr.evaluate(line, f)
        v = math.hypot(f[1], f[4])
        expect = [f[0], f[3], math.atan2(f[4], f[1]), (f[1] * f[5] - f[4] * f[2]) / v ** 3, v, (f[1] * f[2] + f[4] * f[5]) / v]
        assert np.allclose(out, expect, rtol=1e-14, atol=1e-14) and om == 1.0
        # x = s and y = l exactly: d x / d s = d y / d l = 1 and nothing else moves them
        assert np.allclose(J[:2], [[1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0]], atol=1e-25)


@pytest.mark.parametrize("rho", [20.0, -35.0])
def test_on_an_arc_a_constant_offset_is_a_circle_of_radius_rho_minus_l(rho):
    line = line_of(synth.refline_arc(40.0, 0.25, rho, x0=1.0, y0=2.0, theta0=0.4))
    cx, cy = 1.0 - rho * math.sin(0.4), 2.0 + rho * math.cos(0.4)        # the centre
    rng = np.random.default_rng(6)
    for _ in range(40):
        i = int(rng.integers(0, 160))
        s, l, sd, sdd = 0.25 * i, rng.uniform(-3, 3), rng.uniform(0.5, 12), rng.uniform(-3, 3)
        out, _, om = cr.evaluate(line, np.array([s, sd, sdd, l, 0.0, 0.0]))
        assert abs(math.hypot(out[cr.X] - cx, out[cr.Y] - cy) - abs(rho - l)) < 1e-12
        assert abs(out[cr.KAPPA] - 1.0 / (rho - l)) < 1e-14
        assert abs(out[cr.V] - sd * (1.0 - l / rho)) < 1e-13 and abs(om - (1.0 - l / rho)) < 1e-15
        assert abs(out[cr.A] - sdd * (1.0 - l / rho)) < 1e-13
        assert abs(math.remainder(out[cr.THETA] - (0.4 + s / rho), 2 * math.pi)) < 1e-14


def test_the_interval_is_the_documented_one():
    rs = np.array([0.0, 1.0, 2.5, 4.0])
    assert [cr.interval(rs, s) for s in (0.0, 0.5, 1.0, 2.4999, 2.5, 3.9, 4.0)] == [0, 0, 1, 1, 2, 2, 2]
    assert cr.is_outside(rs, np.nextafter(0.0, -1)) and cr.is_outside(rs, np.nextafter(4.0, 5)) and cr.is_outside(rs, float("nan"))
    assert not cr.is_outside(rs, 0.0) and not cr.is_outside(rs, 4.0)
