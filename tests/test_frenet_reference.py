"""The yardstick of the projection onto the reference line (tests/frenet_reference.py) held to what is known without it:
the reference's own float64 cartesian_to_frenet3D (tests/golden/frenet_goldens.json, queries on the normals of table
points, where the given matched point IS the projection), the identity on a straight line of heading 0, and the closed
form on a circular arc.  No GPU, no library."""
import json
import os

import numpy as np
import pytest

import frenet_reference as fr
from spectral_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frenet_goldens.json")


@pytest.fixture(scope="module")
def gold():
    return json.load(open(GOLD))


def test_the_references_own_function_is_within_the_bound(gold):
    lines = {k: {f: np.array(v[f]) for f in fr.FIELDS} for k, v in gold["lines"].items()}
    worst = 0.0
    assert len(gold["samples"]) >= 150
    for smp in gold["samples"]:
        c = np.array(smp["cart"])
        res = fr.evaluate(lines[smp["line"]], c)
        # on the normal of table point i the root is that point, from either side
        assert res["i"] in (smp["i"], smp["i"] - 1) and res["ncand"] == 1
        ratio = np.abs(np.array(smp["frenet"]) - res["out"]) / fr.bound(c, res)
        assert (ratio <= 1.0).all(), (smp, res["out"], ratio)
        worst = max(worst, float(ratio.max()))
    print("the reference's float64 cartesian_to_frenet3D: worst ratio to the bound %.3f" % worst)


def test_a_straight_line_of_heading_zero_is_the_identity():
    rl = synth.refline_straight(40.0, 0.5, x0=3.0, y0=-2.0, theta0=0.0)
    line = {k: rl.host[k][0] for k in fr.FIELDS}
    rng = np.random.default_rng(5)
    for _ in range(20):
        x, y = rng.uniform(3.0, 43.0), rng.uniform(-8.0, 4.0)
        th, k, v, a = rng.uniform(-1.2, 1.2), rng.uniform(-0.1, 0.1), rng.uniform(0.0, 12.0), rng.uniform(-3.0, 3.0)
        res = fr.evaluate(line, [x, y, th, k, v, a])
        want = [x - 3.0, v * np.cos(th), a * np.cos(th) - v * v * k * np.sin(th), y + 2.0, v * np.sin(th),
                a * np.sin(th) + v * v * k * np.cos(th)]
        assert res["ncand"] == 1 and np.allclose(res["out"], want, rtol=0, atol=8 * 2.0 ** -53 * (1 + np.abs(want).max()))
        assert np.allclose(res["J"][[0, 3]][:, :2], np.eye(2), rtol=0, atol=1e-15) and np.all(res["J"][[0, 3]][:, 2:] == 0)


@pytest.mark.parametrize("radius", [80.0, -30.0, 10.0])
def test_an_arc_has_a_closed_form_on_the_normals_of_its_table_points(radius):
    rl = synth.refline_arc(20.0, 0.5, radius)                  # from the origin, heading 0: centre (0, radius)
    line = {k: rl.host[k][0] for k in fr.FIELDS}
    rng = np.random.default_rng(7)
    for k in rng.choice(np.arange(1, rl.M - 1), 8, replace=False):
        l = rng.uniform(-6.0, 6.0)
        phi = line["rs"][k] / radius
        x, y = (radius - l) * np.sin(phi), radius - (radius - l) * np.cos(phi)
        v = 3.0
        res = fr.evaluate(line, [x, y, phi, 1.0 / (radius - l), v, 0.0])     # driving the concentric circle through p
        # inputs rounded to float64 (1.4e-14 at these sizes), a conditioning of at most 1 / (1 - 6 / 10) = 2.5: 1e-12 is safe
        assert abs(res["out"][0] - line["rs"][k]) <= 1e-12 and abs(res["out"][3] - l) <= 1e-12
        want = np.array([v * radius / (radius - l), 0.0, 0.0, 0.0])          # ds = v / omega; l stays, nothing accelerates
        assert np.allclose(res["out"][[1, 2, 4, 5]], want, rtol=0, atol=1e-11)
        assert abs(res["omega"] - (1 - l / radius)) <= 1e-12
