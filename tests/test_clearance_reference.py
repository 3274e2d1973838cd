"""The yardstick of the clearance stage (tests/clearance_reference.py: the signed distance of the origin to the hull of the
vertex differences, mpmath at 50 digits) against closed forms: axis-aligned boxes face to face, corner to corner, nested
and touching, one box turned by 45 degrees against an edge; its derivatives against the closed forms' own; and the share
of the drawn cases whose margin falls below TAU, with the yardstick alone (no product code)."""
import mpmath as mp
import pytest

import clearance_cases as cc
import clearance_reference as cr

EPS = mp.mpf("1e-45")
FOOT0 = (2, 1, 0)   # half extents 2 x 1, the pose's point is the centre


def test_face_to_face_is_the_gap_between_the_faces():
    assert abs(cr.pair_clearance((0, 0, 0), FOOT0, (5, 0.25, 0, 1, 1)) - 2) < EPS            # 5 - 2 - 1
    assert abs(cr.pair_clearance((0, 0, 0), FOOT0, (0.5, -4, 0, 1, 1.5)) - 1.5) < EPS        # 4 - 1 - 1.5


def test_corner_to_corner_is_the_distance_of_the_corners():
    # A's corner (2, 1), B's corner (5, 5)
    assert abs(cr.pair_clearance((0, 0, 0), FOOT0, (6, 6, 0, 1, 1)) - 5) < EPS


def test_nested_is_minus_the_smallest_shift_that_separates():
    # B inside A at the centre: out through the nearer face pair, h_w(A) + h_w(B) = 1.25
    assert abs(cr.pair_clearance((0, 0, 0), FOOT0, (0, 0, 0, 0.5, 0.25)) + 1.25) < EPS
    # off the centre by 0.5 in y: 1 + 0.25 - 0.5
    assert abs(cr.pair_clearance((0, 0, 0), FOOT0, (0, 0.5, 0, 0.5, 0.25)) + 0.75) < EPS


def test_touching_is_zero():
    assert abs(cr.pair_clearance((0, 0, 0), FOOT0, (3, 0, 0, 1, 1))) < EPS
    assert abs(cr.pair_clearance((0, 0, 0), FOOT0, (3, 2, 0, 1, 1))) < EPS                   # at a corner


def test_a_box_turned_by_45_degrees_against_an_edge():
    # a unit square turned by 45 degrees reaches sqrt(2) from its centre: its corner faces A's edge x = 2
    d = cr.pair_clearance((0, 0, 0), FOOT0, (5, 0.3, mp.pi / 4, 1, 1))
    assert abs(d - (3 - mp.sqrt(2))) < EPS
    # overlapping by 0.5 along x: the depth along A's axis is 0.5, along the square's own axes (2 + 1/sqrt 2 ... ) more
    d = cr.pair_clearance((0, 0, 0), FOOT0, (1.5 + mp.sqrt(2), 0.3, mp.pi / 4, 1, 1))
    assert abs(d + 0.5) < EPS


def test_the_centre_offset_moves_the_rectangle_along_its_heading():
    # heading pi/2, offset 1.5: the centre is (0, 1.5); B above it
    d = cr.pair_clearance((0, 0, mp.pi / 2), (2, 1, 1.5), (0, 8, 0, 1, 1))
    assert abs(d - (8 - 1 - 3.5)) < EPS


def test_derivatives_of_the_closed_forms():
    # B turned by 0.01 and raised: A's corner (2, 1) is nearest, against B's face x_B = -1, so n = -u_B and the
    # clearance is -1 - u_B . ((2, 1) - c_B)
    th = mp.mpf(float(0.01))
    c, s = mp.cos(th), mp.sin(th)
    assert abs(cr.pair_clearance((0, 0, 0), FOOT0, (5, 0.25, 0.01, 1, 1)) - (3 * c - 0.75 * s - 1)) < EPS
    g = cr.gradient((0, 0, 0), FOOT0, (5, 0.25, 0.01, 1, 1))
    assert abs(g[0] + c) < EPS and abs(g[1] + s) < EPS and abs(g[3] - c) < EPS and abs(g[4] - s) < EPS
    # corner to corner: the direction is (3, 4) / 5 from A to B, so n (from B to A) = -(0.6, 0.8)
    g = cr.gradient((0, 0, 0), FOOT0, (6, 6, 0, 1, 1))
    assert abs(g[0] + mp.mpf(3) / 5) < EPS and abs(g[1] + mp.mpf(4) / 5) < EPS
    # A's corner (2, 1) about the pose's point: lever = (2, 1) x n = 2 (-0.8) - 1 (-0.6) = -1
    assert abs(g[2] + 1) < EPS
    # B's corner (-1, -1) about its centre, sign reversed: -((-1)(-0.8) - (-1)(-0.6)) = -0.2
    assert abs(g[5] + mp.mpf(1) / 5) < EPS


def test_the_enumeration_names_the_winner_and_its_twin():
    e = cr.enumerate_pair((0, 0, 0), FOOT0, (6, 6, 0, 1, 1))
    assert e["feature"] == 4 and e["same"] == {4, 10} and e["corner"]       # A's (+,+) against B's (-,-): one function
    e = cr.enumerate_pair((0, 0, 0), FOOT0, (0, 0.5, 0, 0.5, 0.25))
    assert e["feature"] == 1 and e["value"] == mp.mpf(-0.75)


@pytest.mark.parametrize("R,n,O", [(3, 65, 4), (2, 40, 16), (2, 64, 1)])
def test_the_drawn_cases_stay_under_the_cap_of_skipped_samples(R, n, O):
    case = cc.make_case(R, n, O, seed=R)
    samples = cc.pick_samples(case, 150)
    ref = cc.reference(case, samples)
    with_obstacle = [s for s in ref.values() if s is not None and s["obstacle"] >= 0]
    below = sum(1 for s in with_obstacle if s["margin"] < cr.TAU)
    assert len(with_obstacle) >= 60 and below <= 0.10 * len(with_obstacle), (below, len(with_obstacle))
