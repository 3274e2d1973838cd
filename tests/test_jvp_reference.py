"""The yardstick of the JVP (tests/jvp_reference.py) validated on the CPU, two ways: against the VJP's yardstick by the
adjoint identity <xbar, J d> + cbar dcost = <J' (xbar, cbar), d>, and against central differences of the oracle's exact
solve along the direction.

Families and seeds are those of test_vjp_reference.py.  Strict complementarity (Adjoint.strict) is a property of the
oracle's solution alone; counted once over the 8 candidates of every family: generic 8, scenario_1 8, cuboid 6
(candidates 2 and 3 are not).  Each test requires exactly that many (no silent skip).
"""
import numpy as np
import pytest

from jvp_reference import KEYS, Tangent, moved, random_direction
from test_vjp_reference import FAMILIES
from vjp_reference import Adjoint, exact_x, one

STRICT = {"generic": 8, "scenario_1": 8, "cuboid": 6}


def _strict_candidates(family):
    batch, sh = FAMILIES[family]()
    out = []
    for b in range(batch.B):
        bt = one(batch, b)
        if Adjoint(bt, sh, np.zeros(12 * bt.S), 0.0).strict:
            out.append(b)
    print("%s: strictly complementary candidates %s" % (family, out))
    return batch, sh, out


@pytest.mark.parametrize("family", list(FAMILIES))
def test_adjoint_identity_against_the_vjp_yardstick(family):
    """Tolerance 1e-5 of sum |terms|.  Both sides difference the same assembly, linear or bilinear in every input, with
    h = 1e-4: rounding 1e-16 / 1e-4 = 1e-12 of its entries, nothing else.  The two least-squares solves of the KKT matrix
    are what limits the identity: its entries span 1 (rows) to 1e5 (P, weights over t^3) and dependent active rows make
    it singular, so a condition of 1e9-1e10 on the range leaves 1e-7 to 1e-6 in double precision; one decade above."""
    batch, sh, strict = _strict_candidates(family)
    assert len(strict) == STRICT[family], (family, strict)
    rng = np.random.default_rng(5)
    worst = 0.0
    for b in strict:
        bt = one(batch, b)
        xbar = rng.standard_normal(12 * bt.S); cbar = float(rng.standard_normal())
        adj = Adjoint(bt, sh, xbar, cbar)
        g = adj.grads(h=1e-4)
        um = adj.unique_mask()
        for keys in (KEYS,) + tuple((k,) for k in KEYS):
            d = random_direction(rng, bt.S, keys)
            for k in KEYS:   # (a bound two fields supply at a joint has no unique gradient: that entry of the direction is 0)
                d[k] = np.where(um[k], d[k], 0.0)
            t = Tangent(bt, sh, d, h=1e-4, adj=adj)
            lhs = xbar @ t.dx + cbar * t.dcost
            rhs = sum(float((g[k] * d[k]).sum()) for k in KEYS)
            mag = np.abs(xbar * t.dx).sum() + abs(cbar * t.dcost) + sum(float(np.abs(g[k] * d[k]).sum()) for k in KEYS)
            worst = max(worst, abs(lhs - rhs) / max(mag, 1e-300))
            assert abs(lhs - rhs) <= 1e-5 * mag, (family, b, keys, lhs, rhs)
    print("%s: worst adjoint-identity error %.3e of sum |terms|" % (family, worst))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_yardstick_matches_finite_differences_of_the_exact_solve(family):
    """Tolerance of test_vjp_reference.py for the same comparison: 1e-4 scale + 1e-4 |fd|; scale: the largest entry of dx,
    and for dcost -- a sum of terms that cancel -- the sum of the terms' magnitudes (Tangent.dcost_scale)."""
    batch, sh, strict = _strict_candidates(family)
    assert len(strict) == STRICT[family], (family, strict)
    rng = np.random.default_rng(6)
    h = 1e-5
    for b in strict[:4]:
        bt = one(batch, b)
        adj = Adjoint(bt, sh, np.zeros(12 * bt.S), 0.0)
        adj.grads()
        um = adj.unique_mask()
        d = random_direction(rng, bt.S)
        for k in KEYS:
            d[k] = np.where(um[k], d[k], 0.0)
        t = Tangent(bt, sh, d, adj=adj)
        xp, cp = exact_x(*moved(bt, sh, d, h))
        xm, cm = exact_x(*moved(bt, sh, d, -h))
        fdx, fdc = (xp - xm) / (2 * h), (cp - cm) / (2 * h)
        scale = max(np.abs(t.dx).max(), 1e-12)
        err = np.abs(t.dx - fdx)
        assert (err <= 1e-4 * scale + 1e-4 * np.abs(fdx)).all(), (family, b, err.max(), scale)
        assert abs(t.dcost - fdc) <= 1e-4 * t.dcost_scale + 1e-4 * abs(fdc), (family, b, t.dcost, fdc)
