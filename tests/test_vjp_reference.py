"""The yardstick of the VJP (tests/vjp_reference.py) against central differences of the oracle's exact solve: validates
the yardstick itself, on the CPU."""
import numpy as np
import pytest

from spectral_amd import layout as L
from spectral_amd import synth
from vjp_reference import exact_x, one, reference_vjp, shared_with

FAMILIES = {
    "generic": lambda: synth.make_batch(8, 4, config=3, variant=0, seed=11),
    "scenario_1": lambda: synth.make_scenario1_batch(8, 5, 0, seed=12),
    "cuboid": lambda: synth.make_scenario1_batch(8, 5, 1, seed=13),
}
# one field of every class: position line, reference line, ds bound, initial state, ref_end, dl bound, weights / limits
SEG_CHECK = [L.F_DOWN_BIAS, L.F_UPP_SKEW, L.F_L_UPP_BIAS, L.F_X_BIAS, L.F_Y_SKEW, L.F_DS_HI, L.F_BEG_L, L.F_END_L]


def _fd(batch, sh, xbar, cbar, plus, minus, h):
    xp, cp = exact_x(*plus)
    xm, cm = exact_x(*minus)
    return (xbar @ (xp - xm) + cbar * (cp - cm)) / (2 * h)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_yardstick_matches_finite_differences_of_the_exact_solve(family):
    batch, sh = FAMILIES[family]()
    rng = np.random.default_rng(5)
    checked = 0
    for b in range(batch.B):
        bt = one(batch, b)
        xbar = rng.standard_normal(12 * bt.S)
        cbar = float(rng.standard_normal())
        g, adj = reference_vjp(bt, sh, 0, xbar, cbar)
        if not adj.strict:
            continue
        um = adj.unique_mask()   # (a bound two fields supply at a joint has no unique gradient: skipped)
        checked += 1
        h = 1e-5
        cases = []
        for f in SEG_CHECK:
            if f in (L.F_BEG_L, L.F_END_L) and sh.variant != 1:
                continue
            k = b % bt.S
            p = one(bt, 0); m = one(bt, 0)
            hh = h * (1 + abs(bt.seg[f, 0, k])); p.seg[f, 0, k] += hh; m.seg[f, 0, k] -= hh
            if um["seg"][f, k]:
                cases.append((g["seg"][f, k], (p, sh), (m, sh), hh))
        for attr, i in (("init", 1), ("init", 3), ("ref_end", 0), ("dl_bounds", 3)):
            p = one(bt, 0); m = one(bt, 0)
            hh = h * (1 + abs(getattr(bt, attr)[0, i]))
            getattr(p, attr)[0, i] += hh; getattr(m, attr)[0, i] -= hh
            if um[attr][i]:
                cases.append((g[attr][i], (p, sh), (m, sh), hh))
        arr = sh.as_array()
        for j in (0, 1, 3, 5, 8, 10, 11, 14):
            hh = h * (1 + abs(arr[j]))
            if um["shared"][j]:
                cases.append((g["shared"][j], (bt, shared_with(sh, j, hh)), (bt, shared_with(sh, j, -hh)), hh))
        scale = max(max(abs(c[0]) for c in cases), 1e-12)
        for val, plus, minus, hh in cases:
            fd = _fd(bt, sh, xbar, cbar, plus, minus, hh)
            assert abs(val - fd) <= 1e-4 * scale + 1e-4 * abs(fd), (family, b, val, fd)
        if checked >= 4:
            break
    assert checked >= 2, "too few strictly complementary candidates in the %s family" % family
