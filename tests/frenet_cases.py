"""Cases and checks the host and the GPU tests of the projection onto the reference line share (tests/test_frenet_host.py,
tests/test_gpu_frenet.py): queries forward-mapped from Frenet draws through the existing host forward, with the special
ones planted at known places, the hairpin, and the comparisons against the yardstick (tests/frenet_reference.py) within
its bound.  A test hands in what the entry point under test returned; nothing here calls the entry points under test.

Exclusions are conditions: a comparison that needs a well-posed query leaves out |omega| < 0.2 and near-ties (runner-up
d^2 within 1e-6 relative of the winner's), and asserts that at most 5 % of what it drew is left out."""
import numpy as np

import cartesian_cases as cc
import frenet_reference as fr
from spectral_amd import layout, native

YARD = fr.Yardstick()          # one cache for the session: host and GPU tests meet the same queries
SENTINEL = -12345.678
ISENT = -77
make_lines, line_of, to_states, from_states, counts_of = cc.make_lines, cc.line_of, cc.to_states, cc.from_states, cc.counts_of


def make_queries(seed, R, n, rl, line_index=None, count=None, plant=True):
    """cart [R, 6, n]: the existing host forward of Frenet draws (ds >= 0.5, |l| <= 3 on lines of radius >= 25), so every
    query that is read on an existing line has an answer.  Planted, first at a lane's edges (samples 0, 63, 64 and the
    last one read of a row), two of each kind where there is room: "table" (on the normal of a table point), "first",
    "last" (2^-20 m inside the normals of the table's ends: ON them the sign of a g that is zero up to rounding decides
    between the end interval and OUTSIDE, which only a line of heading 0 makes exact -- test_the_table_ends_where_g_is_exact),
    "nan" (x is NaN), "behind" (5 m before the first normal: no candidate).
    Returns (cart, f, planted: kind -> [(r, j)])."""
    f, _ = cc.make_samples(seed, R, n, rl, line_index=line_index, special=False)
    rng = np.random.default_rng(seed + 1000)
    cnt = counts_of(count, R, n)
    line = lambda r: 0 if line_index is None else int(line_index[r])
    rows = [r for r in range(R) if 0 <= line(r) < rl.n_lines and cnt[r] > 0]
    kinds = ("table", "first", "last", "nan", "behind")
    planted = {k: [] for k in kinds}
    if plant:
        edge = [(r, j) for r in rows for j in sorted({0, 63, 64, int(cnt[r]) - 1}) if j < cnt[r]]
        rest = [(r, j) for r in rows for j in range(int(cnt[r])) if j not in (0, 63, 64, int(cnt[r]) - 1)]
        slots = [edge[q] for q in rng.permutation(len(edge))] + [rest[q] for q in rng.permutation(len(rest))]
        todo = (list(kinds) * 2)[:len(slots) // 2]
        for (r, j), kind in zip(slots, todo):
            rs = rl.host["rs"][line(r)]
            if kind == "table":
                f[r, 0, j] = rs[int(rng.integers(1, rl.M - 1))] if rl.M > 2 else rs[0]
            elif kind == "behind":
                f[r, 0, j] = rs[0]
            elif kind == "first":
                f[r, 0, j] = rs[0] + 2.0 ** -20
            elif kind == "last":
                f[r, 0, j] = rs[-1] - 2.0 ** -20
            planted[kind].append((r, j))
    li = None if line_index is None else np.ascontiguousarray(line_index, dtype=np.int32)
    cart = native.cartesian_host(f, rl, line_index=li, want=("cart",))["cart"]
    for r, j in planted["nan"]:
        cart[r, 0, j] = np.nan
    for r, j in planted["behind"]:
        th = rl.host["rtheta"][line(r)][0]
        cart[r, 0, j] -= 5.0 * np.cos(th); cart[r, 1, j] -= 5.0 * np.sin(th)
    # rows without a line: the forward gave NaN; give them numbers, so that only line_index makes them OUTSIDE
    bad = [r for r in range(R) if not 0 <= line(r) < rl.n_lines]
    cart[bad] = rng.uniform(-1.0, 1.0, (len(bad), 6, n))
    return cart, f, planted


def picks_of(planted, R, n, count, extra, seed=0):
    """The samples a comparison visits: every planted one, and `extra` others among those read."""
    cnt = counts_of(count, R, n)
    must = [p for k in planted for p in planted[k]]
    rest = [(r, j) for r in range(R) for j in range(int(cnt[r])) if (r, j) not in set(must)]
    rng = np.random.default_rng(seed)
    return must + [rest[q] for q in rng.permutation(len(rest))[:extra]]


def yard(rl, li, c, order, window=None):
    key = (rl.M, hash(rl.host["rx"][li].tobytes()), hash(rl.host["rtheta"][li].tobytes()))
    return YARD.query(key, line_of(rl, li), c, order, window)


def check_values(rl, cart, got, interval, picks, order=2, line_index=None, window=None, must=()):
    """got [R, 6, n] (BTRAPZ_FRENET_SAMPLES order) and interval [R, n] against the yardstick at `picks`.  OUTSIDE: NaN in
    all six and -1, bit for bit.  Otherwise every output within its bound, the outputs above the order exactly 0, and
    the interval the yardstick's -- or its neighbour when the root is within 1e-9 of that end of the interval (on the
    normal of a table point the sign of a g that is zero up to rounding picks the side; s is continuous there).
    Returns (worst ratio, {(r, j): yardstick result} of the compared samples whose interval agrees)."""
    worst, left_out, same = 0.0, 0, {}
    for r, j in picks:
        li = 0 if line_index is None else int(line_index[r])
        if not 0 <= li < rl.n_lines:
            assert np.isnan(got[r, :, j]).all() and interval[r, j] == -1, (r, j)
            continue
        res = yard(rl, li, cart[r, :, j], order, None if window is None else window[r])
        if res["i"] < 0:
            assert np.isnan(got[r, :, j]).all() and interval[r, j] == -1, (r, j, got[r, :, j], interval[r, j])
            continue
        assert interval[r, j] >= 0, (r, j, "OUTSIDE, yardstick: interval %d" % res["i"])
        if (abs(res["omega"]) < 0.2 or res["gap"] < 1e-6) and (r, j) not in must:
            left_out += 1
            continue
        rs = rl.host["rs"][li]
        s = res["out"][0]
        if interval[r, j] != res["i"]:
            i = res["i"]
            near = (interval[r, j] == i - 1 and abs(s - rs[i]) <= 1e-9 * (rs[i + 1] - rs[i])) or \
                   (interval[r, j] == i + 1 and abs(s - rs[i + 1]) <= 1e-9 * (rs[i + 1] - rs[i]))
            assert near, (r, j, interval[r, j], res["i"], s)
        else:
            same[(r, j)] = res
        upto = [q for q in range(6) if q % 3 <= order]
        ratio = np.abs(got[r, upto, j] - res["out"][upto]) / res["bound"][upto]
        assert (ratio <= 1.0).all(), (r, j, order, got[r, :, j], res["out"], ratio)
        above = [q for q in range(6) if q % 3 > order]
        assert all(got[r, q, j] == 0.0 and not np.signbit(got[r, q, j]) for q in above), (r, j, got[r, :, j])
        worst = max(worst, float(ratio.max()))
    assert left_out <= 0.05 * max(len(picks), 1), (left_out, len(picks))
    return worst, same


def jacobian_from_jvp(jvp, cart, **kw):
    """The full per-sample Jacobian [R, 6 (row), 6 (column), n] from six unit tangents; jvp(cart_dot) -> [6, R, 6, n]."""
    R, _, n = cart.shape
    cd = np.zeros((6, R, 6, n))
    for t in range(6):
        cd[t, :, t] = 1.0
    return np.moveaxis(jvp(cd), 0, 2)


def check_jacobian(Kgot, same, order=2):
    """Kgot [R, 6, 6, n] against the yardstick's mp.diff Jacobian at the samples of `same`; rows above the order exactly 0."""
    worst = 0.0
    for (r, j), res in same.items():
        ratio = np.abs(Kgot[r, :, :, j] - res["J"]) / res["jbound"]
        assert (ratio <= 1.0).all(), (r, j, order, Kgot[r, :, :, j], res["J"], ratio)
        assert all((Kgot[r, q, :, j] == 0.0).all() for q in range(6) if q % 3 > order)
        worst = max(worst, float(ratio.max()))
    return worst


# ---- the hairpin: 32 m out along y = 0, a half circle of radius 4 to the left, 32 m back along y = 8; h = 0.5 on the
#      straights (dyadic coordinates), 16 intervals on the half circle -------------------------------------------------
def hairpin():
    out_x = np.arange(0.0, 32.0 + 0.25, 0.5)
    k = np.arange(1, 16)
    phi = np.pi * k / 16.0
    arc_x, arc_y, arc_t = 32.0 + 4.0 * np.sin(phi), 4.0 - 4.0 * np.cos(phi), phi
    back_x = np.arange(32.0, -0.25, -0.5)
    rx = np.concatenate([out_x, arc_x, back_x])
    ry = np.concatenate([np.zeros_like(out_x), arc_y, np.full_like(back_x, 8.0)])
    rt = np.concatenate([np.zeros_like(out_x), arc_t, np.full_like(back_x, np.pi)])
    rk = np.concatenate([np.zeros(len(out_x) - 1), np.full(17, 0.25), np.zeros(len(back_x) - 1)])
    rs = np.concatenate([out_x, 32.0 + 4.0 * phi, 32.0 + 4.0 * np.pi + (32.0 - back_x)])
    return layout.RefLine(rs, rx, ry, rt, rk, np.zeros_like(rs))
