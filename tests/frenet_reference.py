"""The yardstick of the projection onto the reference line (include/btrapz_hip_frenet.h): mpmath at 50 digits.

It is NOT the product's statement in higher precision.  The product sweeps the table in float64, refines by a safeguarded
Newton iteration and maps time derivatives; the yardstick

  - finds the candidates and the winner by the definition: g at every table point (float64 where its sign is beyond
    doubt, 50 digits where |g| is within 1e-9 of its scale), the chord distances of the candidates at 50 digits, ties to
    the lowest index, and reports the runner-up so that a test can leave near-ties out;
  - takes the root of g(w) from mp.findroot on the bracket [0, 1];
  - evaluates the REFERENCE'S OWN cartesian_to_frenet3D formulas (cart_frenet.py:306-344) at the matched point -- the
    signed distance copysign(|p - r|, cross), d' = om tan D, d'' and s'' in arc-length form -- and converts with
    dl = d' ds, ddl = d'' ds^2 + d' dds.  The two agree for cos D > 0, which is where toleranced cases are drawn;
  - differentiates by mp.diff entry by entry with the interval frozen (the columns x and y move the root, which is found
    again for every perturbed point).

The bound of output i of a sample is, as the issue states it,

    K 2^-53 (sum_j |K_ij| |in_j| + |out_i|),     plus, for s and l,     K 2^-53 (|x| + |y| + |rx| + |ry|) / |g'|,

with K_ij the Jacobian of the inverse and g' the slope of g per metre of arc length (which gives the second term the
unit of s and l): the cancellation in p - r.  K = 64: the longest chain of roundings in frenet_core.h is that of dds --
theta's interpolation (3), D (1), sincos (2), vt (1), rkappa's interpolation (3), om (2), ds (1), ds^2 (1), rdkappa's
interpolation (3), its two products (2), at (5), the two sums (2), the quotient (1): 27, bounded by 32 and doubled as
in DESIGN 3.19 (intermediates that exceed the scale, fused multiply-adds reordering the sums).  Not tuned to the product:
the reference's own float64 function (tests/golden/frenet_goldens.json) is held to the same bound.

Derivatives.  An entry of the Jacobian is held to KJ 2^-53 (|K_ij| + S_i), KJ = 4 K, S_i the forward's bound of row i
over K 2^-53, the term of s and l included in every row (every row is evaluated at the computed s and l): the same
argument as in cartesian_reference.py."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
K = 64
KJ = 4 * K
U = 2.0 ** -53
FIELDS = ("rs", "rx", "ry", "rtheta", "rkappa", "rdkappa")
S, DS, DDS, L, DL, DDL = range(6)       # rows of the result
X, Y, THETA, KAPPA, V, A = range(6)     # rows of cart


def wrap(a):
    r = a + mp.pi
    return r - 2 * mp.pi * mp.floor(r / (2 * mp.pi)) - mp.pi


def _g_signs(line, x, y):
    """g at every table point as floats whose SIGN is exact (sign decided at 50 digits where float64 could be wrong)."""
    rx, ry, th = line["rx"], line["ry"], line["rtheta"]
    g = (x - rx) * np.cos(th) + (y - ry) * np.sin(th)
    scale = np.abs(x - rx) + np.abs(y - ry)
    for k in np.nonzero(np.abs(g) <= 1e-9 * scale)[0]:
        e = (mp.mpf(x) - mp.mpf(float(rx[k]))) * mp.cos(mp.mpf(float(th[k]))) + (mp.mpf(y) - mp.mpf(float(ry[k]))) * mp.sin(mp.mpf(float(th[k])))
        g[k] = float(mp.sign(e)) * max(abs(float(e)), 5e-324)
    return g


def _chord_d2(line, i, x, y):
    ax, ay, bx, by = [mp.mpf(float(line[k][i + d])) for d in (0, 1) for k in ("rx", "ry")]
    ex, ey, px, py = bx - ax, by - ay, mp.mpf(x) - ax, mp.mpf(y) - ay
    t = min(max((px * ex + py * ey) / (ex * ex + ey * ey), mp.mpf(0)), mp.mpf(1))
    return (px - t * ex) ** 2 + (py - t * ey) ** 2


def find_interval(line, x, y, window=None):
    """(winner i or -1, relative gap of the runner-up's d^2 to the winner's or inf, number of candidates) by the definition."""
    rs = line["rs"]
    M = len(rs)
    if not (x == x and y == y):
        return -1, np.inf, 0
    if window is not None and not (window[0] <= window[1]):
        return -1, np.inf, 0
    g = _g_signs(line, float(x), float(y))
    cand = []
    for i in range(M - 1):
        if not (g[i] >= 0 and (g[i + 1] < 0 or (i == M - 2 and g[i + 1] == 0))):
            continue
        if window is not None and not (rs[i + 1] >= window[0] and rs[i] <= window[1]):
            continue
        cand.append((_chord_d2(line, i, x, y), i))
    if not cand:
        return -1, np.inf, 0
    cand.sort()
    gap = np.inf if len(cand) < 2 else float((cand[1][0] - cand[0][0]) / cand[1][0]) if cand[1][0] > 0 else 0.0
    return cand[0][1], gap, len(cand)


def _ends(line, i):
    return {k: (mp.mpf(float(line[k][i])), mp.mpf(float(line[k][i + 1]))) for k in FIELDS}


def _at(q, w):
    lin = lambda k: q[k][0] + w * (q[k][1] - q[k][0])
    return lin("rx"), lin("ry"), q["rtheta"][0] + w * wrap(q["rtheta"][1] - q["rtheta"][0]), lin("rkappa"), lin("rdkappa")


def _g(q, w, x, y):
    rx, ry, th, _, _ = _at(q, w)
    return (x - rx) * mp.cos(th) + (y - ry) * mp.sin(th)


def _root(q, x, y, near=None):
    """The root of g on the interval: bracketed on [0, 1], or (for a perturbed point of the Jacobian) from `near`."""
    if near is not None:
        return mp.findroot(lambda w: _g(q, w, x, y), near, tol=mp.mpf(10) ** -44, maxsteps=60)
    g0, g1 = _g(q, mp.mpf(0), x, y), _g(q, mp.mpf(1), x, y)
    if g0 == 0:
        return mp.mpf(0)
    if g1 == 0:
        return mp.mpf(1)
    return mp.findroot(lambda w: _g(q, w, x, y), (mp.mpf(0), mp.mpf(1)), solver="anderson", tol=mp.mpf(10) ** -44, maxsteps=200)


def _map(q, w, c, order):
    """(s, ds, dds, l, dl, ddl) at the root w: the reference's cartesian_to_frenet3D at the matched point."""
    x, y, theta, kappa, v, a = c
    rx, ry, rth, rk, rdk = _at(q, w)
    s = q["rs"][0] + w * (q["rs"][1] - q["rs"][0])
    dx, dy = x - rx, y - ry
    cross = mp.cos(rth) * dy - mp.sin(rth) * dx
    d = mp.sqrt(dx * dx + dy * dy) * (1 if cross >= 0 else -1)
    out = [s, mp.mpf(0), mp.mpf(0), d, mp.mpf(0), mp.mpf(0)]
    if order < 1:
        return out
    dt = theta - rth
    tan_dt, cos_dt = mp.tan(dt), mp.cos(dt)
    om = 1 - rk * d
    d1 = om * tan_dt
    sd = v * cos_dt / om
    out[DS], out[DL] = sd, d1 * sd
    if order < 2:
        return out
    kprime = rdk * d + rk * d1
    d2 = -kprime * tan_dt + om / cos_dt / cos_dt * (kappa * om / cos_dt - rk)
    dtp = om / cos_dt * kappa - rk
    sdd = (a * cos_dt - sd * sd * (d1 * dtp - kprime)) / om
    out[DDS], out[DDL] = sdd, d2 * sd * sd + d1 * sdd
    return out


def evaluate(line, c, order=2, window=None, jacobian=True):
    """line: dict of the six float64 arrays of ONE line; c: the six float64 inputs (x, y, theta, kappa, v, a) of one query.
    Returns a dict: i (-1: OUTSIDE), gap, ncand, out [6], J [6, 6] or None, omega, cond = (|x| + |y| + |rx| + |ry|) / |g'|."""
    i, gap, ncand = find_interval(line, c[0], c[1], window)
    res = dict(i=i, gap=gap, ncand=ncand, out=np.full(6, np.nan), J=None, omega=np.nan, cond=np.nan)
    if i < 0:
        return res
    q = _ends(line, i)
    u = [mp.mpf(float(v)) if rd else mp.mpf(0) for v, rd in zip(c, read_mask(order))]   # rows above the order are not read
    w = _root(q, u[0], u[1])
    out = _map(q, w, u, order)
    rx, ry, rth, rk, _ = _at(q, w)
    h = q["rs"][1] - q["rs"][0]
    slope = mp.diff(lambda t: _g(q, t, u[0], u[1]), w) / h
    res.update(out=np.array([float(v) for v in out]), omega=float(1 - rk * out[L]),
               cond=float((abs(u[0]) + abs(u[1]) + abs(rx) + abs(ry)) / abs(slope)))
    if jacobian:
        J = np.zeros((6, 6))
        for j in range(6):
            cache = {}

            def column(t, j=j, cache=cache):
                if t not in cache:
                    uu = u[:j] + [t] + u[j + 1:]
                    cache[t] = _map(q, _root(q, uu[0], uu[1], near=w) if j < 2 else w, uu, order)
                return cache[t]
            for r in range(6):
                J[r, j] = float(mp.diff(lambda t, r=r: column(t)[r], u[j]))
        res["J"] = J
    return res


def read_mask(order):
    """The rows of cart an order reads."""
    return np.array([True, True, order >= 1, order >= 2, order >= 1, order >= 2])


def scale(c, res, order=2):
    """S_i per output, [6]: sum_j |K_ij| |in_j| + |out_i|, plus the root's term on every row (for the Jacobian's bound)."""
    cin = np.where(read_mask(order), np.abs(np.asarray(c, dtype=np.float64)), 0.0)
    return np.abs(res["J"]) @ cin + np.abs(res["out"])


def bound(c, res, order=2):
    """The bound of the six outputs of one query, [6]."""
    b = K * U * scale(c, res, order)
    b[[S, L]] += K * U * res["cond"]
    return b


def jacobian_bound(c, res, order=2):
    return KJ * U * (np.abs(res["J"]) + (scale(c, res, order) + res["cond"])[:, None])


class Yardstick:
    """evaluate() over the queries of an array, cached by (line, inputs, order, window): the tests of one module share it."""

    def __init__(self):
        self.cache = {}

    def query(self, key, line, c, order=2, window=None):
        k = (key, tuple(float(v) for v in c), order, None if window is None else tuple(float(v) for v in window))
        if k not in self.cache:
            res = evaluate(line, c, order, window)
            if res["i"] >= 0:
                res["bound"], res["jbound"] = bound(c, res, order), jacobian_bound(c, res, order)
            self.cache[k] = res
        return self.cache[k]
