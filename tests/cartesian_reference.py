"""The yardstick of the Cartesian stage (include/btrapz_hip_cartesian.h): mpmath at 50 digits.

It is NOT the product's statement in higher precision.  The product maps time derivatives (ds, dds, dl, ddl) without
dividing by ds; the yardstick converts to the reference's arc-length form -- d' = dl / ds, d'' = (ddl - d' dds) / ds^2 --
and evaluates the formulas of the reference's frenet_to_cartesian3D (cart_frenet.py:347-381) behind the documented
lookup.  The two agree for ds > 0 and 1 - kappa_r l > 0, which is where toleranced cases are drawn (v >= 0.5); the
degenerate cases have exact defined-value tests instead.

What is part of the DEFINITION and taken over in floating point: the interval i of the lookup (the largest index with
rs[i] <= s, clamped to M - 2) and the OUTSIDE test.  Everything after that is evaluated at 50 digits on the inputs'
float64 values.

The Jacobian is mp.diff entry by entry with the interval frozen.  The bound of entry i of a sample is

    K 2^-53 (sum_j |J_ij| |in_j| + |out_i|),      K = 64,

with ONE addition for the row theta, outside the factor K: 8 2^-53 pi.  NormalizeAngle is fmod(a + pi, 2 pi), plus
2 pi if negative, minus pi: it rounds numbers of size pi whatever the size of the result, so a heading carries an
absolute error that no multiple of |theta| covers.  On a straight line of heading 0 the sum above is 2 |theta| for a small
theta = atan2(dl, ds), and any float64 evaluation of that statement -- the reference's own function included -- exceeds
K 2^-53 2 |theta| once |theta| < pi / (2 K), about one random sample in fifty, through no defect.  The roundings of size pi
are few and are charged one by one, not K times: a + pi, a number of at most |theta| + 3 pi when the sum wrapped (2^-53
3 pi); the conditional + 2 pi (2^-53 2 pi); the interpolated rtheta itself, which is up to 2 pi larger than the result
when the table's headings are not wrapped (2^-53 2 pi); and, when the sum wrapped, the float64 2 pi the remainder is
taken by against the number 2 pi the yardstick takes (2.4e-16 = 2^-53 0.7 pi): 7.7, rounded to 8.

K: the longest chain of roundings of the product's statement is kappa's -- w (3: two differences and a quotient), the
interpolation of rkappa and rdkappa (3 each), omega (2), vt (1), ds^2 (1), at (7), an (3), the cross product (3), v^2 and
v^3 (5), the quotient (1): 32.  sin, cos and atan2 of the device's and the host's libraries are within 2 units in the
last place and sit on shorter chains (theta: 16).  Each rounding is charged against the scale above, which is built from
Jacobian products rather than from the magnitudes of the intermediates; the factor 2 on top (K = 64) is for
intermediates that exceed it and for fused multiply-adds reordering the sums.  The bound is not tuned to the product:
it comes from these counts, and the reference's float64 function is held to the same one.

Derivatives.  An entry of the Jacobian is held to KJ 2^-53 (|J_ij| + S_i), S_i the forward's scale of row i (without
the wrap's term: its derivative is 1) and KJ = 4 K: the entry is a sum of products of the forward's intermediates
with the same chains plus the quotient rule's (at most 4 times as many terms), and its terms are bounded by the forward
scale per unit of input for inputs of size >= 1/2, which is what the cases draw (ds >= 0.5).  A VJP / JVP result is
held to the entries' bounds summed with the weights it applies."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
K = 64
KJ = 4 * K
U = 2.0 ** -53
FIELDS = ("rs", "rx", "ry", "rtheta", "rkappa", "rdkappa")
X, Y, THETA, KAPPA, V, A = range(6)


def wrap(a):
    """NormalizeAngle at 50 digits: into [-pi, pi)."""
    r = a + mp.pi
    return r - 2 * mp.pi * mp.floor(r / (2 * mp.pi)) - mp.pi


def is_outside(rs, s):
    return not (s >= rs[0] and s <= rs[-1])


def interval(rs, s):
    """The float decision: the largest i with rs[i] <= s, clamped to M - 2."""
    return int(min(max(np.searchsorted(rs, s, side="right") - 1, 0), len(rs) - 2))


def _ref_point(line, i, s):
    q = {k: [mp.mpf(float(line[k][i])), mp.mpf(float(line[k][i + 1]))] for k in FIELDS}
    w = (s - q["rs"][0]) / (q["rs"][1] - q["rs"][0])
    lin = lambda k: q[k][0] + w * (q[k][1] - q[k][0])
    return lin("rx"), lin("ry"), q["rtheta"][0] + w * wrap(q["rtheta"][1] - q["rtheta"][0]), lin("rkappa"), lin("rdkappa")


def _map(line, i, u):
    """The six outputs (x, y, theta, kappa, v, a) at the mp inputs u = (s, ds, dds, l, dl, ddl), interval i frozen: the
    reference's arc-length formulas."""
    s, sd, sdd, d, ld, ldd = u
    rx, ry, rth, rk, rdk = _ref_point(line, i, s)
    d1 = ld / sd
    d2 = (ldd - d1 * sdd) / (sd * sd)
    x = rx - mp.sin(rth) * d
    y = ry + mp.cos(rth) * d
    om = 1 - rk * d
    tan_dt = d1 / om
    dt = mp.atan2(d1, om)
    cdt = mp.cos(dt)
    theta = wrap(dt + rth)
    kprime = rdk * d + rk * d1
    kappa = (((d2 + kprime * tan_dt) * cdt * cdt) / om + rk) * cdt / om
    v = mp.sqrt(om * om * sd * sd + (d1 * sd) ** 2)
    dtp = om / cdt * kappa - rk
    a = sdd * om / cdt + sd * sd / cdt * (d1 * dtp - kprime)
    return [x, y, theta, kappa, v, a]


def evaluate(line, f, jacobian=True):
    """line: dict of the six float64 arrays of ONE line; f: the six float64 inputs of one sample (inside the line, ds > 0).
    Returns (out [6] float64, J [6, 6] float64 or None, omega float) -- the values rounded once, from 50 digits."""
    i = interval(line["rs"], float(f[0]))
    u = [mp.mpf(float(v)) for v in f]
    out = _map(line, i, u)
    omega = float(1 - _ref_point(line, i, u[0])[3] * u[3])
    if not jacobian:
        return np.array([float(v) for v in out]), None, omega
    J = np.zeros((6, 6))
    for j in range(6):
        cache = {}

        def column(x, j=j, cache=cache):
            if x not in cache:
                cache[x] = _map(line, i, u[:j] + [x] + u[j + 1:])
            return cache[x]
        for r in range(6):
            J[r, j] = float(mp.diff(lambda x, r=r: column(x)[r], u[j]))
    return np.array([float(v) for v in out]), J, omega


WRAP = 8          # roundings of size pi in NormalizeAngle and the unwrapped rtheta (the docstring counts them)


def scale(f, out, J):
    """S_i = sum_j |J_ij| |in_j| + |out_i| per output, [6]: the issue's scale."""
    return np.abs(J) @ np.abs(np.asarray(f, dtype=np.float64)) + np.abs(out)


def bound(f, out, J):
    """The bound of the six outputs of one sample, [6]: K 2^-53 S_i, and on the row theta WRAP 2^-53 pi on top."""
    b = K * U * scale(f, out, J)
    b[THETA] += WRAP * U * np.pi
    return b


def jacobian_bound(f, out, J):
    """The bound of the 36 entries of one sample's Jacobian, [6, 6] (the wrap's derivative is 1: no term of its own)."""
    return KJ * U * (np.abs(J) + scale(f, out, J)[:, None])


class Yardstick:
    """evaluate() over the samples of an array, cached by (line, inputs): the tests of one module share it."""

    def __init__(self):
        self.cache = {}

    def sample(self, key, line, f):
        k = (key, tuple(float(v) for v in f))
        if k not in self.cache:
            out, J, om = evaluate(line, f)
            self.cache[k] = (out, J, om, bound(f, out, J), jacobian_bound(f, out, J))
        return self.cache[k]
