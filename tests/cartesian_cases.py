"""Cases and checks the host and the GPU tests of the Cartesian stage share (tests/test_cartesian_host.py,
tests/test_gpu_cartesian.py): reference lines of any number of points, Frenet samples with the special ones planted at
known places, and the comparisons against the yardstick (tests/cartesian_reference.py) within its bound.  A test hands
in what the entry point under test returned; nothing here calls the library."""
import hashlib

import numpy as np

import cartesian_reference as cr
from spectral_amd import layout, synth

LENGTH = 40.0
YARD = cr.Yardstick()          # one cache for the session: host and GPU tests meet the same samples
SENTINEL = -12345.678


def make_lines(M, n_lines=1):
    """n_lines lines of M points over LENGTH metres: an arc to the left, a clothoid that bends right, an arc to the right
    whose heading crosses pi.  With M = 2 or 3 the intervals are 40 or 20 m long: the interpolation is all there is."""
    h = LENGTH / (M - 1)
    made = [synth.refline_arc(LENGTH, h, 30.0, x0=2.0, y0=-1.0, theta0=0.3),
            synth.refline_clothoid(LENGTH, h, 0.03, -0.002, x0=-5.0, y0=4.0, theta0=-0.5),
            synth.refline_arc(LENGTH, h, -25.0, theta0=2.8)][:n_lines]
    assert all(r.M == M for r in made), [r.M for r in made]
    stack = lambda k: np.concatenate([r.host[k] for r in made], 0)
    rl = layout.RefLine(*[stack(k) for k in layout.REFLINE_FIELDS])
    # the table's last point is LENGTH up to rounding: samples are drawn inside [rs[0], rs[M-1]] of every line
    return rl


def line_of(rl, li):
    return {k: rl.host[k][li] for k in cr.FIELDS}


KINDS = ("table", "first", "last", "below", "above", "nan", "still")     # "beyond" only where a test asks for it


def make_samples(seed, R, n, rl, line_index=None, special=True, kinds=KINDS, count=None):
    """f [R, 6, n] (BTRAPZ_FRENET_SAMPLES) with v >= 0.5 everywhere but at the planted samples; returns (f, planted) with
    planted: dict kind -> list of (r, j).  Kinds: "table" (s == rs[i]), "first", "last" (s == rs[0], rs[M-1]), "below",
    "above" (one unit in the last place outside), "nan", "still" (ds = dl = 0: v == 0), "beyond" (1 - kappa l < 0).
    Every kind is planted three times where the array has room (at most half of the samples that are read), only at
    samples that ARE read -- j < min(count[r], n) in a row whose line exists -- and first at a lane's edges: samples 0, 63,
    64 and the last one read of a row.  must_check() names the planted samples a comparison has to include."""
    rng = np.random.default_rng(seed)
    f = np.empty((R, 6, n))
    s_end = min(rl.host["rs"][:, -1])
    f[:, 0] = rng.uniform(0.0, s_end, (R, n))
    f[:, 1] = rng.uniform(0.5, 12.0, (R, n))
    f[:, 2] = rng.uniform(-3.0, 3.0, (R, n))
    f[:, 3] = rng.uniform(-3.0, 3.0, (R, n))
    f[:, 4] = rng.uniform(-2.0, 2.0, (R, n))
    f[:, 5] = rng.uniform(-2.0, 2.0, (R, n))
    planted = {k: [] for k in kinds}
    if not special:
        return f, planted
    cnt = counts_of(count, R, n)
    line = lambda r: 0 if line_index is None else int(line_index[r])
    rows = [r for r in range(R) if 0 <= line(r) < rl.n_lines and cnt[r] > 0]
    edge = [(r, j) for r in rows for j in sorted({0, 63, 64, int(cnt[r]) - 1}) if j < cnt[r]]
    rest = [(r, j) for r in rows for j in range(int(cnt[r])) if j not in (0, 63, 64, int(cnt[r]) - 1)]
    slots = [edge[q] for q in rng.permutation(len(edge))] + [rest[q] for q in rng.permutation(len(rest))]
    todo = (list(kinds) * 3)[:len(slots) // 2]
    for (r, j), kind in zip(slots, todo):
        li = line(r)
        rs = rl.host["rs"][li]
        if kind == "table":
            f[r, 0, j] = rs[int(rng.integers(1, rl.M - 1))] if rl.M > 2 else rs[0]
        elif kind == "first":
            f[r, 0, j] = rs[0]
        elif kind == "last":
            f[r, 0, j] = rs[-1]
        elif kind == "below":
            f[r, 0, j] = np.nextafter(rs[0], -np.inf)
        elif kind == "above":
            f[r, 0, j] = np.nextafter(rs[-1], np.inf)
        elif kind == "nan":
            f[r, 0, j] = np.nan
        elif kind == "still":
            f[r, 1, j] = 0.0; f[r, 4, j] = 0.0
        elif kind == "beyond":
            if li != 0:
                continue
            f[r, 3, j] = 45.0          # past the centre of the arc of radius 30
        planted[kind].append((r, j))
    return f, planted


def must_check(planted):
    """The planted samples every comparison with the yardstick includes: on a table point, at either end of the table and
    beyond the centre of curvature (the other kinds are OUTSIDE or stand still: exact defined values, no yardstick)."""
    return [p for k in ("table", "first", "last", "beyond") for p in planted.get(k, [])]


def to_states(f):
    """[R, 6, n] (BTRAPZ_FRENET_SAMPLES) -> [R, 2, n, 3] (BTRAPZ_FRENET_STATES), and the same with leading axes."""
    lead = f.shape[:-2]
    n = f.shape[-1]
    return np.ascontiguousarray(np.moveaxis(f.reshape(lead + (2, 3, n)), -1, -2))


def from_states(x):
    """The inverse of to_states."""
    lead = x.shape[:-3]
    n = x.shape[-2]
    return np.ascontiguousarray(np.moveaxis(x, -1, -2).reshape(lead + (6, n)))


def counts_of(count, R, n):
    return np.full(R, n) if count is None else np.clip(np.asarray(count), 0, n)


def classify(rl, f, count, line_index):
    """read [R, n] (the sample is read), inside [R, n] (read and not OUTSIDE), by the documented rules."""
    R, _, n = f.shape
    cnt = counts_of(count, R, n)
    read = np.arange(n)[None, :] < cnt[:, None]
    inside = np.zeros((R, n), dtype=bool)
    for r in range(R):
        li = 0 if line_index is None else int(line_index[r])
        if 0 <= li < rl.n_lines:
            rs = rl.host["rs"][li]
            inside[r] = read[r] & (f[r, 0] >= rs[0]) & (f[r, 0] <= rs[-1])
    return read, inside


def toleranced(f, inside):
    """The samples held to the yardstick: inside, moving (ds >= 0.5; the yardstick divides by ds)."""
    return inside & (f[:, 1] >= 0.5)


def pick(mask, limit, seed=0, must=()):
    """The samples of `must` that are in mask, ALL of them, and beside them at most `limit` of the other samples of mask:
    always its first and last, the rest drawn with a seed."""
    idx = np.argwhere(mask)
    forced = [(int(r), int(j)) for r, j in must if mask[r, j]]
    if len(idx) <= limit:
        return [tuple(int(v) for v in p) for p in idx]
    rng = np.random.default_rng(seed)
    keep = set(rng.choice(len(idx), limit - 2, replace=False).tolist()) | {0, len(idx) - 1}
    drawn = [tuple(int(v) for v in idx[q]) for q in sorted(keep)]
    return forced + [p for p in drawn if p not in set(forced)]


def yard(rl, f, line_index, r, j):
    li = 0 if line_index is None else int(line_index[r])
    if not hasattr(rl, "_digests"):
        rl._digests = [hashlib.sha1(b"".join(rl.host[k][q].tobytes() for k in cr.FIELDS)).hexdigest() for q in range(rl.n_lines)]
    return YARD.sample(rl._digests[li], line_of(rl, li), f[r, :, j])


def check_forward(rl, f, count, line_index, cart, before=None, limit=200, must=()):
    """cart [R, 6, n] as returned, for f and the row options; before: what cart held before the call (the sentinel
    check of what must not be written).  Returns the worst |error| / bound per output."""
    R, _, n = f.shape
    read, inside = classify(rl, f, count, line_index)
    assert np.isnan(cart[(read & ~inside)[:, None, :].repeat(6, 1)]).all(), "an OUTSIDE sample must be NaN in all six rows"
    valid = inside & ~np.isnan(f).any(1)
    assert not np.isnan(cart[valid[:, None, :].repeat(6, 1)]).any()
    if before is not None:
        keep = (~read)[:, None, :].repeat(6, 1)
        assert (cart[keep].view(np.int64) == before[keep].view(np.int64)).all(), "entries beyond a row's count were written"
    worst = np.zeros(6)
    assert all(toleranced(f, inside)[r, j] for r, j in must), "a planted sample is not read, or not inside: it would not be compared"
    for r, j in pick(toleranced(f, inside), limit, must=must):
        out, J, om, b, _ = yard(rl, f, line_index, r, j)
        err = np.abs(cart[r, :, j] - out)
        assert (err <= b).all(), ("sample", r, j, f[r, :, j], "got", cart[r, :, j], "expected", out, "bound", b)
        worst = np.maximum(worst, err / b)
    return worst


def check_vjp(rl, f, count, line_index, cart_bar, f_bar, limit=200, must=()):
    """f_bar [R, 6, n] against J' cart_bar of the yardstick; 0 (exactly) where nothing was read or the sample is OUTSIDE."""
    read, inside = classify(rl, f, count, line_index)
    zero = (~inside)[:, None, :].repeat(6, 1)
    assert (f_bar[zero] == 0.0).all(), "f_bar must be 0 at samples that are not read or OUTSIDE"
    worst = 0.0
    for r, j in pick(toleranced(f, inside), limit, must=must):
        out, J, om, _, bJ = yard(rl, f, line_index, r, j)
        cb = cart_bar[r, :, j]
        expect, tol = cb @ J, np.abs(cb) @ bJ
        err = np.abs(f_bar[r, :, j] - expect)
        assert (err <= tol).all(), ("sample", r, j, "got", f_bar[r, :, j], "expected", expect, "bound", tol)
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    return worst


def check_jvp(rl, f, count, line_index, f_dot, cart_dot, before=None, limit=200, must=()):
    """cart_dot [T, R, 6, n] against J f_dot of the yardstick; 0 at OUTSIDE samples; untouched beyond a row's count."""
    T = f_dot.shape[0]
    read, inside = classify(rl, f, count, line_index)
    zero = (read & ~inside)[None, :, None, :].repeat(T, 0).repeat(6, 2)
    assert (cart_dot[zero] == 0.0).all(), "cart_dot must be 0 at OUTSIDE samples"
    if before is not None:
        keep = (~read)[None, :, None, :].repeat(T, 0).repeat(6, 2)
        assert (cart_dot[keep].view(np.int64) == before[keep].view(np.int64)).all(), "entries beyond a row's count were written"
    worst = 0.0
    for r, j in pick(toleranced(f, inside), limit, must=must):
        out, J, om, _, bJ = yard(rl, f, line_index, r, j)
        for t in range(T):
            ud = f_dot[t, r, :, j]
            expect, tol = J @ ud, bJ @ np.abs(ud)
            err = np.abs(cart_dot[t, r, :, j] - expect)
            assert (err <= tol).all(), ("sample", r, j, "tangent", t, "got", cart_dot[t, r, :, j], "expected", expect, "bound", tol)
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    return worst


def check_adjoint(f, count, cart_bar, f_bar, f_dot, cart_dot):
    """<cart_bar, J f_dot> = <J' cart_bar, f_dot> over the samples that were read, per tangent: both sides are sums of the
    same 36 products per sample in another order, so they agree to the rounding of sums of that many terms."""
    R, _, n = f.shape
    read = (np.arange(n)[None, :] < counts_of(count, R, n)[:, None])[:, None, :].repeat(6, 1)
    for t in range(f_dot.shape[0]):
        lhs = float((cart_bar[read] * cart_dot[t][read]).sum())
        rhs = float((f_bar * f_dot[t]).sum())
        size = float(np.abs(cart_bar[read] * cart_dot[t][read]).sum() + np.abs(f_bar * f_dot[t]).sum())
        assert abs(lhs - rhs) <= 64 * 36 * 2.0 ** -53 * size + 1e-300, (t, lhs, rhs, size)


AUDIT_ROWS = (("kappa_abs_max", lambda c, w: np.abs(c[3]), np.argmax, -np.inf), ("alat_abs_max", lambda c, w: c[4] * c[4] * np.abs(c[3]), np.argmax, -np.inf),
              ("a_min", lambda c, w: c[5], np.argmin, np.inf), ("a_max", lambda c, w: c[5], np.argmax, -np.inf),
              ("v_max", lambda c, w: c[4], np.argmax, -np.inf), ("frame_min", lambda c, w: w, np.argmin, np.inf))


def ulps(a, b):
    """Distance of two finite float64 arrays in units in the last place."""
    ia, ib = np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)
    key = lambda i: np.where(i < 0, np.int64(-2 ** 63) - i, i)
    return np.abs(key(ia) - key(ib))


def check_audit(rl, f, count, line_index, cart, audit):
    """The audit against NumPy reductions of the call's OWN cart: kappa_abs_max, a_min, a_max, v_max, n_outside and worst
    bit for bit; alat_abs_max and frame_min within 2 units in the last place of the NumPy recomputation (v v |kappa| and
    1 - rkappa l contract differently), their worst sample being one that attains the reported value."""
    R, _, n = f.shape
    read, inside = classify(rl, f, count, line_index)
    assert (audit["n_outside"] == (read & ~inside).sum(1)).all(), (audit["n_outside"], (read & ~inside).sum(1))
    for r in range(R):
        li = 0 if line_index is None else int(line_index[r])
        js = np.flatnonzero(inside[r])
        c = cart[r][:, js]
        w = np.empty(len(js))
        for q, j in enumerate(js):        # the frame factor from the documented lookup, in float64
            ln = line_of(rl, li)
            i = cr.interval(ln["rs"], f[r, 0, j])
            ww = (f[r, 0, j] - ln["rs"][i]) / (ln["rs"][i + 1] - ln["rs"][i])
            w[q] = 1.0 - (ln["rkappa"][i] + ww * (ln["rkappa"][i + 1] - ln["rkappa"][i])) * f[r, 3, j]
        for col, (name, value, arg, nobody) in enumerate(AUDIT_ROWS):
            vals = value(c, w)
            ok = ~np.isnan(vals)
            got, at = audit[name][r], int(audit["worst"][r, col])
            if not ok.any():
                assert got == nobody and at == -1, (name, r, got, at)
                continue
            best = int(js[ok][arg(vals[ok])])
            expect = vals[ok][arg(vals[ok])]
            if name in ("alat_abs_max", "frame_min"):
                assert ulps(got, expect) <= 2, (name, r, got, expect)
                assert at in js and ulps(got, value(cart[r][:, [at]], w[[list(js).index(at)]])[0]) <= 2, (name, r, at)
            else:
                assert np.float64(got).view(np.int64) == np.float64(expect).view(np.int64), (name, r, got, expect)
                assert at == best, (name, r, at, best)
