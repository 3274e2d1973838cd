"""Yardstick of the prism stage's backward pass (btrapz_prism_bounds_vjp_device, btrapz_prism_bounds_vjp_host).

The map of oracle/prism_oracle.py restated in numpy WITHOUT the two-decimal rounding of the faces, for one scene given as
its prisms array [P, 8] (s0, l0, t0, vel_s, vel_l, T, active, -).  The discrete decisions are taken ONCE at the base point
and held (freeze): the active flags, ahead = (t0 == 0), window membership per knot, the vel_l >= 0 branch, the order of the
distinct edges and the candidate that supplied each (the lowest-index one: l_min of cars 0..P-1, l_max of cars 0..P-1, the
road), the cars that cover a strip.  The max / min over a strip's cars are evaluated LIVE on the unrounded faces
s0 -+ l_safe + vel_s (i / 10 - t0), the first covering car replacing the road's limits as the forward has it.

The Jacobian comes from central differences of that map, h = 1e-6 per parameter.  The frozen map is at most bilinear in
each parameter, so central differences have no truncation error and the tolerance of an entry is the rounding bound,
computed as tests/corridor_vjp_reference.py computes it:  4 * sum_r |ybar_r| * 4 ulp(|y_r|) / (2 h).
A column is SKIPPED when +-h flips a max / min winner, and the face columns (s0, t0, vel_s, T) of a car are skipped when,
somewhere, the winner the forward takes (on the ROUNDED faces) is not the winner on the unrounded ones and the car is one of
the two: there the rounding alone decides, and the backward follows the forward.  check_cap() holds the skipped columns of a
set of scenes to 2 % of the active cars' columns."""
import numpy as np

from oracle import prism_oracle as PO

H_STEP = 1e-6
S_LO, S_HI, L_LO, L_HI = 0.0, 50.0, -2.0, 8.0     # CRoad.reference(), prism_oracle.prism_bounds' defaults
RATE = 10.0
FACE_COLUMNS = (0, 2, 3, 5)


def car_dict(row):
    return dict(centre=(float(row[0]), float(row[1]), float(row[2])), vel_s=float(row[3]), vel_l=float(row[4]), time=float(row[5]))


def active_cars(pr):
    """The oracle's input: the active slots of pr [P, 8], in slot order."""
    return [car_dict(r) for r in pr if r[6] != 0.0]


class Frozen:
    pass


def freeze(pr, N):
    """The decisions of the scene pr [P, 8] at N knots, taken as the forward takes them."""
    P = pr.shape[0]
    f = Frozen()
    f.P, f.N = P, N
    f.active = [bool(pr[q, 6] != 0.0) for q in range(P)]
    f.ahead = [bool(pr[q, 2] == 0.0) for q in range(P)]
    f.branch = [bool(pr[q, 4] >= 0) for q in range(P)]
    ext = [PO.lateral_extent(car_dict(pr[q])) for q in range(P)]
    cand = [e[0] for e in ext] + [e[1] for e in ext]
    on = f.active + f.active
    live = [v for v, o in zip(cand, on) if o]
    cand += [L_LO, L_HI]
    on = on + [(min(live) if live else 1e300) > L_LO, (max(live) if live else -1e300) < L_HI]
    firsts = [c for c in range(2 * P + 2) if on[c] and not any(on[j] and cand[j] == cand[c] for j in range(c))]
    f.supplier = sorted(firsts, key=lambda c: cand[c])          # edge j <- candidate supplier[j]
    f.edges = [cand[c] for c in f.supplier]
    f.strips = max(len(f.edges) - 1, 0)
    f.cover = [[q for q in range(P) if f.active[q] and ext[q][0] <= f.edges[j] and f.edges[j + 1] <= ext[q][1]] for j in range(f.strips)]
    i = np.arange(N)
    f.inside = [~((i < pr[q, 2] * RATE) | (i > (pr[q, 2] + pr[q, 5]) * RATE)) for q in range(P)]
    f.rounded = []
    for q in range(P):
        s0, t0, vs, T = pr[q, 0], pr[q, 2], pr[q, 3], pr[q, 5]
        fs = s0 + vs * T
        y1, y2 = (s0 - PO.L_SAFE, fs - PO.L_SAFE) if f.ahead[q] else (s0 + PO.L_SAFE, fs + PO.L_SAFE)
        with np.errstate(all="ignore"):
            f.rounded.append(np.array(PO.face_line(float(t0), float(y1), float(t0 + T), float(y2), N)) if f.active[q] and T != 0 else np.zeros(N))
    return f


def faces(f, x):
    """The unrounded faces [P, N] at the parameters x [P, 6]."""
    t = np.arange(f.N) / RATE
    sign = np.array([-1.0 if a else 1.0 for a in f.ahead])
    return x[:, 0:1] + sign[:, None] * PO.L_SAFE + x[:, 3:4] * (t[None, :] - x[:, 2:3])


def edge_values(f, x):
    out = []
    for c in f.supplier:
        if c >= 2 * f.P:
            out.append(L_LO if c == 2 * f.P else L_HI)
            continue
        q = c % f.P
        l0, vl, T = x[q, 1], x[q, 4], x[q, 5]
        moving = l0 + vl * T
        if c < f.P:
            out.append(l0 - PO.W_SAFE if f.branch[q] else moving - PO.W_SAFE)
        else:
            out.append(moving + PO.W_SAFE if f.branch[q] else l0 + PO.W_SAFE)
    return out


def strips_of(f, face):
    """(s [strips, N, 2], winners [strips, N, 2]) for the face values face [P, N]: the forward's walk, winners tracked."""
    N = f.N
    s = np.zeros((f.strips, N, 2)); w = np.full((f.strips, N, 2), -1, dtype=np.int64)
    for j in range(f.strips):
        lo = np.full(N, S_LO); hi = np.full(N, S_HI)
        wl = np.full(N, -1); wh = np.full(N, -1)
        first = True
        for q in f.cover[j]:
            take_lo = f.inside[q] & (not f.ahead[q]); take_hi = f.inside[q] & f.ahead[q]
            c_lo = np.where(take_lo, face[q], S_LO); c_hi = np.where(take_hi, face[q], S_HI)
            q_lo = np.where(take_lo, q, -1); q_hi = np.where(take_hi, q, -1)
            if first:
                lo, hi, wl, wh, first = c_lo, c_hi, q_lo, q_hi, False
            else:
                m = c_lo > lo; lo = np.where(m, c_lo, lo); wl = np.where(m, q_lo, wl)
                m = c_hi < hi; hi = np.where(m, c_hi, hi); wh = np.where(m, q_hi, wh)
        s[j, :, 0], s[j, :, 1], w[j, :, 0], w[j, :, 1] = lo, hi, wl, wh
    return s, w


def evaluate(f, x):
    """The frozen map at x [P, 6]: (s [strips, N, 2], l [strips, N, 2], winners)."""
    s, w = strips_of(f, faces(f, x))
    e = edge_values(f, x)
    l = np.zeros((f.strips, f.N, 2))
    for j in range(f.strips):
        l[j, :, 0], l[j, :, 1] = e[j], e[j + 1]
    return s, l, w


_cache = {}


def jacobian(pr, N, key=None):
    """Central differences of the scene's frozen map: dict with strips, y [rows] (s then l, flat), s, l, J [rows, P * 6],
    skipped [P * 6], columns (the active cars').  Computed once per `key` and shared."""
    if key is not None and key in _cache:
        return _cache[key]
    pr = np.asarray(pr, dtype=np.float64)
    P = pr.shape[0]
    f = freeze(pr, N)
    x0 = pr[:, :6].copy()
    s0, l0, w0 = evaluate(f, x0)
    y0 = np.concatenate([s0.ravel(), l0.ravel()])
    J = np.zeros((y0.size, P * 6)); skipped = np.zeros(P * 6, dtype=bool)
    _, w_round = strips_of(f, np.array(f.rounded).reshape(P, N))
    for a, b in {(int(a), int(b)) for a, b in zip(w0[w0 != w_round], w_round[w0 != w_round])}:
        for q in (a, b):
            if q >= 0:
                skipped[[q * 6 + k for k in FACE_COLUMNS]] = True
    for q in range(P):
        if not f.active[q]:
            continue
        for k in range(6):
            c = q * 6 + k
            if skipped[c]:
                continue
            x = x0.copy(); x[q, k] = x0[q, k] + H_STEP; sp, lp, wp = evaluate(f, x)
            x[q, k] = x0[q, k] - H_STEP; sm, lm, wm = evaluate(f, x)
            if not (np.array_equal(wp, w0) and np.array_equal(wm, w0)):
                skipped[c] = True
                continue
            J[:, c] = (np.concatenate([sp.ravel(), lp.ravel()]) - np.concatenate([sm.ravel(), lm.ravel()])) / (2 * H_STEP)
    out = dict(strips=f.strips, y=y0, s=s0, l=l0, J=J, skipped=skipped, columns=6 * sum(f.active), frozen=f)
    if key is not None:
        _cache[key] = out
    return out


def flat_cotangent(jac, s_bar, l_bar):
    """The cotangent of y from s_bar, l_bar [O, N, 2] (None: zero): the strips the scene has; padding strips are ignored."""
    n = jac["strips"]
    N = jac["frozen"].N
    z = np.zeros((n, N, 2))
    return np.concatenate([(z if s_bar is None else s_bar[:n]).ravel(), (z if l_bar is None else l_bar[:n]).ravel()])


def reference_gradient(jac, s_bar, l_bar, O):
    """(prisms_bar [P, 8], tolerance) for cotangents s_bar, l_bar [O, N, 2]; zeros when the scene has more than O strips."""
    P = jac["frozen"].P
    g = np.zeros((P, 8))
    if jac["strips"] > O:
        return g, 0.0
    ybar = flat_cotangent(jac, s_bar, l_bar)
    g[:, :6] = (jac["J"].T @ ybar).reshape(P, 6)
    ulp = np.spacing(np.abs(jac["y"]))
    return g, 4.0 * float(np.sum(np.abs(ybar) * 4.0 * ulp)) / (2 * H_STEP)


def check_cap(jacs):
    """At most 2 % of the active cars' columns of these scenes are skipped."""
    total = sum(j["columns"] for j in jacs); skipped = sum(int(j["skipped"].sum()) for j in jacs)
    assert total > 0 and skipped <= 0.02 * total, (skipped, total)
    return skipped, total


def compare(jac, got, s_bar, l_bar, O, what=""):
    """got [P, 8] against the reference on every column that is not skipped; returns the worst error / tolerance."""
    g, tol = reference_gradient(jac, s_bar, l_bar, O)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == g.shape and not got[:, 6:].any(), (what, got[:, 6:])
    keep = ~jac["skipped"].reshape(-1, 6)
    err = np.abs(got[:, :6] - g[:, :6])
    if tol == 0.0:
        assert not got.any(), (what, got)
        return 0.0
    bad = np.argwhere(keep & (err > tol))
    assert bad.size == 0, (what, bad[:5], got[:, :6][keep & (err > tol)][:5], g[:, :6][keep & (err > tol)][:5], tol)
    return float((err[keep] / tol).max()) if keep.any() else 0.0
