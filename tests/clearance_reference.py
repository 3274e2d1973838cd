"""The yardstick of the clearance stage (include/btrapz_hip_clearance.h), in mpmath at 50 digits.

It is NOT the product's statement in higher precision.  The signed clearance of two rectangles A and B is taken from the
Minkowski difference: the 16 differences b_i - a_j of their vertices are formed in the plane, their convex hull is the
set B - A, and the signed clearance is the signed distance of the origin to that polygon -- positive outside (the
Euclidean distance of the rectangles), negative inside (minus the penetration depth).  One definition covers both
branches and knows nothing of face normals or vertex-to-box distances.  The derivatives are mp.diff of that same function.

mp.diff is exact where the clearance is smooth, and it is smooth where the winner is alone.  `enumerate_pair` evaluates the
PRODUCT'S enumeration (four face gaps, eight vertex-to-box distances) in mpmath, from vertices placed in the plane, only to
say how far the runner-up is: the margin.  Two disjoint features whose witness points coincide (a vertex of A nearest a
vertex of B is also that vertex of B nearest that vertex of A) are the same function and count as one; either name is
accepted for `which`.  The margin of a sample is the smallest of: winner to runner-up feature, winner to runner-up
obstacle, and |g| of the winning pair (the change of branch).

TOLERANCES.  u = 2^-53.  M = |c_A|_1 + |c_B|_1 + the four half extents + |off|.

  Values: |clear - yardstick| <= K u M with K = 32, counted from the product's statement (clearance_core.h) on its longest
  path, the disjoint branch; each rounding is charged u times a magnitude bounded by M:
    sin, cos of both headings (2 u each, the device's sincos)                     -> enters the products below
    c_A = p + off (cos, sin): 1 product (3 u |off| with the cosine's error), 1 sum
    d = c_B - c_A: 1 difference; so far d carries <= u (2 |c_A|_1 + |c_B|_1 + 5 |off|) ...................  <= 5
    d in a frame: 2 products, 1 sum, the frame's cos / sin (2 u): 4 u |d|_1, and the error of d
      arrives times (|cos| + |sin|) <= 1.42 ..........................................................  <= 4 + 1.42 * 5
    c and s of the heading difference: 2 products of (2 + 2 + 1) u, 1 sum: 6 u; a vertex coordinate
      a_x c + a_y s - d_u: 2 products, 2 sums: 7 u (h_l + h_w) + 2 u (h_l + h_w + |d|) ....................  <= 9
    q = |p| - h: 1 difference ........................................................................  <= 1
    per component of q: 5 + 4 + 7.1 + 9 + 1 < 20 (the terms overlap in what M they charge: this adds them anyway);
    sqrt(m0^2 + m1^2): the two components' errors combine to <= 1.42 * 20 u M, and 2 products, 1 sum, 1 square root
      add 2.5 u times the distance, itself <= M .......................................................  28.4 + 2.5 < 32
  The overlap branch is shorter (no vertex, no square root) and is held to the same K.

  Derivatives (the four numbers n_x, n_y, lever_A, lever_B of a sample): |J - yardstick| <= K_D u (1 + M) (1 + (1 + L) / rho),
  K_D = 32, L = the larger lever arm |W - P_A|, |W - c_B| of the witness point, rho = the clearance when the winner is a
  vertex against a vertex (both offsets positive: the direction is m / |m| and inherits the error of m, <= 28.4 u M by the
  count above, divided by |m| = rho, twice for numerator and norm) and infinity otherwise (the direction is a rectangle's
  own axis: 4 u).  The lever arms are cross products of W (error <= 5 u M, the error of d) with n: L err(n) + 5 u M + 3 u L.

  TAU = 1e-9 (metres): derivative comparisons skip samples whose margin is below it; value comparisons skip nothing."""
import mpmath as mp

mp.mp.dps = 50

K_VALUE = 32
K_GRAD = 32
TAU = mp.mpf("1e-9")
U = mp.mpf(2) ** -53
SIGNS = ((1, 1), (-1, 1), (-1, -1), (1, -1))   # the vertex order of the header


def _f(v):
    return mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v


def rect_vertices(cx, cy, th, hl, hw):
    c, s = mp.cos(th), mp.sin(th)
    return [(cx + sx * hl * c - sy * hw * s, cy + sx * hl * s + sy * hw * c) for sx, sy in SIGNS]


def ego_rect(pose, foot):
    """pose (x, y, theta), foot (half_length, half_width, centre_offset) -> (cx, cy, theta, hl, hw)."""
    x, y, th = [_f(v) for v in pose]
    hl, hw, off = [_f(v) for v in foot]
    return x + off * mp.cos(th), y + off * mp.sin(th), th, hl, hw


def _hull(points):
    """Andrew's monotone chain, counter-clockwise, collinear points dropped."""
    pts = sorted(set(points))
    if len(pts) < 3:
        return pts
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def _origin_to_segment(a, b):
    ex, ey = b[0] - a[0], b[1] - a[1]
    t = -(a[0] * ex + a[1] * ey) / (ex * ex + ey * ey)
    t = min(max(t, mp.mpf(0)), mp.mpf(1))
    return mp.hypot(a[0] + t * ex, a[1] + t * ey)


def rect_clearance(ra, rb):
    """The signed distance of the origin to the hull of the 16 vertex differences of rectangles ra, rb = (cx, cy, theta,
    hl, hw)."""
    va, vb = rect_vertices(*ra), rect_vertices(*rb)
    h = _hull([(b[0] - a[0], b[1] - a[1]) for a in va for b in vb])
    m = len(h)
    inside = True
    dist = None
    for i in range(m):
        a, b = h[i], h[(i + 1) % m]
        if a[0] * b[1] - a[1] * b[0] < 0:      # the origin lies to the right of a counter-clockwise edge
            inside = False
        d = _origin_to_segment(a, b)
        dist = d if dist is None or d < dist else dist
    return -dist if inside else dist


def pair_clearance(pose, foot, obs):
    """Ego pose (x, y, theta), footprint, obstacle (ox, oy, otheta, hl, hw) -> the signed clearance (the yardstick)."""
    return rect_clearance(ego_rect(pose, foot), tuple(_f(v) for v in obs))


# ---- the product's enumeration, only for margins and for the names of features ----
def _to_box(p, rect):
    """The point p against the box rect: (distance, the nearest point of the box)."""
    cx, cy, th, hl, hw = rect
    c, s = mp.cos(th), mp.sin(th)
    u, n = (p[0] - cx) * c + (p[1] - cy) * s, -(p[0] - cx) * s + (p[1] - cy) * c
    cu, cn = min(max(u, -hl), hl), min(max(n, -hw), hw)
    return mp.hypot(u - cu, n - cn), (cx + cu * c - cn * s, cy + cu * s + cn * c), (abs(u) > hl and abs(n) > hw)


def enumerate_pair(pose, foot, obs):
    """-> dict(g = the four face gaps, value, feature = the product's winner, same = the features that are the same
    function as the winner, margin, lever = (|W - P_A|, |W - c_B|) of the winner's witness, corner = the winner is a
    vertex against a vertex)."""
    ra, rb = ego_rect(pose, foot), tuple(_f(v) for v in obs)
    px, py = _f(pose[0]), _f(pose[1])
    dx, dy = rb[0] - ra[0], rb[1] - ra[1]
    g = []
    for (cx, cy, th, hl, hw), k in ((ra, 0), (ra, 1), (rb, 0), (rb, 1)):
        ex, ey = (mp.cos(th), mp.sin(th)) if k == 0 else (-mp.sin(th), mp.cos(th))
        rad = lambda r: r[3] * abs(ex * mp.cos(r[2]) + ey * mp.sin(r[2])) + r[4] * abs(-ex * mp.sin(r[2]) + ey * mp.cos(r[2]))
        g.append(abs(ex * dx + ey * dy) - rad(ra) - rad(rb))
    gmax = max(g)
    lever = lambda w: (mp.hypot(w[0] - px, w[1] - py), mp.hypot(w[0] - rb[0], w[1] - rb[1]))
    if gmax <= 0:
        k = g.index(gmax)
        rest = sorted(g, reverse=True)[1]
        # the witness: some point of the contact; its lever arms are bounded by the rectangles' reach
        reach = mp.hypot(dx, dy) + mp.hypot(ra[3], ra[4]) + mp.hypot(rb[3], rb[4]) + abs(_f(foot[2]))
        return dict(g=g, value=gmax, feature=k, same={k}, margin=min(gmax - rest, -gmax), lever=(reach, reach), corner=False)
    va, vb = rect_vertices(*ra), rect_vertices(*rb)
    feats = []
    for i in range(4):
        d, q, corner = _to_box(va[i], rb)
        feats.append((d, va[i], q, corner))
    for i in range(4):
        d, q, corner = _to_box(vb[i], ra)
        feats.append((d, q, vb[i], corner))
    best = min(f[0] for f in feats)
    k = [f[0] for f in feats].index(best)
    close = lambda p, q: abs(p[0] - q[0]) + abs(p[1] - q[1]) < mp.mpf("1e-30")
    same = {4 + i for i, f in enumerate(feats) if close(f[1], feats[k][1]) and close(f[2], feats[k][2])}
    others = [f[0] for i, f in enumerate(feats) if 4 + i not in same]
    margin = min(min(others) - best if others else mp.inf, gmax)
    wa, wb = feats[k][1], feats[k][2]
    la, lb = lever(wa if k < 4 else wb), lever(wa if k < 4 else wb)
    return dict(g=g, value=best, feature=4 + k, same=same, margin=margin, lever=(la[0], lb[1]), corner=feats[k][3])


def magnitude(pose, foot, obs):
    ra = ego_rect(pose, foot)
    return abs(ra[0]) + abs(ra[1]) + abs(_f(obs[0])) + abs(_f(obs[1])) + ra[3] + ra[4] + _f(obs[3]) + _f(obs[4]) + abs(_f(foot[2]))


def sample(pose, foot, obstacles):
    """One ego sample against its scene.  obstacles: a list of (ox, oy, otheta, hl, hw) in the scene's order, None or a
    NaN pose for an absent one.  -> dict(clear = the yardstick's clearance (+inf: nobody), obstacle, which = the set of
    accepted names, margin, value_bound, grad_bound, present)."""
    best = None
    vals = []
    for o, ob in enumerate(obstacles):
        if ob is None or any(v != v for v in ob[:3]):
            continue
        vals.append((pair_clearance(pose, foot, ob), o))
    if not vals:
        return dict(clear=mp.inf, obstacle=-1, which={-1}, margin=mp.inf, value_bound=mp.mpf(0), grad_bound=mp.mpf(0), present=0)
    best = min(vals)                                  # (value, lowest obstacle on a tie)
    o = best[1]
    e = enumerate_pair(pose, foot, obstacles[o])
    runner = min([v for v, oo in vals if oo != o], default=mp.inf)
    mag = magnitude(pose, foot, obstacles[o])
    rho = e["value"] if e["corner"] else mp.inf
    return dict(clear=best[0], obstacle=o, which={o * 16 + k for k in e["same"]}, margin=min(e["margin"], runner - best[0]),
                value_bound=K_VALUE * U * mag, present=len(vals),
                grad_bound=K_GRAD * U * (1 + mag) * (1 + (1 + max(e["lever"])) / rho))


def gradient(pose, foot, ob):
    """mp.diff of the yardstick in (x, y, theta) of the ego and (ox, oy, otheta) of the obstacle: six numbers; in the
    product's terms (n_x, n_y, lever_A, -n_x, -n_y, -lever_B)."""
    pose = [_f(v) for v in pose]
    ob = [_f(v) for v in ob]
    out = []
    for i in range(3):
        out.append(mp.diff(lambda t: pair_clearance(pose[:i] + [t] + pose[i + 1:], foot, ob), pose[i]))
    for i in range(3):
        out.append(mp.diff(lambda t: pair_clearance(pose, foot, ob[:i] + [t] + ob[i + 1:]), ob[i]))
    return out
