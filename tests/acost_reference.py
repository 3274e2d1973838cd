"""NumPy restatement of a_cost (spectral_amd/csrc/traj_cost.h: trp_wrapper.cpp:207-286 / cub_wrapper.cpp:201-262) on the
samples of btrapz_sample_device, and its analytic gradient with respect to the control points, the initial state, the
scoring parameters and the reference lines: the yardstick of btrapz_traj_cost_device / btrapz_traj_cost_vjp_device."""
import numpy as np

BC0, BC1, BC2 = np.array([1, 5, 10, 10, 5, 1.0]), np.array([1, 4, 6, 4, 1.0]), np.array([1, 3, 3, 1.0])


def sample_count(t, delta):
    """(np accumulated in double as solve_3d.cc:1279-1282, the int sum + 1 of :1407)."""
    n = 1
    for tk in t:
        n = int(float(n) + tk / delta)
    return n, 1 + sum(int(tk / delta) for tk in t)


def _basis(tau):
    pw, qw = tau ** np.arange(6), (1.0 - tau) ** np.arange(6)
    b0 = BC0 * pw * qw[5::-1]
    b1 = BC1 * pw[:5] * qw[4::-1]
    b2 = BC2 * pw[:4] * qw[3::-1]
    # d sample / d c_j for x (before the factor t), dx, ddx (before the factor 1 / t)
    d1 = np.zeros(6); d1[1:] += 5 * b1; d1[:5] -= 5 * b1
    d2 = np.zeros(6); d2[2:] += 20 * b2; d2[1:5] -= 40 * b2; d2[:4] += 20 * b2
    return b0, d1, d2


def sample_matrix(t, delta):
    """Samples 1..total as linear maps of one axis' 6 S control points: (rows [total, 3, 6 S]) for x, dx, ddx."""
    rows = []
    S = len(t)
    for k in range(S):
        lin = int(t[k] / delta)
        for l in range(1, lin + 1):
            b0, d1, d2 = _basis(l / lin)
            r = np.zeros((3, 6 * S))
            r[0, 6 * k:6 * k + 6] = b0 * t[k]
            r[1, 6 * k:6 * k + 6] = d1
            r[2, 6 * k:6 * k + 6] = d2 / t[k]
            rows.append(r)
    return np.array(rows).reshape(-1, 3, 6 * S)


def samples(t, delta, ctrl, init):
    """s, ds, dds, l, dl, ddl [6, np] (sample 0 = init)."""
    S = len(t)
    M = sample_matrix(t, delta)
    out = np.zeros((6, M.shape[0] + 1))
    out[:, 0] = init
    for ax in range(2):
        c = ctrl[6 * S * ax:6 * S * (ax + 1)]
        out[3 * ax:3 * ax + 3, 1:] = (M @ c).T
    return out


def _terms(variant, p, x, xref_i, ax, dt):
    """(cost, d cost / d(x, dx, ddx) [3, np], d cost / d params-row entries, d cost / d (x - ref) per sample)."""
    s, ds, dds = x
    n = len(s)
    e = s - xref_i
    J = np.empty(n)
    J[0] = ((dds[1] if n > 1 else dds[0]) - dds[0]) / dt
    J[1:] = (dds[1:] - dds[:-1]) / dt
    w = p[4 * ax:4 * ax + 4] if variant == 0 else np.ones(4)
    quartic = variant == 1 and ax == 0
    pw_a = 4 if quartic else 2
    T = np.array([(e * e).sum() * dt, (ds * ds).sum() * dt, (dds ** pw_a).sum() * dt, (J ** pw_a).sum() * dt])
    cost = (w * T).sum()
    g = np.zeros((3, n))
    g[0] = w[0] * 2 * e * dt
    g[1] = w[1] * 2 * ds * dt
    g[2] = w[2] * pw_a * dds ** (pw_a - 1) * dt
    q = w[3] * pw_a * J ** (pw_a - 1)   # d(w J^pw dt)/dJ * (1 / dt)
    if n > 1:
        g[2, 1:] += q[1:]
        g[2, :-1] -= q[1:]
        g[2, 1] += q[0]; g[2, 0] -= q[0]
    if variant == 1:
        a = np.abs(dds)
        m = int(np.argmax(a)) if a.max() > 0 else 0
        M = a.max()
        cost += M ** 4 if ax == 0 else M ** 2
        g[2, m] += (4 * M ** 3 if ax == 0 else 2 * M) * np.sign(dds[m])
    return cost, g, (T if variant == 0 else np.zeros(4)), g[0]


def a_cost(variant, p, t, delta, ctrl, init, s_ref, l_ref, grad=False):
    """a_cost of one candidate: p = the [20] parameter row (layout.Shared.as_array order); t: its S durations; ctrl
    [12 S]; init [6]; s_ref, l_ref [N].  grad: also (cost, dict(ctrl, init, params, s_ref, l_ref)).  None when the
    sample-count check fails."""
    npd, npi = sample_count(t, delta)
    if npd != npi or npd < 1:
        return None
    S, N = len(t), len(s_ref)
    smp = samples(t, delta, ctrl, init)
    n = smp.shape[1]
    ri = np.minimum(np.arange(n), N - 1)
    cost = 0.0
    gsmp = np.zeros_like(smp)
    gp = np.zeros(20)
    gref = [np.zeros(N), np.zeros(N)]
    for ax, ref in enumerate((s_ref, l_ref)):
        c, g, T, ge = _terms(variant, p, smp[3 * ax:3 * ax + 3], ref[ri], ax, delta)
        cost += c
        gsmp[3 * ax:3 * ax + 3] = g
        gp[4 * ax:4 * ax + 4] = T
        np.add.at(gref[ax], ri, -ge)
    if variant == 0:
        ie = min(N - 1, n - 1)
        e = smp[3, ie] - l_ref[N - 1]
        cost += p[9] * e * e * delta
        gp[9] = e * e * delta
        gsmp[3, ie] += p[9] * 2 * e * delta
        gref[1][N - 1] -= p[9] * 2 * e * delta
    if not grad:
        return cost
    M = sample_matrix(t, delta)
    gc = np.zeros(12 * S)
    for ax in range(2):
        gc[6 * S * ax:6 * S * (ax + 1)] = np.einsum("ir,irc->c", gsmp[3 * ax:3 * ax + 3, 1:].T, M)
    return cost, dict(ctrl=gc, init=gsmp[:, 0].copy(), params=gp, s_ref=gref[0], l_ref=gref[1])
