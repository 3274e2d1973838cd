"""NumPy restatement of the two linear maps from control points to what a caller looks at, and of their transposes: the
yardstick of btrapz_sample_vjp_device and btrapz_eval_states_vjp_device.

Sampling builds on sample_matrix / sample_count of tests/acost_reference.py (the forward of btrapz_sample_device).  The
state evaluation restates eval_states_kernel's branches (spectral_amd/csrc/btrapz_kernels.hip): a time that is not > 0 is
clamped to 0, the walk `while k < S - 1 and rem > t[k]` finds the segment, and beyond the last segment the end state is
extrapolated at constant velocity.  Conventions are the forward's: position is the Bernstein sum TIMES the duration,
velocity is unscaled, acceleration is DIVIDED by the duration."""
import numpy as np

from acost_reference import _basis, sample_count, sample_matrix


# ---- sampling ---------------------------------------------------------------------------------------------------------
def sample_forward(t, delta, ctrl, init, max_points, absolute=False):
    """The rows btrapz_sample_device writes for one candidate: (out [6, max_points], npoints).  Sample 0 is init, rows at
    index >= max_points are not written (they stay 0).  absolute: with |J| in place of J (the scale of a rounding
    bound, for |ctrl| and |init|)."""
    S = len(t)
    M = sample_matrix(t, delta)
    if absolute:
        M = np.abs(M)
    out = np.zeros((6, max_points))
    out[:, 0] = init
    n = min(M.shape[0], max_points - 1)
    for ax in range(2):
        out[3 * ax:3 * ax + 3, 1:1 + n] = (M[:n] @ ctrl[6 * S * ax:6 * S * (ax + 1)]).T
    return out, sample_count(t, delta)[0]


def sample_vjp(t, delta, out_bar, absolute=False):
    """Transpose of sample_forward for the cotangent out_bar [6, max_points]: (ctrl_bar [12 S], init_bar [6]).  Rows at
    and beyond min(max_points, npoints) are ignored.  absolute: |J|^T |out_bar| instead (the scale of the rounding
    bound)."""
    S = len(t)
    max_points = out_bar.shape[1]
    M = sample_matrix(t, delta)
    npd = sample_count(t, delta)[0]
    n = max(0, min(M.shape[0], max_points - 1, npd - 1))
    g = np.abs(out_bar) if absolute else out_bar
    Mn = np.abs(M[:n]) if absolute else M[:n]
    cb = np.zeros(12 * S)
    for ax in range(2):
        cb[6 * S * ax:6 * S * (ax + 1)] = np.einsum("ri,irc->c", g[3 * ax:3 * ax + 3, 1:1 + n], Mn)
    return cb, g[:, 0].copy()


def samples_per_segment(t, delta):
    return max(int(tk / delta) for tk in t)


# ---- state evaluation -------------------------------------------------------------------------------------------------
def walk(t, time):
    """eval_states_kernel's float walk for one time: (k, rem, over, clamped) -- the segment, the time left inside it,
    the time beyond the horizon (0 inside it) and whether the time was not > 0."""
    S = len(t)
    rem = time
    clamped = not (rem > 0.0)
    if clamped:
        rem = 0.0
    k = 0
    while k < S - 1 and rem > t[k]:
        rem -= t[k]
        k += 1
    over = rem - t[k] if rem > t[k] else 0.0
    return k, rem, over, clamped


def locate(t, time):
    """eval_states_kernel's branches for one time: (k, tau, over, clamped)."""
    k, rem, over, clamped = walk(t, time)
    tau = 1.0 if over > 0.0 else rem / t[k]
    return k, tau, over, clamped


def state_rows(t, time):
    """(k, R [3, 6], clamped, beyond): p, v, a of one axis at `time` as R @ c_k (the 6 control points of segment k)."""
    k, tau, over, clamped = locate(t, time)
    b0, d1, d2 = _basis(tau)
    beyond = over > 0.0
    R = np.zeros((3, 6))
    R[0] = b0 * t[k] + d1 * over
    R[1] = d1
    if not beyond:
        R[2] = d2 / t[k]
    return k, R, clamped, beyond, tau


def states_forward(t, ctrl, times):
    """x [2, n_times, 3] of one candidate (ctrl [12 S])."""
    S = len(t)
    x = np.zeros((2, len(times), 3))
    for j, tm in enumerate(times):
        k, R, _, _, _ = state_rows(t, tm)
        for ax in range(2):
            x[ax, j] = R @ ctrl[6 * S * ax + 6 * k:6 * S * ax + 6 * k + 6]
    return x


def states_matrix(t, times):
    """J [2 * n_times * 3, 12 S]: x.ravel() = J @ ctrl."""
    S = len(t)
    J = np.zeros((2, len(times), 3, 12 * S))
    for j, tm in enumerate(times):
        k, R, _, _, _ = state_rows(t, tm)
        for ax in range(2):
            J[ax, j, :, 6 * S * ax + 6 * k:6 * S * ax + 6 * k + 6] = R
    return J.reshape(-1, 12 * S)


def _jerk_row(tau, tk):
    """d a / d time as a row on the segment's control points: the third Bezier derivative over t^2."""
    om = 1.0 - tau
    b2 = np.array([om * om, 2 * tau * om, tau * tau])
    r = np.zeros(6)
    for i in range(3):
        r[i + 3] += 60 * b2[i]; r[i + 2] -= 180 * b2[i]; r[i + 1] += 180 * b2[i]; r[i] -= 60 * b2[i]
    return r / (tk * tk)


def states_time_derivative(t, ctrl, times, absolute=False):
    """d x / d time [2, n_times, 3] along the trajectory: (v, a, jerk) inside a segment, (v, 0, 0) beyond the horizon, 0
    for a time that is not > 0.  absolute: the sums of absolute values of the terms instead."""
    S = len(t)
    d = np.zeros((2, len(times), 3))
    for j, tm in enumerate(times):
        k, R, clamped, beyond, tau = state_rows(t, tm)
        if clamped:
            continue
        rows = [R[1]] if beyond else [R[1], _basis(tau)[2] / t[k], _jerk_row(tau, t[k])]
        for ax in range(2):
            c = ctrl[6 * S * ax + 6 * k:6 * S * ax + 6 * k + 6]
            for q, r in enumerate(rows):
                d[ax, j, q] = (np.abs(r) @ np.abs(c)) if absolute else (r @ c)
    return d


def states_vjp(t, ctrl, times, x_bar, absolute=False):
    """(ctrl_bar [12 S], times_bar [n_times]) for the cotangent x_bar [2, n_times, 3]; absolute: from absolute values."""
    J = states_matrix(t, times)
    g = x_bar.reshape(-1)
    cb = (np.abs(J).T @ np.abs(g)) if absolute else (J.T @ g)
    d = states_time_derivative(t, ctrl, times, absolute=absolute)
    tb = ((np.abs(x_bar) if absolute else x_bar) * d).sum(axis=(0, 2))
    return cb, tb
