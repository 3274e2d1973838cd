"""The yardstick of the sampling and state gradients (tests/states_reference.py) on the CPU, checked before anything is
checked against it: its forwards reproduce the oracle's samples and the Bezier formula, its transposes satisfy the
adjoint identity, and its time derivative matches central differences of its own forward off the branch points."""
import os
from math import comb

import numpy as np
import pytest

import states_reference as R
from helpers import O

GOLD = os.path.join(os.path.dirname(__file__), "golden")
W = np.loadtxt(os.path.join(GOLD, "inputs", "weights.txt"))
CASES = [("c1", 0), ("c1", 1), ("c2", 0), ("c3", 1), ("c4", 0)]


def _candidate(name, variant):
    path = os.path.join(GOLD, "inputs", name + ".txt")
    inp = O.ParsedInput(path)
    cost, S, ctrl, cubes, info = O.find_traj(variant, path, None, O.params_from_weights(W))
    assert cost < 1e10 and S <= 64
    return inp, np.asarray(ctrl, dtype=np.float64), cubes


def bezier_state(c, t, tau):
    """(tests/test_gpu_warm_start.py restates the same formula)"""
    B = lambda n, i: comb(n, i) * tau ** i * (1 - tau) ** (n - i)
    p = t * sum(c[i] * B(5, i) for i in range(6))
    v = sum(5 * (c[i + 1] - c[i]) * B(4, i) for i in range(5))
    a = sum(20 * (c[i + 2] - 2 * c[i + 1] + c[i]) * B(3, i) for i in range(4)) / t
    return np.array([p, v, a])


@pytest.mark.parametrize("name,variant", CASES)
def test_sampling_forward_reproduces_the_oracle(name, variant):
    inp, ctrl, cubes = _candidate(name, variant)
    t = np.array([c.t for c in cubes])
    init = np.concatenate([inp.init_s, inp.init_l])
    rc, smp = O.sample(cubes, inp.delta, ctrl, inp.init_s, inp.init_l)
    assert rc == 0
    want = np.array([np.asarray(a, dtype=np.float64) for a in smp])
    n = want.shape[1]
    got, npts = R.sample_forward(t, inp.delta, ctrl, init, n + 3)
    assert npts == n
    # both sides sum the same 6 (5, 4) products per entry: compare against the sum of their magnitudes
    scale, _ = R.sample_forward(t, inp.delta, np.abs(ctrl), np.abs(init), n + 3, absolute=True)
    assert (np.abs(got[:, :n] - want) <= 1e-13 * scale[:, :n]).all(), (np.abs(got[:, :n] - want) / scale[:, :n]).max()
    assert (got[:, n:] == 0).all()
    # a max_points that truncates writes the leading rows only
    cut, _ = R.sample_forward(t, inp.delta, ctrl, init, n // 2)
    assert np.array_equal(cut, got[:, :n // 2])


@pytest.mark.parametrize("name,variant", CASES[:3])
def test_states_forward_reproduces_the_bezier_formula(name, variant):
    inp, ctrl, cubes = _candidate(name, variant)
    t = np.array([c.t for c in cubes])
    S = len(t)
    edges = np.concatenate([[0.0], np.cumsum(t)])
    rng = np.random.default_rng(3)
    times = rng.uniform(0.0, 1.0, 9) * edges[-1]
    times[0] = 0.0; times[1] = edges[-1] + 0.35; times[2] = -1.0
    x = R.states_forward(t, ctrl, times)
    for j, tm in enumerate(times):
        tm = max(tm, 0.0)
        for ax in range(2):
            c = ctrl[6 * S * ax:6 * S * (ax + 1)].reshape(S, 6)
            if tm > edges[-1]:
                e = bezier_state(c[S - 1], t[S - 1], 1.0)
                want = np.array([e[0] + e[1] * (tm - edges[-1]), e[1], 0.0])
            else:
                k = max(min(int(np.searchsorted(edges, tm, side="left")) - 1, S - 1), 0) if tm > 0 else 0
                want = bezier_state(c[k], t[k], (tm - edges[k]) / t[k])
            assert np.allclose(x[ax, j], want, rtol=1e-11, atol=1e-11), (j, ax, x[ax, j], want)


@pytest.mark.parametrize("S", [1, 3, 10])
def test_transposes_satisfy_the_adjoint_identity(S):
    rng = np.random.default_rng(10 + S)
    t = rng.uniform(0.35, 1.6, S)
    delta = 0.1
    c = rng.standard_normal(12 * S)
    init = rng.standard_normal(6)
    # sampling: <J (c, init), v> = <(c, init), J^T v>, also when max_points truncates
    total = sum(int(tk / delta) for tk in t)
    for mp in (total + 3, max(2, total // 2)):
        v = rng.standard_normal((6, mp))
        out, npts = R.sample_forward(t, delta, c, init, mp)
        cb, ib = R.sample_vjp(t, delta, v)
        lhs = (out[:, :npts] * v[:, :npts]).sum()
        rhs = c @ cb + init @ ib
        scale = np.abs(out).ravel() @ np.abs(v).ravel()
        assert abs(lhs - rhs) <= 1e-13 * scale, (lhs, rhs)
    # states: times inside, on the clamp, beyond the horizon
    times = np.concatenate([rng.uniform(0, t.sum(), 7), [-0.5, 0.0, t.sum() + 0.7]])
    x = R.states_forward(t, c, times)
    v = rng.standard_normal(x.shape)
    cb, _ = R.states_vjp(t, c, times, v)
    scale = np.abs(x).ravel() @ np.abs(v).ravel()
    assert abs((x * v).sum() - c @ cb) <= 1e-13 * scale
    assert np.allclose(R.states_matrix(t, times) @ c, x.ravel(), rtol=0, atol=1e-13 * np.abs(x).max())


@pytest.mark.parametrize("S", [1, 4, 10])
def test_time_derivative_matches_central_differences_off_the_branch_points(S):
    rng = np.random.default_rng(20 + S)
    t = rng.uniform(0.35, 1.6, S)
    c = rng.standard_normal(12 * S)
    joints = np.concatenate([[0.0], np.cumsum(t)])
    times, steps = [], []
    for k in range(S):
        for f in (0.137, 0.61):
            times.append(joints[k] + f * t[k]); steps.append(1e-6 * t[k])
    times.append(joints[-1] + 0.5); steps.append(1e-6 * t[-1])
    times, steps = np.array(times), np.array(steps)
    branch = np.concatenate([joints, [0.0]])
    left_out = sum(1 for tm, h in zip(times, steps) if np.abs(branch - tm).min() <= h)
    assert left_out == 0
    d = R.states_time_derivative(t, c, times)
    mag = R.states_time_derivative(t, c, times, absolute=True)
    for j, (tm, h) in enumerate(zip(times, steps)):
        fd = (R.states_forward(t, c, [tm + h])[:, 0] - R.states_forward(t, c, [tm - h])[:, 0]) / (2 * h)
        x0 = np.abs(R.states_forward(t, c, [tm])[:, 0])
        # central differences: truncation h^2 / 6 of the next derivatives (bounded through mag) and rounding eps |x| / h
        tol = 1e-7 * (mag[:, j] + mag[:, j].max()) + 4 * 2.3e-16 * (x0 + x0.max()) / h + 1e-9
        assert (np.abs(fd - d[:, j]) <= tol).all(), (j, fd, d[:, j], tol)
    # a clamped time does not move the state
    assert (R.states_time_derivative(t, c, np.array([-1.0, 0.0])) == 0).all()
