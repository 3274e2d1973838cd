"""The a_cost yardstick (tests/acost_reference.py) on the CPU: against the oracle's orc_sample + orc_acost, both variants,
with the reference-line clamps active; its gradient against central differences; and, on the oracle's exact solve, the
premise of the homogeneity test of tests/test_gpu_acost.py."""
import ctypes as C
import os

import numpy as np
import pytest

from acost_reference import a_cost, sample_count
from helpers import O
from spectral_amd import synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")
W = np.loadtxt(os.path.join(GOLD, "inputs", "weights.txt"))
CASES = [("c1", 0), ("c1", 1), ("c2", 0), ("c3", 1), ("c4", 0)]


def _row(w, inp):
    """weights.txt order -> the [20] parameter row (layout.Shared.as_array order)."""
    return np.array([w[4], w[5], w[0], w[1], w[6], w[7], w[2], w[3], w[8], w[9], inp.ds_ref, inp.dl_ref,
                     *inp.dds, *inp.ddds, *inp.ddl, *inp.dddl])


def _candidate(name, variant):
    path = os.path.join(GOLD, "inputs", name + ".txt")
    inp = O.ParsedInput(path)
    cost, S, ctrl, cubes, info = O.find_traj(variant, path, None, O.params_from_weights(W))
    assert cost < 1e10 and S <= 64
    return inp, cost, ctrl, cubes


def _oracle_acost(variant, inp, cubes, ctrl, N=None, jitter=None):
    rc, smp = O.sample(cubes, inp.delta, ctrl, inp.init_s, inp.init_l)
    assert rc == 0
    raw = inp.raw
    n0 = raw.N
    if N is not None:
        raw.N = N   # (fewer reference knots than samples: the clamps of x_ref[i] and l[N - 1])
    try:
        v = O.lib().orc_acost(variant, C.byref(O.params_from_weights(W)), C.byref(raw), len(smp[0]),
                              *[np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_double)) for a in smp])
    finally:
        raw.N = n0
    return v


@pytest.mark.parametrize("name,variant", CASES)
@pytest.mark.parametrize("clamp", [False, True])
def test_yardstick_matches_the_oracle(name, variant, clamp):
    inp, cost, ctrl, cubes = _candidate(name, variant)
    t = np.array([c.t for c in cubes])
    n_samples, _ = sample_count(t, inp.delta)
    N = max(2, n_samples // 2) if clamp else inp.N
    init = np.concatenate([inp.init_s, inp.init_l])
    rng = np.random.default_rng(len(name) + variant)
    for jitter in (0.0, 0.05):
        c = ctrl * (1 + jitter * rng.standard_normal(ctrl.shape))
        want = _oracle_acost(variant, inp, cubes, c, N=N)
        got = a_cost(variant, _row(W, inp), t, inp.delta, c, init, inp.x_ref[:N], inp.y_ref[:N])
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
        if jitter == 0.0 and not clamp:
            assert abs(got - cost) <= 1e-12 * abs(cost)


@pytest.mark.parametrize("name,variant", CASES)
@pytest.mark.parametrize("clamp", [False, True])
def test_yardstick_gradient_matches_central_differences(name, variant, clamp):
    inp, _, ctrl, cubes = _candidate(name, variant)
    t = np.array([c.t for c in cubes])
    n_samples, _ = sample_count(t, inp.delta)
    N = max(2, n_samples // 2) if clamp else inp.N
    init = np.concatenate([inp.init_s, inp.init_l])
    p = _row(W, inp)
    s_ref, l_ref = inp.x_ref[:N].copy(), inp.y_ref[:N].copy()
    args = dict(ctrl=ctrl.copy(), init=init, params=p, s_ref=s_ref, l_ref=l_ref)
    f = lambda a: a_cost(variant, a["params"], t, inp.delta, a["ctrl"], a["init"], a["s_ref"], a["l_ref"])
    a0, g = a_cost(variant, p, t, inp.delta, ctrl, init, s_ref, l_ref, grad=True)
    rng = np.random.default_rng(3)
    for key in ("ctrl", "init", "params", "s_ref", "l_ref"):
        n = len(args[key])
        idx = sorted(set(rng.choice(n, size=min(n, 12), replace=False).tolist()) | {n - 1})
        if key == "params":
            idx = list(range(10))
        for i in idx:
            h = 1e-6 * (1 + abs(args[key][i]))
            ap = {k: v.copy() for k, v in args.items()}; am = {k: v.copy() for k, v in args.items()}
            ap[key][i] += h; am[key][i] -= h
            fd = (f(ap) - f(am)) / (2 * h)
            scale = max(np.abs(g[key]).max(), 1e-12)
            assert abs(fd - g[key][i]) <= 1e-5 * scale + 1e-7 * abs(a0), (key, i, fd, g[key][i])
    if variant == 1:
        assert (g["params"] == 0).all()


@pytest.mark.parametrize("variant", [0, 1])
def test_doubling_weights_and_ref_end_leaves_the_optimum(variant):
    """The QP's objective is homogeneous of degree 1 in the ten weights and ref_end together (the end term of q
    multiplies ref_end by ds_ref / dl_ref, not by a weight: doubling the weights alone moves x*)."""
    batch, sh = synth.make_scenario1_batch(4, 6, variant, seed=21)
    x1, _, st1, _ = O.batch_solve(batch, sh, exact=True)
    arr = sh.as_array()
    two = synth.Shared(w_s=tuple(2 * arr[0:4]), w_l=tuple(2 * arr[4:8]), weight_end_s=2 * arr[8], weight_end_l=2 * arr[9],
                       ds_ref=sh.ds_ref, dl_ref=sh.dl_ref, dds=sh.dds, ddds=sh.ddds, ddl=sh.ddl, dddl=sh.dddl,
                       delta=sh.delta, variant=sh.variant)
    b2 = synth.Batch(B=batch.B, S=batch.S, seg=batch.seg.copy(), init=batch.init.copy(), ref_end=2 * batch.ref_end,
                     dl_bounds=batch.dl_bounds.copy())
    x2, _, st2, _ = O.batch_solve(b2, two, exact=True)
    ok = (st1 == 1) & (st2 == 1)
    assert ok.sum() >= 2
    assert np.abs(x2[ok] - x1[ok]).max() <= 1e-7 * np.abs(x1[ok]).max()
    b3 = synth.Batch(B=batch.B, S=batch.S, seg=batch.seg.copy(), init=batch.init.copy(), ref_end=batch.ref_end.copy(),
                     dl_bounds=batch.dl_bounds.copy())
    x3, _, st3, _ = O.batch_solve(b3, two, exact=True)
    ok3 = ok & (st3 == 1)
    assert np.abs(x3[ok3] - x1[ok3]).max() > 1e-6 * np.abs(x1[ok3]).max()
