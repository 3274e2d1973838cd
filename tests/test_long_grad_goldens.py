"""tests/golden/long_grad_yardstick.npz held to its generator (tests/golden/make_long_grad_goldens.py) without a GPU and without
the exact solves that make it slow (15 s a candidate at 129 segments, two minutes at 256: those are the script's):

  * the stored hashes are those of freshly generated batches -- the file and spectral_amd.synth are in step;
  * the candidate the GPU tests hold to the LIVE yardstick at 65 segments is what they take it for: strictly complementary,
    every gradient unique, active rows on both sides of the wavefront seam (segments <= 63 and segment 64);
  * one stored case of 129 segments, the KKT system rebuilt from the stored solution by the assembly alone: x is feasible, its
    active rows sit on their bounds, a multiplier of the right sign on every one of them makes it stationary; the stored tangent
    meets the active rows' targets and reproduces dcost and its scale; and the stored gradient and the stored tangent satisfy the
    adjoint identity <xbar, dx> + cbar dcost = <g, d> -- which holds the gradient arrays without the adjoint vector v."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_long_grad_goldens as G   # noqa: E402
from jvp_reference import H_PQ, KEYS, dense, moved   # noqa: E402
from vjp_reference import Adjoint, one   # noqa: E402


@pytest.fixture(scope="module")
def stored():
    return np.load(G.OUT)


def test_the_file_holds_every_case_of_its_generator(stored):
    for i, (gen, S, b) in enumerate(G.CASES):
        p = "c%d_" % i
        batch, sh = G.make(gen, S)
        assert str(stored[p + "hash"]) == G.case_hash(batch, sh, b), (i, gen, S, b)
        assert int(stored[p + "seed"]) == G.case_seed(S, b) and float(stored[p + "cbar"]) == G.CBAR
        assert np.array_equal(stored[p + "xbar"], np.random.default_rng(G.case_seed(S, b)).standard_normal(12 * S))
        assert stored[p + "g_seg"].shape == (17, S) and stored[p + "dx0"].shape == (12 * S,) and stored[p + "dx1"].shape == (12 * S,)
        for k in KEYS:
            assert stored[p + "um_" + k].dtype == bool and stored[p + "um_" + k].shape == stored[p + "g_" + k].shape
            assert np.isfinite(stored[p + "g_" + k]).all() and np.isfinite(stored[p + "d0_" + k]).all()
            if gen != "scenario1":
                assert stored[p + "um_" + k].all(), (i, k)           # every gradient unique
        assert np.abs(stored[p + "g_seg"]).max() > 0 and np.abs(stored[p + "dx0"]).max() > 0
    # which candidates of the seam batches the central differences may be held to: five flags per shape, a majority usable,
    # and the four generic cases above among the strict ones
    for gen, S in G.SEAMS:
        strict, weak = stored["strict_%s_%d" % (gen, S)], stored["weak_%s_%d" % (gen, S)]
        assert strict.dtype == bool and weak.dtype == bool and strict.shape == weak.shape == (5,)
        assert (strict & ~weak).sum() >= 2, (gen, S, strict, weak)
    assert stored["strict_generic_129"][:2].all() and stored["strict_generic_256"][0] and stored["strict_scenario1_128"].any()
    assert os.path.getsize(G.OUT) < 1 << 20


def test_the_live_candidate_at_65_segments_is_nondegenerate_with_active_rows_on_both_sides_of_the_seam():
    batch, sh = G.make("generic", 65)
    adj = Adjoint(one(batch, 0), sh, np.zeros(12 * 65), 0.0)
    adj.grads()
    assert adj.status == 1 and adj.strict and adj.unique
    ineq = (adj.u - adj.l) > 1e-12
    segs = set(int(s) for s in adj.row_seg[adj.act & ineq])
    assert 64 in segs and any(s <= 63 for s in segs), sorted(segs)


def test_a_stored_case_of_129_segments_against_the_rebuilt_kkt_system(stored):
    i = 0
    gen, S, b = G.CASES[i]
    p = "c%d_" % i
    batch, sh = G.make(gen, S)
    bt = one(batch, b)
    _, P, A, q, l, u = dense(bt, sh)
    x, act, lower = stored[p + "x"], stored[p + "act"], stored[p + "lower"]
    Ax = A @ x
    eq = (u - l) <= 1e-12
    scale = 1.0 + np.maximum(np.abs(np.where(np.abs(l) < 1e9, l, 0)), np.abs(np.where(np.abs(u) < 1e9, u, 0)))
    # feasible; the active rows on their bounds (vjp_reference.Adjoint's margin: 1e-6 of the row's scale)
    assert (Ax >= l - 1e-6 * scale).all() and (Ax <= u + 1e-6 * scale).all()
    assert eq[~act].sum() == 0
    on = np.where(lower | eq, Ax - l, u - Ax)
    assert (np.abs(on[act]) <= 1e-6 * scale[act]).all()
    ia = act & ~eq
    assert 10 <= ia.sum() <= 15                     # (the issue's count for this batch)
    seg_of = (np.argmax(A != 0, axis=1) % (6 * S)) // 6
    segs = set(seg_of[ia].tolist())                 # active rows in every wavefront of the three: 0..63, 64..127, 128
    assert 128 in segs and any(s <= 63 for s in segs) and any(64 <= s <= 127 for s in segs), sorted(segs)
    # stationary with multipliers of the right sign (the oracle's convention: y < 0 on a lower bound)
    Aa = A[act]
    ya, res = np.linalg.lstsq(Aa.T, -(P @ x + q), rcond=None)[:2]
    r = P @ x + q + Aa.T @ ya
    assert np.abs(r).max() <= 1e-6 * np.abs(q).max(), np.abs(r).max()
    y = np.zeros(A.shape[0]); y[act] = ya
    assert (y[ia & lower] < 0).all() and (y[ia & ~lower] > 0).all()
    # the stored tangents: targets of the active rows, dcost and its scale, and the adjoint identity with the stored gradient
    xbar, cbar = stored[p + "xbar"], float(stored[p + "cbar"])
    g = {k: stored[p + "g_" + k] for k in KEYS}
    for t in range(2):
        dr = {k: stored[p + "d%d_%s" % (t, k)] for k in KEYS}
        dx = stored[p + "dx%d" % t]
        h = 1e-4
        _, _, _, _, lp, up = dense(*moved(bt, sh, dr, h))
        _, _, _, _, lm, um_ = dense(*moved(bt, sh, dr, -h))
        _, Pp, _, qp_, _, _ = dense(*moved(bt, sh, dr, H_PQ))
        _, Pm, _, qm, _, _ = dense(*moved(bt, sh, dr, -H_PQ))
        fin = lambda a_, b_: np.where((np.abs(a_) < 1e9) & (np.abs(b_) < 1e9), a_ - b_, 0.0)
        dP, dq, dl, du = (Pp - Pm) / (2 * H_PQ), (qp_ - qm) / (2 * H_PQ), fin(lp, lm) / (2 * h), fin(up, um_) / (2 * h)
        db = np.where(lower | eq, dl, du)
        assert np.abs(Aa @ dx - db[act]).max() <= 1e-7 * max(1.0, np.abs(db[act]).max())
        dcost = float((P @ x + q) @ dx + 0.5 * x @ (dP @ x) + dq @ x)
        dscale = float(np.abs((P @ x + q) * dx).sum() + 0.5 * np.abs(x * (dP @ x)).sum() + np.abs(dq * x).sum())
        assert abs(dcost - float(stored[p + "dcost%d" % t])) <= 1e-9 * dscale
        assert abs(dscale - float(stored[p + "dcost_scale%d" % t])) <= 1e-9 * dscale
        lhs = xbar @ dx + cbar * dcost
        rhs = sum(float((g[k] * dr[k]).sum()) for k in KEYS)
        mag = np.abs(xbar * dx).sum() + abs(cbar * dcost)
        print("stored case %d tangent %d: |lhs - rhs| / sum |terms| = %.2e" % (i, t, abs(lhs - rhs) / mag))
        assert abs(lhs - rhs) <= 1e-4 * mag, (t, lhs, rhs, mag)
