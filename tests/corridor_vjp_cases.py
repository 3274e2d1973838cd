"""Inputs shared by the CPU and GPU tests of the corridor stage's backward pass."""
import os

import numpy as np

import helpers as H
from spectral_amd import knots, layout as L, synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SEG_STRIDE = 16


def distinct_ds(kb, seed=5):
    """ds bounds with distinct per-knot values (as helpers.fuzz_knot_batch has): no two knots tie for an extreme."""
    kb.ds_bounds = np.tile(np.array([0.0, 20.0]), (kb.B, kb.N, 1)) + np.random.default_rng(seed).uniform(0, 1, (kb.B, kb.N, 2))
    return kb


def scenario(B):
    return distinct_ds(synth.scenario1_knots(B, 8))


def c1(B, seed=1):
    return distinct_ds(knots.jittered(knots.parse_corridor_file(os.path.join(GOLD, "inputs", "c1.txt")), B, seed=seed))


def fuzz(seed):
    """A small finite fuzz batch (helpers.fuzz_knot_batch with the horizon and the obstacle count pinned)."""
    kb = H.fuzz_knot_batch(seed, B=4, N=(21, 71)[seed % 2], num_obs=(2, 3)[seed % 2])
    assert all(np.isfinite(a).all() for a in (kb.s_bounds, kb.l_bounds, kb.s_ref, kb.l_ref)), seed
    return kb


FUZZ_SEEDS = (1, 14)     # finite, with corridors of 1..11 segments
MIXED_SEED = 9             # a batch with seg_count 0, 16, 7 and -1


def tied(seed, B=4):
    """helpers.tied_lanes_knot_batch at N = 201: two lanes whose segments open at the same knots, 17-26 selected segments
    (beyond the 16 up to which std::sort's order is the stable one), with distinct ds bounds.  Needs TIED_STRIDE."""
    return distinct_ds(H.tied_lanes_knot_batch(seed, B, 201))


TIED_SEED, TIED_STRIDE = 1, 32   # candidate 0: 25 segments, the overlap step moves the beg_t of segment 3


def full(seed=15):
    """The same family at N = 401 with the selection aimed at the stage's capacity: seed 15 has corridors of 64 (every output
    slot of seg_stride 64 in use), 60 and 63 segments and a candidate whose selection overflows the 64 (seg_count -1)."""
    return distinct_ds(H.tied_lanes_knot_batch(seed, 4, 401, n_range=(60, 66)))


def moved_spans(jac, spans, N, delta):
    """The checked segments whose beg_t the overlap step moved.  The yardstick's Jacobian tells where segment k came from:
    down_bias_k = lo(i0) + h additions of down_skew reads lo(i0) and, for h > 0, lo(i0 + 1) with d / d lo(i0 + 1) = h / delta;
    CorridorSplit opens the piece behind h others at knot i0 + 10 h.  (A segment with a skipped column among its own is
    not counted.)"""
    n = jac["n"]
    J = jac["J"]["s_bounds"][(L.F_DOWN_BIAS - 1) * n + np.arange(n)]
    moved = []
    for k in range(n):
        cols = np.flatnonzero(J[k])
        if cols.size not in (1, 2) or (cols % 2).any() or (cols.size == 2 and cols[1] != cols[0] + 2):
            continue
        i0 = (int(cols[0]) // 2) % N
        h = int(round(J[k, cols[1]] * delta)) if cols.size == 2 else 0
        if spans[k][0] != i0 + 10 * h:
            moved.append(k)
    return moved


def cotangents(B, seed=0, seg_stride=SEG_STRIDE):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((L.NUM_SEG_FIELDS, B, seg_stride)), rng.standard_normal((B, 2)), rng.standard_normal((B, 10))


def host_grads(kb, b, variant, seg_bar, ref_end_bar, dl_bar, seg_stride=SEG_STRIDE, **kw):
    from spectral_amd import native
    return native.corridor_vjp_host(variant, kb.delta, kb.s_bounds[b], kb.l_bounds[b], kb.ds_bounds[b], kb.dl_bounds[b], kb.s_ref[b],
                                    kb.l_ref[b], seg_stride, None if seg_bar is None else seg_bar[:, b], None if ref_end_bar is None else ref_end_bar[b],
                                    None if dl_bar is None else dl_bar[b], **kw)
