"""Writes tests/golden/long_rescue_yardstick.npz: the yardstick of btrapz_solve_long_rescue_device
(include/btrapz_hip_long_rescue.h) -- the oracle's relaxed solve, AssembledQp.solve_elastic, at widths where it is too slow
to run in a test: 30-75 s a candidate at 193 segments, 60-180 s at 256.

    python tests/golden/make_long_rescue_goldens.py [193 255 256 find_traj]

Batches (seam_batch): five candidates of synth.make_batch(5, S, config=2, seed=500 + S).  Slot 0 is untouched; slots 1..4 are
damaged as tests/test_gpu_rescue_edges.py damages its candidates: the initial state outside segment 0's rows by 0.004 / 0.030,
the last joint's two rows apart by 0.008 / 0.060 -- least violations 0.004 and 0.030, either side of the product's tolerance
(elastic_tol of acceptance_table.json).  A generic candidate may have no solution of its own (at 256 segments, seed 756,
candidates 2 and 3 carry violations of 0.05 and 0.035 undamaged): damage on top of that measures nothing.  So every
candidate of the batch is first put to the oracle's exact solve and to its relaxed solve UNDAMAGED, and a slot whose own
candidate is not feasible (exact status 1, relaxed violation below 1e-5) holds a copy of one that is (`bases_<S>`: the
candidate each slot is a copy of).  Asserted per width: slot 0 feasible, a least violation <= tol - 0.002 and one >= tol + 0.005.

Per width S: `bases_<S>` [5], `hash_<S>` (sha256 of the batch as built: tests/test_long_rescue_goldens.py holds the file to
this generator), `x_<S>` [5, 12 S] (slot 0: the exact solve's x*; slots 1..4: the relaxed solve's x), `viol_<S>` [5] (least
violation in control-point units; 0 for slot 0), `status_<S>` [5] (the oracle's status of that solve), and what the selection
saw, `pool_status_<S>` / `pool_viol_<S>` [5].

find_traj: synth.scenario1_knots(1, 200) with the initial lateral position 0.004 below the first segment's lower line;
`ft_hash`, `ft_n` (segments), `ft_l0`, `ft_x` [12 n], `ft_viol`, `ft_status` of the relaxed solve of the oracle's restatement of
the call (ParsedInput -> pipeline -> AssembledQp), as tests/test_gpu_long.py::test_rescue_pass_of_the_long_form compares."""
import hashlib
import json
import os
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OUT = os.path.join(HERE, "long_rescue_yardstick.npz")
TOL = json.load(open(os.path.join(HERE, "acceptance_table.json")))["elastic_tol"]
SIZES = (193, 255, 256)
B = 5
DAMAGE = (("outside_initial_state", 0.004), ("outside_initial_state", 0.030), ("conflict_at_last_joint", 0.008),
          ("conflict_at_last_joint", 0.060))      # slots 1..4, in this order
FT_SEGMENTS, FT_GAP = 200, 0.004
WORKERS = 8


def pool_batch(S):
    from spectral_amd import layout as L
    from spectral_amd import synth
    batch, sh = synth.make_batch(B, S, config=2, seed=500 + S)
    return L.Batch(B=B, S=S, seg=batch.seg.copy(), init=batch.init.copy(), ref_end=batch.ref_end.copy(), dl_bounds=batch.dl_bounds.copy()), sh


def seam_batch(S, bases):
    """The batch the tests solve: slot b a copy of candidate bases[b] of pool_batch(S), slots 1..4 damaged."""
    import test_gpu_rescue_edges as E
    from spectral_amd import layout as L
    pool, sh = pool_batch(S)
    idx = np.asarray(bases, dtype=int)
    batch = L.Batch(B=B, S=S, seg=pool.seg[:, idx].copy(), init=pool.init[idx].copy(), ref_end=pool.ref_end[idx].copy(),
                    dl_bounds=pool.dl_bounds[idx].copy())
    for b, (fn, gap) in enumerate(DAMAGE, start=1):
        getattr(E, fn)(batch, b, gap)
    return batch, sh


def batch_hash(batch, sh):
    h = hashlib.sha256()
    for a in (batch.seg, batch.init, batch.ref_end, batch.dl_bounds, sh.as_array()):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def ft_scene(l0=None):
    """The scene of the find_traj case; l0: its damaged initial lateral position (None: as generated)."""
    from spectral_amd import synth
    kb = synth.scenario1_knots(1, FT_SEGMENTS)
    if l0 is not None:
        kb.init[0, 3] = l0
    return kb


def knots_hash(kb):
    h = hashlib.sha256()
    for k in sorted(vars(kb)):
        v = getattr(kb, k)
        if isinstance(v, np.ndarray):
            h.update(k.encode()); h.update(np.ascontiguousarray(v, dtype=np.float64).tobytes())
    return h.hexdigest()


def screen(task):
    """(S, b) -> (exact status, undamaged relaxed violation; 1.0 where the exact solve already says no)."""
    from helpers import oracle_qp_from_batch
    S, b = task
    batch, sh = pool_batch(S)
    x, _, info = oracle_qp_from_batch(batch, sh, b).solve_exact(max_iter=120)
    viol = 1.0
    if info.status == 1:
        viol = oracle_qp_from_batch(batch, sh, b).solve_elastic()[3]
    print("screen S=%d b=%d: exact status %d, relaxed violation undamaged %.3g" % (S, b, info.status, viol), flush=True)
    return int(info.status), float(viol), x


def relax(task):
    from helpers import oracle_qp_from_batch
    S, bases, b = task
    batch, sh = seam_batch(S, bases)
    x, _, info, viol = oracle_qp_from_batch(batch, sh, b).solve_elastic()
    print("relaxed S=%d slot %d (candidate %d, %s %.3f): status %d, least violation %.6f" % ((S, b, bases[b]) + DAMAGE[b - 1] + (info.status, viol)), flush=True)
    return x, float(viol), int(info.status)


def generate_seams(sizes, pool):
    out = {}
    tasks = [(S, b) for S in sorted(sizes, reverse=True) for b in range(B)]
    seen = dict(zip(tasks, pool.map(screen, tasks)))
    plans = {}
    for S in sizes:
        good = [b for b in range(B) if seen[(S, b)][0] == 1 and seen[(S, b)][1] < 1e-5]
        assert good, (S, [seen[(S, b)][:2] for b in range(B)])
        plans[S] = [b if b in good else good[b % len(good)] for b in range(B)]
    rtasks = [(S, plans[S], b) for S in sorted(sizes, reverse=True) for b in range(1, B)]
    res = dict(zip([(t[0], t[2]) for t in rtasks], pool.map(relax, rtasks)))
    for S in sizes:
        bases = plans[S]
        batch, sh = seam_batch(S, bases)
        x = np.zeros((B, 12 * S)); viol = np.zeros(B); status = np.zeros(B, dtype=np.int32)
        x[0] = seen[(S, bases[0])][2]; status[0] = seen[(S, bases[0])][0]
        for b in range(1, B):
            x[b], viol[b], status[b] = res[(S, b)]
        assert status[0] == 1 and (np.isin(status[1:], (1, 2))).all(), (S, status)
        assert (viol[1:] <= TOL - 0.002).any() and (viol[1:] >= TOL + 0.005).any(), (S, viol)
        out.update({"bases_%d" % S: np.array(bases, dtype=np.int32), "hash_%d" % S: np.array(batch_hash(batch, sh)), "x_%d" % S: x,
                    "viol_%d" % S: viol, "status_%d" % S: status,
                    "pool_status_%d" % S: np.array([seen[(S, b)][0] for b in range(B)], dtype=np.int32),
                    "pool_viol_%d" % S: np.array([seen[(S, b)][1] for b in range(B)])})
        print("S=%d: bases %s, least violations %s" % (S, bases, viol), flush=True)
    return out


def generate_find_traj():
    from oracle import oracle as O
    from spectral_amd import knots, synth
    path = os.path.join(tempfile.mkdtemp(), "scene.txt")
    knots.write_corridor_file(path, ft_scene(), 0)
    cubes = O.pipeline(0, O.ParsedInput(path))[1]
    l0 = float(cubes[0].l_down_bias) - FT_GAP          # below the first segment's lower l line at its start
    kb = ft_scene(l0)
    knots.write_corridor_file(path, kb, 0)
    inp = O.ParsedInput(path)
    n, cubes = O.pipeline(0, inp)
    assert 200 <= n <= 256, n
    qp = O.AssembledQp(0, cubes, O.params_from_weights(synth.REFERENCE_WEIGHTS), inp)
    x, _, info, viol = qp.solve_elastic()
    print("find_traj scene: %d segments, l0 %.6f, relaxed status %d, least violation %.6f" % (n, l0, info.status, viol), flush=True)
    assert info.status in (1, 2) and 1e-4 <= viol <= TOL - 0.002, (info.status, viol)
    return {"ft_hash": np.array(knots_hash(kb)), "ft_n": np.array(n), "ft_l0": np.array(l0), "ft_x": x, "ft_viol": np.array(viol),
            "ft_status": np.array(int(info.status))}


def main():
    want = sys.argv[1:] or [str(S) for S in SIZES] + ["find_traj"]
    sizes = [int(w) for w in want if w != "find_traj"]
    data = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    from oracle import oracle as O
    O.lib()                                                         # (built and loaded once, before the threads ask for it)
    with ThreadPoolExecutor(max_workers=WORKERS) as pool:           # (the C solver runs outside the interpreter's lock)
        ft = pool.submit(generate_find_traj) if "find_traj" in want else None
        if sizes:
            data.update(generate_seams(sizes, pool))
        if ft is not None:
            data.update(ft.result())
    np.savez_compressed(OUT, **data)
    print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
