"""tests/golden/long_rescue_yardstick.npz held to its generator (tests/golden/make_long_rescue_goldens.py) without a GPU and without
the relaxed solves that make it slow (one to three minutes a candidate: those are the script's), and include/btrapz_hip_long_rescue.h
held to the rules tests/test_long_warm_abi.py applies to its sibling:

  * the stored checksums are those of freshly built batches and of the find_traj scene -- the file, spectral_amd.synth and the two
    damage constructions of tests/test_gpu_rescue_edges.py are in step;
  * every width holds the three kinds of candidate the GPU tests need, each clear of the tolerance: slot 0 untouched and feasible
    by the oracle's exact solve, a least violation <= tol - 0.002, one >= tol + 0.005 -- and every slot is a copy of a candidate
    the oracle found feasible undamaged (exact status 1, relaxed violation below 1e-5);
  * the stored solutions are what they are taken for, by the assembly alone: slot 0's x* keeps every row, a damaged slot's x
    violates its rows by exactly the stored least violation, and the damage sits where the docstrings say (193 segments: the
    last joint between lane 63 of the third wavefront and lane 0 of the fourth);
  * the header compiles as plain C99 on its own, its symbol is exported and in a prototype table of its own, and without a
    context the entry point refuses instead of crashing."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_long_rescue_goldens as G   # noqa: E402
from helpers import oracle_qp_from_batch   # noqa: E402
from spectral_amd import native   # noqa: E402

HEADER = os.path.join(ROOT, "include", "btrapz_hip_long_rescue.h")
NAME = "btrapz_solve_long_rescue_device"


@pytest.fixture(scope="module")
def stored():
    return np.load(G.OUT)


def row_violations(qp, x):
    """Violation of every inequality row by x in the row's own norm, and the segment of the row's first column."""
    import scipy.sparse as sp
    A = sp.csc_matrix((qp.A_x, qp.A_i, qp.A_p), shape=(qp.m, qp.n)).tocsr()
    Ax = A @ x
    ineq = (qp.u - qp.l) > 1e-12
    nrm = np.sqrt(np.asarray(A.multiply(A).sum(axis=1)).ravel())
    first_col = A.indices[A.indptr[:-1]]
    S = qp.n // 12
    return (np.abs(Ax - np.clip(Ax, qp.l, qp.u)) / nrm)[ineq], ((first_col % (6 * S)) // 6)[ineq], (first_col // (6 * S))[ineq]


@pytest.mark.parametrize("S", G.SIZES)
def test_the_file_holds_every_width_of_its_generator_with_the_margins(stored, S):
    bases, viol, status = stored["bases_%d" % S], stored["viol_%d" % S], stored["status_%d" % S]
    batch, sh = G.seam_batch(S, bases)
    assert str(stored["hash_%d" % S]) == G.batch_hash(batch, sh)
    assert stored["x_%d" % S].shape == (G.B, 12 * S) and np.isfinite(stored["x_%d" % S]).all()
    # every slot a copy of a candidate the oracle found feasible undamaged; a feasible candidate stays in its own slot
    ps, pv = stored["pool_status_%d" % S], stored["pool_viol_%d" % S]
    good = (ps == 1) & (pv < 1e-5)
    assert good[bases].all(), (bases, ps, pv)
    assert all(bases[b] == b for b in range(G.B) if good[b])
    # the three kinds, each clear of the tolerance
    assert status[0] == 1 and viol[0] == 0 and np.isin(status[1:], (1, 2)).all()
    assert (viol[1:] <= G.TOL - 0.002).any() and (viol[1:] >= G.TOL + 0.005).any(), viol
    # where a construction meets nothing else it gives what tests/test_gpu_rescue_edges.py says: gap, gap, gap / 2, gap / 2 -- on at
    # least one slot either side of the tolerance (a base's own tight rows may add to it: 193 segments, slot 1)
    want = np.array([gap if fn == "outside_initial_state" else gap / 2 for fn, gap in G.DAMAGE])
    pure = np.abs(viol[1:] - want) <= 1e-4
    assert (pure & (want < G.TOL)).any() and (pure & (want > G.TOL)).any(), (viol, want)
    assert os.path.getsize(G.OUT) < 1 << 20


@pytest.mark.parametrize("S", G.SIZES)
def test_the_stored_solutions_against_the_assembled_rows(stored, S):
    bases, viol, x = stored["bases_%d" % S], stored["viol_%d" % S], stored["x_%d" % S]
    batch, sh = G.seam_batch(S, bases)
    v0, _, _ = row_violations(oracle_qp_from_batch(batch, sh, 0), x[0])
    assert v0.max() <= 1e-7
    for b in range(1, G.B):
        v, seg, axis = row_violations(oracle_qp_from_batch(batch, sh, b), x[b])
        assert abs(v.max() - viol[b]) <= 1e-9, (S, b, v.max(), viol[b])
        fn, gap = G.DAMAGE[b - 1]
        if abs(viol[b] - (gap if fn == "outside_initial_state" else gap / 2)) > 1e-4:
            continue                           # (the construction met the base's own tight rows: no statement about where)
        worst = v >= 0.9 * v.max()               # (the joint's two rows share the gap: 0.004004 and 0.003996)
        if fn == "outside_initial_state":      # the l axis, segment 0: lane 0 of wavefront 0
            assert set(seg[worst]) == {0} and set(axis[worst]) == {1}, (S, b, set(seg[worst]), set(axis[worst]))
        else:                                  # the s axis, the last joint: segments S - 2 and S - 1
            assert set(seg[worst]) == {S - 2, S - 1} and set(axis[worst]) == {0}, (S, b, set(seg[worst]), set(axis[worst]))
    if S == 193:
        assert (S - 2) // 64 == 2 and (S - 2) % 64 == 63 and (S - 1) // 64 == 3 and (S - 1) % 64 == 0


def test_the_find_traj_scene(stored):
    l0 = float(stored["ft_l0"])
    kb = G.ft_scene(l0)
    assert str(stored["ft_hash"]) == G.knots_hash(kb)
    n = int(stored["ft_n"])
    assert 200 <= n <= 256 and stored["ft_x"].shape == (12 * n,) and int(stored["ft_status"]) in (1, 2)
    assert 1e-4 <= float(stored["ft_viol"]) <= G.TOL - 0.002
    assert abs(float(stored["ft_viol"]) - G.FT_GAP) <= 1e-4
    assert kb.init[0, 3] == l0 and l0 < float(kb.l_bounds[0, :, 0, 0].min())     # below every lane's lower line at the first knot


# ---- the header ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_header_is_plain_c_on_its_own(tmp_path):
    src = tmp_path / "only.c"
    src.write_text('#include "btrapz_hip_long_rescue.h"\nint (*entry)(btrapz_ctx *, const btrapz_shared *, const btrapz_options *, const btrapz_warm *, '
                   'int, int, const double *, const int *, const double *, const double *, const double *, double *, double *, int *, '
                   'int *, void *) = btrapz_solve_long_rescue_device;\nint (*sibling)(btrapz_ctx *, const btrapz_shared *, const btrapz_options *, '
                   'const btrapz_warm *, int, int, const double *, const int *, const double *, const double *, const double *, double *, '
                   'double *, int *, int *, void *) = btrapz_solve_long_warm_device;\nint limit = BTRAPZ_MAX_SEGMENTS_LONG;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           "-o", str(tmp_path / "only.o"), str(src)])


def test_the_declared_symbol_is_exported_and_in_a_table_of_its_own(built):
    names = sorted(set(re.findall(r"\b(btrapz_[a-z_]+)\s*\(", header_without_comments())))
    assert names == [NAME]
    assert set(names) == set(native.PROTOTYPES_LONG_RESCUE) == set(native.EXPORTS_LONG_RESCUE)
    assert not set(names) & (set(native.PROTOTYPES) | set(native.PROTOTYPES_LONG) | set(native.PROTOTYPES_LONG_GRAD) | set(native.PROTOTYPES_CHECK))
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    assert NAME in {l.split()[-1] for l in out.splitlines() if " T " in l}
    m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % NAME, header_without_comments())
    fn = getattr(built, NAME)
    assert len(fn.argtypes) == len(m.group(1).split(",")) == 16 and fn.restype is C.c_int
    assert native.PROTOTYPES_LONG_RESCUE[NAME] == native.PROTOTYPES_LONG["btrapz_solve_long_warm_device"]


def test_no_context_is_refused_without_a_device(built):
    assert getattr(built, NAME)(None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None) == -1   # BTRAPZ_EINVAL


def test_python_surface_is_there():
    from spectral_amd.solver import BatchSolver
    sig = inspect.signature(BatchSolver.solve_long_rescue)
    assert list(sig.parameters) == ["self", "dbatch_or_rec", "shared", "warm", "keep_multipliers", "max_iter", "eps", "out", "elastic",
                                    "elastic_tol"]
    assert [sig.parameters[k].default for k in ("warm", "keep_multipliers", "max_iter", "eps", "out", "elastic", "elastic_tol")] == \
        [None, False, 0, 0.0, None, 1, 0.0]
    sib = inspect.signature(native.Context.solve_long_warm_device)
    mine = inspect.signature(native.Context.solve_long_rescue_device)
    assert [p.name for p in mine.parameters.values()] == [p.name for p in sib.parameters.values()]
    assert mine.parameters["elastic"].default == 1
