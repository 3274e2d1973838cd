"""include/btrapz_hip_long_sets.h held to the rules tests/test_long_warm_abi.py applies to include/btrapz_hip_long.h: the header
compiles as plain C99 on its own, the declared symbol is exported, the ninth prototype table of spectral_amd.native follows the
header's prototype, without a context the entry point refuses instead of crashing, and the Python surface is there."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from spectral_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "btrapz_hip_long_sets.h")
NAMES = ["btrapz_solve_long_sets_device"]


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_header_is_plain_c_on_its_own(tmp_path):
    src = tmp_path / "only.c"
    src.write_text('#include "btrapz_hip_long_sets.h"\nint (*entry)(btrapz_ctx *, const btrapz_shared *, int, const int *, const btrapz_options *, '
                   'const btrapz_warm *, int, int, const double *, const int *, const double *, const double *, const double *, double *, '
                   'double *, int *, int *, void *) = btrapz_solve_long_sets_device;\n'
                   'int (*sibling)(btrapz_ctx *, const btrapz_shared *, const btrapz_options *, const btrapz_warm *, int, int, const double *, '
                   'const int *, const double *, const double *, const double *, double *, double *, int *, int *, void *) = '
                   'btrapz_solve_long_rescue_device;\nint limit = BTRAPZ_MAX_SEGMENTS_LONG;\nint sets = BTRAPZ_MAX_SETS;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           "-o", str(tmp_path / "only.o"), str(src)])


def test_the_declared_symbol_is_exported_and_in_the_ninth_table(built):
    names = sorted(set(re.findall(r"\b(btrapz_[a-z_]+)\s*\(", header_without_comments())))
    assert names == NAMES
    assert set(names) == set(native.PROTOTYPES_LONG_SETS) == set(native.EXPORTS_LONG_SETS)
    assert not set(names) & (set(native.PROTOTYPES) | set(native.PROTOTYPES_STAGE_JVP) | set(native.PROTOTYPES_SCHEDULE) |
                             set(native.PROTOTYPES_SELECT) | set(native.PROTOTYPES_CHECK) | set(native.PROTOTYPES_LONG) |
                             set(native.PROTOTYPES_LONG_RESCUE) | set(native.PROTOTYPES_LONG_GRAD))
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_argument_count_and_return_type_follow_the_header_and_the_sibling(built):
    m = re.search(r"\bint\s+btrapz_solve_long_sets_device\s*\(([^()]*)\)\s*;", header_without_comments())
    params = [p.strip() for p in m.group(1).split(",")]
    fn = built.btrapz_solve_long_sets_device
    assert len(fn.argtypes) == len(params) == len(native.PROTOTYPES_LONG_SETS["btrapz_solve_long_sets_device"][1]) == 18
    assert fn.restype is C.c_int
    # "the arguments and layouts are those of btrapz_solve_sets_device": the same ctypes row, and the header's parameter list
    # is that of btrapz_hip.h's prototype, type for type and name for name
    assert native.PROTOTYPES_LONG_SETS["btrapz_solve_long_sets_device"] == native.PROTOTYPES["btrapz_solve_sets_device"]
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "btrapz_hip.h")).read(), flags=re.S)
    s = re.search(r"\bint\s+btrapz_solve_sets_device\s*\(([^()]*)\)\s*;", main)
    assert [re.sub(r"\s+", " ", p) for p in params] == [re.sub(r"\s+", " ", p.strip()) for p in s.group(1).split(",")]


def test_no_context_is_refused_without_a_device(built):
    assert built.btrapz_solve_long_sets_device(None, None, 0, None, None, None, 0, 0, None, None, None, None, None, None, None, None, None,
                                               None) == -1   # BTRAPZ_EINVAL


def test_python_surface_is_there():
    from spectral_amd import diff
    from spectral_amd.solver import BatchSolver
    sig = inspect.signature(BatchSolver.solve_long_sets)
    assert list(sig.parameters) == ["self", "dbatch_or_rec", "sets", "set_index", "warm", "keep_multipliers", "out", "elastic", "elastic_tol",
                                    "max_iter", "eps", "lean"]
    assert [sig.parameters[k].default for k in ("warm", "keep_multipliers", "out", "elastic", "elastic_tol", "max_iter", "eps", "lean")] == \
        [None, False, None, 0, 0.0, 0, 0.0, 0]
    old = inspect.signature(native.Context.solve_sets_device)
    new = inspect.signature(native.Context.solve_long_sets_device)
    assert [p for p in old.parameters] == [p for p in new.parameters if p != "elastic_tol"]
    # diff.solve_long / solve_long_jacobian keep their signatures (tests/test_long_grad_abi.py); the sets forms are theirs with
    # a required keyword-only set_index in front of the other keywords
    for new, old in ((diff.solve_long_sets, diff.solve_long), (diff.solve_long_sets_jacobian, diff.solve_long_jacobian)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        assert [n for n in a if n != "set_index"] == list(b) and "set_index" not in b
        assert a["set_index"].kind is inspect.Parameter.KEYWORD_ONLY and a["set_index"].default is inspect.Parameter.empty
        assert all(a[n].default == b[n].default and a[n].kind == b[n].kind for n in b)
