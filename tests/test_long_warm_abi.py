"""include/btrapz_hip_long.h held to the rules tests/test_abi.py applies to include/btrapz_hip.h: the header compiles as plain
C99 on its own, the declared symbol is exported, the sixth prototype table of spectral_amd.native follows the header's
prototype, without a context the entry point refuses instead of crashing, and the Python surface is there."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from spectral_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "btrapz_hip_long.h")
NAMES = ["btrapz_solve_long_warm_device"]


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_header_is_plain_c_on_its_own(tmp_path):
    src = tmp_path / "only.c"
    src.write_text('#include "btrapz_hip_long.h"\nint (*entry)(btrapz_ctx *, const btrapz_shared *, const btrapz_options *, const btrapz_warm *, '
                   'int, int, const double *, const int *, const double *, const double *, const double *, double *, double *, int *, '
                   'int *, void *) = btrapz_solve_long_warm_device;\nint limit = BTRAPZ_MAX_SEGMENTS_LONG;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           "-o", str(tmp_path / "only.o"), str(src)])


def test_the_declared_symbol_is_exported_and_in_the_sixth_table(built):
    names = sorted(set(re.findall(r"\b(btrapz_[a-z_]+)\s*\(", header_without_comments())))
    assert names == NAMES
    assert set(names) == set(native.PROTOTYPES_LONG) == set(native.EXPORTS_LONG)
    assert not set(names) & (set(native.PROTOTYPES) | set(native.PROTOTYPES_STAGE_JVP) | set(native.PROTOTYPES_SCHEDULE) |
                             set(native.PROTOTYPES_SELECT) | set(native.PROTOTYPES_CHECK))
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_argument_count_and_return_type_follow_the_header_and_the_sibling(built):
    m = re.search(r"\bint\s+btrapz_solve_long_warm_device\s*\(([^()]*)\)\s*;", header_without_comments())
    n_params = len(m.group(1).split(","))
    fn = built.btrapz_solve_long_warm_device
    assert len(fn.argtypes) == n_params == len(native.PROTOTYPES_LONG["btrapz_solve_long_warm_device"][1]) == 16
    assert fn.restype is C.c_int
    # "the arguments of btrapz_solve_warm_device"
    assert native.PROTOTYPES_LONG["btrapz_solve_long_warm_device"] == native.PROTOTYPES["btrapz_solve_warm_device"]


def test_no_context_is_refused_without_a_device(built):
    assert built.btrapz_solve_long_warm_device(None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None) == -1   # BTRAPZ_EINVAL


def test_python_surface_is_there():
    from spectral_amd.solver import BatchSolver
    sig = inspect.signature(BatchSolver.solve_long)
    assert list(sig.parameters) == ["self", "dbatch_or_rec", "shared", "warm", "keep_multipliers", "max_iter", "eps", "out"]
    assert [sig.parameters[k].default for k in ("warm", "keep_multipliers", "max_iter", "eps", "out")] == [None, False, 0, 0.0, None]
    warm = inspect.signature(native.Context.solve_warm_device)
    long = inspect.signature(native.Context.solve_long_warm_device)
    assert [(p.name, p.default) for p in long.parameters.values()] == [(p.name, p.default) for p in warm.parameters.values()]
