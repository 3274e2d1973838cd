"""include/btrapz_hip_check.h held to the rules tests/test_abi.py applies to include/btrapz_hip.h: the declared symbol is
exported, the fifth prototype table of spectral_amd.native follows the header's prototype, the ctypes mirror of
btrapz_row_check has the C struct's layout, the header is plain C99, and without a context the entry point refuses instead
of crashing."""
import ctypes as C
import os
import re
import subprocess

import pytest

from spectral_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "btrapz_hip_check.h")
NAMES = ["btrapz_check_rows_device"]


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_declared_symbol_is_exported_and_in_the_fifth_table(built):
    names = sorted(set(re.findall(r"\b(btrapz_[a-z_]+)\s*\(", header_without_comments())))
    assert names == NAMES
    assert set(names) == set(native.PROTOTYPES_CHECK) == set(native.EXPORTS_CHECK)
    assert not set(names) & (set(native.PROTOTYPES) | set(native.PROTOTYPES_STAGE_JVP) | set(native.PROTOTYPES_SCHEDULE) | set(native.PROTOTYPES_SELECT))
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_argument_count_and_return_type_follow_the_header(built):
    m = re.search(r"\bint\s+btrapz_check_rows_device\s*\(([^()]*)\)\s*;", header_without_comments())
    n_params = len(m.group(1).split(","))
    fn = built.btrapz_check_rows_device
    assert len(fn.argtypes) == n_params == len(native.PROTOTYPES_CHECK["btrapz_check_rows_device"][1]) == 14
    assert fn.restype is C.c_int


def test_struct_layout_is_the_headers(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "btrapz_hip_check.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(btrapz_row_check), offsetof(btrapz_row_check, struct_size), offsetof(btrapz_row_check, unit), '
                   'offsetof(btrapz_row_check, margin), offsetof(btrapz_row_check, worst), offsetof(btrapz_row_check, eq_res), '
                   'offsetof(btrapz_row_check, obj)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = native.CRowCheck
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in ("struct_size", "unit", "margin", "worst", "eq_res", "obj")]


def test_no_context_is_refused_without_a_device(built):
    assert built.btrapz_check_rows_device(None, None, 0, None, 0, 0, None, None, None, None, None, None, None, None) == -1   # BTRAPZ_EINVAL


def test_python_surface_is_there():
    from spectral_amd.solver import BatchSolver
    assert callable(BatchSolver.check_rows) and callable(BatchSolver.admissible) and callable(native.Context.check_rows_device)


def test_admissible_is_false_for_what_is_no_number():
    import torch
    from spectral_amd.solver import BatchSolver
    m = torch.zeros(6, 2, 4, dtype=torch.float64); e = torch.zeros(6, 2, 2, dtype=torch.float64)
    m[1, 1, 3] = float("nan"); m[2, 0, 0] = -float("inf"); e[3, 1, 1] = float("nan"); e[4, 0, 0] = float("inf"); m[5, 0, 1] = -2e-3
    adm = BatchSolver.admissible(dict(margin=m, eq_res=e), 1e-3, 1e-9)
    assert adm.tolist() == [True, False, False, False, False, False]
    m[0] = float("inf")                      # (a class without a bound is met)
    assert BatchSolver.admissible(dict(margin=m, eq_res=e), 0.0, 0.0)[0]
    assert BatchSolver.admissible(dict(margin=m, eq_res=e), 1e-2, 1e-9).tolist() == [True, False, False, False, False, True]
