"""include/btrapz_hip_select.h held to the rules tests/test_abi.py applies to include/btrapz_hip.h: every declared symbol
is exported, the fourth prototype table of spectral_amd.native follows the header's prototypes, the header is plain C99,
and without a context the entry points refuse instead of crashing."""
import ctypes as C
import os
import re
import subprocess

import pytest

from spectral_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "btrapz_hip_select.h")
NAMES = ["btrapz_gather_rows_device", "btrapz_topk_device", "btrapz_topk_pairs_device"]


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def declared_prototypes():
    """name -> (return type as written, number of parameters) of every prototype of the header."""
    out = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z_ ]*?[\s*]+)\b(btrapz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header_without_comments()):
        ret, name, params = " ".join(m.group(1).replace("*", " * ").split()), m.group(2), m.group(3).strip()
        out[name] = (ret, 0 if params == "void" else len(params.split(",")))
    return out


def test_every_declared_symbol_is_exported_and_in_the_fourth_table(built):
    names = sorted(set(re.findall(r"\b(btrapz_[a-z_]+)\s*\(", header_without_comments())))
    assert names == sorted(declared_prototypes()) == NAMES
    for n in names:
        assert hasattr(built, n), n
    assert set(names) == set(native.PROTOTYPES_SELECT) == set(native.EXPORTS_SELECT)
    assert not set(names) & (set(native.PROTOTYPES) | set(native.PROTOTYPES_STAGE_JVP) | set(native.PROTOTYPES_SCHEDULE))
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported


def test_argument_counts_and_return_types_follow_the_header(built):
    ctype = {"int": C.c_int}
    for name, (ret, n_params) in declared_prototypes().items():
        fn = getattr(built, name)
        assert len(fn.argtypes) == n_params == len(native.PROTOTYPES_SELECT[name][1]), name
        assert fn.restype is ctype[ret] and native.PROTOTYPES_SELECT[name][0] is ctype[ret], (name, ret)


def test_the_limit_is_the_headers(built):
    assert int(re.search(r"#define BTRAPZ_MAX_TOPK (\d+)", open(HEADER).read()).group(1)) == native.MAX_TOPK == 64


def test_no_context_is_refused_without_a_device(built):
    assert built.btrapz_topk_device(None, 8, 8, 1, 0, None, None, None, None) == -1       # BTRAPZ_EINVAL
    assert built.btrapz_topk_pairs_device(None, 1, 1, 1, None, None, None, None) == -1
    assert built.btrapz_gather_rows_device(None, 1, None, 0, 1, 1, None, None, None) == -1


def test_python_surface_is_there():
    from spectral_amd import dist
    from spectral_amd.solver import BatchSolver
    assert callable(BatchSolver.topk) and callable(dist.global_topk)
    for m in ("topk_device", "topk_pairs_device", "gather_rows_device"):
        assert callable(getattr(native.Context, m))


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "btrapz_hip_select.h"\nint main(void) { return btrapz_topk_device((btrapz_ctx *)0, 1, 1, BTRAPZ_MAX_TOPK, 0, '
                   '(const double *)0, (long long *)0, (double *)0, (void *)0) == -1 ? 0 : 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
