"""include/btrapz_hip_long_grad.h held to the rules tests/test_abi.py applies to include/btrapz_hip.h: the header compiles as
plain C99 on its own, the two declared symbols are exported, the seventh prototype table of spectral_amd.native follows the
header's prototypes and the siblings', without a context the entry points refuse instead of crashing, and the Python surface
is there."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from spectral_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "btrapz_hip_long_grad.h")
NAMES = ["btrapz_solve_long_jvp_device", "btrapz_solve_long_vjp_device"]
SIBLING = {"btrapz_solve_long_vjp_device": "btrapz_solve_vjp_device", "btrapz_solve_long_jvp_device": "btrapz_solve_jvp_device"}


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_header_is_plain_c_on_its_own(tmp_path):
    src = tmp_path / "only.c"
    head = "btrapz_ctx *, const btrapz_shared *, int, const int *, int, int, const double *, const int *, const double *, const double *, " \
           "const double *, const double *, const double *, const int *, "
    src.write_text('#include "btrapz_hip_long_grad.h"\n'
                   'int (*vjp)(' + head + 'const double *, const double *, const btrapz_grads *, void *) = btrapz_solve_long_vjp_device;\n'
                   'int (*jvp)(' + head + 'int, const btrapz_tangents *, double *, double *, void *) = btrapz_solve_long_jvp_device;\n'
                   'int (*vjp64)(' + head + 'const double *, const double *, const btrapz_grads *, void *) = btrapz_solve_vjp_device;\n'
                   'int (*jvp64)(' + head + 'int, const btrapz_tangents *, double *, double *, void *) = btrapz_solve_jvp_device;\n'
                   'int limit = BTRAPZ_MAX_SEGMENTS_LONG;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           "-o", str(tmp_path / "only.o"), str(src)])


def test_the_declared_symbols_are_exported_and_in_the_seventh_table_only(built):
    names = sorted(set(re.findall(r"\b(btrapz_[a-z_]+)\s*\(", header_without_comments())))
    assert names == NAMES
    assert set(names) == set(native.PROTOTYPES_LONG_GRAD) == set(native.EXPORTS_LONG_GRAD)
    assert not set(names) & (set(native.PROTOTYPES) | set(native.PROTOTYPES_STAGE_JVP) | set(native.PROTOTYPES_SCHEDULE) |
                             set(native.PROTOTYPES_SELECT) | set(native.PROTOTYPES_CHECK) | set(native.PROTOTYPES_LONG))
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("name,count", [("btrapz_solve_long_vjp_device", 18), ("btrapz_solve_long_jvp_device", 19)])
def test_argument_count_and_return_type_follow_the_header_and_the_sibling(built, name, count):
    m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, header_without_comments())
    n_params = len(m.group(1).split(","))
    fn = getattr(built, name)
    assert len(fn.argtypes) == n_params == len(native.PROTOTYPES_LONG_GRAD[name][1]) == count
    assert fn.restype is C.c_int
    # "the parameter list of the sibling": the table's entry, and the header's text with the name replaced
    assert native.PROTOTYPES_LONG_GRAD[name] == native.PROTOTYPES[SIBLING[name]]
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "btrapz_hip.h")).read(), flags=re.S)
    s = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % SIBLING[name], main)
    assert re.sub(r"\s+", " ", s.group(1)) == re.sub(r"\s+", " ", m.group(1))


def test_no_context_is_refused_without_a_device(built):
    head = lambda B, stride: [None, None, 0, None, B, stride] + [None] * 8
    assert built.btrapz_solve_long_vjp_device(*(head(0, 0) + [None] * 4)) == -1   # BTRAPZ_EINVAL
    assert built.btrapz_solve_long_jvp_device(*(head(0, 0) + [0] + [None] * 4)) == -1
    # ... at a width the siblings would take and at one only these take
    assert built.btrapz_solve_long_vjp_device(*(head(1, 200) + [None] * 4)) == -1
    assert built.btrapz_solve_long_jvp_device(*(head(1, 200) + [1] + [None] * 4)) == -1


def test_python_surface_is_there():
    from spectral_amd import diff
    from spectral_amd.solver import BatchSolver
    same = lambda a, b: [(p.name, p.default, p.kind) for p in inspect.signature(a).parameters.values()] == \
        [(p.name, p.default, p.kind) for p in inspect.signature(b).parameters.values()]
    assert same(native.Context.solve_long_vjp_device, native.Context.solve_vjp_device)
    assert same(native.Context.solve_long_jvp_device, native.Context.solve_jvp_device)
    assert same(BatchSolver.solve_long_vjp, BatchSolver.solve_vjp)
    assert same(BatchSolver.solve_long_jvp, BatchSolver.solve_jvp)
    sig = inspect.signature(diff.solve_long)
    assert list(sig.parameters) == ["solver", "seg", "init", "ref_end", "dl_bounds", "params", "seg_count", "variant", "delta"]
    assert [sig.parameters[k].default for k in ("seg_count", "variant", "delta")] == [None, 0, 0.1]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("seg_count", "variant", "delta"))
    jac, ref = inspect.signature(diff.solve_long_jacobian), inspect.signature(diff.solve_jacobian)
    assert [n for n in ref.parameters if n != "set_index"] == list(jac.parameters)   # (solve_long has no sets)
