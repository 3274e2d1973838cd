"""include/btrapz_hip_frenet.h held to the rules tests/test_abi_cartesian.py applies to its header: it compiles as plain C99
on its own, the six declared symbols are exported, the eleventh prototype table of spectral_amd.native follows the
header's prototypes and is disjoint from the other ten, without a context or with bad arguments the entry points refuse
instead of crashing, and the Python surface is there."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from spectral_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "btrapz_hip_frenet.h")
COUNTS = {"btrapz_frenet_device": 14, "btrapz_frenet_vjp_device": 14, "btrapz_frenet_jvp_device": 15,
          "btrapz_frenet_host": 12, "btrapz_frenet_vjp_host": 12, "btrapz_frenet_jvp_host": 13}


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_header_is_plain_c_on_its_own(tmp_path):
    src = tmp_path / "only.c"
    head = "const btrapz_refline *, const int *, int, int, int, int, const double *, "
    grad = head + "const double *, const int *, const int *, "
    src.write_text('#include "btrapz_hip_frenet.h"\n'
                   'int (*fwd)(btrapz_ctx *, ' + head + 'const int *, const double *, double *, int *, int *, void *) = btrapz_frenet_device;\n'
                   'int (*vjp)(btrapz_ctx *, ' + grad + 'const double *, double *, void *) = btrapz_frenet_vjp_device;\n'
                   'int (*jvp)(btrapz_ctx *, ' + grad + 'int, const double *, double *, void *) = btrapz_frenet_jvp_device;\n'
                   'int (*fwd_h)(' + head + 'const int *, const double *, double *, int *, int *) = btrapz_frenet_host;\n'
                   'int (*vjp_h)(' + grad + 'const double *, double *) = btrapz_frenet_vjp_host;\n'
                   'int (*jvp_h)(' + grad + 'int, const double *, double *) = btrapz_frenet_jvp_host;\n'
                   'int layouts[2] = {BTRAPZ_FRENET_SAMPLES, BTRAPZ_FRENET_STATES};\n'
                   'unsigned long size = sizeof(btrapz_refline);\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           "-o", str(tmp_path / "only.o"), str(src)])


def test_the_declared_symbols_are_exported_and_in_the_eleventh_table_only(built):
    names = sorted(set(re.findall(r"\b(btrapz_[a-z_]+)\s*\(", header_without_comments())))
    assert names == sorted(COUNTS)
    assert set(names) == set(native.PROTOTYPES_FRENET) == set(native.EXPORTS_FRENET)
    others = (native.PROTOTYPES, native.PROTOTYPES_STAGE_JVP, native.PROTOTYPES_SCHEDULE, native.PROTOTYPES_SELECT,
              native.PROTOTYPES_CHECK, native.PROTOTYPES_LONG, native.PROTOTYPES_LONG_RESCUE, native.PROTOTYPES_LONG_GRAD,
              native.PROTOTYPES_LONG_SETS, native.PROTOTYPES_CARTESIAN)
    assert not any(set(names) & set(t) for t in others)
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("name,count", sorted(COUNTS.items()))
def test_argument_count_and_return_type_follow_the_header(built, name, count):
    m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, header_without_comments())
    params = [p.strip() for p in m.group(1).split(",")]
    fn = getattr(built, name)
    assert len(fn.argtypes) == len(params) == len(native.PROTOTYPES_FRENET[name][1]) == count
    assert fn.restype is C.c_int
    # parameter by parameter: an int in the header is a c_int in the table, everything else a pointer
    for text, ctype in zip(params, fn.argtypes):
        assert (ctype is C.c_int) == (re.fullmatch(r"int\s+\w+", text) is not None), (name, text, ctype)
    # the host twin takes the device call's parameters without the context and the stream
    if name.endswith("_host"):
        dev = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name.replace("_host", "_device"), header_without_comments())
        dev_params = [re.sub(r"\s+", " ", p.strip()) for p in dev.group(1).split(",")]
        assert [re.sub(r"\s+", " ", p) for p in params] == dev_params[1:-1]


def test_no_context_and_bad_arguments_are_refused_without_a_device(built):
    t = native.CRefLine(1, 2, *[0] * 6)
    assert built.btrapz_frenet_device(None, C.byref(t), None, 1, 1, 0, 2, None, None, None, None, None, None, None) == -1   # BTRAPZ_EINVAL
    assert built.btrapz_frenet_vjp_device(None, C.byref(t), None, 1, 1, 0, 2, None, None, None, None, None, None, None) == -1
    assert built.btrapz_frenet_jvp_device(None, C.byref(t), None, 1, 1, 0, 2, None, None, None, None, 1, None, None, None) == -1
    assert built.btrapz_frenet_host(None, None, 1, 1, 0, 2, None, None, None, None, None, None) == -1
    assert built.btrapz_frenet_host(C.byref(t), None, 1, 1, 0, 2, None, None, None, None, None, None) == -1
    assert built.btrapz_frenet_vjp_host(C.byref(t), None, 1, 1, 0, 2, None, None, None, None, None, None) == -1
    assert built.btrapz_frenet_jvp_host(C.byref(t), None, 1, 1, 0, 2, None, None, None, None, 1, None, None) == -1


def test_python_surface_is_there():
    from spectral_amd import diff
    from spectral_amd.solver import BatchSolver
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(BatchSolver.frenet) == ["self", "cart", "refline", "layout", "order", "count", "line_index", "s_window"]
    assert names(BatchSolver.frenet_vjp) == ["self", "cart", "refline", "frenet", "interval", "frenet_bar", "layout", "order", "count",
                                             "line_index"]
    assert names(BatchSolver.frenet_jvp) == ["self", "cart", "refline", "frenet", "interval", "cart_dot", "layout", "order", "count",
                                             "line_index"]
    assert names(BatchSolver.init_from_cartesian)[:3] == ["self", "states", "refline"]
    assert names(BatchSolver.prisms_from_cartesian)[:3] == ["self", "obstacles", "refline"]
    assert names(diff.frenet) == ["cart", "refline", "solver", "layout", "order", "count", "line_index", "s_window"]
    assert names(diff.frenet_jvp)[:6] == ["solver", "cart", "refline", "frenet", "interval", "cart_dot"]
    for fn in (native.Context.frenet_device, native.Context.frenet_vjp_device, native.Context.frenet_jvp_device,
               native.frenet_host, native.frenet_vjp_host, native.frenet_jvp_host):
        assert callable(fn)
