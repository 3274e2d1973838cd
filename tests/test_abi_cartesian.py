"""include/btrapz_hip_cartesian.h held to the rules tests/test_long_grad_abi.py applies to its header: it compiles as plain
C99 on its own, the six declared symbols are exported, the tenth prototype table of spectral_amd.native follows the
header's prototypes and is disjoint from the other nine, the ctypes mirrors of the two structs have the header's fields,
without a context or with bad arguments the entry points refuse instead of crashing, and the Python surface is there."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from spectral_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "btrapz_hip_cartesian.h")
COUNTS = {"btrapz_cartesian_device": 11, "btrapz_cartesian_vjp_device": 11, "btrapz_cartesian_jvp_device": 12,
          "btrapz_cartesian_host": 9, "btrapz_cartesian_vjp_host": 9, "btrapz_cartesian_jvp_host": 10}


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_header_is_plain_c_on_its_own(tmp_path):
    src = tmp_path / "only.c"
    head = "const btrapz_refline *, const int *, int, int, int, const double *, const int *, "
    src.write_text('#include "btrapz_hip_cartesian.h"\n'
                   'int (*fwd)(btrapz_ctx *, ' + head + 'double *, const btrapz_kin_audit *, void *) = btrapz_cartesian_device;\n'
                   'int (*vjp)(btrapz_ctx *, ' + head + 'const double *, double *, void *) = btrapz_cartesian_vjp_device;\n'
                   'int (*jvp)(btrapz_ctx *, ' + head + 'int, const double *, double *, void *) = btrapz_cartesian_jvp_device;\n'
                   'int (*fwd_h)(' + head + 'double *, const btrapz_kin_audit *) = btrapz_cartesian_host;\n'
                   'int (*vjp_h)(' + head + 'const double *, double *) = btrapz_cartesian_vjp_host;\n'
                   'int (*jvp_h)(' + head + 'int, const double *, double *) = btrapz_cartesian_jvp_host;\n'
                   'int layouts[2] = {BTRAPZ_FRENET_SAMPLES, BTRAPZ_FRENET_STATES};\n'
                   'int rows[6] = {BTRAPZ_CART_X, BTRAPZ_CART_Y, BTRAPZ_CART_THETA, BTRAPZ_CART_KAPPA, BTRAPZ_CART_V, BTRAPZ_CART_A};\n'
                   'unsigned long sizes[2] = {sizeof(btrapz_refline), sizeof(btrapz_kin_audit)};\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           "-o", str(tmp_path / "only.o"), str(src)])


def test_the_declared_symbols_are_exported_and_in_the_tenth_table_only(built):
    names = sorted(set(re.findall(r"\b(btrapz_[a-z_]+)\s*\(", header_without_comments())))
    assert names == sorted(COUNTS)
    assert set(names) == set(native.PROTOTYPES_CARTESIAN) == set(native.EXPORTS_CARTESIAN)
    others = (native.PROTOTYPES, native.PROTOTYPES_STAGE_JVP, native.PROTOTYPES_SCHEDULE, native.PROTOTYPES_SELECT,
              native.PROTOTYPES_CHECK, native.PROTOTYPES_LONG, native.PROTOTYPES_LONG_RESCUE, native.PROTOTYPES_LONG_GRAD,
              native.PROTOTYPES_LONG_SETS)
    assert not any(set(names) & set(t) for t in others)
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("name,count", sorted(COUNTS.items()))
def test_argument_count_and_return_type_follow_the_header(built, name, count):
    m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, header_without_comments())
    params = [p.strip() for p in m.group(1).split(",")]
    fn = getattr(built, name)
    assert len(fn.argtypes) == len(params) == len(native.PROTOTYPES_CARTESIAN[name][1]) == count
    assert fn.restype is C.c_int
    # parameter by parameter: an int in the header is a c_int in the table, everything else a pointer
    for text, ctype in zip(params, fn.argtypes):
        assert (ctype is C.c_int) == (re.fullmatch(r"int\s+\w+", text) is not None), (name, text, ctype)
    # the host twin takes the device call's parameters without the context and the stream
    if name.endswith("_host"):
        dev = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name.replace("_host", "_device"), header_without_comments())
        dev_params = [re.sub(r"\s+", " ", p.strip()) for p in dev.group(1).split(",")]
        assert [re.sub(r"\s+", " ", p) for p in params] == dev_params[1:-1]


def test_the_struct_mirrors_have_the_headers_fields():
    text = header_without_comments()
    ref = re.search(r"typedef struct btrapz_refline \{(.*?)\} btrapz_refline;", text, flags=re.S).group(1)
    assert [n for n, _ in native.CRefLine._fields_] == re.findall(r"\*?(\w+)\s*[,;]", ref)
    assert C.sizeof(native.CRefLine) == 2 * C.sizeof(C.c_int) + 6 * C.sizeof(C.c_void_p)
    aud = re.search(r"typedef struct btrapz_kin_audit \{(.*?)\} btrapz_kin_audit;", text, flags=re.S).group(1)
    assert [n for n, _ in native.CKinAudit._fields_] == re.findall(r"\*(\w+)\s*;", aud) == list(native.KIN_AUDIT)
    assert (native.FRENET_SAMPLES, native.FRENET_STATES) == tuple(int(re.search(r"#define %s (\d+)" % n, text).group(1))
                                                                  for n in ("BTRAPZ_FRENET_SAMPLES", "BTRAPZ_FRENET_STATES"))
    assert native.MAX_TANGENTS == 32


def test_no_context_is_refused_without_a_device(built):
    t = native.CRefLine(1, 2, *[0] * 6)
    assert built.btrapz_cartesian_device(None, C.byref(t), None, 1, 1, 0, None, None, None, None, None) == -1   # BTRAPZ_EINVAL
    assert built.btrapz_cartesian_vjp_device(None, C.byref(t), None, 1, 1, 0, None, None, None, None, None) == -1
    assert built.btrapz_cartesian_jvp_device(None, C.byref(t), None, 1, 1, 0, None, None, 1, None, None, None) == -1
    assert built.btrapz_cartesian_host(None, None, 1, 1, 0, None, None, None, None) == -1
    assert built.btrapz_cartesian_vjp_host(C.byref(t), None, 1, 1, 0, None, None, None, None) == -1
    assert built.btrapz_cartesian_jvp_host(C.byref(t), None, 1, 1, 0, None, None, 1, None, None) == -1


def test_python_surface_is_there():
    from spectral_amd import diff, layout, synth
    from spectral_amd.solver import BatchSolver
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(BatchSolver.cartesian) == ["self", "frenet", "refline", "layout", "count", "line_index", "want"]
    assert inspect.signature(BatchSolver.cartesian).parameters["want"].default == ("cart", "audit")
    assert names(BatchSolver.cartesian_vjp) == ["self", "frenet", "refline", "cart_bar", "layout", "count", "line_index"]
    assert names(BatchSolver.cartesian_jvp) == ["self", "frenet", "refline", "frenet_dot", "layout", "count", "line_index"]
    assert names(BatchSolver.kinematic_admissible) == ["audit", "kappa_max", "alat_max", "a_lo", "a_hi", "frame_margin"]
    assert isinstance(inspect.getattr_static(BatchSolver, "kinematic_admissible"), staticmethod)
    assert names(diff.cartesian) == ["frenet", "refline", "solver", "layout", "count", "line_index"]
    assert names(diff.cartesian_jvp)[:4] == ["solver", "frenet", "refline", "frenet_dot"]
    assert names(diff.scene_jacobian_cartesian)[:2] == ["solver", "refline"] and set(names(diff.scene_jacobian)) < set(names(diff.scene_jacobian_cartesian))
    for fn in (native.Context.cartesian_device, native.Context.cartesian_vjp_device, native.Context.cartesian_jvp_device,
               native.cartesian_host, native.cartesian_vjp_host, native.cartesian_jvp_host, layout.RefLine, synth.refline_straight,
               synth.refline_arc, synth.refline_clothoid):
        assert callable(fn)
