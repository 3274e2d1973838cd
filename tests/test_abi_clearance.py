"""include/btrapz_hip_clearance.h held to the rules tests/test_abi_cartesian.py applies to its header: it compiles as plain
C99 on its own, the six declared symbols are exported, the twelfth prototype table of spectral_amd.native follows the
header's prototypes and is disjoint from the other eleven, the three structs have the header's layout, without a context
or with bad arguments the entry points refuse instead of crashing, and the Python surface is there."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from spectral_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "btrapz_hip_clearance.h")
COUNTS = {"btrapz_clearance_device": 13, "btrapz_clearance_vjp_device": 12, "btrapz_clearance_jvp_device": 14,
          "btrapz_clearance_host": 11, "btrapz_clearance_vjp_host": 10, "btrapz_clearance_jvp_host": 12}


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_header_is_plain_c_on_its_own_and_the_structs_match(tmp_path):
    src = tmp_path / "only.c"
    head = "const btrapz_footprint *, const btrapz_obstacles *, const int *, int, int, const double *, const int *, "
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "btrapz_hip_clearance.h"\n'
                   'int (*fwd)(btrapz_ctx *, ' + head + 'double, double *, int *, const btrapz_clear_audit *, void *) = btrapz_clearance_device;\n'
                   'int (*vjp)(btrapz_ctx *, ' + head + 'const int *, const double *, double *, void *) = btrapz_clearance_vjp_device;\n'
                   'int (*jvp)(btrapz_ctx *, ' + head + 'const int *, int, const double *, const double *, double *, void *) = btrapz_clearance_jvp_device;\n'
                   'int (*fwd_h)(' + head + 'double, double *, int *, const btrapz_clear_audit *) = btrapz_clearance_host;\n'
                   'int (*vjp_h)(' + head + 'const int *, const double *, double *) = btrapz_clearance_vjp_host;\n'
                   'int (*jvp_h)(' + head + 'const int *, int, const double *, const double *, double *) = btrapz_clearance_jvp_host;\n'
                   'int main(void) {\n'
                   '  printf("%d %d %d %d ", (int)sizeof(btrapz_footprint), (int)sizeof(btrapz_obstacles), (int)sizeof(btrapz_clear_audit), BTRAPZ_CLEAR_FEATURES);\n'
                   '  printf("%d %d %d %d %d\\n", (int)offsetof(btrapz_footprint, centre_offset), (int)offsetof(btrapz_obstacles, n), (int)offsetof(btrapz_obstacles, pose),\n'
                   '         (int)offsetof(btrapz_obstacles, obs_count), (int)offsetof(btrapz_clear_audit, n_invalid));\n'
                   '  return 0;\n}\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", inc, "-c", "-o", str(tmp_path / "only.o"), str(src)])
    # the layout, from a program that uses the types without the library
    sizes = tmp_path / "sizes.c"
    sizes.write_text(src.read_text().replace("= btrapz_clearance_device", "= 0").replace("= btrapz_clearance_vjp_device", "= 0")
                     .replace("= btrapz_clearance_jvp_device", "= 0").replace("= btrapz_clearance_host", "= 0")
                     .replace("= btrapz_clearance_vjp_host", "= 0").replace("= btrapz_clearance_jvp_host", "= 0"))
    subprocess.check_call(["gcc", "-std=c99", "-I", inc, "-o", str(tmp_path / "sizes"), str(sizes)])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")], text=True).split()]
    F, O, A = native.CFootprint, native.CObstacles, native.CClearAudit
    assert got == [C.sizeof(F), C.sizeof(O), C.sizeof(A), native.CLEAR_FEATURES, F.centre_offset.offset, O.n.offset, O.pose.offset,
                   O.obs_count.offset, A.n_invalid.offset]
    assert [f[0] for f in A._fields_] == list(native.CLEAR_AUDIT) == re.findall(r"\*(\w+);", re.search(
        r"typedef struct btrapz_clear_audit \{(.*?)\}", header_without_comments(), flags=re.S).group(1))


def test_the_declared_symbols_are_exported_and_in_the_twelfth_table_only(built):
    names = sorted(set(re.findall(r"\b(btrapz_[a-z_]+)\s*\(", header_without_comments())))
    assert names == sorted(COUNTS)
    assert set(names) == set(native.PROTOTYPES_CLEARANCE) == set(native.EXPORTS_CLEARANCE)
    others = (native.PROTOTYPES, native.PROTOTYPES_STAGE_JVP, native.PROTOTYPES_SCHEDULE, native.PROTOTYPES_SELECT,
              native.PROTOTYPES_CHECK, native.PROTOTYPES_LONG, native.PROTOTYPES_LONG_RESCUE, native.PROTOTYPES_LONG_GRAD,
              native.PROTOTYPES_LONG_SETS, native.PROTOTYPES_CARTESIAN, native.PROTOTYPES_FRENET)
    assert not any(set(names) & set(t) for t in others)
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}


@pytest.mark.parametrize("name,count", sorted(COUNTS.items()))
def test_argument_count_and_return_type_follow_the_header(built, name, count):
    m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, header_without_comments())
    params = [p.strip() for p in m.group(1).split(",")]
    fn = getattr(built, name)
    assert len(fn.argtypes) == len(params) == len(native.PROTOTYPES_CLEARANCE[name][1]) == count
    assert fn.restype is C.c_int
    # parameter by parameter: an int in the header is a c_int in the table, a double a c_double, everything else a pointer
    for text, ctype in zip(params, fn.argtypes):
        assert (ctype is C.c_int) == (re.fullmatch(r"int\s+\w+", text) is not None), (name, text, ctype)
        assert (ctype is C.c_double) == (re.fullmatch(r"double\s+\w+", text) is not None), (name, text, ctype)
    # the host twin takes the device call's parameters without the context and the stream
    if name.endswith("_host"):
        dev = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name.replace("_host", "_device"), header_without_comments())
        dev_params = [re.sub(r"\s+", " ", p.strip()) for p in dev.group(1).split(",")]
        assert [re.sub(r"\s+", " ", p) for p in params] == dev_params[1:-1]


def test_no_context_and_bad_arguments_are_refused_without_a_device(built):
    ft, ob = native.CFootprint(2.0, 1.0, 0.0), native.CObstacles(1, 1, 1, None, None, None)
    f, o = C.byref(ft), C.byref(ob)
    assert built.btrapz_clearance_device(None, f, o, None, 1, 1, None, None, 0.0, None, None, None, None) == -1   # BTRAPZ_EINVAL
    assert built.btrapz_clearance_vjp_device(None, f, o, None, 1, 1, None, None, None, None, None, None) == -1
    assert built.btrapz_clearance_jvp_device(None, f, o, None, 1, 1, None, None, None, 1, None, None, None, None) == -1
    assert built.btrapz_clearance_host(None, None, None, 1, 1, None, None, 0.0, None, None, None) == -1
    assert built.btrapz_clearance_host(f, o, None, 1, 1, None, None, 0.0, None, None, None) == -1
    assert built.btrapz_clearance_vjp_host(f, o, None, 1, 1, None, None, None, None, None) == -1
    assert built.btrapz_clearance_jvp_host(f, o, None, 1, 1, None, None, None, 1, None, None, None) == -1


def test_python_surface_is_there():
    from spectral_amd import diff, layout, synth
    from spectral_amd.solver import BatchSolver
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(BatchSolver.clearance) == ["self", "cart", "obstacles", "footprint", "scene_index", "count", "d_safe", "want"]
    assert names(BatchSolver.clearance_vjp) == ["self", "cart", "obstacles", "footprint", "which", "clear_bar", "scene_index", "count"]
    assert names(BatchSolver.clearance_jvp) == ["self", "cart", "obstacles", "footprint", "which", "cart_dot", "obs_dot", "scene_index",
                                                "count"]
    assert names(BatchSolver.collision_free) == ["audit", "d_safe"]
    assert names(diff.clearance) == ["cart", "obstacles", "footprint", "solver", "scene_index", "count"]
    assert names(diff.clearance_jvp)[:6] == ["solver", "cart", "obstacles", "footprint", "which", "cart_dot"]
    assert names(synth.obstacles_on_line)[:4] == ["refline", "s0", "l0", "v"]
    assert names(layout.Obstacles.__init__) == ["self", "pose", "half", "obs_count"]
    for fn in (native.Context.clearance_device, native.Context.clearance_vjp_device, native.Context.clearance_jvp_device,
               native.clearance_host, native.clearance_vjp_host, native.clearance_jvp_host):
        assert callable(fn)


def test_obstacles_on_line_places_rectangles_through_the_cartesian_twin():
    import numpy as np
    from spectral_amd import synth
    rl = synth.refline_straight(50.0, 0.5)
    ob = synth.obstacles_on_line(rl, [[10.0, 45.0]], [[1.0, -2.0]], [[5.0, 10.0]], n=11, dt=0.1, half=(2.0, 1.0), dtheta=0.25)
    assert (ob.n_scenes, ob.O, ob.n) == (1, 2, 11)
    p = ob.host["pose"]
    assert np.allclose(p[0, 0, 0], 10.0 + 0.5 * np.arange(11)) and np.array_equal(p[0, 0, 1], np.full(11, 1.0)) and np.allclose(p[0, 0, 2], 0.25)
    # the second one runs off the table (50 m) after sample 5: absent from there on
    assert np.isfinite(p[0, 1, :, :6]).all() and np.isnan(p[0, 1, :, 6:]).all()
