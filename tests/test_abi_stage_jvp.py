"""include/btrapz_hip_stage_jvp.h held to the rules tests/test_abi.py applies to include/btrapz_hip.h: every declared symbol
is exported, the second prototype table of spectral_amd.native follows the header's prototypes, and the header is plain C99."""
import ctypes as C
import os
import re
import subprocess

import pytest

from spectral_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "btrapz_hip_stage_jvp.h")


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


def test_every_declared_symbol_is_exported_and_in_the_second_table(built):
    names = sorted(set(re.findall(r"\b(btrapz_[a-z_]+)\s*\(", header_without_comments())))
    assert names == sorted(declared_prototypes()) and len(names) == 4
    for n in names:
        assert hasattr(built, n), n
    assert set(names) == set(native.PROTOTYPES_STAGE_JVP) == set(native.EXPORTS_STAGE_JVP)
    assert not set(names) & set(native.PROTOTYPES)          # the first table keeps to include/btrapz_hip.h
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported


def test_argument_counts_and_return_types_follow_the_header(built):
    ctype = {"int": C.c_int, "double": C.c_double, "const char *": C.c_char_p, "long long": C.c_longlong, "void": None}
    for name, (ret, n_params) in declared_prototypes().items():
        fn = getattr(built, name)
        assert len(fn.argtypes) == n_params == len(native.PROTOTYPES_STAGE_JVP[name][1]), name
        assert fn.restype is ctype[ret] and native.PROTOTYPES_STAGE_JVP[name][0] is ctype[ret], (name, ret)


def test_the_first_header_names_nothing_new():
    first = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "btrapz_hip.h")).read(), flags=re.S)
    for word in ("jvp_host", "prism_bounds_jvp", "corridor_batch_jvp", "corridor_jvp", "btrapz_knot_tangents", "stage_jvp"):
        assert word not in first, word


def test_header_is_plain_c99_and_the_struct_matches_its_mirror(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "btrapz_hip_stage_jvp.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d\\n", sizeof(btrapz_knot_tangents), offsetof(btrapz_knot_tangents, dl_bounds_knots), '
                   'offsetof(btrapz_knot_tangents, l_ref), BTRAPZ_MAX_TANGENTS); return 0; }\n')
    exe = tmp_path / "hdr"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    K = native.CKnotTangents
    assert got == [C.sizeof(K), K.dl_bounds_knots.offset, K.l_ref.offset, native.MAX_TANGENTS]
    assert [f[0] for f in K._fields_] == list(native.KNOT_GRADS)
