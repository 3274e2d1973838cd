"""The kernel of btrapz_solve_jvp_device, read from the code object the build produced (no GPU): exactly one kernel in its
translation unit, no scratch, one wavefront per SIMD or better (tests/test_kernel_resources.py reads the code objects)."""
from test_kernel_resources import kernels_of


def test_jvp_kernel_has_no_scratch():
    ks = kernels_of("btrapz_jvp.o")
    assert len(ks) == 1 and all("jvp_kernel" in n for n in ks), sorted(ks)
    for name, r in ks.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 512, (name, r)
