"""The kernel of btrapz_solve_vjp_device, read from the code object the build produced (no GPU): no scratch, one
wavefront per SIMD or better (tests/test_kernel_resources.py reads the code objects)."""
from test_kernel_resources import kernels_of


def test_vjp_kernel_has_no_scratch():
    ks = {n: r for n, r in kernels_of("btrapz_vjp.o").items() if "vjp_kernel" in n}
    assert len(ks) == 1, sorted(ks)
    for name, r in ks.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 512, (name, r)
