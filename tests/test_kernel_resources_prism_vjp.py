"""The kernel of btrapz_prism_bounds_vjp_device, read from the code object the build produced (no GPU): no scratch, and
registers that leave the read-bound kernel its wavefronts (tests/test_kernel_resources.py reads the code objects)."""
from test_kernel_resources import kernels_of


def test_prism_vjp_kernel_has_no_scratch():
    ks = kernels_of("prism_vjp.o")
    names = sorted(n for n in ks if "prism_bounds_vjp_kernel" in n)
    assert len(names) == 1, names
    r = ks[names[0]]
    assert r["scratch"] == 0, (names[0], r)
    assert r["vgpr"] + r["agpr"] <= 128, (names[0], r)   # four wavefronts per SIMD at the least
