"""The kernel of btrapz_corridor_batch_vjp_device, read from the code object the build produced (no GPU): no scratch, and
within the register file (tests/test_kernel_resources.py reads the code objects)."""
from test_kernel_resources import kernels_of


def test_corridor_vjp_kernel_has_no_scratch():
    ks = kernels_of("corridor_vjp.o")
    names = sorted(n for n in ks if "corridor_vjp_kernel" in n)
    assert len(names) == 1, names
    r = ks[names[0]]
    assert r["scratch"] == 0, (names[0], r)
    assert r["vgpr"] + r["agpr"] <= 512, (names[0], r)
