"""The kernels of btrapz_solve_long_vjp_device / btrapz_solve_long_jvp_device, read from the code object the build produced (no
GPU): exactly the three kernels of btrapz_long_grad.hip, no scratch, one wavefront per SIMD or better
(tests/test_kernel_resources.py reads the code objects)."""
from test_kernel_resources import kernels_of

KERNELS = ("long_vjp_kernel", "long_jvp_kernel", "long_cost_dot_kernel")


def test_long_grad_kernels_have_no_scratch():
    ks = kernels_of("btrapz_long_grad.o")
    assert len(ks) == len(KERNELS), sorted(ks)
    for want in KERNELS:
        assert sum(want in n for n in ks) == 1, (want, sorted(ks))
    for name, r in ks.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 512, (name, r)


def test_the_64_segment_kernels_keep_their_translation_units():
    """The new kernels went into a translation unit of their own: btrapz_vjp.o and btrapz_jvp.o still hold one kernel each."""
    assert len(kernels_of("btrapz_vjp.o")) == 1 and len(kernels_of("btrapz_jvp.o")) == 1
