"""What the compiler made of the kernels behind btrapz_cartesian_device, _vjp_device and _jvp_device, read
from the code object the build produced (no GPU): the six instantiations of the forward (layout x cart / audit / both) and the
four of the derivative kernel (layout x VJP / JVP) are there once each, none spills, each keeps its wavefronts' four slices
of 1 024 doubles in LDS and nothing else there, and each fits at least two wavefronts per SIMD."""
from test_kernel_resources import kernels_of


def test_the_ten_kernels_are_there_once_and_do_not_spill():
    ks = kernels_of("btrapz_cartesian.o")
    forward = {n: r for n, r in ks.items() if "16cartesian_kernelI" in n}
    grad = {n: r for n, r in ks.items() if "21cartesian_grad_kernelI" in n}
    assert len(forward) == 6 and len(grad) == 4 and len(ks) == 10, sorted(ks)
    for name, r in ks.items():
        assert r["scratch"] == 0, (name, r)
        assert r["lds"] == 4 * 1024 * 8, (name, r)
        assert r["vgpr"] <= 256 and r["agpr"] == 0, (name, r)   # 512 registers per SIMD lane: at least two wavefronts per SIMD
