"""What the compiler made of the kernels behind btrapz_frenet_device, _vjp_device and _jvp_device, read
from the code object the build produced (no GPU): the two instantiations of the forward (one per layout) and the four of
the derivative kernel (layout x VJP / JVP) are there once each and none spills; the forward keeps four arrays of 1 024
doubles (rx, ry, cos, sin of the staged line), the 256 flags of n_outside and the barrier reductions' words in LDS and
fits at least two wavefronts per SIMD; the derivative kernels use no LDS."""
from test_kernel_resources import kernels_of


def test_the_six_kernels_are_there_once_and_do_not_spill():
    ks = kernels_of("btrapz_frenet.o")
    forward = {n: r for n, r in ks.items() if "13frenet_kernelI" in n}
    grad = {n: r for n, r in ks.items() if "18frenet_grad_kernelI" in n}
    assert len(forward) == 2 and len(grad) == 4 and len(ks) == 6, sorted(ks)
    for name, r in ks.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 256 and r["agpr"] == 0, (name, r)   # 512 registers per SIMD lane: at least two wavefronts per SIMD
    for name, r in forward.items():
        assert 4 * 1024 * 8 + 256 * 4 <= r["lds"] <= 4 * 1024 * 8 + 256 * 4 + 512, (name, r)
    for name, r in grad.items():
        assert r["lds"] == 0, (name, r)
