"""What the compiler made of the kernels behind btrapz_clearance_device, _vjp_device and _jvp_device, read
from the code object the build produced (no GPU): the seven instantiations of the forward (every non-empty choice of clear,
which, audit) and the two of the derivative kernel (VJP, JVP) are there once each, none spills, none uses LDS (the stage
has no staging and no barrier), and all fit at least two wavefronts per SIMD -- in fact four: 128 registers or fewer."""
from test_kernel_resources import kernels_of


def test_the_nine_kernels_are_there_once_and_do_not_spill():
    ks = kernels_of("btrapz_clearance.o")
    forward = {n: r for n, r in ks.items() if "16clearance_kernelI" in n}
    grad = {n: r for n, r in ks.items() if "21clearance_grad_kernelI" in n}
    assert len(forward) == 7 and len(grad) == 2 and len(ks) == 9, sorted(ks)
    forms = sorted(n.split("16clearance_kernelI")[1][:11] for n in forward)
    assert forms == sorted("Lb%dELb%dELb%d" % (c, w, a) for c in (0, 1) for w in (0, 1) for a in (0, 1) if c + w + a), forms
    for name, r in ks.items():
        assert r["scratch"] == 0, (name, r)
        assert r["lds"] == 0, (name, r)
        assert r["vgpr"] <= 256 and r["agpr"] == 0, (name, r)   # 512 registers per SIMD lane: at least two wavefronts per SIMD
        assert r["vgpr"] <= 128, (name, r)                      # what DESIGN 3.21 states: four
