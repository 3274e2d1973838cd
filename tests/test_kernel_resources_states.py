"""The kernels of btrapz_sample_vjp_device / btrapz_eval_states_vjp_device, read from the code object the build produced
(no GPU): no scratch, and within the register file (tests/test_kernel_resources.py reads the code objects)."""
from test_kernel_resources import kernels_of


def test_states_kernels_have_no_scratch():
    ks = kernels_of("btrapz_states.o")
    names = sorted(n for n in ks if "vjp_kernel" in n)
    assert len(names) == 2 and any("sample_vjp" in n for n in names) and any("eval_states_vjp" in n for n in names), names
    for name in names:
        r = ks[name]
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 512, (name, r)
