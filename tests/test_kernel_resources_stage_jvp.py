"""The kernels of btrapz_prism_bounds_jvp_device and btrapz_corridor_batch_jvp_device, read from the code objects the build
produced (no GPU): no scratch; the prism kernel within 128 registers (four wavefronts per SIMD, as the backward kernel); the
corridor kernel's register count is printed and recorded in DESIGN 3.13, not pinned."""
from test_kernel_resources import kernels_of


def only(obj, word):
    ks = kernels_of(obj)
    names = sorted(n for n in ks if word in n)
    assert len(names) == 1, names
    return names[0], ks[names[0]]


def test_prism_jvp_kernel_has_no_scratch_and_at_most_128_registers():
    name, r = only("prism_jvp.o", "prism_bounds_jvp_kernel")
    print(name, r)
    assert r["scratch"] == 0 and r["lds"] == 0, (name, r)      # (its LDS is dynamic: tables, owners, the staged tangents)
    assert r["vgpr"] + r["agpr"] <= 128, (name, r)


def test_corridor_jvp_kernel_has_no_scratch():
    name, r = only("corridor_jvp.o", "corridor_jvp_kernel")
    print(name, "registers:", r["vgpr"] + r["agpr"], r)
    assert r["scratch"] == 0, (name, r)
    assert r["vgpr"] + r["agpr"] <= 512, (name, r)
