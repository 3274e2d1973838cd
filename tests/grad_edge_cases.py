"""Cases and helpers shared by the CPU and GPU tests of the solve's derivative kernels (vjp_kernel, jvp_kernel) at the
edges of their lane mapping: one lane per segment, a group of S lanes per axis problem, gpw = 64 // S problems per
wavefront, the spare lanes of a wavefront aliased onto its last group, the groups beyond the batch clamped onto
candidate B - 1 (headers of btrapz_vjp.hip and btrapz_jvp.hip).

Per width the candidates held to the oracle-based yardsticks (tests/vjp_reference.py, tests/jvp_reference.py) sit in

    gpw - 1   the last group of wavefront 0, next to the aliased spare lanes,
    gpw       the first group of wavefront 1,
    B - 1     alone in the last wavefront (B = 253 = 1 mod gpw for every gpw in 21, 12, 6, 3, 2), beside the lanes
              clamped onto it;

from 33 segments on a wavefront holds one group and the first two collapse to slot 1; at 63 only B - 1 of scenario_1
is compared (one candidate's yardstick costs seconds of CPU there).  build() puts a solved, strictly complementary
candidate into every such slot, so that no comparison is ever skipped."""
import numpy as np

from jvp_reference import KEYS
from spectral_amd import layout as L, synth
from vjp_reference import Adjoint, one

WIDTHS = (3, 5, 10, 20, 21, 32, 33, 63)
B = 253
B_EXT = 256   # the batch extended for the independence-of-B checks: the last wavefront full (gpw 2) or fuller
FAMILIES = {
    "generic": lambda S, seed: synth.make_batch(B, S, config=3, variant=0, seed=seed),
    "scenario_1": lambda S, seed: synth.make_scenario1_batch(B, S, 0, seed=seed),
    "cuboid": lambda S, seed: synth.make_scenario1_batch(B, S, 1, seed=seed),
}
CASES = [(family, S) for S in WIDTHS for family in FAMILIES if S != 63 or family == "scenario_1"]
# primal-side gradients: unique even where the multipliers are not
PRIMAL_SEG = [L.F_X_SKEW, L.F_X_BIAS, L.F_Y_SKEW, L.F_Y_BIAS]
PRIMAL_SHARED = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
SHAPES = lambda T, B_, S: dict(seg=(T, L.NUM_SEG_FIELDS, B_, S), init=(T, B_, 6), ref_end=(T, B_, 2), dl_bounds=(T, B_, 10),
                               shared=(T, B_, 20))
# strides of the mixed-count records (neither divides 64) and the counts compared with uniform calls: 1, 2, stride - 1,
# stride and the counts either side of 64 / 3 and 64 / 2 (where another number of groups fits a wavefront)
RAGGED_STRIDES = (21, 33)
RAGGED_FAMILIES = ("scenario_1", "cuboid")


def gpw(S):
    return 64 // S


def target_slots(S):
    if S == 63:
        return (B - 1,)
    return tuple(sorted({max(gpw(S) - 1, 1), gpw(S), B - 1}))


def ragged_counts(stride):
    return tuple(sorted({n for n in (1, 2, 21, 22, 32, 33, stride - 1, stride) if n <= stride}))


def generate(family, S):
    """The family's batch of B candidates as generated (seed 100 + S, as test_gpu_vjp.py)."""
    return FAMILIES[family](S, 100 + S)


def _swap(batch, i, j):
    for a in (batch.init, batch.ref_end, batch.dl_bounds):
        a[[i, j]] = a[[j, i]]
    batch.seg[:, [i, j]] = batch.seg[:, [j, i]]


_built = {}


def build(family, S):
    """(batch, sh, targets, perm, adjoints): the family's batch with a solved (status 1), strictly complementary candidate
    in every target slot.  The yardstick alone decides (Adjoint(one(batch, b), sh, 0, 0): status 1 and .strict); a target
    slot that is not such a candidate is swapped (seg[:, b], init, ref_end and dl_bounds rows) with the first such
    candidate of the batch, scanned in order, that is no target slot itself.  perm[b]: the generated candidate now in
    slot b.  adjoints[b]: the yardstick's Adjoint of target slot b with zero cotangents (unique_masks() for its masks).
    Computed once per case and shared; nobody changes what it returns."""
    if (family, S) in _built:
        return _built[(family, S)]
    batch, sh = generate(family, S)
    batch = L.Batch(B=batch.B, S=batch.S, seg=batch.seg.copy(), init=batch.init.copy(), ref_end=batch.ref_end.copy(),
                    dl_bounds=batch.dl_bounds.copy())
    targets = target_slots(S)
    perm = np.arange(B)
    zero = np.zeros(12 * S)

    def yardstick(b):
        adj = Adjoint(one(batch, b), sh, zero, 0.0)
        return adj if adj.status == 1 and adj.strict else None

    adjoints = {}
    scan = 0
    for t in targets:
        adj = yardstick(t)
        while adj is None:
            while scan in targets:
                scan += 1
            assert scan < B, (family, S, "no strictly complementary candidate left for slot", t)
            adj = yardstick(scan)
            if adj is not None:
                _swap(batch, t, scan)
                perm[[t, scan]] = perm[[scan, t]]
            scan += 1
        adjoints[t] = adj
    _built[(family, S)] = (batch, sh, targets, perm, adjoints)
    return _built[(family, S)]


_masks = {}


def unique_masks(family, S):
    """{target slot: Adjoint.unique_mask()} of a case: where the derivatives are unique (no two fields tie at a joint, not
    at the cuboid's kink).  The masks do not depend on the cotangents.  Computed once per case."""
    if (family, S) not in _masks:
        adjoints = build(family, S)[4]
        for adj in adjoints.values():
            adj.grads()
        _masks[(family, S)] = {b: adj.unique_mask() for b, adj in adjoints.items()}
    return _masks[(family, S)]


# ---- helpers of the GPU tests (test_gpu_vjp.py, test_gpu_jvp.py and their *_edges.py) ---------------------------------

def _solve_and_vjp(solver, batch, sh, xbar, cbar, lean=0):
    import torch
    db = solver.upload(batch)
    o = solver.solve(db, sh, keep_multipliers=True, lean=lean, out={
        "ctrl": torch.zeros((batch.B, 12 * batch.S), dtype=torch.float64, device=solver.device),
        "cost": torch.empty(batch.B, dtype=torch.float64, device=solver.device),
        "status": torch.empty(batch.B, dtype=torch.int32, device=solver.device),
        "iters": torch.empty(batch.B, dtype=torch.int32, device=solver.device)})
    g = solver.solve_vjp(db, sh, o, xbar, cbar)
    torch.cuda.synchronize()
    return o, {k: v.cpu().numpy() for k, v in g.items()}


def _cand(g, b):
    return dict(seg=g["seg"][:, b], init=g["init"][b], ref_end=g["ref_end"][b], dl_bounds=g["dl_bounds"][b],
                shared=g["shared"][b])


def _close(a, r, tol=1e-4):
    return np.abs(a - r).max() <= tol * max(np.abs(r).max(), np.abs(a).max(), 1e-300)


def _solve(solver, batch, sh, lean=0):
    import torch
    db = solver.upload(batch)
    d = solver.device
    o = solver.solve(db, sh, keep_multipliers=True, lean=lean, out={
        "ctrl": torch.zeros((batch.B, 12 * batch.S), dtype=torch.float64, device=d),
        "cost": torch.empty(batch.B, dtype=torch.float64, device=d),
        "status": torch.empty(batch.B, dtype=torch.int32, device=d),
        "iters": torch.empty(batch.B, dtype=torch.int32, device=d)})
    return db, o


def _directions(rng, T, B_, S, keys=KEYS):
    """Dense random tangents [T, ...] in the named arrays (numpy); field 0 of seg random too: it must be ignored."""
    return {k: rng.standard_normal(SHAPES(T, B_, S)[k]) for k in keys}


def _dev(solver, tan):
    import torch
    return {k: torch.tensor(v, device=solver.device) for k, v in tan.items()}


def _ragged(solver, batch, W, counts):
    """The batch in a ragged record of stride W with the given segment counts (candidates keep their first count segments)."""
    import torch
    d = solver.device
    seg = np.zeros((L.NUM_SEG_FIELDS, batch.B, W)); seg[:, :, :batch.S] = batch.seg
    return dict(B=batch.B, seg_stride=W, seg=torch.tensor(seg, device=d), seg_count=torch.tensor(counts, dtype=torch.int32, device=d),
                init=torch.tensor(batch.init, device=d), ref_end=torch.tensor(batch.ref_end, device=d),
                dl_bounds=torch.tensor(batch.dl_bounds, device=d))


FLOOR = 1e-3


def _per_tangent_ratios(cd, cs, ref_x, ref_c):
    """Errors of ctrl_dot [T, 12 S] and cost_dot [T] of one candidate, each tangent relative to ITS OWN reference's largest
    entry.  A tangent whose reference is (nearly) 0 is measured against FLOOR = 1e-3 of the candidate's largest tangent.
    The floor comes from the yardstick's own error: its least-squares solve of the singular KKT matrix differs from a
    null-space solve of the same system by up to 7e-8 of the largest tangent (64 segments, CPU only), so a reference
    of exactly 0 comes back as 1e-10 to 1e-8, and 1e-4 x 1e-3 = 1e-7 of the largest tangent is what it can certify."""
    nx = np.abs(ref_x).max(1); nc = np.abs(ref_c)
    sx = np.maximum(nx, max(FLOOR * nx.max(), 1e-300)); sc = np.maximum(nc, max(FLOOR * nc.max(), 1e-300))
    return np.abs(cd - ref_x).max(1) / sx, np.abs(cs - ref_c) / sc


def _fmt(v):
    return "[" + " ".join("%.1e" % x for x in np.atleast_1d(v)) + "]"


def _identity(solver, rec, sets, o, set_index, S, T=3, seed=0, keys=KEYS):
    import torch
    rng = np.random.default_rng(seed)
    Bn = rec["B"] if isinstance(rec, dict) else rec.B
    d = solver.device
    tan = _directions(rng, T, Bn, S)
    for k in KEYS:
        if k not in keys:
            tan[k][:] = 0.0
    xbar = rng.standard_normal((Bn, 12 * S)); cbar = rng.standard_normal(Bn)
    g = solver.solve_vjp(rec, sets, o, torch.tensor(xbar, device=d), torch.tensor(cbar, device=d), set_index=set_index)
    j = solver.solve_jvp(rec, sets, o, _dev(solver, tan), set_index=set_index)
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in g.items()}
    cd, cs = j["ctrl"].cpu().numpy(), j["cost"].cpu().numpy()
    st = o["status"].cpu().numpy()
    solved = (st == 1) | (st == 2)
    assert solved.sum() >= Bn // 2
    worst = 0.0
    for t in range(T):
        lhs = (xbar * cd[t]).sum(1) + cbar * cs[t]
        mag = (np.abs(xbar) * np.abs(cd[t])).sum(1) + np.abs(cbar) * np.abs(cs[t])
        rhs = (np.moveaxis(g["seg"], 1, 0) * np.moveaxis(tan["seg"][t], 1, 0)).sum((1, 2))
        for k in ("init", "ref_end", "dl_bounds", "shared"):
            rhs = rhs + (g[k] * tan[k][t]).sum(1)
        ratio = np.abs(lhs - rhs)[solved] / np.maximum(mag[solved], 1e-300)
        worst = max(worst, float(ratio.max()))
    return worst


# ---- what both edge files do alike ------------------------------------------------------------------------------------

def extended(a, axis):
    """A device tensor with B entries along `axis`, extended to B_EXT by copies of its first entries."""
    import torch
    idx = torch.arange(B_EXT - B, device=a.device)
    return torch.cat([a, a.index_select(axis, idx)], dim=axis).contiguous()


def extended_solve(db, o):
    """The record and the kept solve of B candidates as one of B_EXT: candidates B ... B_EXT - 1 repeat the first ones
    (record, ctrl, lam and status alike, so they are solved candidates like any other)."""
    from spectral_amd.solver import DeviceBatch
    rec = DeviceBatch.from_tensors(extended(db.seg, 1), extended(db.init, 0), extended(db.ref_end, 0), extended(db.dl_bounds, 0),
                                   None, B=B_EXT, S=db.S)
    return rec, dict(ctrl=extended(o["ctrl"], 0), lam=extended(o["lam"], 2), status=extended(o["status"], 0))


def ragged_solve(solver, family, stride):
    """(rec, sh, o, counts): the family's batch of `stride` segments as a ragged record of that stride whose segment counts
    cycle over 1 ... stride, and its kept solve."""
    import torch
    batch, sh = generate(family, stride)
    counts = 1 + np.arange(B) % stride
    rec = _ragged(solver, batch, stride, counts)
    idx0 = torch.zeros(B, dtype=torch.int32, device=solver.device)
    o = solver.solve_sets_ragged(rec, [sh], idx0, keep_multipliers=True)
    return rec, sh, o, counts


def uniform_part(rec, o, counts, n):
    """The candidates of a ragged solve whose count is n as a uniform record of stride n with its solve: (sel, record, out).
    ctrl of a ragged candidate has the s axis at [0, 6 n) and the l axis at [6 n, 12 n); lam is lam[..., :n]."""
    import torch
    from spectral_amd.solver import DeviceBatch
    sel_np = np.flatnonzero(counts == n)
    sel = torch.tensor(sel_np, device=rec["seg"].device)
    u = DeviceBatch.from_tensors(rec["seg"][:, sel, :n].contiguous(), rec["init"][sel].contiguous(), rec["ref_end"][sel].contiguous(),
                                 rec["dl_bounds"][sel].contiguous(), None, B=len(sel_np), S=n)
    ou = dict(ctrl=o["ctrl"][sel, :12 * n].contiguous(), lam=o["lam"][:, :, sel, :n].contiguous(), status=o["status"][sel].contiguous())
    return sel, u, ou
