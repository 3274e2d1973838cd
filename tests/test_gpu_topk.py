"""Deterministic K-best selection on the GPU (include/btrapz_hip_select.h): btrapz_topk_device, btrapz_topk_pairs_device,
btrapz_gather_rows_device, BatchSolver.topk.

Every comparison is exact -- int64 indices and the bit patterns of the costs; no tolerance is involved.  The yardstick, in
numpy on the downloaded costs: the candidates that take part are `cost < inf` (NaN is false), order = np.lexsort((idx,
cost)), the first K, padded with (-1, +inf).  The data is small integers as float64, so ties are everywhere; about 10 %
are +inf, a few are NaN, and where there are several groups the last one is entirely +inf.

Group sizes: the edges of a wavefront (63, 64, 65), of the one-wavefront / 256-thread block choice (255, 256, 257), of the
block's stride (1 023, 1 025), of the split over blocks, which sits where the arg-min's does (8 191, 8 192, 8 193), and
65 536 (64 blocks and the merging launch).  The merging launch takes 4 partial lists per wavefront: 10 241 and 20 481 give
it 3 and 6 wavefronts (an odd count and one that is no power of two in its LDS tree), 300 001 is beyond the cap of 256
blocks per group."""
import numpy as np
import pytest
import torch

from spectral_amd import dist, native, synth
from spectral_amd.native import BtrapzError

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 8191, 8192, 8193, 10241, 20481, 65536, 300001]
KS = [1, 2, 5, 63, 64]            # (K > group: at group sizes 1, 2 and 63)


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def groups_of(size):
    return 3 if size <= 1025 else 2 if size <= 8193 else 1


def make_costs(rng, groups, size):
    c = rng.integers(0, 7, groups * size).astype(np.float64)
    c[rng.random(c.size) < 0.10] = np.inf
    c[rng.random(c.size) < 0.01] = np.nan
    if groups > 1:
        c[(groups - 1) * size:] = np.inf
    return c


def yardstick(cost, idx, K):
    """The K best of the entries (cost, idx) that take part, padded with (-1, +inf)."""
    m = (cost < np.inf) & (idx >= 0)
    c, i = cost[m], idx[m]
    order = np.lexsort((i, c))[:K]
    bi, bc = np.full(K, -1, np.int64), np.full(K, np.inf)
    bi[:order.size] = i[order]; bc[:order.size] = c[order]
    return bi, bc


def yardstick_groups(cost, group, K, base=0):
    G = cost.size // group
    out = [yardstick(cost[g * group:(g + 1) * group], np.arange(g * group, (g + 1) * group, dtype=np.int64) + base, K)
           for g in range(G)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def same(got_i, got_c, want_i, want_c):
    return np.array_equal(got_i, want_i) and np.array_equal(got_c.view(np.int64), want_c.view(np.int64))


def topk(solver, cost, group, K, base=0):
    bi, bc = solver.topk(torch.from_numpy(cost).to(solver.device), K, group=group, index_base=base)
    torch.cuda.synchronize()
    return bi.cpu().numpy(), bc.cpu().numpy()


def argmin(solver, cost, group, base=0):
    bi, bc = solver.argmin(torch.from_numpy(cost).to(solver.device), group=group, index_base=base)
    torch.cuda.synchronize()
    return bi.cpu().numpy(), bc.cpu().numpy()


@pytest.mark.parametrize("size", SIZES)
def test_every_size_and_k_equals_the_yardstick_and_k1_the_argmin(solver, size):
    groups = groups_of(size)
    cost = make_costs(np.random.default_rng(1000 + size), groups, size)
    for K in KS:
        bi, bc = topk(solver, cost, size, K)
        wi, wc = yardstick_groups(cost, size, K)
        assert bi.shape == (groups, K) and same(bi, bc, wi, wc), (size, K)
    ai, ac = argmin(solver, cost, size)
    bi, bc = topk(solver, cost, size, 1)
    assert same(bi[:, 0], bc[:, 0], ai, ac), size
    if groups > 1:
        assert (bi[-1] == -1).all() and np.isinf(bc[-1]).all()          # the group nobody solved


def test_config5_shape(solver):
    cost = make_costs(np.random.default_rng(5), 128, 512)
    bi, bc = topk(solver, cost, 512, 8)
    assert same(bi, bc, *yardstick_groups(cost, 512, 8))
    ai, ac = argmin(solver, cost, 512)
    b1, c1 = topk(solver, cost, 512, 1)
    assert same(b1[:, 0], c1[:, 0], ai, ac)


def test_equal_costs_across_blocks_come_out_in_index_order(solver):
    cost = make_costs(np.random.default_rng(6), 1, 65536)
    at = [0, 1023, 1024, 40000, 65535]
    cost[at] = -3.0
    for K in (5, 8, 64):
        bi, bc = topk(solver, cost, 65536, K)
        assert bi[0, :5].tolist() == at and (bc[0, :5] == -3.0).all()
        assert same(bi, bc, *yardstick_groups(cost, 65536, K))


@pytest.mark.parametrize("size", [63, 512, 8193])
def test_index_base_is_exact_and_minus_one_stays(solver, size):
    base = 2**40 + 3
    groups = groups_of(size)
    cost = make_costs(np.random.default_rng(7 + size), groups, size)
    for K in (1, 5, 64):
        bi, bc = topk(solver, cost, size, K, base)
        assert same(bi, bc, *yardstick_groups(cost, size, K, base))
        assert (bi[-1] == -1).all() and (bi[0][bi[0] >= 0] >= base).all()
    ai, ac = argmin(solver, cost, size, base)
    b1, c1 = topk(solver, cost, size, 1, base)
    assert same(b1[:, 0], c1[:, 0], ai, ac)


def pairs_merge(solver, lists_i, lists_c, K):
    """lists [world][n][K] -> btrapz_topk_pairs_device's (idx, cost) [n][K]."""
    world, n = lists_i.shape[:2]
    pairs = np.stack([lists_c.view(np.int64), lists_i], axis=-1)
    d_pairs = torch.from_numpy(np.ascontiguousarray(pairs)).to(solver.device)
    out_c = torch.empty(n, K, dtype=torch.float64, device=solver.device); out_i = torch.empty(n, K, dtype=torch.int64, device=solver.device)
    solver.ctx.topk_pairs_device(world, n, K, d_pairs, out_c, out_i, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_c.cpu().numpy()


@pytest.mark.parametrize("B", [4096, 10])
def test_shards_merged_equal_the_whole_group(solver, B):
    """G contiguous dist.shard_bounds shards of one group (trailing shards short; empty at B = 10), top-K per shard with
    its index_base, merged by btrapz_topk_pairs_device == top-K of the whole group."""
    cost = make_costs(np.random.default_rng(8 + B), 1, B)
    for K in (1, 5, 64):
        whole_i, whole_c = topk(solver, cost, B, K)
        assert same(whole_i, whole_c, *yardstick_groups(cost, B, K))
        for G in range(1, 8):
            li, lc = np.full((G, 1, K), -1, np.int64), np.full((G, 1, K), np.inf)     # an empty shard: K x (-1, +inf)
            for r in range(G):
                lo, hi = dist.shard_bounds(B, G, r)
                if hi > lo:
                    li[r], lc[r] = topk(solver, cost[lo:hi], hi - lo, K, lo)
            if B == 10 and G == 7:
                assert dist.shard_bounds(B, G, 6) == (10, 10)
            mi, mc = pairs_merge(solver, li, lc, K)
            assert same(mi, mc, whole_i, whole_c), (B, K, G)


@pytest.mark.parametrize("world", [1, 2, 7])
def test_pairs_alone_against_numpy(solver, world):
    rng = np.random.default_rng(90 + world)
    n = 3
    for K in (1, 5, 64):
        li = np.stack([rng.permutation(10 * world * K)[:world * K].reshape(world, K) for _ in range(n)], axis=1).astype(np.int64)
        li += 2**41                                                    # (distinct global indices per group, in shuffled order)
        lc = rng.integers(0, 4, (world, n, K)).astype(np.float64)
        lc[rng.random(lc.shape) < 0.15] = np.nan
        lc[rng.random(lc.shape) < 0.15] = np.inf
        li[rng.random(li.shape) < 0.2] = -1
        li[:, n - 1] = -1                                              # a group nobody solved
        gi, gc = pairs_merge(solver, li, lc, K)
        for g in range(n):
            wi, wc = yardstick(lc[:, g].ravel(), li[:, g].ravel(), K)
            assert same(gi[g], gc[g], wi, wc), (world, K, g)
        assert (gi[n - 1] == -1).all()


def test_gather_rows(solver):
    rng = np.random.default_rng(10)
    B, P, base, n = 37, 13, 2**40 + 3, 9
    src = rng.normal(size=(B, P))
    idx = np.array([base + 36, base, -1, base + 5, base - 1, base + B, 4, base + 5, base + 17], dtype=np.int64)
    rows = torch.full((n + 2, P), 7.25, dtype=torch.float64, device=solver.device)          # two guard rows behind the n
    solver.ctx.gather_rows_device(n, torch.from_numpy(idx).to(solver.device), base, B, P, torch.from_numpy(src).to(solver.device),
                                  rows, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = rows.cpu().numpy()
    for j, i in enumerate(idx):
        if base <= i < base + B:
            assert np.array_equal(got[j], src[i - base]), j
        else:
            assert np.isnan(got[j]).all(), j
    assert (got[n:] == 7.25).all()


def test_end_to_end_the_four_best_of_a_solved_batch(solver):
    batch, sh = synth.make_batch(64, 10, config=2)
    db = solver.upload(batch)
    o = solver.solve(db, sh)
    bi, bc = solver.topk(o["cost"], 4)
    torch.cuda.synchronize()
    cost, status = o["cost"].cpu().numpy(), o["status"].cpu().numpy()
    wi, wc = yardstick_groups(cost, 64, 4)
    assert same(bi.cpu().numpy(), bc.cpu().numpy(), wi, wc)
    assert (wi >= 0).all() and (status[wi[0]] > 0).all()
    sel = bi.flatten()                                                  # index_base 0: the indices are the selection
    out, npts = solver.sample(db, o["ctrl"], sel, sh.delta)
    torch.cuda.synchronize()
    for j in range(4):
        one, n1 = solver.sample(db, o["ctrl"], sel[j:j + 1], sh.delta)
        torch.cuda.synchronize()
        assert int(n1[0]) == int(npts[j]) > 0 and torch.equal(one[0].view(torch.int64), out[j].view(torch.int64))


def test_refusals_name_the_argument(solver):
    d = solver.device
    cost = torch.zeros(8, dtype=torch.float64, device=d)
    bi = torch.empty(8, dtype=torch.int64, device=d); bc = torch.empty(8, dtype=torch.float64, device=d)
    pairs = torch.zeros(2 * 2 * 2 * 2, dtype=torch.int64, device=d)
    ctx = solver.ctx

    def refused(what, fn, *args):
        with pytest.raises(BtrapzError) as e:
            fn(*args)
        assert "(-1)" in str(e.value) and what in str(e.value).split("invalid argument:")[1].split("(")[0], (what, str(e.value))

    for K in (0, -1, native.MAX_TOPK + 1):
        refused("K", ctx.topk_device, 8, 8, K, 0, cost, bi, bc)
        refused("K", ctx.topk_pairs_device, 2, 2, K, pairs, bc, bi)
    refused("B", ctx.topk_device, 0, 8, 1, 0, cost, bi, bc)
    refused("group", ctx.topk_device, 8, 0, 1, 0, cost, bi, bc)
    refused("group", ctx.topk_device, 8, 3, 1, 0, cost, bi, bc)
    refused("cost", ctx.topk_device, 8, 8, 1, 0, None, bi, bc)
    refused("best_idx", ctx.topk_device, 8, 8, 1, 0, cost, None, bc)
    refused("best_cost", ctx.topk_device, 8, 8, 1, 0, cost, bi, None)
    refused("world", ctx.topk_pairs_device, 0, 2, 2, pairs, bc, bi)
    refused("n", ctx.topk_pairs_device, 2, 0, 2, pairs, bc, bi)
    refused("pairs", ctx.topk_pairs_device, 2, 2, 2, None, bc, bi)
    refused("best_cost", ctx.topk_pairs_device, 2, 2, 2, pairs, None, bi)
    refused("best_idx", ctx.topk_pairs_device, 2, 2, 2, pairs, bc, None)
    refused("n", ctx.gather_rows_device, 0, bi, 0, 8, 1, cost, bc)
    refused("B", ctx.gather_rows_device, 1, bi, 0, 0, 1, cost, bc)
    refused("row_doubles", ctx.gather_rows_device, 1, bi, 0, 8, 0, cost, bc)
    refused("idx", ctx.gather_rows_device, 1, None, 0, 8, 1, cost, bc)
    refused("src", ctx.gather_rows_device, 1, bi, 0, 8, 1, None, bc)
    refused("rows", ctx.gather_rows_device, 1, bi, 0, 8, 1, cost, None)
    assert native.lib().btrapz_topk_device(None, 8, 8, 1, 0, None, None, None, None) == -1       # no context
    # a refused call leaves the context usable
    b, c = solver.topk(cost, 2)
    torch.cuda.synchronize()
    assert b.cpu().tolist() == [[0, 1]] and c.cpu().tolist() == [[0.0, 0.0]]


def test_global_topk_on_device_through_the_collective(solver, tmp_path):
    """dist.global_topk on device tensors with a context: the gather runs (a gloo group of one rank, forced), the merge is
    btrapz_topk_pairs_device, the rows follow their indices -- and the torch fallback gives the same bits."""
    import torch.distributed as td
    rng = np.random.default_rng(12)
    n, K, P = 3, 5, 4
    li = (rng.permutation(100)[:n * K].reshape(n, K) + 2**41).astype(np.int64)
    lc = rng.integers(0, 3, (n, K)).astype(np.float64)
    lc[0, 1] = np.nan; lc[1, 2] = np.inf; li[1, 0] = -1; li[2] = -1
    rows = rng.normal(size=(n, K, P))
    d = lambda a: torch.from_numpy(a).to(solver.device)
    td.init_process_group("gloo", init_method="file://" + str(tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        c, i, r = dist.global_topk(d(lc), d(li), ctx=solver.ctx, force_collective=True, local_rows=d(rows))
        c2, i2 = dist.global_topk(d(lc), d(li), ctx=solver.ctx, force_collective=True)
        fc, fi, fr = dist.global_topk(d(lc), d(li), force_collective=True, local_rows=d(rows))      # no context: torch ops
        torch.cuda.synchronize()
    finally:
        td.destroy_process_group()
    c, i, r = c.cpu().numpy(), i.cpu().numpy(), r.cpu().numpy()
    for g in range(n):
        wi, wc = yardstick(lc[g], li[g], K)
        assert same(i[g], c[g], wi, wc), g
        for k in range(K):
            if wi[k] < 0:
                assert np.isnan(r[g, k]).all()
            else:
                assert np.array_equal(r[g, k], rows[g, list(li[g]).index(wi[k])])
    assert same(i2.cpu().numpy(), c2.cpu().numpy(), i, c) and same(fi.cpu().numpy(), fc.cpu().numpy(), i, c)
    assert np.array_equal(fr.cpu().numpy().view(np.int64), r.view(np.int64))
