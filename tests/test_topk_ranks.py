"""dist.global_topk on CPU: world-2 gloo with the harness of tests/test_multi_rank.py, the torch fallback of the merge.

The yardstick is numpy on the union of the ranks' candidates: those with cost < inf (NaN is false), order =
np.lexsort((idx, cost)), the first K, padded with (-1, +inf).  Comparisons are exact: int64 indices, cost bits, row bits."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from spectral_amd.dist import global_argmin, global_topk, shard_bounds
from test_multi_rank import _free_port

GROUPS, PER, P = 4, 300, 6          # 4 groups, 300 candidates of each on every rank; rows of 6 doubles
BASE = (1 << 60) + 12345            # indices beyond 2^53: exact only as integers


def make_costs():
    """[world 2][GROUPS][PER] small integers (ties everywhere), +inf and NaN entries, a tie for the minimum across the
    ranks in group 0, rank 0 all failed in group 1, group 3 failed on both ranks."""
    rng = np.random.default_rng(21)
    c = rng.integers(0, 7, (2, GROUPS, PER)).astype(np.float64)
    c[rng.random(c.shape) < 0.1] = np.inf
    c[rng.random(c.shape) < 0.01] = np.nan
    c[0, 0, 17] = c[1, 0, 4] = -5.0
    c[0, 1] = np.inf
    c[:, 3] = np.inf
    return c


def global_index(rank, g, j):
    return BASE + (rank * GROUPS + g) * PER + j


def rows_of(idx):
    """The row that belongs to a global index: recomputable anywhere."""
    return np.sin(np.asarray(idx, dtype=np.float64)[..., None] % 1000.0 + np.arange(P))


def yardstick(cost, idx, K):
    m = (cost < np.inf) & (idx >= 0)
    c, i = cost[m], idx[m]
    order = np.lexsort((i, c))[:K]
    bi, bc = np.full(K, -1, np.int64), np.full(K, np.inf)
    bi[:order.size] = i[order]; bc[:order.size] = c[order]
    return bi, bc


def local_lists(costs, rank, K):
    idx = np.stack([global_index(rank, g, np.arange(PER, dtype=np.int64)) for g in range(GROUPS)])
    out = [yardstick(costs[rank, g], idx[g], K) for g in range(GROUPS)]
    return np.stack([o[1] for o in out]), np.stack([o[0] for o in out])


def _worker(rank, world, port, costs, K, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    bc, bi = local_lists(costs, rank, K)
    rows = rows_of(bi); rows[bi < 0] = 1.5                                        # any finite filler
    tc, ti = torch.from_numpy(bc), torch.from_numpy(bi)
    c, i = global_topk(tc, ti)
    c2, i2, r2 = global_topk(tc, ti, local_rows=torch.from_numpy(rows))
    ac, ai = global_argmin(tc[:, 0].contiguous(), ti[:, 0].contiguous())
    q.put((rank, c.numpy().copy(), i.numpy().copy(), c2.numpy().copy(), i2.numpy().copy(), r2.numpy().copy(), ac.numpy().copy(),
           ai.numpy().copy()))
    dist.barrier(); dist.destroy_process_group()


@pytest.mark.parametrize("K", [1, 5])
def test_global_topk_equals_the_yardstick_on_the_union(K):
    costs = make_costs()
    ctx = mp.get_context("spawn"); q = ctx.Queue(); port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, costs, K, q)) for r in range(2)]
    [p.start() for p in procs]
    res = [q.get(timeout=120) for _ in range(2)]
    [p.join(timeout=60) for p in procs]
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    for rank, c, i, c2, i2, r2, ac, ai in res:
        for g in range(GROUPS):
            idx = np.concatenate([global_index(r, g, np.arange(PER, dtype=np.int64)) for r in range(2)])
            wi, wc = yardstick(costs[:, g].ravel(), idx, K)
            assert np.array_equal(i[g], wi) and np.array_equal(bits(c[g]), bits(wc)), (rank, g)
        assert np.array_equal(i2, i) and np.array_equal(bits(c2), bits(c))        # with local_rows: the same lists ...
        want_rows = rows_of(i)
        assert np.array_equal(bits(r2[i >= 0]), bits(want_rows[i >= 0])) and np.isnan(r2[i < 0]).all()   # ... and the owners' rows
        assert (i[3] == -1).all() and np.isinf(c[3]).all()                        # the all-failed group
        assert i[0, 0] == global_index(0, 0, 17) and c[0, 0] == -5.0              # the tie across the ranks -> lowest index
        if K > 1:
            assert i[0, 1] == global_index(1, 0, 4) and c[0, 1] == -5.0
        assert (i[1][i[1] >= 0] >= global_index(1, 0, 0)).all()                   # group 1: rank 0 failed
        if K == 1:
            assert np.array_equal(i[:, 0], ai) and np.array_equal(bits(c[:, 0]), bits(ac))   # == global_argmin
    for r in res[1:]:                                                             # every rank agrees
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(res[0][1:], r[1:]))


def test_the_single_process_shortcut_returns_its_input():
    c = torch.tensor([[1.0, 2.0, float("inf")], [float("inf")] * 3], dtype=torch.float64)
    i = torch.tensor([[7, 3, -1], [-1, -1, -1]])
    oc, oi = global_topk(c, i)
    assert oc is c and oi is i
    rows = torch.arange(2 * 3 * 4, dtype=torch.float64).view(2, 3, 4)
    oc, oi, r = global_topk(c, i, local_rows=rows)
    assert oc is c and oi is i
    assert torch.equal(r[0, :2], rows[0, :2]) and torch.isnan(r[0, 2]).all() and torch.isnan(r[1]).all()
    assert torch.equal(rows, torch.arange(2 * 3 * 4, dtype=torch.float64).view(2, 3, 4))   # the input is left alone


def test_k1_of_a_single_process_is_global_argmin():
    c = torch.tensor([[2.5], [float("inf")]], dtype=torch.float64); i = torch.tensor([[7], [-1]])
    oc, oi = global_topk(c, i)
    ac, ai = global_argmin(c[:, 0], i[:, 0])
    assert torch.equal(oc[:, 0], ac) and torch.equal(oi[:, 0], ai)
    assert shard_bounds(10, 7, 6) == (10, 10)                                     # (the empty trailing shard the GPU test merges)
