"""Edge-list candidates on a row shard (dgg_amd.parallel.ShardedDGGConv with cand=) WITHOUT a GPU: gloo worlds of 2 and 3 on CPU
tensors.  The kernel namespace is the oracle stand-in of test_parallel_gloo, extended by the `rows=` forms of the edge-list entries
(evaluated on the whole graph and sliced).  The concatenated rows and the summed gradients -- the edge-MLP scorer's included, identical on
every rank -- must equal the one-rank run on the same inputs."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_parallel_gloo import CpuKern, make_inputs  # noqa: E402


class RowKern(CpuKern):
    """CpuKern with the row-range forms of the edge-list entries: (rowptr, col) is the shard's rebased CSR slice (include/dgg_hip.h,
    dgg_edgelist_topk_softk_rows); the stand-in puts it back into a whole-graph CSR whose other rows are empty, runs the oracle and
    keeps the shard's rows (the noise is keyed on global ids, and the slice's edge ids are its own)."""

    def __init__(self):
        self.row_calls = []

    @staticmethod
    def _whole(rowptr, rows, N):
        r0, r1 = rows
        rp = rowptr.numpy()
        return torch.from_numpy(np.concatenate([np.zeros(r0, np.int64), rp, np.full(N - r1, rp[-1], np.int64)]))

    def edgelist_topk(self, xp, rowptr, col, K, t, noise_mode, G, seed, rows=None):
        if rows is None:
            return super().edgelist_topk(xp, rowptr, col, K, t, noise_mode, G, seed)
        self.row_calls.append("edgelist_topk")
        idx, val = super().edgelist_topk(xp, self._whole(rowptr, rows, xp.shape[0]), col, K, t, noise_mode, G, seed)
        return idx[rows[0]:rows[1]].contiguous(), val[rows[0]:rows[1]].contiguous()

    def edgelist_topk_p(self, p_edge, N, rowptr, col, K, noise_mode, G, seed, rows=None):
        if rows is None:
            return super().edgelist_topk_p(p_edge, N, rowptr, col, K, noise_mode, G, seed)
        self.row_calls.append("edgelist_topk_p")
        out = super().edgelist_topk_p(p_edge, N, self._whole(rowptr, rows, N), col, K, noise_mode, G, seed)
        return tuple(a[rows[0]:rows[1]].contiguous() for a in out)

    def edge_mlp_bwd(self, AB, idx, eid, val, dval, deg, ex, wdu, wdv, wex, b1, w2, b2, act=1, perturb=False, need_dex=False, rows=None):
        if rows is None:
            return super().edge_mlp_bwd(AB, idx, eid, val, dval, deg, ex, wdu, wdv, wex, b1, w2, b2, act, perturb, need_dex)
        self.row_calls.append("edge_mlp_bwd")
        N, (r0, r1) = AB.shape[0], rows

        def pad(a, fill):
            out = torch.full((N,) + tuple(a.shape[1:]), fill, dtype=a.dtype)
            out[r0:r1] = a
            return out
        dAB, dpar, dex = super().edge_mlp_bwd(AB, pad(idx, -1), pad(eid, -1), pad(val, 0.0), pad(dval, 0.0), deg, ex, wdu, wdv, wex, b1, w2,
                                              b2, act, perturb, need_dex)
        return dAB, dpar, (dex[r0:r1].contiguous() if need_dex else None)


def candidates(N, world, seed=3, hi=12, wide=(7,)):
    """CSR candidate lists with self loops, 0..hi neighbours a row, rows in `wide` with 100 (wider than the list); the LAST rank's rows
    (of `world`) hold only their self loop"""
    sys.path.insert(0, ROOT)
    from dgg_amd.parallel import shard_bounds
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, hi + 1, N)
    for r in wide:
        deg[r] = min(100, N - 1)
    q0 = shard_bounds(N, world, world - 1)[0]
    deg[q0:] = 0
    rows, cols = [], []
    for i in range(N):
        c = np.unique(np.append(rng.choice(N, deg[i], replace=False), i)).astype(np.int32)
        rows.append(np.full(c.shape, i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    rowptr = np.zeros(N + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return torch.from_numpy(np.cumsum(rowptr)), torch.from_numpy(cols.astype(np.int32))


def scorer(name, N, h, rowptr, col):
    """the per-node / per-edge terms of an edge-MLP scorer (as DGG_LearnableK_debug._fused_scorer passes them), or None (u-v-dist)"""
    if name == "u-v-dist":
        return None
    erow = torch.repeat_interleave(torch.arange(N, dtype=torch.int32), rowptr[1:] - rowptr[:-1])
    gen = torch.Generator().manual_seed(21)
    hw = h // 2 if name == "edge_conv" else h
    rnd = lambda *sh: torch.randn(*sh, generator=gen) * 0.3  # noqa: E731
    sc = dict(Wcat=rnd(2 * hw, h), wdu=None, wdv=None, wex=None, b1=rnd(hw), w2=rnd(hw), b2=rnd(1), erow=erow, ex_in=None, ex_mode=0, t_ex=0.0,
              act=0 if name == "edge_conv" else 1)
    if name == "u-v-deg":
        sc.update(wdu=rnd(hw) * 0.1, wdv=rnd(hw) * 0.1)
    return sc


def run(N, world, name, noise_mode):
    """one step on this process's rows (of the gloo group, or all N rows without a process group) -> (r0, r1, Z, grads, row calls);
    `world` picks the graph (its last rank's rows hold only self loops)"""
    sys.path.insert(0, ROOT)
    from dgg_amd.parallel import ShardedDGGConv
    d, h = 12, 16
    x, deg, P, cot = make_inputs(N, d, h)
    rowptr, col = candidates(N, world)
    kern = RowKern()
    lay = ShardedDGGConv(kern, N, K=64, noise_mode=noise_mode, seed=(5, 6), x_full=x, hybrid=True, cand=(rowptr, col))
    lay.scorer = scorer(name, N, h, rowptr, col)
    r0, r1 = lay.r0, lay.r1
    Z = lay.forward(x[r0:r1].contiguous(), deg, P)
    assert lay.saved["idx"].shape[0] == r1 - r0
    g = lay.backward(cot[r0:r1].contiguous(), x[r0:r1].contiguous(), P)
    sg = g.pop("scorer", None)
    g = {k: v.numpy() for k, v in g.items()}
    if sg is not None:
        g.update({"scorer." + k: v.numpy() for k, v in sg.items() if v is not None})
    return r0, r1, Z.numpy(), g, list(kern.row_calls)


def _worker(rank, world, port, ret, N, name, noise_mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = run(N, world, name, noise_mode)
    finally:
        dist.destroy_process_group()


CASES = [("u-v-dist", 0), ("u-v-dist", 2), ("u-v-dist", 3), ("u-v-deg", 2), ("edge_conv", 3)]


@pytest.mark.parametrize("world,N", [(2, 90), (3, 91)])
@pytest.mark.parametrize("name,noise_mode", CASES)
def test_edge_list_shards_match_one_rank(world, N, name, noise_mode):
    r0, r1, Z1, g1, calls1 = run(N, world, name, noise_mode)          # one rank, no process group: the whole graph
    assert (r0, r1) == (0, N) and calls1 == [], "one rank: the edge-list calls are exactly the calls without rows="
    port = 29700 + (os.getpid() + 11 * world + 17 * CASES.index((name, noise_mode))) % 2000
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_worker, args=(r, world, port, ret, N, name, noise_mode)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        if p.is_alive():
            p.kill()
            pytest.fail("a rank did not finish")
    assert all(p.exitcode == 0 for p in procs) and len(ret) == world
    assert ret[0][0] == 0 and ret[world - 1][1] == N and all(ret[r][1] == ret[r + 1][0] for r in range(world - 1))
    for r in range(world):
        want = ["edgelist_topk"] if name == "u-v-dist" else ["edgelist_topk_p", "edge_mlp_bwd"]
        assert ret[r][4] == want, (r, ret[r][4])
    Z2 = np.concatenate([ret[r][2] for r in range(world)])
    np.testing.assert_allclose(Z2, Z1, rtol=1e-5, atol=1e-6)
    assert set(ret[0][3]) == set(g1)
    if name != "u-v-dist":
        assert any(k.startswith("scorer.") for k in g1)
    for k, ref in g1.items():
        got = ret[0][3][k]
        for r in range(1, world):
            np.testing.assert_array_equal(ret[r][3][k], got, err_msg=k)       # all-reduced: identical on every rank
        np.testing.assert_allclose(got.reshape(ref.shape), ref, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(ref).max()), err_msg=k)
