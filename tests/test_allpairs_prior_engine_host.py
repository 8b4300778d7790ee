"""u-v-A_uv on ALL-PAIRS candidates that carry a prior graph inside the engine (dgg_amd.parallel.ShardedDGGConv with scorer["prior"] set and
cand = None) WITHOUT a GPU: gloo worlds of 2 and 3 on CPU tensors, and the module's host logic under the opt-in
args.dgg_allpairs_prior_fused = True.

The kernel namespace is AllPairsMlpKern (tests/test_allpairs_mlp_engine_host.py) whose allpairs_mlp_topk takes prior= and feeds
edge_mlp_fwd the DENSE prior value of every (row, column) pair of the rows asked for as ex_in, with ex_mode 1 -- the definition of
DESIGN.md ("what the edge-list path returns on the complete candidate pattern with ex_in = the prior's dense values, 0 where nothing is
stored").  The concatenated rows and the all-reduced gradients -- scorer.wex among them, identical on every rank -- must equal the
one-process step, under the bars of test_all_pairs_mlp_shards_match_one_process."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_allpairs_mlp_engine_host import AllPairsMlpKern, _gpu_like  # noqa: E402
from test_allpairs_mlp_host import module_args  # noqa: E402
from test_parallel_gloo import make_inputs  # noqa: E402

WORLDS = [(2, 150), (3, 151)]
OPT_IN = dict(dgg_allpairs_prior_fused=True)                   # enough alone: no dgg_allpairs_mlp_fused beside it


def dense_of(prior, N):
    rowptr, col, val = prior
    out = torch.zeros(N, N)
    out[torch.arange(N).repeat_interleave(rowptr.diff()), col.long()] = val
    return out


class PriorKern(AllPairsMlpKern):
    """AllPairsMlpKern whose allpairs_mlp_topk looks the extra of a pair up in a prior graph: ex_in = the dense prior value of every
    (row, column) pair, ex_mode 1 (include/dgg_hip.h, dgg_allpairs_mlp_topk_prior); the arrays are the whole graph's under rows="""

    def allpairs_mlp_topk(self, AB, xp, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, K, noise_mode, G, seed, rows=None, prior=None):
        assert prior is not None and ex_mode == 1 and wex is not None, "the engine must hand the scorer's prior on"
        N = xp.shape[0]
        assert prior[0].shape[0] == N + 1, "the WHOLE graph's prior on every rank"
        r0, r1 = (0, N) if rows is None else rows
        self.calls.append(("allpairs_mlp_topk", (r0, r1)))
        n = r1 - r0
        erow = torch.arange(r0, r1, dtype=torch.int32).repeat_interleave(N)
        col = torch.arange(N, dtype=torch.int32).repeat(n)
        ex_in = dense_of(prior, N)[r0:r1].reshape(-1).contiguous()
        p, ex = self.edge_mlp_fwd(AB, xp, erow, col, deg, ex_in, 1, t_ex, wdu, wdv, wex, b1, w2, b2, act)
        rowptr = torch.cat([torch.zeros(r0, dtype=torch.int64), torch.arange(n + 1, dtype=torch.int64) * N, torch.full((N - r1,), n * N, dtype=torch.int64)])
        idx, val, eid = self.edgelist_topk_p(p, N, rowptr, col, K, noise_mode, None, seed)
        idx, val, eid = idx[r0:r1].contiguous(), val[r0:r1].contiguous(), eid[r0:r1]
        return idx, val, torch.where(eid >= 0, ex[eid.clamp(min=0).long()], torch.zeros(())).contiguous()


def boundaries(N):
    from dgg_amd.parallel import shard_bounds
    return sorted({shard_bounds(N, w, r)[0] for w, _ in WORLDS for r in range(1, w)})


def make_prior(N):
    """-> (rowptr int64 [N+1], col int32, val float32) of a prior with: row 2 empty; row 5 storing 80 columns; row 7 storing exactly the
    columns 63, 64, N - 1 and a 0.0 at column 9; for every shard boundary b of the two worlds, rows b - 1 and b storing the columns b - 1
    and b (entries that cross the boundary in both directions); about 4 random entries in every other row, values of order 1, both signs"""
    rng = np.random.default_rng(11 + N)
    stored = rng.random((N, N)) < 4.0 / N
    v = rng.standard_normal((N, N))
    P = np.sign(v) * (0.5 + np.abs(v))
    stored[2] = False
    stored[5] = False
    stored[5, rng.choice(N, 80, replace=False)] = True
    stored[7] = False
    stored[7, [63, 64, N - 1, 9]] = True
    P[7, 9] = 0.0
    for b in boundaries(N):
        stored[b - 1:b + 1, b - 1:b + 1] = True
    rows, cols = np.nonzero(stored)
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=N))
    return torch.from_numpy(rowptr), torch.from_numpy(cols.astype(np.int32)), torch.from_numpy(P[rows, cols].astype(np.float32))


@pytest.mark.parametrize("N", [n for _, n in WORLDS])
def test_the_prior_holds_what_the_cases_need(N):
    rowptr, col, val = make_prior(N)
    row = lambda i: col[rowptr[i]:rowptr[i + 1]].tolist()  # noqa: E731
    assert row(2) == [] and len(row(5)) == 80 and row(7) == [9, 63, 64, N - 1]
    assert float(val[rowptr[7]]) == 0.0, "a stored 0.0"
    bs = boundaries(N)
    assert bs == ([50, 75, 100] if N == 150 else [51, 76, 102])
    for b in bs:
        assert {b - 1, b} <= set(row(b - 1)) and {b - 1, b} <= set(row(b)), "entries on both sides of the boundary, crossing it both ways"
    assert all((col[rowptr[i]:rowptr[i + 1]].diff() > 0).all() for i in range(N)), "columns strictly ascending within a row"


def scorer(h, N):
    """the terms of u-v-A_uv as DGG_LearnableK_debug._fused_scorer passes them for AllPairs with a prior: no degree terms, no per-edge
    inputs, the prior's CSR arrays.  wex = 0.5 sign(w2): a positive prior value raises the score of its pair, a negative one lowers it"""
    gen = torch.Generator().manual_seed(21)
    rnd = lambda *sh: torch.randn(*sh, generator=gen) * 0.3  # noqa: E731
    Wcat, b1, w2, b2 = rnd(2 * h, h), rnd(h), rnd(h), rnd(1)
    return dict(Wcat=Wcat, wdu=None, wdv=None, wex=0.5 * torch.where(w2 >= 0, 1.0, -1.0), b1=b1, w2=w2, b2=b2, erow=None, ex_in=None,
                ex_mode=1, t_ex=0.0, act=1, prior=make_prior(N))


def run(N, hybrid):
    """one step on this process's rows (of the gloo group, or all N rows without one) -> (r0, r1, Z, grads, kernel calls, kept extras)"""
    sys.path.insert(0, ROOT)
    from dgg_amd.parallel import ShardedDGGConv
    d, h = 12, 16
    x, deg, P, cot = make_inputs(N, d, h)
    kern = PriorKern()
    lay = ShardedDGGConv(kern, N, K=64, noise_mode=2, seed=(5, 6), x_full=x, hybrid=hybrid)
    lay.scorer = scorer(h, N)
    r0, r1 = lay.r0, lay.r1
    Z = lay.forward(x[r0:r1].contiguous(), deg, P)
    s = lay.saved
    assert s["idx"].shape == (r1 - r0, 64) and s["layout"] is None and s["sdeg"] is None
    assert s["ex"].shape == ((r1 - r0) * 64,), "the extras of the kept slots, flat"
    dense = dense_of(lay.scorer["prior"], N)
    want = dense[torch.arange(r0, r1)[:, None].expand_as(s["idx"]), s["idx"].clamp(min=0).long()]
    assert torch.equal(s["ex"].view(r1 - r0, 64), torch.where(s["idx"] >= 0, want, torch.zeros(()))), "ex is the prior's value of each kept pair"
    g = lay.backward(cot[r0:r1].contiguous(), x[r0:r1].contiguous(), P)
    sg = g.pop("scorer")
    g = {k: v.numpy() for k, v in g.items()}
    g.update({"scorer." + k: v.numpy() for k, v in sg.items() if v is not None})
    return r0, r1, Z.numpy(), g, list(kern.calls), s["ex"].numpy()


def _worker(rank, world, port, ret, N, hybrid):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = run(N, hybrid)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("world,N", WORLDS)
def test_prior_shards_match_one_process(world, N, hybrid):
    """(fails before this feature: the engine does not hand the scorer's prior to the kernel namespace)"""
    r0, r1, Z1, g1, calls1, ex1 = run(N, hybrid)                 # one process, no process group: the whole graph
    assert (r0, r1) == (0, N) and calls1 == [("allpairs_mlp_topk", (0, N))], "one rank: the MLP backward runs without rows="
    assert {"scorer.Wcat", "scorer.wex", "scorer.b1", "scorer.w2", "scorer.b2"} <= set(g1) and not {"scorer.wdu", "scorer.wdv"} & set(g1)
    assert np.abs(g1["scorer.wex"]).max() > 0, "the weights of the prior column get a gradient"
    assert (ex1 != 0).mean() > 0.01 and (ex1 == 0).mean() > 0.01, "kept entries: prior edges and non-edges"
    port = 32300 + (os.getpid() + 11 * world + 5 * hybrid) % 2000
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_worker, args=(r, world, port, ret, N, hybrid)) for r in range(world)]
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
        rows = (ret[r][0], ret[r][1])
        assert ret[r][4] == [("allpairs_mlp_topk", rows), ("edge_mlp_bwd", rows)], (r, ret[r][4])
    assert np.array_equal(np.concatenate([ret[r][5] for r in range(world)]), ex1), "the shards' kept extras are the one process's"
    Z2 = np.concatenate([ret[r][2] for r in range(world)])
    np.testing.assert_allclose(Z2, Z1, rtol=1e-5, atol=1e-6)
    assert set(ret[0][3]) == set(g1)
    for k, ref in g1.items():
        got = ret[0][3][k]
        for r in range(1, world):
            np.testing.assert_allclose(ret[r][3][k], got, rtol=0, atol=0, err_msg=k)   # all-reduced: identical on every rank
        np.testing.assert_allclose(got.reshape(ref.shape), ref, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(ref).max()), err_msg=k)
    assert np.abs(ret[0][3]["scorer.wex"]).max() > 0


def test_a_scorer_without_a_prior_calls_the_namespace_as_before():
    """the contract's entries (and the stand-in of tests/test_allpairs_mlp_engine_host.py) take no prior=: it is handed on only when the
    scorer carries one"""
    from dgg_amd.parallel import ShardedDGGConv
    from test_allpairs_mlp_engine_host import scorer as plain_scorer
    x, deg, P, _ = make_inputs(40, 12, 16)
    lay = ShardedDGGConv(AllPairsMlpKern(), 40, K=64, noise_mode=2, seed=(5, 6), x_full=x)
    lay.scorer = plain_scorer(16)
    lay.forward(x, deg, P)


# ---- the module's host logic ---------------------------------------------------------------------------------------------------
def graph(n=6):
    ind = torch.tensor([[0, 0, 1, 3, 3, 5], [1, 4, 0, 2, 5, 5]])
    return torch.sparse_coo_tensor(ind, torch.tensor([1.0, 2.0, -0.5, 0.25, 1.5, 3.0]), (n, n))


def _dgg(scorer_name, latent=32, **kw):
    import dgg_amd
    return dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=latent, args=module_args(scorer_name, **kw))


def test_fused_outside_lets_u_v_a_uv_with_a_prior_through_under_its_opt_in():
    """(fails before this feature: the clause that reads "(u-v-A_uv / A_uv)" stood whatever the arguments)"""
    import dgg_amd
    A = dgg_amd.AllPairs.from_graph(graph())
    for kw in (OPT_IN, dict(OPT_IN, dgg_allpairs_mlp_fused=True), dict(OPT_IN, dgg_allpairs_mlp_rows="chunked")):
        assert _dgg("u-v-A_uv", **kw)._fused_outside(_gpu_like(6, 8), A, torch.zeros(32, 16)) is None
    assert _dgg("u-v-A_uv", latent=16, **OPT_IN)._fused_outside(_gpu_like(6, 8), A, torch.zeros(16, 16)) is None


def test_without_the_new_argument_every_clause_is_what_it_was():
    import dgg_amd
    A = dgg_amd.AllPairs.from_graph(graph())
    x, W = _gpu_like(6, 8), torch.zeros(32, 16)
    for kw in ({}, {"dgg_allpairs_prior_fused": False}):
        assert _dgg("u-v-A_uv", **kw)._fused_outside(x, A, W) == "edge-MLP scorer on all-pairs candidates"
        assert _dgg("u-v-A_uv", dgg_allpairs_mlp_fused=True, **kw)._fused_outside(x, A, W) == \
            "edge-MLP scorer on all-pairs candidates that reads the stored values of in_adj (u-v-A_uv / A_uv)"
    # the new argument is u-v-A_uv's: the other scorers keep their own opt-in
    assert _dgg("u-v-deg", **OPT_IN)._fused_outside(x, A, W) == "edge-MLP scorer on all-pairs candidates"
    assert _dgg("u-v-deg", dgg_allpairs_mlp_fused=True, **OPT_IN)._fused_outside(x, A, W) is None


def test_the_clause_still_stands_without_a_prior_for_a_uv_and_for_latent_48():
    import dgg_amd
    x, W = _gpu_like(6, 8), torch.zeros(32, 16)
    plain, A = dgg_amd.AllPairs(torch.ones(6)), dgg_amd.AllPairs.from_graph(graph())
    reads = "edge-MLP scorer on all-pairs candidates that reads the stored values of in_adj (u-v-A_uv / A_uv)"
    for kw in (OPT_IN, dict(OPT_IN, dgg_allpairs_mlp_fused=True)):
        assert _dgg("u-v-A_uv", **kw)._fused_outside(x, plain, W) == reads
    assert _dgg("A_uv", **OPT_IN)._fused_outside(x, A, W) == "edge-MLP scorer on all-pairs candidates"
    assert _dgg("A_uv", dgg_allpairs_mlp_fused=True, **OPT_IN)._fused_outside(x, A, W) == reads
    why = _dgg("u-v-A_uv", latent=48, **OPT_IN)._fused_outside(x, A, torch.zeros(48, 16))
    assert "all-pairs candidates" in why and "width outside {16, 32, 64, 128}" in why


def test_fused_scorer_hands_the_prior_on_and_reads_no_pattern():
    import dgg_amd
    A = dgg_amd.AllPairs.from_graph(graph())                     # (has no coalesce() / indices(): reading a pattern would raise)
    mlp, static = _dgg("u-v-A_uv", **OPT_IN)._fused_scorer(A)
    assert static["erow"] is None and static["ex_in"] is None and static["ex_mode"] == 1
    assert len(static["prior"]) == 3 and all(a is b for a, b in zip(static["prior"], A.prior_csr()[:3]))
    assert static["packed"] == (32, (None, None, 64)) and mlp["Wcat"].shape == (32, 65), "edge_encode.0.weight whole: column 2h is the prior's"
    assert not any(t_.requires_grad for t_ in static["prior"]), "the prior's values are data"
    # the scorers that do not read the prior carry none, with or without one on the candidates
    _, static = _dgg("u-v-deg", dgg_allpairs_mlp_fused=True)._fused_scorer(A)
    assert "prior" not in static


def test_pack_scorer_puts_the_prior_column_into_wex():
    from dgg_amd.dgm import _pack_scorer
    import dgg_amd
    A = dgg_amd.AllPairs.from_graph(graph())
    m = _dgg("u-v-A_uv", **OPT_IN)
    mlp, static = m._fused_scorer(A)
    packed, sc = _pack_scorer(static, mlp["Wcat"], mlp["wdu"], mlp["wdv"], mlp["wex"], mlp["b1"], mlp["w2"], mlp["b2"])
    assert packed == static["packed"] and sc["wdu"] is None and sc["wdv"] is None
    assert torch.equal(sc["wex"], m.edge_encode[0].weight.detach()[:, 64]) and sc["prior"] is static["prior"] and sc["ex_mode"] == 1


def test_sharded_wrapper_takes_the_configuration_and_still_refuses_a_uv():
    """(fails before this feature: _check raised NotImplementedError naming u-v-A_uv)"""
    import dgg_amd
    from dgg_amd.distributed import ShardedGCN_DGG
    N = 64
    A = dgg_amd.AllPairs.from_graph(torch.eye(N).to_sparse())
    for kw in ({}, {"dgg_allpairs_mlp_rows": "chunked"}):
        m = dgg_amd.GCN_DGG(nfeat=32, nhidden=32, nclass=16, args=module_args("u-v-A_uv", dgg_wide_rows="auto", **OPT_IN, **kw))
        ShardedGCN_DGG(m)._check(_gpu_like(N, 32), A, None)
    m = dgg_amd.GCN_DGG(nfeat=32, nhidden=32, nclass=16, args=module_args("A_uv", dgg_wide_rows="auto", **OPT_IN))
    with pytest.raises(NotImplementedError, match="edge-MLP scorer on all-pairs candidates"):
        ShardedGCN_DGG(m)._check(_gpu_like(N, 32), A, None)
    m = dgg_amd.GCN_DGG(nfeat=32, nhidden=32, nclass=16, args=module_args("u-v-A_uv", dgg_wide_rows="auto", **OPT_IN))
    with pytest.raises(NotImplementedError, match="u-v-A_uv"):           # (no prior on the candidates)
        ShardedGCN_DGG(m)._check(_gpu_like(N, 32), dgg_amd.AllPairs(torch.ones(N)), None)
    m = dgg_amd.GCN_DGG(nfeat=32, nhidden=32, nclass=16, args=module_args("u-v-A_uv", dgg_wide_rows="auto"))
    with pytest.raises(NotImplementedError, match="edge-MLP scorer on all-pairs candidates"):
        ShardedGCN_DGG(m)._check(_gpu_like(N, 32), A, None)
