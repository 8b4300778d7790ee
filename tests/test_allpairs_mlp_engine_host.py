"""An edge-MLP scorer on ALL-PAIRS candidates inside the engine (dgg_amd.parallel.ShardedDGGConv with scorer set and cand = None) WITHOUT
a GPU: gloo worlds of 2 and 3 on CPU tensors.  The kernel namespace is the oracle stand-in of test_parallel_gloo with allpairs_mlp_topk
composed from its own edge_mlp_fwd + edgelist_topk_p on the complete candidate pattern of the rows asked for (what the HIP kernel is
specified as, bit for bit) and the rows= form of edge_mlp_bwd.  The concatenated rows and the summed gradients -- the scorer's included,
identical on every rank -- must equal the one-process step, as test_sharded_step_matches_single_process asserts it.  And the host logic of
the module under the opt-in args.dgg_allpairs_mlp_fused = True (and without it): which clauses of _fused_outside are left, that _fused_scorer reads no pattern, what ShardedGCN_DGG._check refuses."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_parallel_gloo import CpuKern, make_inputs  # noqa: E402


class AllPairsMlpKern(CpuKern):
    """CpuKern with the all-pairs form of the edge-MLP scorer: every column of the rows asked for is a candidate (include/dgg_hip.h,
    dgg_allpairs_mlp_topk: the bits of dgg_edge_mlp_fwd + dgg_edgelist_topk_p on the complete pattern; the noise is keyed on the global
    pair, so the rows sit at their own place in a whole-graph CSR whose other rows are empty)."""

    def __init__(self):
        self.calls = []

    def allpairs_mlp_topk(self, AB, xp, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, K, noise_mode, G, seed, rows=None):
        N = xp.shape[0]
        r0, r1 = (0, N) if rows is None else rows
        self.calls.append(("allpairs_mlp_topk", (r0, r1)))
        n = r1 - r0
        erow = torch.arange(r0, r1, dtype=torch.int32).repeat_interleave(N)
        col = torch.arange(N, dtype=torch.int32).repeat(n)
        p, ex = self.edge_mlp_fwd(AB, xp, erow, col, deg, None, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act)
        rowptr = torch.cat([torch.zeros(r0, dtype=torch.int64), torch.arange(n + 1, dtype=torch.int64) * N, torch.full((N - r1,), n * N, dtype=torch.int64)])
        idx, val, eid = self.edgelist_topk_p(p, N, rowptr, col, K, noise_mode, None, seed)
        idx, val, eid = idx[r0:r1].contiguous(), val[r0:r1].contiguous(), eid[r0:r1]
        ex_sel = None if ex is None else torch.where(eid >= 0, ex[eid.clamp(min=0).long()], torch.zeros(())).contiguous()
        return idx, val, ex_sel

    def edge_mlp_bwd(self, AB, idx, eid, val, dval, deg, ex, wdu, wdv, wex, b1, w2, b2, act=1, perturb=False, need_dex=False, rows=None):
        if rows is None:
            return super().edge_mlp_bwd(AB, idx, eid, val, dval, deg, ex, wdu, wdv, wex, b1, w2, b2, act, perturb, need_dex)
        self.calls.append(("edge_mlp_bwd", tuple(rows)))
        N, (r0, r1) = AB.shape[0], rows

        def pad(a, fill):
            out = torch.full((N,) + tuple(a.shape[1:]), fill, dtype=a.dtype)
            out[r0:r1] = a
            return out
        dAB, dpar, dex = super().edge_mlp_bwd(AB, pad(idx, -1), pad(eid, -1), pad(val, 0.0), pad(dval, 0.0), deg, ex, wdu, wdv, wex, b1, w2,
                                              b2, act, perturb, need_dex)
        return dAB, dpar, (dex[r0:r1].contiguous() if need_dex else None)


def scorer(h):
    """the per-node terms of u-v-deg as DGG_LearnableK_debug._fused_scorer passes them for AllPairs: no per-edge inputs"""
    gen = torch.Generator().manual_seed(21)
    rnd = lambda *sh: torch.randn(*sh, generator=gen) * 0.3  # noqa: E731
    return dict(Wcat=rnd(2 * h, h), wdu=rnd(h) * 0.1, wdv=rnd(h) * 0.1, wex=None, b1=rnd(h), w2=rnd(h), b2=rnd(1), erow=None, ex_in=None,
                ex_mode=0, t_ex=0.0, act=1)


def run(N, hybrid):
    """one step on this process's rows (of the gloo group, or all N rows without one) -> (r0, r1, Z, grads, kernel calls)"""
    sys.path.insert(0, ROOT)
    from dgg_amd.parallel import ShardedDGGConv
    d, h = 12, 16
    x, deg, P, cot = make_inputs(N, d, h)
    kern = AllPairsMlpKern()
    lay = ShardedDGGConv(kern, N, K=64, noise_mode=2, seed=(5, 6), x_full=x, hybrid=hybrid)
    lay.scorer = scorer(h)
    r0, r1 = lay.r0, lay.r1
    Z = lay.forward(x[r0:r1].contiguous(), deg, P)
    s = lay.saved
    assert s["idx"].shape == (r1 - r0, 64) and s["layout"] is None
    assert torch.equal(s["eid"], torch.arange((r1 - r0) * 64, dtype=torch.int32).view(r1 - r0, 64)), "eid is the slot index"
    g = lay.backward(cot[r0:r1].contiguous(), x[r0:r1].contiguous(), P)
    sg = g.pop("scorer")
    g = {k: v.numpy() for k, v in g.items()}
    g.update({"scorer." + k: v.numpy() for k, v in sg.items() if v is not None})
    return r0, r1, Z.numpy(), g, list(kern.calls)


def _worker(rank, world, port, ret, N, hybrid):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = run(N, hybrid)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("world,N", [(2, 150), (3, 151)])
def test_all_pairs_mlp_shards_match_one_process(world, N, hybrid):
    r0, r1, Z1, g1, calls1 = run(N, hybrid)                      # one process, no process group: the whole graph
    assert (r0, r1) == (0, N) and calls1 == [("allpairs_mlp_topk", (0, N))], "one rank: the MLP backward runs without rows="
    assert {"scorer.Wcat", "scorer.wdu", "scorer.wdv", "scorer.b1", "scorer.w2", "scorer.b2"} <= set(g1) and "scorer.wex" not in g1
    port = 30300 + (os.getpid() + 11 * world + 5 * hybrid) % 2000
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
    Z2 = np.concatenate([ret[r][2] for r in range(world)])
    np.testing.assert_allclose(Z2, Z1, rtol=1e-5, atol=1e-6)
    assert set(ret[0][3]) == set(g1)
    for k, ref in g1.items():
        got = ret[0][3][k]
        for r in range(1, world):
            np.testing.assert_allclose(ret[r][3][k], got, rtol=0, atol=0, err_msg=k)   # all-reduced: identical on every rank
        np.testing.assert_allclose(got.reshape(ref.shape), ref, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(ref).max()), err_msg=k)


def test_several_ranks_need_replicated_features():
    from dgg_amd.parallel import ShardedDGGConv
    x, deg, P, _ = make_inputs(40, 12, 16)
    lay = ShardedDGGConv(AllPairsMlpKern(), 40, K=64, noise_mode=2, seed=(5, 6), x_grad=True)
    lay.scorer = scorer(16)
    lay.world, lay.r0, lay.r1 = 2, 0, 20                         # (a rank of two without replicated features)
    with pytest.raises(AssertionError, match="replicated features"):
        lay.forward(x[:20].contiguous(), deg, P)


def test_a_namespace_without_the_kernel_is_an_error_not_a_fallback():
    from dgg_amd.parallel import ShardedDGGConv
    x, deg, P, _ = make_inputs(40, 12, 16)
    lay = ShardedDGGConv(CpuKern(), 40, K=64, noise_mode=2, seed=(5, 6), x_grad=True)
    lay.scorer = scorer(16)
    with pytest.raises(NotImplementedError, match="allpairs_mlp_topk"):
        lay.forward(x, deg, P)


# ---- the module's host logic ---------------------------------------------------------------------------------------------------
OPT_IN = dict(dgg_allpairs_mlp_fused=True)                     # the fused layer takes this configuration as an opt-in


def _dgg(scorer_name, latent=32, **kw):
    import dgg_amd
    from test_allpairs_mlp_host import module_args
    return dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=latent, args=module_args(scorer_name, **dict(OPT_IN, **kw)))


def _gpu_like(N, d):
    """what _fused_outside and ShardedGCN_DGG._check read of the features, saying it is on the GPU (no tensor is touched)"""
    return types.SimpleNamespace(shape=(N, d), is_cuda=True, dtype=torch.float32, requires_grad=False)


@pytest.mark.parametrize("scorer_name", ["u-v-deg", "u-v-deg-dist", "edge_conv"])
def test_fused_outside_lets_the_scorers_through_and_names_the_width_limits(scorer_name):
    import dgg_amd
    A = dgg_amd.AllPairs(torch.ones(4))
    assert _dgg(scorer_name)._fused_outside(_gpu_like(4, 8), A, torch.zeros(32, 16)) is None
    why = _dgg(scorer_name, latent=48)._fused_outside(_gpu_like(4, 8), A, torch.zeros(48, 16))
    assert "all-pairs candidates" in why and "width outside {16, 32, 64, 128}" in why
    why16 = _dgg(scorer_name, latent=16)._fused_outside(_gpu_like(4, 8), A, torch.zeros(16, 16))
    if scorer_name == "edge_conv":                               # (its hidden width is latent_dim / 2)
        assert "all-pairs candidates" in why16 and "edge_conv" in why16
    else:
        assert why16 is None
    # an edge list keeps every width the fused layer took before
    assert "all-pairs" not in str(_dgg(scorer_name, latent=48)._fused_outside(_gpu_like(4, 8), torch.eye(4).to_sparse(), torch.zeros(48, 16)))


@pytest.mark.parametrize("scorer_name", ["u-v-deg", "u-v-deg-dist", "edge_conv"])
def test_without_the_opt_in_the_forward_keeps_the_separate_modules(scorer_name):
    """args.dgg_allpairs_mlp_fused absent or False: the clause every earlier forward of this configuration was counted under, so
    GCN_DGG keeps the separate modules (their bits and autograd edges) and ShardedGCN_DGG keeps refusing, naming the clause"""
    import dgg_amd
    from dgg_amd.distributed import ShardedGCN_DGG
    from test_allpairs_mlp_host import module_args
    A = dgg_amd.AllPairs(torch.ones(4))
    for kw in ({}, {"dgg_allpairs_mlp_fused": False}):
        m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args(scorer_name, **kw))
        assert m._fused_outside(_gpu_like(4, 8), A, torch.zeros(32, 16)) == "edge-MLP scorer on all-pairs candidates"
    net = ShardedGCN_DGG(dgg_amd.GCN_DGG(nfeat=32, nhidden=32, nclass=16, args=module_args(scorer_name, dgg_wide_rows="auto")))
    with pytest.raises(NotImplementedError, match="edge-MLP scorer on all-pairs candidates"):
        net._check(_gpu_like(4, 32), A, None)


@pytest.mark.parametrize("scorer_name", ["u-v-A_uv", "A_uv"])
def test_fused_outside_keeps_the_scorers_that_read_adjacency_values_out(scorer_name):
    import dgg_amd
    why = _dgg(scorer_name)._fused_outside(_gpu_like(4, 8), dgg_amd.AllPairs(torch.ones(4)), torch.zeros(32, 16))
    assert why.startswith("edge-MLP scorer on all-pairs candidates") and "A_uv" in why


@pytest.mark.parametrize("scorer_name", ["u-v-deg", "u-v-deg-dist", "edge_conv"])
def test_fused_scorer_reads_no_pattern_of_all_pairs_candidates(scorer_name):
    import dgg_amd
    A = dgg_amd.AllPairs(torch.ones(4))                          # (has no coalesce() / indices(): reading a pattern would raise)
    mlp, static = _dgg(scorer_name)._fused_scorer(A)
    assert static["erow"] is None and static["ex_in"] is None
    assert static["ex_mode"] == {"u-v-deg": 0, "u-v-deg-dist": 2, "edge_conv": 0}[scorer_name]
    assert (static["packed"] is None) == (scorer_name == "edge_conv") and mlp["Wcat"] is not None


def test_sharded_wrapper_takes_the_configuration_and_still_refuses_a_uv():
    import dgg_amd
    from dgg_amd.distributed import ShardedGCN_DGG
    from test_allpairs_mlp_host import module_args
    N = 64
    A = dgg_amd.AllPairs(torch.full((N,), 8.0))
    for scorer_name in ("u-v-deg", "u-v-deg-dist", "edge_conv"):
        for kw in ({}, {"dgg_allpairs_mlp_rows": "chunked"}):
            m = dgg_amd.GCN_DGG(nfeat=32, nhidden=32, nclass=16, args=module_args(scorer_name, dgg_wide_rows="auto", **OPT_IN, **kw))
            ShardedGCN_DGG(m)._check(_gpu_like(N, 32), A, None)                 # (raised NotImplementedError before)
    m = dgg_amd.GCN_DGG(nfeat=32, nhidden=32, nclass=16, args=module_args("u-v-A_uv", dgg_wide_rows="auto", **OPT_IN))
    with pytest.raises(NotImplementedError, match="u-v-A_uv"):
        ShardedGCN_DGG(m)._check(_gpu_like(N, 32), A, None)
    m = dgg_amd.GCN_DGG(nfeat=48, nhidden=48, nclass=16, args=module_args("u-v-deg", dgg_wide_rows="auto", **OPT_IN))
    with pytest.raises(NotImplementedError, match="width outside"):
        ShardedGCN_DGG(m)._check(_gpu_like(N, 48), A, None)
