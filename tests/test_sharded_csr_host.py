"""Host side of ShardedGCN_DGG's CSR form (no GPU): CsrAdjacency as a row shard holds it, the slice helper, and what _check admits."""
import os
import sys
from argparse import Namespace
from datetime import timedelta

import pytest
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def small_graph():
    """6 nodes: row 2 is empty, row 4 has one entry"""
    ind = torch.tensor([[0, 0, 1, 3, 3, 3, 4, 5, 5], [1, 5, 0, 0, 2, 3, 4, 1, 2]])
    return torch.sparse_coo_tensor(ind, torch.arange(1.0, 10.0), (6, 6)).coalesce()


def test_csr_adjacency_as_a_row_shard_and_its_defaults():
    from dgg_amd.adjacency import CsrAdjacency, csr_pattern, csr_pattern_rows
    A = small_graph()
    rowptr, col, erow = csr_pattern(A)
    whole = CsrAdjacency(rowptr, col, erow, A.values(), 6)
    assert whole.shape == (6, 6) and whole.row0 == 0
    assert torch.equal(whole.to_dense(), A.to_dense()) and torch.equal(whole.to_sparse().to_dense(), A.to_dense())
    assert torch.equal(whole.indices(), A.indices())
    for r0, r1 in ((0, 6), (0, 3), (3, 6), (2, 3), (4, 5), (3, 3), (6, 6)):
        (rp, cl, er), (e0, e1) = csr_pattern_rows(A, (r0, r1))
        assert rp.dtype == torch.int64 and cl.dtype == torch.int32 and er.dtype == torch.int32
        assert rp.shape[0] == r1 - r0 + 1 and int(rp[0]) == 0 and int(rp[-1]) == e1 - e0 == cl.shape[0] == er.shape[0]
        assert torch.equal(rp, rowptr[r0:r1 + 1] - rowptr[r0]) and torch.equal(cl, col[e0:e1])
        assert torch.equal(er, erow[e0:e1]) and (er.numel() == 0 or (int(er.min()) >= r0 and int(er.max()) < r1))       # (global rows)
        part = CsrAdjacency(rp, cl, er, A.values()[e0:e1], 6, row0=r0, n_rows=r1 - r0)
        assert part.shape == (r1 - r0, 6)
        assert torch.equal(part.to_dense(), A.to_dense()[r0:r1]) and torch.equal(part.to_sparse().to_dense(), A.to_dense()[r0:r1])
        if (r0, r1) != (0, 6):
            with pytest.raises(NotImplementedError):
                part.normalize()
    assert csr_pattern_rows(A, (0, 3))[0][0] is csr_pattern_rows(A, (0, 3))[0][0]          # (cached with the graph)


def model(scorer="u-v-dist", policy="csr"):
    import dgg_amd
    args = Namespace(extra_edge_dim=2 if scorer == "u-v-deg" else 0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288,
                     dgg_mode_edge_net=scorer, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=True,
                     symmetric_noise=False, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1, dgg_wide_rows=policy)
    return dgg_amd.GCN_DGG(nfeat=16, nhidden=16, nclass=4, args=args)


def test_check_admits_the_csr_policies_for_edge_lists_on_two_gloo_ranks():
    from dgg_amd.adjacency import AllPairs
    from dgg_amd.distributed import ShardedGCN_DGG
    port = 29500 + os.getpid() % 400
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, timeout=timedelta(seconds=60))
    try:
        x, A = torch.randn(6, 16), small_graph()
        for scorer in ("u-v-dist", "u-v-deg"):
            for policy in ("csr", "csr_auto"):
                net = ShardedGCN_DGG(model(scorer, policy))
                net.world = 2                                 # (two ranks as far as _check is concerned; it enters no collective)
                assert net._edge_lists(A)
                with pytest.raises(NotImplementedError, match="edge-list candidates.*input not on the GPU"):
                    net._check(x, A, None)
                with pytest.raises(NotImplementedError, match="dgg_wide_rows"):          # all-pairs candidates keep refusing them
                    net._check(x, AllPairs(torch.ones(6)), None)
        net = ShardedGCN_DGG(model("u-v-dist", "ell"))
        net.world = 2
        with pytest.raises(NotImplementedError, match="dgg_wide_rows = 'ell'"):
            net._check(x, A, None)
    finally:
        dist.destroy_process_group()


def test_coras_fixture_is_inside_the_csr_forms_coverage():
    from helpers import load_fixture
    a = load_fixture("cora_gcn_dgg")["meta"]["args"]
    assert a["dgg_mode_k_net"] == "x" and a["dgg_mode_k_select"] in ("k_times_edge_prob", "k_only") and not a["dgg_hard"]
    assert a["dgg_mode_edge_net"] in ("u-v-dist", "u-v-deg", "u-v-A_uv", "u-v-deg-dist", "edge_conv", "A_uv") and a["debug_step"] not in (0, 1)
