"""Host-side checks of all-pairs candidates that carry a sparse prior graph (no GPU): the AllPairs constructor and from_graph, the C ABI
of the two new entries, and the configurations that keep refusing -- with the present wording where there was one."""
import ctypes
import os
import re

import pytest
import torch

from helpers import ROOT
from test_allpairs_mlp_host import SCORERS, module_args
from test_allpairs_mlp_engine_host import _gpu_like

PRIOR_ARGS = ["prior_rowptr", "prior_col", "prior_val"]


def graph(n=6):
    ind = torch.tensor([[0, 0, 1, 3, 3, 5], [1, 4, 0, 2, 5, 5]])
    return torch.sparse_coo_tensor(ind, torch.tensor([1.0, 2.0, -0.5, 0.25, 1.5, 3.0]), (n, n))


# ---------------------------------------------------------------------------------------------------------------
# the constructor
# ---------------------------------------------------------------------------------------------------------------
def test_plain_all_pairs_is_what_it_was():
    import dgg_amd
    deg = torch.ones(4)
    A = dgg_amd.AllPairs(deg)
    assert A.prior_degree is deg and A.shape == (4, 4) and A.device == deg.device and A.prior is None and A.prior_csr() is None


def test_prior_is_coalesced_and_kept_in_csr_form_on_the_object():
    import dgg_amd
    ind = torch.tensor([[3, 0, 0, 3, 0, 5], [5, 4, 1, 2, 4, 5]])                  # unsorted, (0, 4) twice
    P = torch.sparse_coo_tensor(ind, torch.tensor([1.5, 2.0, 1.0, 0.25, 0.5, 0.0]), (6, 6))
    A = dgg_amd.AllPairs(torch.ones(6), prior=P)
    rowptr, col, val, erow = A.prior_csr()
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32 and erow.dtype == torch.int32
    assert rowptr.tolist() == [0, 2, 2, 2, 4, 4, 5] and col.tolist() == [1, 4, 2, 5, 5] and erow.tolist() == [0, 0, 3, 3, 5]
    assert val.tolist() == [1.0, 2.5, 0.25, 1.5, 0.0], "duplicates are summed; an explicit zero stays stored"
    assert all(a is b for a, b in zip(A.prior_csr(), A.prior_csr())), "the CSR form is cached on the object"
    for i in range(6):
        assert (col[rowptr[i]:rowptr[i + 1]].diff() > 0).all(), "columns strictly ascending within a row"


def test_dense_prior_is_converted():
    import dgg_amd
    D = graph().to_dense()
    A, B = dgg_amd.AllPairs(torch.ones(6), prior=D), dgg_amd.AllPairs(torch.ones(6), prior=graph())
    assert A.prior.is_sparse
    for a, b in zip(A.prior_csr(), B.prior_csr()):
        assert torch.equal(a, b)


def test_empty_prior_keeps_arrays_with_a_data_pointer():
    import dgg_amd
    A = dgg_amd.AllPairs(torch.ones(5), prior=torch.zeros(5, 5))
    rowptr, col, val, erow = A.prior_csr()
    assert rowptr.tolist() == [0] * 6 and col.numel() == 1 and val.numel() == 1 and erow.numel() == 0


def test_shape_and_device_mismatches_name_both_shapes():
    import dgg_amd
    with pytest.raises(ValueError) as e:
        dgg_amd.AllPairs(torch.ones(5), prior=graph(6))
    assert "(5,)" in str(e.value) and "(6, 6)" in str(e.value) and "(5, 5)" in str(e.value)
    with pytest.raises(ValueError):
        dgg_amd.AllPairs(torch.ones(6), prior=torch.zeros(6, 7))
    with pytest.raises(ValueError) as e:
        dgg_amd.AllPairs(torch.ones(6), prior=torch.zeros(6, 6, device="meta"))
    assert "meta" in str(e.value) and "cpu" in str(e.value) and "(6,)" in str(e.value) and "(6, 6)" in str(e.value)


@pytest.mark.parametrize("loops", [False, True])
def test_from_graph_degrees_are_csr_candidates_degrees(loops):
    import dgg_amd
    G = graph()
    A = dgg_amd.AllPairs.from_graph(G, self_loops=loops)
    want = G.to_dense() + (torch.eye(6) if loops else 0)
    assert torch.equal(A.prior.to_dense(), want)
    assert torch.equal(A.prior_degree, dgg_amd.csr_candidates(want.to_sparse().coalesce())[2])
    assert torch.equal(A.prior_degree, want.sum(1))
    assert A.shape == (6, 6) and A.prior_csr()[1].dtype == torch.int32
    D = dgg_amd.AllPairs.from_graph(G.to_dense(), self_loops=loops)
    assert torch.equal(D.prior.to_dense(), want)


def test_models_pass_all_pairs_through_unchanged():
    import dgg_amd
    from dgg_amd.model import _with_self_loops
    A = dgg_amd.AllPairs.from_graph(graph())
    assert _with_self_loops(A) is A


# ---------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------
def _declared(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dgg_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m, f"include/dgg_hip.h does not declare {name}"
    return [re.sub(r".*[\s\*]", "", a.strip()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("base", ["dgg_allpairs_mlp_topk", "dgg_allpairs_mlp_topk_wide"])
def test_header_declares_the_prior_entries_as_the_existing_ones_plus_the_csr_arrays(base):
    old, new = _declared(base), _declared(base + "_prior")
    assert new == old[:-1] + PRIOR_ARGS + ["stream"]
    import dgg_amd
    L = ctypes.CDLL(dgg_amd._lib.SO_PATH)
    assert hasattr(L, base + "_prior"), f"libdgg_hip.so does not export {base}_prior"
    assert len(dgg_amd._lib.PROTOTYPES[base + "_prior"]) == len(new) == len(dgg_amd._lib.PROTOTYPES[base]) + 3


def test_header_states_the_input_contract_and_cites_the_reference():
    txt = open(os.path.join(ROOT, "include", "dgg_hip.h")).read()
    doc = txt[txt.index("dgg_allpairs_mlp_topk with ex_mode 1"):txt.index("int dgg_allpairs_mlp_topk_wide_prior")]
    assert "STRICTLY ASCENDING" in doc
    for cite in ("dgm.py:1628-1644", "1211-1229", "1404"):
        assert cite in doc


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scorer", ["u-v-A_uv", "A_uv"])
def test_plain_all_pairs_still_refuses_the_scorers_that_read_the_graph(scorer):
    import dgg_amd
    m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args(scorer))
    with pytest.raises(NotImplementedError) as e:
        m(torch.zeros(4, 8), dgg_amd.AllPairs(torch.ones(4)))
    assert all(s in str(e.value) for s in SCORERS) and scorer in str(e.value)
    assert "reads the stored values of in_adj" in str(e.value) and "which all-pairs candidates do not have" in str(e.value)


def test_gcn_x_deg_still_refuses_plain_all_pairs():
    import dgg_amd
    m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args("u-v-deg", dgg_mode_k_net="gcn-x-deg"))
    with pytest.raises(NotImplementedError) as e:
        m(torch.zeros(6, 8), dgg_amd.AllPairs(torch.ones(6)))
    assert "gcn-x-deg" in str(e.value) and "aggregates over the stored entries of in_adj, which all-pairs candidates do not have" in str(e.value)


def test_a_uv_with_a_prior_refuses_and_names_the_reason():
    import dgg_amd
    m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args("A_uv"))
    with pytest.raises(NotImplementedError) as e:
        m(torch.zeros(6, 8), dgg_amd.AllPairs.from_graph(graph()))
    assert "hidden width 1" in str(e.value) and "ties" in str(e.value) and "u-v-A_uv" in str(e.value)


def test_u_v_a_uv_with_a_prior_gets_past_the_refusals():
    import dgg_amd
    m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args("u-v-A_uv"))
    with pytest.raises(AssertionError, match="GPU"):             # (CPU tensors: the first kernel wrapper)
        m(torch.zeros(6, 8), dgg_amd.AllPairs.from_graph(graph()))
    for rows in ("list", "chunked"):
        m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args("u-v-A_uv", dgg_allpairs_mlp_rows=rows))
        for noise_mode in range(6):
            assert m.wide_row_plan(100, True, noise_mode) == rows


@pytest.mark.parametrize("what", ["debug_step", "edge_p-cdf", "dgg_hard_literal", "latent 48"])
def test_what_all_pairs_never_covered_still_refuses_with_a_prior(what):
    import dgg_amd
    kw = {"debug_step": dict(debug_step=1), "edge_p-cdf": dict(dgg_mode_k_select="edge_p-cdf"),
          "dgg_hard_literal": dict(dgg_hard=True, dgg_hard_literal=True), "latent 48": {}}[what]
    m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=48 if what == "latent 48" else 32, args=module_args("u-v-A_uv", **kw))
    with pytest.raises(NotImplementedError):
        m(torch.zeros(6, 8), dgg_amd.AllPairs.from_graph(graph()))


def test_fused_layer_and_row_shards_keep_refusing_with_a_prior():
    import dgg_amd
    from dgg_amd.distributed import ShardedGCN_DGG
    A = dgg_amd.AllPairs.from_graph(graph())
    for opt_in in ({}, {"dgg_allpairs_mlp_fused": True}):
        m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args("u-v-A_uv", **opt_in))
        why = m._fused_outside(_gpu_like(6, 8), A, torch.zeros(32, 16))
        assert why.startswith("edge-MLP scorer on all-pairs candidates")
        if opt_in:
            assert "A_uv" in why
    net = dgg_amd.GCN_DGG(nfeat=32, nhidden=32, nclass=16, args=module_args("u-v-A_uv", dgg_wide_rows="auto", dgg_allpairs_mlp_fused=True))
    with pytest.raises(NotImplementedError, match="u-v-A_uv"):
        ShardedGCN_DGG(net)._check(_gpu_like(6, 32), A, None)
