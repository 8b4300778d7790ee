"""Host-side checks of the edge-MLP scorers on all-pairs candidates (no GPU): the C ABI declares and exports dgg_allpairs_mlp_topk, the
wide-row policy answers "list" for them, and the configurations that stay unsupported say so before any kernel runs."""
import ctypes
import os
import re
import shutil
import subprocess
from argparse import Namespace

import pytest
import torch

from helpers import ROOT

SCORERS = ("u-v-deg", "u-v-deg-dist", "edge_conv")


def module_args(scorer, **kw):
    base = dict(extra_edge_dim={"u-v-deg": 2, "u-v-deg-dist": 3, "u-v-A_uv": 1}.get(scorer, 0), extra_k_dim=1, dgg_hard=False, deg_mean=3.899,
                deg_std=5.288, dgg_mode_edge_net=scorer, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3,
                perturb_edge_prob=True, symmetric_noise=False, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
    base.update(kw)
    return Namespace(**base)


def header_text():
    return open(os.path.join(ROOT, "include", "dgg_hip.h")).read()


def test_header_declares_the_entry_with_the_issue_s_argument_list():
    txt = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"\bint\s+dgg_allpairs_mlp_topk\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m, "include/dgg_hip.h does not declare dgg_allpairs_mlp_topk"
    names = [re.sub(r".*[\s\*]", "", a.strip()) for a in m.group(1).split(",")]
    assert names == ["AB", "xp", "N", "h", "hw", "row0", "row1", "deg", "ex_mode", "t_ex", "wdu", "wdv", "wex", "b1", "w2", "b2", "act",
                     "noise_mode", "G", "ldG", "s0", "s1", "K", "idx", "val", "ex_out", "stream"]


def test_header_with_the_entry_compiles_as_c(tmp_path):
    """a C caller of the new entry compiles against the public header (prototype usable from plain C)"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "dgg_hip.h"\n'
                   "int call(const float *f, int32_t *i, float *o) {\n"
                   "    return dgg_allpairs_mlp_topk(f, f, 8, 16, 16, 0, 8, f, 0, -1.0f, f, f, 0, f, f, f, DGG_ACT_LEAKY, DGG_NOISE_HASH, 0, 0, 1u, 2u, 64,\n"
                   "                                 i, o, 0, 0);\n}\n")
    r = subprocess.run(["gcc", "-fsyntax-only", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_entry_and_the_binding_knows_it():
    import dgg_amd
    L = ctypes.CDLL(dgg_amd._lib.SO_PATH)
    assert hasattr(L, "dgg_allpairs_mlp_topk"), "libdgg_hip.so does not export dgg_allpairs_mlp_topk"
    proto = dgg_amd._lib.PROTOTYPES["dgg_allpairs_mlp_topk"]
    assert len(proto) == 27                                                    # (the header's argument list, checked above)
    assert hasattr(dgg_amd.ops, "allpairs_mlp_topk")


@pytest.mark.parametrize("scorer", SCORERS)
def test_wide_row_plan_is_the_list_for_these_scorers_on_all_pairs(scorer):
    import dgg_amd
    for policy in ("auto", "ell", "csr", "csr_auto", "chunked"):
        m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args(scorer, dgg_wide_rows=policy))
        for noise_mode in range(6):
            assert m.wide_row_plan(100, True, noise_mode) == "list"
            assert m.wide_row_plan(100000, True, noise_mode) == "list"
    # edge lists and the u-v-dist scorer keep their answers
    m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args(scorer))
    assert m.wide_row_plan(100, False, 2) == "csr_when_needed"
    u = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args("u-v-dist"))
    assert u.wide_row_plan(100, True, 2) == "chunked"
    assert not m._chunk_policy(2) and u._chunk_policy(2)                       # (the chunked form keeps its condition: u-v-dist only)


@pytest.mark.parametrize("scorer", ["u-v-A_uv", "A_uv"])
def test_scorers_that_read_adjacency_values_refuse_all_pairs_before_any_kernel(scorer):
    import dgg_amd
    m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args(scorer))
    with pytest.raises(NotImplementedError) as e:
        m(torch.zeros(4, 8), dgg_amd.AllPairs(torch.ones(4)))                   # (CPU tensors: the refusal comes first)
    assert all(s in str(e.value) for s in SCORERS) and scorer in str(e.value)


def test_literal_dgg_hard_refuses_before_any_kernel():
    import dgg_amd
    m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args("u-v-deg", dgg_hard=True, dgg_hard_literal=True))
    with pytest.raises(NotImplementedError) as e:
        m(torch.zeros(4, 8), dgg_amd.AllPairs(torch.ones(4)))
    assert "dgg_hard_literal" in str(e.value) and all(s in str(e.value) for s in SCORERS)


def test_the_fused_layer_keeps_its_clause():
    """GCN_DGG falls back to the separate modules for this configuration (which now work); ShardedGCN_DGG refuses through the same clause"""
    import dgg_amd
    m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=32, args=module_args("u-v-deg"))
    why = m._fused_outside(torch.zeros(4, 8), dgg_amd.AllPairs(torch.ones(4)), torch.zeros(8, 8))
    assert why == "edge-MLP scorer on all-pairs candidates"


@pytest.mark.parametrize("scorer,latent,kw", [("u-v-deg", 48, {}), ("u-v-deg-dist", 256, {}), ("edge_conv", 16, {}), ("u-v-deg", 32, {"dgg_ell_width": 128})])
def test_widths_the_kernel_is_not_built_for_refuse_before_any_kernel(scorer, latent, kw):
    """latent_dim outside {16, 32, 64, 128} (edge_conv: its hidden width latent_dim / 2 outside it) and lists wider than 64 ranks are
    refused next to the other all-pairs refusals, before the k-net runs (CPU tensors get that far)"""
    import dgg_amd
    m = dgg_amd.DGG_LearnableK_debug(in_dim=8, latent_dim=latent, args=module_args(scorer, **kw))
    with pytest.raises(NotImplementedError, match="latent_dim in"):
        m(torch.zeros(4, 8), dgg_amd.AllPairs(torch.ones(4)))
