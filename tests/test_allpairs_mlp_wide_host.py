"""Host-side checks (no GPU) of the wide-row form of the edge-MLP scorers on all-pairs candidates: the two C entries (and
dgg_edge_mlp_bwd_det, the scorer backward with parameter sums in a fixed order) are declared, exported and prototyped; the module's policy summary answers "chunked" exactly under the opt-in args.dgg_allpairs_mlp_rows."""
import ctypes
import os
import re
import shutil
import subprocess
from argparse import Namespace

import pytest

from helpers import ROOT

ENTRIES = ("dgg_allpairs_mlp_topk_wide", "dgg_softk_bwd_chunked", "dgg_edge_mlp_bwd_det")
SCORERS = ("u-v-deg", "u-v-deg-dist", "edge_conv")
POLICIES = ("auto", "chunked", "csr", "csr_auto", "ell")


def test_header_declares_both_entries_and_compiles_as_c():
    path = os.path.join(ROOT, "include", "dgg_hip.h")
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), f"include/dgg_hip.h does not declare {name}"
    assert shutil.which("gcc") is not None, "the header check needs gcc"
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_both_entries_and_the_prototype_table_knows_them():
    import dgg_amd
    L = ctypes.CDLL(dgg_amd._lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(L, name), f"libdgg_hip.so does not export {name}"
        assert name in dgg_amd._lib.PROTOTYPES
    # one argument per parameter of the declaration
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dgg_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S).group(1)
        assert len(params.split(",")) == len(dgg_amd._lib.PROTOTYPES[name]), name
    assert dgg_amd.ops.APMLP_WIDE_REG_CHUNKS >= 2
    assert callable(dgg_amd.ops.allpairs_mlp_topk_wide) and callable(dgg_amd.ops.softk_bwd_chunked)


def _module(scorer, **kw):
    import dgg_amd
    base = dict(extra_edge_dim={"u-v-deg": 2, "u-v-deg-dist": 3}.get(scorer, 0), extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288,
                dgg_mode_edge_net=scorer, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=True,
                symmetric_noise=False, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
    base.update(kw)
    return dgg_amd.DGG_LearnableK_debug(in_dim=24, latent_dim=32, args=Namespace(**base))


@pytest.mark.parametrize("scorer", SCORERS)
def test_wide_row_plan_answers_chunked_with_the_opt_in(scorer):
    for policy in POLICIES:
        m = _module(scorer, dgg_wide_rows=policy, dgg_allpairs_mlp_rows="chunked")
        for N in (130, 100000):
            for nm in range(6):
                assert m.wide_row_plan(N, True, nm) == "chunked", (policy, N, nm)
        # edge-list candidates are not the opt-in's business
        assert m.wide_row_plan(130, False, 2) == {"ell": "list", "csr": "csr"}.get(policy, "csr_when_needed")


@pytest.mark.parametrize("scorer", SCORERS)
def test_wide_row_plan_answers_list_without_the_opt_in(scorer):
    for policy in POLICIES:
        for kw in ({}, {"dgg_allpairs_mlp_rows": "list"}):
            m = _module(scorer, dgg_wide_rows=policy, **kw)
            for nm in range(6):
                assert m.wide_row_plan(130, True, nm) == "list", (policy, kw, nm)
    with pytest.raises(ValueError, match="dgg_allpairs_mlp_rows"):
        _module(scorer, dgg_allpairs_mlp_rows="csr").wide_row_plan(130, True, 2)
    # the opt-in with a list narrower than a chunk is refused, not ignored
    with pytest.raises(ValueError, match="dgg_ell_width"):
        _module(scorer, dgg_allpairs_mlp_rows="chunked", dgg_ell_width=32).wide_row_plan(130, True, 2)
    assert _module(scorer, dgg_ell_width=32).wide_row_plan(130, True, 2) == "list"


def test_chunk_policy_is_unchanged():
    """_chunk_policy keeps its meaning -- the u-v-dist scorer's chunked rows under args.dgg_wide_rows -- and its answer, opt-in or not"""
    from dgg_amd import ops
    counter_based = (ops.NOISE_NONE, ops.NOISE_HASH, ops.NOISE_HASH_SYM, ops.NOISE_RANKED, ops.NOISE_RANKED_SYM)
    for kw in ({}, {"dgg_allpairs_mlp_rows": "chunked"}):
        for policy in POLICIES:
            for scorer in SCORERS:
                m = _module(scorer, dgg_wide_rows=policy, **kw)
                assert not any(m._chunk_policy(nm) for nm in range(6)), (scorer, policy, kw)
            m = _module("u-v-dist", dgg_wide_rows=policy, **kw)
            for nm in range(6):
                assert m._chunk_policy(nm) == (policy in ("auto", "chunked") and nm in counter_based), (policy, nm, kw)
                # the opt-in does not touch the u-v-dist scorer's plan either
                assert m.wide_row_plan(130, True, nm) == _module("u-v-dist", dgg_wide_rows=policy).wide_row_plan(130, True, nm)
