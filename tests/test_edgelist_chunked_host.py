"""Host-side checks (no GPU) of edge-list candidates on chunked rows: the two C entries are declared in include/dgg_hip_next.h (entry
points since ABI v6; plain C), exported, and bound from tables of their own while PROTOTYPES stays the recorded ABI; the module's
argument args.dgg_edgelist_rows refuses what it cannot do and changes nothing at "list"; the clamped-degree identity the layout rests on."""
import ctypes
import inspect
import json
import os
import re
import shutil
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ROOT

ENTRIES = ("dgg_edgelist_topk_chunked", "dgg_edgelist_topk_p_chunked")
NEXT = os.path.join(ROOT, "include", "dgg_hip_next.h")
POLICIES = ("auto", "chunked", "csr", "csr_auto", "ell")
SCORERS = ("u-v-dist", "u-v-deg", "u-v-A_uv", "u-v-deg-dist", "edge_conv", "A_uv")


def test_next_header_declares_both_entries_and_compiles_as_c():
    txt = re.sub(r"/\*.*?\*/", "", open(NEXT).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), f"include/dgg_hip_next.h does not declare {name}"
    assert re.search(r'#include\s+"dgg_hip.h"', txt)
    assert shutil.which("gcc") is not None, "the header check needs gcc"
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", NEXT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_both_entries_and_binds_them_from_their_own_tables():
    import dgg_amd
    L_ = dgg_amd._lib
    raw = ctypes.CDLL(L_.SO_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), f"libdgg_hip.so does not export {name}"
    assert set(L_.NEXT_PROTOTYPES) == set(L_.NEXT_RESTYPES) == set(ENTRIES)
    assert not set(L_.NEXT_PROTOTYPES) & set(L_.PROTOTYPES), "dgg_hip_next.h declares again what dgg_hip.h declares"
    txt = re.sub(r"/\*.*?\*/", "", open(NEXT).read(), flags=re.S)
    lib = L_.lib()
    for name in ENTRIES:
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S).group(1)
        assert len(params.split(",")) == len(L_.NEXT_PROTOTYPES[name]), name
        fn = getattr(lib, name)                               # lib() binds both sets
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L_.NEXT_PROTOTYPES[name], name


def test_the_recorded_abi_is_untouched():
    import dgg_amd
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_abi as R
    with open(os.path.join(GOLDEN, "abi_v6.json")) as f:
        want = json.load(f)["functions"]
    L_ = dgg_amd._lib
    assert set(L_.PROTOTYPES) == set(want)
    for name, rec in want.items():
        assert R.encode(L_.RESTYPES[name], L_.PROTOTYPES[name]) == rec, name
    assert L_.lib().dgg_abi_version() == 6


def test_ops_and_the_kernel_contract_carry_both_entries():
    from dgg_amd import ops
    from dgg_amd.parallel import KernelContract
    for name in ("edgelist_topk_chunked", "edgelist_topk_p_chunked"):
        want = [p for p in inspect.signature(getattr(KernelContract, name)).parameters if p != "self"]
        assert list(inspect.signature(getattr(ops, name)).parameters)[:len(want)] == want, name
        fn = getattr(KernelContract(), name)
        nargs = sum(p.default is p.empty for p in inspect.signature(fn).parameters.values())
        assert fn(*([None] * nargs)) is None, f"{name}: the contract answers None"
    assert list(inspect.signature(ops.edgelist_topk_chunked).parameters)[:10] == ["xp", "rowptr", "col", "k", "layout", "mode", "t", "noise_mode", "seed", "rows"]
    assert list(inspect.signature(ops.edgelist_topk_p_chunked).parameters)[:11] == ["p_edge", "N", "rowptr", "col", "k", "layout", "mode", "noise_mode", "seed",
                                                                                     "ex_edge", "rows"]


def _module(scorer="u-v-dist", **kw):
    import dgg_amd
    base = dict(extra_edge_dim={"u-v-deg": 2, "u-v-deg-dist": 3, "u-v-A_uv": 1}.get(scorer, 0), extra_k_dim=1, dgg_hard=False, deg_mean=3.899,
                deg_std=5.288, dgg_mode_edge_net=scorer, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3,
                perturb_edge_prob=True, symmetric_noise=False, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
    base.update(kw)
    return dgg_amd.DGG_LearnableK_debug(in_dim=24, latent_dim=32, args=Namespace(**base))


@pytest.mark.parametrize("scorer", SCORERS)
def test_each_refused_combination_raises_and_names_both_arguments(scorer):
    for policy in ("csr", "csr_auto", "ell"):
        with pytest.raises(ValueError, match=r"dgg_edgelist_rows.*dgg_wide_rows"):
            _module(scorer, dgg_edgelist_rows="chunked", dgg_wide_rows=policy).wide_row_plan(130, False, 2)
    with pytest.raises(ValueError, match=r"dgg_edgelist_rows.*dgg_ell_width"):
        _module(scorer, dgg_edgelist_rows="chunked", dgg_ell_width=32).wide_row_plan(130, False, 2)
    with pytest.raises(ValueError, match=r"dgg_edgelist_rows must be 'list' or 'chunked', not 'csr'"):
        _module(scorer, dgg_edgelist_rows="csr").wide_row_plan(130, False, 2)
    for policy in ("auto", "chunked"):
        m = _module(scorer, dgg_edgelist_rows="chunked", dgg_wide_rows=policy)
        assert all(m.wide_row_plan(N, False, nm) == "chunked" for N in (130, 100000) for nm in (0, 2, 3))
    # (the predicate the forwards and ShardedGCN_DGG._check ask)
    with pytest.raises(ValueError, match=r"dgg_edgelist_rows.*dgg_wide_rows"):
        _module(scorer, dgg_edgelist_rows="chunked", dgg_wide_rows="csr")._edgelist_chunked()


def test_list_and_an_absent_argument_are_the_same_module():
    x, W = torch.zeros(4, 24), torch.zeros(24, 16)
    A = torch.sparse_coo_tensor(torch.tensor([[0, 1, 2, 3], [1, 0, 3, 2]]), torch.ones(4), (4, 4)).coalesce()
    for scorer in SCORERS:
        for policy in ("auto", "chunked", "csr"):
            a, b = _module(scorer, dgg_wide_rows=policy), _module(scorer, dgg_wide_rows=policy, dgg_edgelist_rows="list")
            for all_pairs in (False, True):
                for nm in range(6):
                    assert a.wide_row_plan(130, all_pairs, nm) == b.wide_row_plan(130, all_pairs, nm), (scorer, policy, all_pairs, nm)
            assert a.wide_row_plan(130, False, 2) == {"csr": "csr"}.get(policy, "csr_when_needed")
            assert a._fused_outside(x, A, W) == b._fused_outside(x, A, W), (scorer, policy)
            assert a._edgelist_chunked() is False and b._edgelist_chunked() is False
            # the opt-in is the edge lists' alone: all-pairs plans do not move
            if policy != "csr":
                c = _module(scorer, dgg_wide_rows=policy, dgg_edgelist_rows="chunked")
                for nm in range(6):
                    assert c.wide_row_plan(130, True, nm) == a.wide_row_plan(130, True, nm), (scorer, policy, nm)
                assert c._fused_outside(x, A, W) == a._fused_outside(x, A, W)


def test_clamped_degree_identity_in_float32():
    """ceil(min(k, n - 9.5) + 8.5) + 1 == min(n, ceil(k + 8.5) + 1) for every n in 1..5000: the layout of the clamped degrees holds exactly
    the ranks that can carry weight.  All arithmetic in float32, as dgg_chunk_layout and klimit_len do it."""
    f = np.float32
    n = np.arange(1, 5001).astype(f)
    edge = n - f(9.5)
    ks = [np.full_like(n, 1.0), np.full_like(n, 54.5), np.full_like(n, 54.6), edge, np.nextafter(edge, f(np.inf)), np.nextafter(edge, f(-np.inf)),
          np.full_like(n, 1e6), np.full_like(n, np.inf)]
    for k in ks:
        k = k.astype(f)
        assert k.dtype == f and (n - f(9.5)).dtype == f
        lhs = np.ceil(np.minimum(k, n - f(9.5)) + f(8.5)) + f(1.0)
        rhs = np.minimum(n, np.ceil(k + f(8.5)) + f(1.0))
        assert lhs.dtype == f and rhs.dtype == f
        assert np.array_equal(lhs, rhs), k[:3]


def test_engine_raises_when_the_namespace_lacks_the_entry():
    """an engine that has laid wide rows out and whose namespace answers None raises NotImplementedError naming the entry"""
    from dgg_amd.parallel import KernelContract, ShardedDGGConv

    class Lay:
        wide, chunks, maxm, rows = True, 9, 2, 8

    class Kern(KernelContract):
        def chunk_layout(self, k, maxm=None, ccap=None, ncols=None, sticky=None):
            return Lay()

        def linear_fwd(self, x, W, b, act, lay):
            return torch.zeros(x.shape[0], W.shape[0])

        def edge_mlp_fwd(self, *a):
            return torch.zeros(8), None

    rowptr, col = torch.arange(9, dtype=torch.int64), torch.zeros(8, dtype=torch.int32)
    for scorer, name in ((None, "edgelist_topk_chunked"), (dict.fromkeys(("erow", "ex_in", "Wcat", "wdu", "wdv", "wex", "b1", "w2", "b2", "act", "ex_mode", "t_ex")),
                                                           "edgelist_topk_p_chunked")):
        eng = ShardedDGGConv(Kern(), 8, cand=(rowptr, col), noise_mode=2)
        eng.wide_rows, eng.scorer = "auto", scorer
        if scorer is not None:
            scorer["Wcat"] = torch.zeros(32, 16)
        with pytest.raises(NotImplementedError, match=name):
            eng._search({"xp": torch.zeros(8, 16), "k": torch.ones(8)}, torch.ones(8))
        # ... and with the rows left on the list nothing is laid out: the list kernels are asked, as ever
        eng.wide_rows = "off"
        assert eng._chunk_layout(torch.ones(8)) is None
