"""Host-side checks (no GPU) of the mini-batch sampling: the numpy restatement the GPU tests compare against (tests/subgraph_ref.py) cuts
the sub-graph scipy cuts and walks a fixed, recorded walk; include/dgg_hip_sampling.h is C99, parses into a table of its own and collides
with no other header; every refusal of the two entries is decided on the host, before any launch (dummy addresses that are never
dereferenced, as tests/test_adj_loss_host.py does); the samplers refuse bad arguments by name; contiguous_parts; the harness's parser."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import subgraph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dgg_hip_sampling.h")
WALK, CUT = "dgg_random_walk_nodes", "dgg_induced_subgraph"
ARG = 1                                          # DGG_ERR_ARG (include/dgg_hip.h)
P = 0x100000                                     # a dummy address


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_cuts_what_scipy_cuts(seed):
    """indices, their order and the values of A[idx][:, idx], idx = the sorted distinct members of the request; graphs with isolated
    nodes (no out-edge, and nodes no entry points at), requests with duplicates in any order"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    N = 90
    degs = rng.integers(0, 9, N)
    degs[[3, 40]] = 0
    degs[7] = 70                                                     # wider than one 64-lane stride
    rowptr, col, values = R.random_graph(N, degs, seed + 10)
    A = sp.csr_matrix((values, col, rowptr), shape=(N, N))
    for M in (1, 17, 64, 150):
        nodes = rng.integers(0, N, M).astype(np.int32)
        if M > 1:
            nodes[1] = nodes[0]                                      # a duplicate, always
            nodes[-1] = 3                                            # ... and an isolated node
        idx = np.unique(nodes)
        S = A[idx][:, idx].tocsr()
        S.sort_indices()
        got = R.induced(rowptr, col, nodes, values)
        assert got["n"] == len(idx) and np.array_equal(got["orig"], idx)
        assert np.array_equal(got["browptr"], S.indptr) and np.array_equal(got["bcol"], S.indices)
        assert np.array_equal(values[got["beid"]], S.data) and got["e"] == S.nnz
        assert np.array_equal(got["brow"], np.repeat(np.arange(len(idx)), np.diff(S.indptr)))
        assert np.array_equal(got["newid"][idx], np.arange(len(idx))) and (np.delete(got["newid"], idx) == -1).all()
        # the fixed-order row sums are the exact sums here (values of 24 bits, sums far below 2^29 of them): scipy's, rounded once
        exact = np.array([np.float32(S.data[S.indptr[i]:S.indptr[i + 1]].astype(np.float64).sum()) for i in range(len(idx))], np.float32)
        assert np.array_equal(got["bdeg"], exact)


def test_restatement_of_the_whole_graph_is_the_graph():
    rowptr, col, values = R.graph300()
    got = R.induced(rowptr, col, np.arange(R.N300, dtype=np.int32), values)
    assert np.array_equal(got["browptr"], rowptr) and np.array_equal(got["bcol"], col) and np.array_equal(got["beid"], np.arange(col.size))
    assert np.array_equal(np.diff(rowptr)[list(R.SPECIAL_DEGREES)], list(R.SPECIAL_DEGREES.values()))


RECORDED = [[5, 187, 111, 196, 13], [0, 0, 0, 0, 0], [2, 104, 198, 39, 33], [299, 295, 32, 194, 44]]      # roots 5, 0, 2, 299; L = 4; seed (1234, 7)


def test_restatement_walks_inside_the_graph_and_is_a_fixed_function():
    rowptr, col, _ = R.graph300()
    assert [int(v) for v in R.mix32([0, 1, 0xDEADBEEF])] == [0, 1753845952, 3861431939]
    roots = [5, 0, 2, 299]
    w = R.walk(rowptr, col, roots, 4, (1234, 7))
    assert w.tolist() == RECORDED
    big = R.walk(rowptr, col, np.arange(R.N300), 6, (99, 3))
    assert big.min() >= 0 and big.max() < R.N300 and np.array_equal(big[:, 0], np.arange(R.N300))
    for b in range(R.N300):
        for t in range(1, 7):
            u, v = int(big[b, t - 1]), int(big[b, t])
            nb = col[rowptr[u]:rowptr[u + 1]]
            assert (v == u) if nb.size == 0 else (v in nb), (b, t, u, v)
    assert (big[0] == 0).all() and (big[6] == 6).all()                # degree 0: the walk never leaves
    # a function of (seed, b, t) only: the same walk index from the same node takes the same step whatever the other roots are
    again = R.walk(rowptr, col, [5, 7, 2, 1], 4, (1234, 7))
    assert again[0].tolist() == RECORDED[0] and again[2].tolist() == RECORDED[2]
    assert R.walk(rowptr, col, roots, 4, (1234, 8)).tolist() != RECORDED and R.walk(rowptr, col, roots, 4, (1235, 7)).tolist() != RECORDED


@pytest.mark.parametrize("d", [1, 2, 63, 64, 65, 1 << 31])
def test_the_pick_is_below_the_degree(d):
    for x in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF):
        assert 0 <= R.pick(x, d) < d
    assert R.pick(0xFFFFFFFF, d) == d - 1 and R.pick(0, d) == 0       # both ends are reached
    assert R.pick(0xFFFFFFFF, (1 << 32) - 1) == (1 << 32) - 2         # the widest row the entry admits


# ---- the header and its table ----------------------------------------------------------------------------------------------------------
def test_the_header_compiles_as_c99():
    assert shutil.which("gcc") is not None, "the header check needs gcc"
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(HEADER).read()
    assert '#include "dgg_hip.h"' in text and "train_large_graphs.py:402-421" in text and "0x9E3779B9" in text


def test_the_header_has_a_table_of_its_own():
    import dgg_amd
    L_ = dgg_amd._lib
    Pv, I, I64, U32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32
    assert set(L_.SAMPLING_PROTOTYPES) == set(L_.SAMPLING_RESTYPES) == {WALK, CUT}
    #                                      rowptr col N  E    roots B    L  s0   s1   walk status stream
    assert L_.SAMPLING_PROTOTYPES[WALK] == [Pv, Pv, I64, I64, Pv, I64, I, U32, U32, Pv, Pv, Pv]
    #                                     phase rowptr col values N E   nodes M  flag rank newid orig rows bdeg_i bdeg browptr E_b bcol beid brow status stream
    assert L_.SAMPLING_PROTOTYPES[CUT] == [I, Pv, Pv, Pv, I64, I64, Pv, I64, Pv, Pv, Pv, Pv, I64, Pv, Pv, Pv, I64, Pv, Pv, Pv, Pv, Pv]
    assert all(r is ctypes.c_int for r in L_.SAMPLING_RESTYPES.values())
    raw = ctypes.CDLL(L_.SO_PATH)
    for name in (WALK, CUT):
        assert hasattr(raw, name), f"libdgg_hip.so does not export {name}"
        assert list(getattr(L_.lib(), name).argtypes) == L_.SAMPLING_PROTOTYPES[name]          # lib() binds them with the rest
    assert (dgg_amd.ops.SUBGRAPH_MARK, dgg_amd.ops.SUBGRAPH_RELABEL, dgg_amd.ops.SUBGRAPH_COUNT, dgg_amd.ops.SUBGRAPH_FILL) == (0, 1, 2, 3)
    text = open(HEADER).read()
    for k_, v in (("DGG_SUBGRAPH_MARK", 0), ("DGG_SUBGRAPH_RELABEL", 1), ("DGG_SUBGRAPH_COUNT", 2), ("DGG_SUBGRAPH_FILL", 3),
                  ("DGG_SAMPLING_BAD_NODE", 1), ("DGG_SAMPLING_BAD_GRAPH", 2)):
        assert f"#define {k_} {v}\n" in text
    assert set(dgg_amd.ops.SAMPLING_STATUS) == {1, 2}


def test_no_name_collides_with_the_other_headers():
    import dgg_amd
    L_ = dgg_amd._lib
    others = set(L_.PROTOTYPES) | set(L_._INFO) | set(L_.NEXT_PROTOTYPES) | {n for b in L_.NEXT_BLOCKS.values() for n in b} | set(L_.ADJ_LOSS_PROTOTYPES)
    assert not others & set(L_.SAMPLING_PROTOTYPES)
    # ... the recorded tables are what they were, and a header that declares a known name again is refused when it is read
    assert set(L_.ADJ_LOSS_PROTOTYPES) == {"dgg_adj_mse_loss"} and list(L_.NEXT_BLOCKS) == ["norm_spmm", "project_knet", "adj_stats"]
    assert L_.lib().dgg_abi_version() == 6
    src = open(os.path.join(os.path.dirname(L_.__file__), "_lib.py")).read()
    assert "set(_SAMPLING_DECLS) & (set(_DECLS) | set(_NEXT_DECLS) | set(_LATER_DECLS) | set(_ADJ_LOSS_DECLS))" in src


# ---- refusals of the entries, decided before any launch --------------------------------------------------------------------------------
def call_walk(lib_, **over):
    a = dict(rowptr=P, col=P, N=300, E=2000, roots=P, B=64, L=2, s0=1, s1=2, walk=P, status=P)
    a.update(over)
    assert over, "a call without a reason to be refused would launch"
    return lib_.dgg_random_walk_nodes(a["rowptr"], a["col"], a["N"], a["E"], a["roots"], a["B"], a["L"], a["s0"], a["s1"], a["walk"], a["status"], None)


WALK_REFUSALS = [
    ("N < 0", dict(N=-1)), ("N = 2^31", dict(N=1 << 31)), ("E < 0", dict(E=-1)), ("E = 2^32: a degree could reach 2^32", dict(E=1 << 32)),
    ("B < 0", dict(B=-1)), ("B = 2^31", dict(B=1 << 31)), ("L < 0", dict(L=-1)), ("roots on a graph without nodes", dict(N=0, E=0)),
    ("NULL rowptr", dict(rowptr=None)), ("NULL col", dict(col=None)), ("NULL roots", dict(roots=None)), ("NULL walk", dict(walk=None)),
    ("NULL status", dict(status=None)),
]


@pytest.mark.parametrize("what,over", WALK_REFUSALS, ids=[w for w, _ in WALK_REFUSALS])
def test_walk_refusals_are_decided_on_the_host(what, over):
    import dgg_amd
    L = dgg_amd._lib.lib()
    rc = call_walk(L, **over)
    text = L.dgg_last_error().decode()
    assert rc == ARG and text.startswith(WALK + ":"), f"{what}: status {rc} ({text!r})"


def call_cut(L, **over):
    a = dict(phase=0, rowptr=P, col=P, values=None, N=300, E=2000, nodes=P, M=64, flag=P, rank=P, newid=P, orig=P, rows=64, bdeg_i=P, bdeg=P,
             browptr=P, E_b=100, bcol=P, beid=P, brow=P, status=P)
    a.update(over)
    assert over, "a call without a reason to be refused would launch"
    return L.dgg_induced_subgraph(a["phase"], a["rowptr"], a["col"], a["values"], a["N"], a["E"], a["nodes"], a["M"], a["flag"], a["rank"], a["newid"],
                                  a["orig"], a["rows"], a["bdeg_i"], a["bdeg"], a["browptr"], a["E_b"], a["bcol"], a["beid"], a["brow"], a["status"], None)


CUT_REFUSALS = [
    ("phase -1", dict(phase=-1)), ("phase 4", dict(phase=4)), ("N < 0", dict(N=-1)), ("N = 2^31", dict(N=1 << 31)), ("M < 0", dict(M=-1)),
    ("E < 0", dict(E=-1)), ("rows < 0", dict(rows=-1)), ("E_b < 0", dict(E_b=-1)), ("rows > N", dict(rows=301)), ("NULL status", dict(status=None)),
    ("MARK: NULL flag", dict(flag=None)), ("MARK: NULL nodes", dict(nodes=None)),
    ("RELABEL: NULL rank", dict(phase=1, rank=None)), ("RELABEL: NULL newid", dict(phase=1, newid=None)), ("RELABEL: NULL orig", dict(phase=1, orig=None)),
    ("COUNT: NULL rowptr", dict(phase=2, rowptr=None)), ("COUNT: NULL col", dict(phase=2, col=None)), ("COUNT: NULL bdeg_i", dict(phase=2, bdeg_i=None)),
    ("COUNT: values without bdeg", dict(phase=2, values=P, bdeg=None)), ("COUNT: NULL rank", dict(phase=2, rank=None)),
    ("FILL: NULL browptr", dict(phase=3, browptr=None)), ("FILL: NULL bcol", dict(phase=3, bcol=None)), ("FILL: NULL beid", dict(phase=3, beid=None)),
    ("FILL: NULL brow", dict(phase=3, brow=None)), ("FILL: NULL newid", dict(phase=3, newid=None)),
]


@pytest.mark.parametrize("what,over", CUT_REFUSALS, ids=[w for w, _ in CUT_REFUSALS])
def test_cut_refusals_are_decided_on_the_host(what, over):
    import dgg_amd
    L = dgg_amd._lib.lib()
    rc = call_cut(L, **over)
    text = L.dgg_last_error().decode()
    assert rc == ARG and text.startswith(CUT + ":"), f"{what}: status {rc} ({text!r})"


def test_empty_problems_launch_nothing():
    """the returns that come before any launch: with NULL everywhere they would fault if anything were read"""
    import dgg_amd
    L = dgg_amd._lib.lib()
    assert call_walk(L, B=0, rowptr=None, col=None, roots=None, walk=None, status=None) == 0
    none = dict(rowptr=None, col=None, nodes=None, flag=None, rank=None, newid=None, orig=None, bdeg_i=None, bdeg=None, browptr=None, bcol=None, beid=None,
                brow=None)
    for ph in range(4):
        assert call_cut(L, phase=ph, N=0, E=0, M=0, rows=0, E_b=0, **none) == 0                 # a graph without nodes
    assert call_cut(L, phase=2, rows=0, **none) == 0 and call_cut(L, phase=3, rows=0, **none) == 0
    assert call_cut(L, phase=3, E_b=0, **none) == 0


# ---- the samplers ----------------------------------------------------------------------------------------------------------------------
def small_graph(n=12):
    i = torch.arange(n)
    return torch.sparse_coo_tensor(torch.stack([i, (i + 1) % n]), torch.ones(n), (n, n)).coalesce()


def test_samplers_refuse_bad_arguments_by_name():
    import dgg_amd
    g = small_graph()
    with pytest.raises(ValueError, match="parts"):
        dgg_amd.ClusterSampler(g, torch.zeros(11, dtype=torch.int64), batch_size=2)
    with pytest.raises(ValueError, match="parts"):
        dgg_amd.ClusterSampler(g, torch.zeros(12), batch_size=2)                               # float ids
    with pytest.raises(ValueError, match="batch_size"):
        dgg_amd.ClusterSampler(g, torch.zeros(12, dtype=torch.int64), batch_size=0)
    with pytest.raises(ValueError, match="batch_size"):
        dgg_amd.RandomWalkSampler(g, batch_size=0, walk_length=2, num_steps=3)
    with pytest.raises(ValueError, match="walk_length"):
        dgg_amd.RandomWalkSampler(g, batch_size=4, walk_length=-1, num_steps=3)
    with pytest.raises(ValueError, match="num_steps"):
        dgg_amd.RandomWalkSampler(g, batch_size=4, walk_length=1, num_steps=0)
    for make in (lambda a: dgg_amd.RandomWalkSampler(a, 4, 1, 3), lambda a: dgg_amd.ClusterSampler(a, torch.zeros(12, dtype=torch.int64), 2)):
        with pytest.raises(TypeError, match="graph"):
            make(g.to_dense())
        with pytest.raises(ValueError, match="graph"):
            make(torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.ones(1), (12, 13)))


def test_sampler_schedules_are_fixed_functions_of_seed_and_epoch():
    import dgg_amd
    g = small_graph()
    s = dgg_amd.RandomWalkSampler(g, batch_size=5, walk_length=2, num_steps=3, seed=4)
    assert len(s) == 3 and s.roots(0).dtype == torch.int32 and s.roots(0).shape == (5,) and int(s.roots(0).max()) < 12
    r0 = [s.roots(i).tolist() for i in range(3)]
    assert r0 == [s.roots(i).tolist() for i in range(3)] and r0[0] != r0[1]
    s.set_epoch(1)
    assert [s.roots(i).tolist() for i in range(3)] != r0 and s.walk_seed(0) != dgg_amd.RandomWalkSampler(g, 5, 2, 3, seed=4).walk_seed(0)
    c = dgg_amd.ClusterSampler(g, dgg_amd.contiguous_parts(12, 4), batch_size=3, seed=1)
    assert len(c) == 2 and c.num_clusters == 4 and sorted(c.cluster_order()) == [0, 1, 2, 3] and c.cluster_order() == c.cluster_order()
    assert dgg_amd.ClusterSampler(g, dgg_amd.contiguous_parts(12, 4), batch_size=3, shuffle=False).cluster_order() == [0, 1, 2, 3]
    assert sorted(c.batch_nodes([2, 0]).tolist()) == [0, 1, 2, 6, 7, 8]
    # cluster ids need not be 0..k-1
    odd = dgg_amd.ClusterSampler(g, torch.tensor([7, 7, -2, 40, 7, -2, 40, 40, 7, 7, 7, -2]), batch_size=1, shuffle=False)
    assert odd.num_clusters == 3 and [sorted(odd.batch_nodes([i]).tolist()) for i in range(3)] == [[2, 5, 11], [0, 1, 4, 8, 9, 10], [3, 6, 7]]


@pytest.mark.parametrize("N,k", [(12, 4), (700, 7), (10, 3), (5, 5), (9, 1), (1000, 333)])
def test_contiguous_parts_cover_every_node_once(N, k):
    import dgg_amd
    p = dgg_amd.contiguous_parts(N, k)
    assert p.shape == (N,) and p.dtype == torch.int64 and (p[1:] >= p[:-1]).all()              # one id per node: every node in exactly one part
    sizes = torch.bincount(p, minlength=k)
    assert sizes.shape == (k,) and int(sizes.sum()) == N and int(sizes.min()) >= N // k and int(sizes.max()) <= -(-N // k)
    with pytest.raises(ValueError, match="num_parts"):
        dgg_amd.contiguous_parts(N, N + 1)
    with pytest.raises(ValueError, match="num_parts"):
        dgg_amd.contiguous_parts(N, 0)
    assert "NOT METIS" in dgg_amd.contiguous_parts.__doc__


def test_the_harness_parser():
    from dgg_amd import train_large_graphs as H
    a = H.build_parser().parse_args(["--data_dir", "x"])
    assert a.adj_loss_weight == 10000 and a.dataloader == "SAINT" and a.model == "GCN_DGG"
    assert (a.graphsaint_bs, a.graphsaint_wl, a.num_steps, a.cluster_parts, a.cluster_bs) == (2000, 2, 5, 500, 5)
    assert a.edge_noise_level == 0.00014 and a.seed == 42 and a.epochs == 5000
    assert H.build_parser().parse_args(["--data_dir", "x", "--dataloader", "Cluster"]).dataloader == "Cluster"
    with pytest.raises(SystemExit):
        H.build_parser().parse_args(["--data_dir", "x", "--dataloader", "Neighbor"])
    assert "CANNOT be loaded here" in H.__doc__ and "Reddit" in H.__doc__
    # the small-graph harness keeps its own default
    from dgg_amd import train_small_graphs as S
    assert S.build_parser().parse_args(["--data_dir", "x"]).adj_loss_weight == 0.0
