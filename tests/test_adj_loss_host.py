"""Host-side checks (no GPU) of the adjacency supervision loss: the float64 restatement the GPU tests measure against
(tests/adj_loss_ref.py) equals torch's mse_loss on the dense float64 matrices in all three row forms; include/dgg_hip_adj_loss.h is C99,
parses into a table of its own and leaves the recorded tables alone; every refusal of dgg_adj_mse_loss is decided on the host, before
any launch (dummy addresses that are never dereferenced, as tests/test_partp_refusals_host.py does); remove_interclass_edges;
the harness's new flag."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import adj_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "dgg_adj_mse_loss"
HEADER = os.path.join(ROOT, "include", "dgg_hip_adj_loss.h")
ARG = 1                                          # DGG_ERR_ARG (include/dgg_hip.h)
P = 0x100000                                     # an aligned dummy address; P + 4 is not 8-byte aligned


def containers(p):
    """the problem as the package's containers on the CPU (to_dense only) -> (out_adj, target sparse COO)"""
    import dgg_amd
    n, (rowptr, col, val) = p["n"], p["graph"]
    T = torch.from_numpy
    if p["form"] == "list":
        A = dgg_amd.EllAdjacency(T(p["arrs"][0]), T(p["arrs"][1]), n)
    elif p["form"] == "chunked":
        idx, v, cptr = p["arrs"]
        cnt = np.diff(cptr)
        cnode = np.concatenate([np.repeat(np.arange(n), cnt), np.full(idx.shape[0] - int(cptr[n]), n - 1)]).astype(np.int32)
        lay = dgg_amd.ops.ChunkLayout(T(cptr), T(cnode), None, idx.shape[0], int(cnt.max()), n)
        assert lay.wide
        A = dgg_amd.EllAdjacency(T(idx), T(v), n, layout=lay)
    else:
        rowptr_l, col_l, v = p["arrs"]
        live = col_l >= 0                        # (CsrAdjacency.to_dense has no padding: the dense matrix is built from the live entries)
        erow = np.repeat(np.arange(n), np.diff(rowptr_l)).astype(np.int32)
        A = dgg_amd.CsrAdjacency(None, T(col_l[live]), T(erow[live]), T(v[live]), n)
    g_rows = np.repeat(np.arange(n), np.diff(rowptr))
    G = torch.sparse_coo_tensor(T(np.stack([g_rows, col.astype(np.int64)])), T(val), (n, n)).coalesce()
    return A, G


@pytest.mark.parametrize("name", ["small_list", "small_chunked", "small_csr"])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_restatement_equals_the_dense_mse_loss(name, reduction):
    p = R.problem(name)
    assert p["n"] <= 60
    R.check_awkward_cases(p)
    A, G = containers(p)
    dense = torch.nn.functional.mse_loss(A.to_dense().double(), G.to_dense().double(), reduction=reduction)
    rows, cols, vals = R.learned_triplets(p["form"], p["arrs"], p["n"])
    mine, grad = R.loss_and_grad(p["n"], rows, cols, vals, *p["graph"], reduction=reduction)
    assert abs(mine - float(dense)) <= 1e-12 * float(dense), (mine, float(dense))
    # ... and the per-entry gradient is autograd's through the dense matrices
    a = torch.from_numpy(vals.astype(np.float64)).requires_grad_()
    live = torch.from_numpy(cols >= 0)
    D = torch.zeros(p["n"], p["n"], dtype=torch.float64).index_put((torch.from_numpy(rows)[live], torch.from_numpy(cols)[live]), a[live], accumulate=True)
    torch.nn.functional.mse_loss(D, G.to_dense().double(), reduction=reduction).backward()
    assert np.allclose(grad.reshape(-1), a.grad.numpy(), rtol=1e-12, atol=0.0)
    assert np.all(grad.reshape(-1)[cols < 0] == 0)


def test_restatement_by_hand():
    # A = [[., .5], [2, .]], G = [[1, .], [2, 3]]: (0,1) only in A, (0,0) and (1,1) only in G, (1,0) in both with a == g
    rowptr, col, val = np.array([0, 1, 3]), np.array([0, 0, 1], np.int32), np.array([1, 2, 3], np.float32)
    loss, grad = R.loss_and_grad(2, np.array([0, 1, 1]), np.array([1, 0, -1]), np.array([0.5, 2.0, 9.0], np.float32), rowptr, col, val, "sum")
    assert loss == 0.25 + 1.0 + 9.0 and grad.tolist() == [1.0, 0.0, 0.0]
    loss, grad = R.loss_and_grad(2, np.array([0, 1, 1]), np.array([1, 0, -1]), np.array([0.5, 2.0, 9.0], np.float32), rowptr, col, val, "mean")
    assert loss == 10.25 / 4 and grad.tolist() == [0.25, 0.0, 0.0]
    assert R.close(1.0 + 2.0 ** -23, 1.0) and not R.close(1.0 + 2.0 ** -21, 1.0)


def test_the_header_compiles_as_c99_and_cites_the_reference():
    assert shutil.which("gcc") is not None, "the header check needs gcc"
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(HEADER).read()
    assert '#include "dgg_hip.h"' in text and "train_reddit.py:236-251" in text and "dgg_hip_next.h\"" not in text


def test_the_header_has_a_table_of_its_own():
    import dgg_amd
    L_ = dgg_amd._lib
    assert set(L_.ADJ_LOSS_PROTOTYPES) == set(L_.ADJ_LOSS_RESTYPES) == {ENTRY}
    Pv, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    #                                         idx val rows K cptr chunks rowptr_l col_l rowptr col gval reduction scale ws dval out stream
    assert L_.ADJ_LOSS_PROTOTYPES[ENTRY] == [Pv, Pv, I64, I, Pv, I64, Pv, Pv, Pv, Pv, Pv, I, F, Pv, Pv, Pv, Pv]
    assert L_.ADJ_LOSS_RESTYPES[ENTRY] is ctypes.c_int
    raw = ctypes.CDLL(L_.SO_PATH)
    assert hasattr(raw, ENTRY), f"libdgg_hip.so does not export {ENTRY}"
    fn = getattr(L_.bind(raw, [ENTRY]), ENTRY)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == L_.ADJ_LOSS_PROTOTYPES[ENTRY]
    assert list(getattr(L_.lib(), ENTRY).argtypes) == L_.ADJ_LOSS_PROTOTYPES[ENTRY]          # lib() binds it with the rest
    assert dgg_amd.ops.ADJ_LOSS_REDUCTIONS == {"mean": 0, "sum": 1}
    text = open(HEADER).read()
    assert "#define DGG_ADJ_LOSS_MEAN 0\n" in text and "#define DGG_ADJ_LOSS_SUM 1\n" in text


def test_the_recorded_tables_do_not_see_it():
    import dgg_amd
    L_ = dgg_amd._lib
    assert ENTRY not in L_.PROTOTYPES and ENTRY not in L_.NEXT_PROTOTYPES and all(ENTRY not in b for b in L_.NEXT_BLOCKS.values())
    assert set(L_.NEXT_PROTOTYPES) == {"dgg_edgelist_topk_chunked", "dgg_edgelist_topk_p_chunked"}
    assert list(L_.NEXT_BLOCKS) == ["norm_spmm", "project_knet", "adj_stats"]
    assert L_.PROTOTYPES == {n_: a for n_, (_, a) in L_._read_header().items() if n_ not in L_._INFO}
    assert L_.lib().dgg_abi_version() == 6


def call(L, **over):
    """one call of the entry; the defaults are a valid list-form call on 259 rows, which a test must never send as it is"""
    a = dict(idx=P, val=P, rows=259, K=64, cptr=None, chunks=0, rowptr_l=None, col_l=None, rowptr=P, col=P, gval=P, reduction=0, scale=1.0, ws=P,
             dval=None, out=P)
    a.update(over)
    assert over, "a call without a reason to be refused would launch"
    return L.dgg_adj_mse_loss(a["idx"], a["val"], a["rows"], a["K"], a["cptr"], a["chunks"], a["rowptr_l"], a["col_l"], a["rowptr"], a["col"], a["gval"],
                              a["reduction"], a["scale"], a["ws"], a["dval"], a["out"], None)


REFUSALS = [
    ("rows < 0", dict(rows=-1)),
    ("rows = 2^31", dict(rows=1 << 31)),
    ("K = 0", dict(K=0)),
    ("K = 65", dict(K=65)),
    ("K = 65 on an empty graph", dict(K=65, rows=0)),
    ("chunked rows with K = 32", dict(cptr=P, K=32, chunks=300)),
    ("chunked rows with chunks < 0", dict(cptr=P, chunks=-1)),
    ("list and CSR rows at once", dict(rowptr_l=P, col_l=P)),
    ("chunked and CSR rows at once", dict(idx=None, cptr=P, chunks=300, rowptr_l=P, col_l=P)),
    ("idx with col_l", dict(col_l=P)),
    ("a reduction that is neither", dict(reduction=2)),
    ("NULL idx", dict(idx=None)),
    ("NULL val", dict(val=None)),
    ("NULL val, CSR rows", dict(idx=None, rowptr_l=P, col_l=P, val=None)),
    ("CSR rows without col_l", dict(idx=None, rowptr_l=P)),
    ("CSR rows without rowptr_l", dict(idx=None, col_l=P)),
    ("NULL rowptr", dict(rowptr=None)),
    ("NULL col", dict(col=None)),
    ("NULL gval", dict(gval=None)),
    ("NULL ws", dict(ws=None)),
    ("ws not 8-byte aligned", dict(ws=P + 4)),
    ("ws not 8-byte aligned, chunked rows", dict(cptr=P, chunks=300, ws=P + 4)),
    ("ws not 8-byte aligned, CSR rows", dict(idx=None, rowptr_l=P, col_l=P, ws=P + 4)),
    ("NULL out", dict(out=None)),
    ("NULL out on an empty graph", dict(out=None, rows=0)),
]


@pytest.mark.parametrize("what,over", REFUSALS, ids=[w for w, _ in REFUSALS])
def test_refusals_are_decided_on_the_host(what, over):
    import dgg_amd
    L = dgg_amd._lib.lib()
    rc = call(L, **over)
    text = L.dgg_last_error().decode()
    assert rc == ARG, f"{what}: status {rc} ({text})"
    assert text.startswith(ENTRY + ":"), f"{what}: dgg_last_error() does not name the entry: {text!r}"


def test_remove_interclass_edges():
    from dgg_amd.data import remove_interclass_edges
    rng = np.random.default_rng(5)
    n = 40
    labels = torch.from_numpy(rng.integers(0, 3, n))
    ind = torch.from_numpy(rng.integers(0, n, (2, 300)))
    adj = torch.sparse_coo_tensor(ind, torch.from_numpy(rng.random(300).astype(np.float32)) + 2.0, (n, n + 0))      # duplicates: not coalesced
    got = remove_interclass_edges(adj, labels)
    assert got.is_coalesced() and tuple(got.shape) == (n, n) and got.dtype == torch.float32
    pairs = {(int(r), int(c)) for r, c in ind.T.tolist()}
    want = sorted((r, c) for r, c in pairs if labels[r] == labels[c])
    assert [tuple(rc) for rc in got.indices().T.tolist()] == want and 0 < len(want) < len(pairs)
    assert torch.equal(got.values(), torch.ones(len(want)))
    # integer-valued graphs and label arrays of numpy are taken too
    gi = remove_interclass_edges(torch.sparse_coo_tensor(ind, torch.ones(300, dtype=torch.int64), (n, n)), labels.numpy())
    assert torch.equal(gi.indices(), got.indices()) and torch.equal(gi.values(), got.values())
    # nothing kept: an empty graph of the same shape
    none = remove_interclass_edges(torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.ones(1), (2, 2)), torch.tensor([0, 1]))
    assert none._nnz() == 0 and tuple(none.shape) == (2, 2)


def test_the_public_function_refuses_what_it_cannot_take():
    import dgg_amd
    idx, val = torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2)
    G = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.ones(1), (4, 4))
    shard = dgg_amd.CsrAdjacency(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0), 4,
                                 row0=2, n_rows=2)
    with pytest.raises(NotImplementedError, match="row shard"):
        dgg_amd.adjacency_mse_loss(shard, G)
    with pytest.raises(NotImplementedError, match="row shard"):
        dgg_amd.adjacency_mse_loss(dgg_amd.EllAdjacency(idx[:2], val[:2], 4), G)
    with pytest.raises(ValueError, match="reduction"):
        dgg_amd.adjacency_mse_loss(dgg_amd.EllAdjacency(idx, val, 4), G, reduction="none")
    with pytest.raises(TypeError, match="target"):
        dgg_amd.adjacency_mse_loss(dgg_amd.EllAdjacency(idx, val, 4), G.to_dense())
    with pytest.raises(ValueError, match=r"\(5, 5\)"):
        dgg_amd.adjacency_mse_loss(dgg_amd.EllAdjacency(idx, val, 4), torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.ones(1), (5, 5)))

    class Owner:
        def check_ell_bound(self):
            raise RuntimeError("learned k left the ELL width")
    with pytest.raises(RuntimeError, match="ELL width"):          # honoured as in to_dense()
        dgg_amd.adjacency_mse_loss(dgg_amd.EllAdjacency(idx, val, 4, owner=Owner()), G)


def test_the_harness_parses_its_new_flag():
    from dgg_amd import train_small_graphs as T
    a = T.build_parser().parse_args(["--data_dir", "x"])
    assert a.adj_loss_weight == 0.0 and not hasattr(a, "dgg_differentiable_adj")
    assert T.build_parser().parse_args(["--data_dir", "x", "--adj_loss_weight", "10000"]).adj_loss_weight == 10000.0
    help_text = T.build_parser().format_help()
    assert "WITHOUT the self loops" in " ".join(help_text.split())
