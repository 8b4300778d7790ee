"""Mini-batch sampling on the GPU: dgg_random_walk_nodes and dgg_induced_subgraph (ops.random_walk_nodes / ops.induced_subgraph) against
the numpy restatement tests/subgraph_ref.py (itself held against scipy by tests/test_subgraph_host.py), the samplers of dgg_amd.sampling
on top of them, and the harness dgg_amd.train_large_graphs end to end.

Everything from the kernels is compared BIT FOR BIT: the outputs are integers, plus one float32 row sum that the kernel forms in a fixed
order in double (64 lane sums, xor butterfly, one rounding), which subgraph_ref.lane_sum restates.  With the test graph's values (24-bit
floats in [0.5, 1.5), at most 200 a row) every double sum is exact, so the same bits also equal csr_candidates' row sums, which come from
differences of a float64 running sum (exact as well: the running sum stays below 2^12 with 2^-24 as its finest bit, 36 of double's 53).
Shapes: N = 300 with rows of 0, 1, 63, 64, 65, 128, 129 and 200 entries (both sides of the 64-lane stride, up to four strides); walks
of B = 1, 64, 65, 257 (one lane, a full wavefront, one more, a second workgroup of 256) and L = 0, 1, 4.
The harness: losses finite; the printed adjacency term of the first batch within adj_loss_ref.RTOL = 2^-22 (relative) of the dense
F.mse_loss, the bound tests/test_adj_loss.py holds the kernel to."""
import functools
import pickle
import re
from collections import defaultdict

import numpy as np
import pytest
import torch

import adj_loss_ref
import subgraph_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED = (1234, 7)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def graph():
    """the 300-node graph on the host and on the device, and as a sparse COO tensor (built once, never changed)"""
    rowptr, col, values = R.graph300()
    rows = np.repeat(np.arange(R.N300), np.diff(rowptr))
    coo = torch.sparse_coo_tensor(T(np.stack([rows, col.astype(np.int64)])), T(values), (R.N300, R.N300)).coalesce()
    return dict(host=(rowptr, col, values), dev=(T(rowptr), T(col), T(values)), coo=coo)


def roots_for(B):
    """root 0 and 6 are isolated, 5 is the widest row; duplicates from B = 64 on (B > the 9 special nodes cycles through them twice)"""
    special = list(R.SPECIAL_DEGREES)
    r = np.random.default_rng(B).integers(0, R.N300, B).astype(np.int32)
    n = min(B, 2 * len(special))
    r[:n] = (special + special)[:n]
    return r


# ---- the walk ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 1, 4])
@pytest.mark.parametrize("B", [1, 64, 65, 257])
def test_walk_matches_the_restatement(B, L):
    from dgg_amd import ops
    g = graph()
    roots = roots_for(B)
    want = R.walk(g["host"][0], g["host"][1], roots, L, SEED)
    got = ops.random_walk_nodes(g["dev"][0], g["dev"][1], T(roots), L, SEED, check=True)
    again = ops.random_walk_nodes(g["dev"][0], g["dev"][1], T(roots), L, SEED)
    assert got.shape == (B, L + 1) and got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, again)
    assert (got[0] == 0).all()                                       # root 0 has no out-edge: the walk stays
    if B >= 64:
        assert len(set(roots.tolist())) < B                          # duplicate roots: different walks from the same node
    if L == 4 and B >= 64:
        other = ops.random_walk_nodes(g["dev"][0], g["dev"][1], T(roots), L, (SEED[0], SEED[1] + 1))
        assert torch.equal(other[:, 0], got[:, 0]) and not torch.equal(other, got)
        assert roots[5] == roots[14] == 5 and not torch.equal(got[5], got[14])       # the 200-entry row, walks 5 and 14


def test_walk_refuses_roots_outside_the_graph_and_takes_empty_problems():
    from dgg_amd import ops
    g = graph()
    roots = T(np.array([5, 300, 2, -1], np.int32))
    w = ops.random_walk_nodes(g["dev"][0], g["dev"][1], roots, 3, SEED)
    want = R.walk(g["host"][0], g["host"][1], [5, 0, 2, 0], 3, SEED)
    assert np.array_equal(w[[0, 2]].cpu().numpy(), want[[0, 2]]) and (w[[1, 3]] == -1).all()
    with pytest.raises(ValueError, match="outside"):
        ops.random_walk_nodes(g["dev"][0], g["dev"][1], roots, 3, SEED, check=True)
    with pytest.raises(ValueError, match="nodes must lie in"):       # ... and the cut refuses the row of -1
        ops.induced_subgraph(g["dev"][0], g["dev"][1], w.reshape(-1))
    with pytest.raises(ValueError, match="length"):
        ops.random_walk_nodes(g["dev"][0], g["dev"][1], roots, -1, SEED)
    empty = ops.random_walk_nodes(g["dev"][0], g["dev"][1], torch.empty(0, device=DEV, dtype=torch.int32), 4, SEED, check=True)
    assert empty.shape == (0, 5)
    # a graph without any edge: every walk stays on its root
    rp0 = torch.zeros(R.N300 + 1, device=DEV, dtype=torch.int64)
    stay = ops.random_walk_nodes(rp0, torch.empty(0, device=DEV, dtype=torch.int32), T(np.array([3, 7], np.int32)), 2, SEED, check=True)
    assert stay.tolist() == [[3, 3, 3], [7, 7, 7]]


# ---- the induced sub-graph -------------------------------------------------------------------------------------------------------------
def node_sets():
    rowptr, col, _ = graph()["host"]
    rng = np.random.default_rng(4)
    dup = rng.integers(0, R.N300, 150).astype(np.int32)
    dup[:18] = list(R.SPECIAL_DEGREES) * 2
    s65 = np.concatenate([np.array(list(R.SPECIAL_DEGREES)), rng.choice(np.arange(9, R.N300), 56, replace=False)]).astype(np.int32)
    return dict(single=np.array([5], np.int32), all=np.arange(R.N300, dtype=np.int32)[::-1].copy(), duplicates=dup,
                independent=R.independent_set(rowptr, col, 12)[::-1].copy(), sixty_five=s65, empty=np.zeros(0, np.int32))


@pytest.mark.parametrize("with_values", [False, True])
@pytest.mark.parametrize("name", ["single", "all", "duplicates", "independent", "sixty_five", "empty"])
def test_cut_matches_the_restatement(name, with_values):
    from dgg_amd import ops
    g = graph()
    rowptr, col, values = g["host"]
    nodes = node_sets()[name]
    want = R.induced(rowptr, col, nodes, values if with_values else None)
    reads = ops.SUBGRAPH_READBACKS
    got = ops.induced_subgraph(g["dev"][0], g["dev"][1], T(nodes), g["dev"][2] if with_values else None)
    assert ops.SUBGRAPH_READBACKS == reads + (0 if name == "empty" else 1)
    again = ops.induced_subgraph(g["dev"][0], g["dev"][1], T(nodes), g["dev"][2] if with_values else None)
    assert (got.n, got.e) == (want["n"], want["e"])
    for k_, dt in (("orig", torch.int32), ("newid", torch.int32), ("browptr", torch.int64), ("bcol", torch.int32), ("brow", torch.int32), ("beid", torch.int64)):
        a = getattr(got, k_)
        assert a.dtype == dt and np.array_equal(a.cpu().numpy(), want[k_]), k_
        assert torch.equal(a, getattr(again, k_)), k_                # the same bits on every run
    if with_values:
        assert got.bdeg.dtype == torch.float32 and np.array_equal(got.bdeg.cpu().numpy(), want["bdeg"]) and torch.equal(got.bdeg, again.bdeg)
    else:
        assert got.bdeg is None
    # strictly ascending columns within every row
    bc, rp = got.bcol.cpu().numpy(), got.browptr.cpu().numpy()
    assert all((np.diff(bc[rp[i]:rp[i + 1]]) > 0).all() for i in range(got.n))
    if name == "all":
        assert got.n == R.N300 and torch.equal(got.beid, torch.arange(col.size, device=DEV)) and torch.equal(got.bcol, g["dev"][1])
        assert torch.equal(got.browptr, g["dev"][0])
    if name == "independent":
        assert got.e == 0 and got.n == 12 and (got.browptr == 0).all()
    if name == "sixty_five":
        assert got.n == 65
    if name == "duplicates":
        assert got.n < len(nodes)
    if name == "empty":
        assert got.n == 0 and got.e == 0 and (got.newid == -1).all() and got.browptr.tolist() == [0]


def test_batch_adjacency_and_prior_degrees():
    """the SubgraphBatch of a node set: coalesced by construction, equal to the dense cut, and its bdeg the prior degrees csr_candidates
    computes for the batch graph with its values, bit for bit (exact sums on both sides: see the file's docstring)"""
    import dgg_amd
    from dgg_amd import ops
    from dgg_amd.sampling import SubgraphBatch
    g = graph()
    dense = g["coo"].to_dense()
    for name in ("duplicates", "sixty_five", "all", "independent"):
        nodes = node_sets()[name]
        b = SubgraphBatch(ops.induced_subgraph(g["dev"][0], g["dev"][1], T(nodes), g["dev"][2]), g["dev"][2])
        idx = torch.from_numpy(np.unique(nodes)).long().to(DEV)
        assert b.adj.is_coalesced() and b.adj.dtype == torch.float32 and tuple(b.adj.shape) == (len(idx), len(idx))
        assert torch.equal(b.nodes, idx) and b.nodes.dtype == torch.int64
        assert torch.equal(b.adj.to_dense(), dense[idx][:, idx])
        assert torch.equal(b.edge_index, b.adj.indices()) and torch.equal(b.adj.values(), g["dev"][2][b.eid])
        # what a fresh coalesce() makes of the same entries is the same tensor: the flag does not lie
        fresh = torch.sparse_coo_tensor(b.edge_index, b.adj.values(), b.adj.shape).coalesce()
        assert torch.equal(fresh.indices(), b.adj.indices()) and torch.equal(fresh.values(), b.adj.values())
        rowptr, col, deg = dgg_amd.csr_candidates(b.adj)
        assert torch.equal(rowptr, b.sub.browptr) and torch.equal(col, b.sub.bcol) and torch.equal(deg, b.sub.bdeg)
        feats = torch.arange(R.N300 * 3, device=DEV).reshape(R.N300, 3)
        assert torch.equal(b.take(feats), feats[idx])


# ---- the samplers ----------------------------------------------------------------------------------------------------------------------
def test_random_walk_sampler_batches_are_the_walks_unique_nodes():
    import dgg_amd
    g = graph()
    rowptr, col, _ = g["host"]
    s = dgg_amd.RandomWalkSampler(g["coo"], batch_size=40, walk_length=3, num_steps=4, seed=11)
    for epoch in (0, 2):
        s.set_epoch(epoch)
        batches = list(s)
        assert len(batches) == len(s) == 4
        for step, b in enumerate(batches):
            roots = s.roots(step).numpy()
            want = np.unique(R.walk(rowptr, col, roots, 3, s.walk_seed(step)))
            assert np.array_equal(b.nodes.cpu().numpy(), want) and b.num_nodes == len(want)
            ref = R.induced(rowptr, col, want.astype(np.int32))
            assert np.array_equal(b.edge_index.cpu().numpy(), np.stack([ref["brow"], ref["bcol"]]).astype(np.int64))
            assert np.array_equal(b.eid.cpu().numpy(), ref["beid"])
    first = [b.nodes.tolist() for b in batches]
    assert first == [b.nodes.tolist() for b in s]                       # the same epoch again: the same batches
    s.set_epoch(3)
    assert first != [b.nodes.tolist() for b in s]


def test_cluster_sampler_covers_every_node_once():
    import dgg_amd
    g = graph()
    dense = g["coo"].to_dense()
    # 6 parts of 50, batches of 2: three full batches
    c = dgg_amd.ClusterSampler(g["coo"], dgg_amd.contiguous_parts(R.N300, 6), batch_size=2, seed=3)
    batches = list(c)
    assert len(batches) == len(c) == 3 and [b.num_nodes for b in batches] == [100, 100, 100]
    assert sorted(torch.cat([b.nodes for b in batches]).tolist()) == list(range(R.N300))
    for b in batches:                                                    # the edges BETWEEN the batch's clusters are kept
        assert torch.equal(b.adj.to_dense(), dense[b.nodes][:, b.nodes])
        part_of = dgg_amd.contiguous_parts(R.N300, 6).to(DEV)[b.nodes]
        assert bool((part_of[b.edge_index[0]] != part_of[b.edge_index[1]]).any())
    # 7 parts, batches of 2: the last batch is the short one (one cluster)
    parts = dgg_amd.contiguous_parts(R.N300, 7)
    c7 = dgg_amd.ClusterSampler(g["coo"], parts, batch_size=2, seed=3)
    b7 = list(c7)
    sizes = torch.bincount(parts).tolist()
    order = c7.cluster_order()
    assert len(b7) == len(c7) == 4 and [b.num_nodes for b in b7] == [sizes[order[0]] + sizes[order[1]], sizes[order[2]] + sizes[order[3]],
                                                                      sizes[order[4]] + sizes[order[5]], sizes[order[6]]]
    assert sorted(torch.cat([b.nodes for b in b7]).tolist()) == list(range(R.N300))
    c7.set_epoch(1)
    assert c7.cluster_order() != order and sorted(torch.cat([b.nodes for b in c7]).tolist()) == list(range(R.N300))


# ---- the harness -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planetoid_dir(tmp_path_factory):
    """the synthetic 700-node data set in the Planetoid file format that tests/test_adj_loss.py writes for the small-graph harness,
    built the same way (700 nodes: the public split the loader reads takes 500 validation nodes after the training set)"""
    import scipy.sparse as sp
    d_ = tmp_path_factory.mktemp("planetoid")
    rng = np.random.default_rng(0)
    N, d, C, n_train, n_test = 700, 40, 3, 30, 100
    y = rng.integers(0, C, N)
    X = (rng.random((N, d)) < 0.08).astype(np.float32)
    for c in range(C):
        X[y == c, c * 10:(c + 1) * 10] += (rng.random((int((y == c).sum()), 10)) < 0.5)
    onehot = np.eye(C, dtype=np.int32)[y]
    graph_ = defaultdict(list)
    for u in range(N):
        for v in rng.choice(np.flatnonzero(y == y[u]), 3):
            graph_[u].append(int(v))
        graph_[u].append(int(rng.integers(0, N)))                 # ... and inter-class edges for the target to drop
    n_all = N - n_test
    files = {"x": sp.csr_matrix(X[:n_train]), "y": onehot[:n_train], "allx": sp.csr_matrix(X[:n_all]), "ally": onehot[:n_all],
             "tx": sp.csr_matrix(X[n_all:]), "ty": onehot[n_all:], "graph": dict(graph_)}
    for k_, v in files.items():
        with open(d_ / f"ind.toy.{k_}", "wb") as f:
            pickle.dump(v, f)
    with open(d_ / "ind.toy.test.index", "w") as f:
        f.write("\n".join(str(i) for i in rng.permutation(np.arange(n_all, N))))
    return str(d_)


def graph_leaves(fn):
    """ids of the leaf tensors (parameters) the autograd graph below `fn` reaches: its AccumulateGrad nodes"""
    seen_, out, todo = set(), set(), [fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen_:
            continue
        seen_.add(f)
        if hasattr(f, "variable"):
            out.add(id(f.variable))
        todo += [g_ for g_, _ in f.next_functions]
    return out


# the generator's parameters that GCN_DGG's configuration in the harness uses (scorer u-v-deg: the edge encoders; k-net "x": the degree
# encoders and the mean / projection heads).  The class also declares the parameters of the scorers and k-nets that are switched off (t,
# k_W, edge_conv_*, input_degree_*, adj_project, signal_project, k_net.k_logvar, ...): no forward of this configuration reads them, so no
# loss can give them a gradient -- "every parameter has a non-zero gradient" is held for every parameter the learned adjacency depends on
# (found in the autograd graph, not from the gradients), and that set must hold at least these.
USED = ("node_encode_for_edges.0.weight", "node_encode_for_edges.0.bias", "edge_encode.0.weight", "edge_encode.0.bias", "edge_encode.2.weight",
        "edge_encode.2.bias", "node_encode_for_k.0.weight", "node_encode_for_k.0.bias", "k_embed.0.weight", "k_embed.0.bias", "k_net.k_mu.weight",
        "k_net.k_mu.bias", "k_net.k_project.weight", "k_net.k_project.bias")


def run_harness(monkeypatch, capsys, data_dir, extra):
    """-> (per-epoch losses, printed batch lines, epoch lines, [(sparse term, dense float64, dense float32)] per loss call, the models built,
    [{generator parameter: (the learned adjacency depends on it, largest gradient magnitude at the first optimiser step)}])"""
    import dgg_amd
    from dgg_amd import train_large_graphs as H
    seen, made, reach = [], [], []
    real_loss = H.adjacency_mse_loss

    def spy(out_adj, gt, *a, **k):
        if not reach:                                                 # the parameters the first batch's learned adjacency depends on
            reach.append(graph_leaves(out_adj.values().grad_fn))
        term = real_loss(out_adj, gt, *a, **k)
        with torch.no_grad():
            dense = torch.nn.functional.mse_loss(out_adj.to_dense().double(), gt.to_dense().double())
            dense32 = torch.nn.functional.mse_loss(out_adj.to_dense(), gt.to_dense().float())
        seen.append((float(term.detach()), float(dense), float(dense32)))
        return term
    monkeypatch.setattr(H, "adjacency_mse_loss", spy)
    real_init = dgg_amd.GCN_DGG.__init__
    monkeypatch.setattr(dgg_amd.GCN_DGG, "__init__", lambda self, *a_, **k_: (real_init(self, *a_, **k_), made.append(self))[0])
    grads = []
    real_step = torch.optim.Adam.step

    def step_spy(self, *a, **k):
        if made and not grads:                                        # the first step: every parameter of the generator, before the update
            grads.append({n_: (id(p_) in reach[0] if reach else None, None if p_.grad is None else float(p_.grad.abs().max()))
                          for n_, p_ in made[0].dggs[0].named_parameters()})
        return real_step(self, *a, **k)
    monkeypatch.setattr(torch.optim.Adam, "step", step_spy)
    capsys.readouterr()
    hist = H.main(["--data", "toy", "--data_dir", data_dir, "--model", "GCN_DGG", "--hidden", "16", "--epochs", "2", "--graphsaint_bs", "64",
                   "--graphsaint_wl", "2", "--num_steps", "3", "--cluster_parts", "7", "--cluster_bs", "2", "--print_batches", "true"] + extra)
    out = capsys.readouterr().out.splitlines()
    return hist, [ln for ln in out if ln.lstrip().startswith("batch:")], [ln for ln in out if ln.startswith("Epoch:")], seen, made, grads


@pytest.mark.parametrize("loader", ["SAINT", "Cluster"])
def test_harness_trains_on_batches(monkeypatch, capsys, planetoid_dir, loader):
    hist, batch_lines, epoch_lines, seen, made, grads = run_harness(monkeypatch, capsys, planetoid_dir, ["--dataloader", loader])
    n_batches = 2 * (3 if loader == "SAINT" else 4)
    print("\n".join(batch_lines + epoch_lines))
    assert len(hist) == 2 and all(np.isfinite(hist)) and len(epoch_lines) == 2
    assert len(batch_lines) == n_batches and len(seen) == n_batches
    assert all(np.isfinite(float(re.search(r" loss:(\S+)", ln).group(1))) for ln in batch_lines)
    assert made and made[0].differentiable_adj
    # the printed adjacency term of the first batch is the dense mse_loss of that batch, within the sparse kernel's bound
    printed = float(re.search(r"adj loss:(\S+)", batch_lines[0]).group(1))
    sparse, dense, dense32 = seen[0]
    print(f"{loader}: first batch adjacency term printed {printed!r} sparse {sparse!r} dense float64 {dense!r} dense float32 {dense32!r} "
          f"rel {abs(printed - dense) / dense:.3e} (bar {adj_loss_ref.RTOL:.3e})")
    assert dense32 > 0 and abs(printed - dense32) <= adj_loss_ref.RTOL * dense32, (printed, dense32)
    assert abs(printed - dense) <= adj_loss_ref.RTOL * dense, (printed, dense)           # ... and of the same in float64
    # every parameter of the generator got a non-zero gradient on the first step
    assert grads and grads[0], "no optimiser step was seen"
    print({n_: g_ for n_, g_ in grads[0].items()})
    assert all(grads[0][n_][0] for n_ in USED), [n_ for n_ in USED if not grads[0][n_][0]]
    for n_, (used, g_) in grads[0].items():
        assert (g_ is not None and g_ > 0 and np.isfinite(g_)) if used else g_ is None, (n_, used, g_)


@pytest.mark.parametrize("loader", ["SAINT", "Cluster"])
def test_harness_without_the_adjacency_term(monkeypatch, capsys, planetoid_dir, loader):
    hist, batch_lines, epoch_lines, seen, made, _ = run_harness(monkeypatch, capsys, planetoid_dir, ["--dataloader", loader, "--adj_loss_weight", "0"])
    assert len(hist) == 2 and all(np.isfinite(hist)) and not seen and "adj loss" not in " ".join(batch_lines + epoch_lines)
    assert made and not made[0].differentiable_adj
    assert 1 <= len(batch_lines) <= 2 * (3 if loader == "SAINT" else 4)      # batches without a training node are skipped
