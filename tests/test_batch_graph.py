"""The batch edit on the GPU: dgg_batch_graph_edit (ops.batch_graph_edit) against the numpy restatement tests/batch_graph_ref.py (itself
held against a dense construction by tests/test_batch_graph_host.py), SubgraphBatch.with_noise on top of it, and the harness
dgg_amd.train_large_graphs with --batch_noise device end to end.

Everything from the kernel is compared BIT FOR BIT: the outputs are integers and copies of stored float32 values.  Shapes: n = 1, 2, 63,
64, 65, 130, 300 (one lane, both sides of the 64-column window, three and five windows, more than one workgroup of four rows); p = 0,
0.0014 (the reference's default level), 0.5 (rows of more than 64 noisy entries at 130 and 300 nodes, hits that fall on stored
entries) and 1; the five graphs of batch_graph_ref.graph.
The harness: losses finite; the printed adjacency term of the first batch within adj_loss_ref.RTOL = 2^-22 (relative) of the dense
float64 F.mse_loss against remove_interclass_edges of the batch's noisy graph, the bound tests/test_adj_loss.py holds the kernel to."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import adj_loss_ref
import batch_graph_ref as R
from test_subgraph import USED, graph_leaves, planetoid_dir  # noqa: F401  (the 700-node toy data set and the autograd-graph walk)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED = (42, 65537)
PS = (0.0, 0.0014, 0.5, 1.0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def reference(name, n, p):
    """the graph and the restatement's noisy graph for it (computed once, never changed)"""
    rowptr, col, values = R.graph(name, n)
    return (rowptr, col, values), R.edit(rowptr, col, values, R.threshold(p), SEED)


def target_of(want, lab):
    """the target of the restatement's noisy graph under labels `lab` (tests/test_batch_graph_host.py holds R.edit's own to the dense
    mask; this is the same filter on its COO arrays)"""
    keep = lab[want["nrow"]] == lab[want["ncol"]]
    trowptr = np.zeros(want["n"] + 1, np.int64)
    np.cumsum(np.bincount(want["nrow"][keep], minlength=want["n"]), out=trowptr[1:])
    return dict(trowptr=trowptr, tcol=want["ncol"][keep], trow=want["nrow"][keep], e_t=int(keep.sum()))


def ascending_within_rows(rowptr, col):
    rp, c = rowptr.cpu().numpy(), col.cpu().numpy()
    return all((np.diff(c[rp[i]:rp[i + 1]]) > 0).all() for i in range(len(rp) - 1))


NOISY = (("nrowptr", torch.int64), ("ncol", torch.int32), ("nrow", torch.int32), ("nval", torch.float32), ("nsrc", torch.int64))
TARGET = (("trowptr", torch.int64), ("tcol", torch.int32), ("trow", torch.int32))


# ---- the kernel against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.GRAPHS)
@pytest.mark.parametrize("n", R.SIZES)
def test_edit_matches_the_restatement(n, name):
    from dgg_amd import ops
    for p in PS:
        (rowptr, col, values), want = reference(name, n, p)
        dev = (T(rowptr), T(col), T(values))
        for kind in R.LABELS:
            lab = R.labels(kind, n)
            reads = ops.BATCH_EDIT_READBACKS
            got = ops.batch_graph_edit(*dev, p, SEED, None if lab is None else T(lab))
            assert ops.BATCH_EDIT_READBACKS == reads + 1
            again = ops.batch_graph_edit(*dev, p, SEED, None if lab is None else T(lab))
            what = (n, name, p, kind)
            assert (got.n, got.e) == (n, want["e"]), what
            for k_, dt in NOISY:
                a = getattr(got, k_)
                assert a.dtype == dt and np.array_equal(a.cpu().numpy(), want[k_]), (what, k_)
                assert torch.equal(a, getattr(again, k_)), (what, k_)                      # the same bits on every run
            assert ascending_within_rows(got.nrowptr, got.ncol), what
            if lab is None:
                assert got.trowptr is None and got.tcol is None and got.trow is None and got.e_t == 0
                continue
            tw = target_of(want, lab)
            assert got.e_t == tw["e_t"], what
            for k_, dt in TARGET:
                a = getattr(got, k_)
                assert a.dtype == dt and np.array_equal(a.cpu().numpy(), tw[k_]), (what, k_)
                assert torch.equal(a, getattr(again, k_)), (what, k_)
            assert ascending_within_rows(got.trowptr, got.tcol), what
            if kind == "equal":
                assert torch.equal(got.tcol, got.ncol) and torch.equal(got.trowptr, got.nrowptr)
            if kind == "different":                                                        # only stored diagonal entries survive
                assert torch.equal(got.tcol, got.trow) and got.e_t == int((col == np.repeat(np.arange(n), np.diff(rowptr))).sum())
        if p == 0.0:
            assert torch.equal(got.ncol, dev[1]) and torch.equal(got.nrowptr, dev[0]) and torch.equal(got.nval, dev[2])
            assert torch.equal(got.nsrc, torch.arange(col.size, device=DEV))
        if p == 1.0:
            diag = int((col == np.repeat(np.arange(n), np.diff(rowptr))).sum())
            assert got.e == n * (n - 1) + diag
        if p == 0.5 and n >= 130:
            assert int(np.bincount(want["nrow"][want["nsrc"] < 0]).max()) > 64             # rows of more than 64 noisy entries


def test_label_dtypes_and_refused_arguments():
    from dgg_amd import ops
    (rowptr, col, values), want = reference("random", 65, 0.5)
    dev = (T(rowptr), T(col), T(values))
    lab = R.labels("three", 65)
    tw = target_of(want, lab)
    for dt in (torch.int64, torch.int32, torch.int16, torch.uint8):
        got = ops.batch_graph_edit(*dev, 0.5, SEED, torch.from_numpy(lab).to(dt).to(DEV))
        assert np.array_equal(got.tcol.cpu().numpy(), tw["tcol"]) and np.array_equal(got.trowptr.cpu().numpy(), tw["trowptr"])
    got = ops.batch_graph_edit(*dev, 0.5, SEED, torch.from_numpy(lab))                    # labels on the host are moved
    assert np.array_equal(got.tcol.cpu().numpy(), tw["tcol"])
    reads = ops.BATCH_EDIT_READBACKS
    for bad_p in (-0.1, 1.5):
        with pytest.raises(ValueError, match="p must be"):
            ops.batch_graph_edit(*dev, bad_p, SEED)
    with pytest.raises(ValueError, match="labels"):
        ops.batch_graph_edit(*dev, 0.5, SEED, T(lab[:-1]))
    with pytest.raises(ValueError, match="labels"):
        ops.batch_graph_edit(*dev, 0.5, SEED, T(lab.astype(np.float32)))
    assert ops.BATCH_EDIT_READBACKS == reads                                               # refused before anything was launched or read
    other = ops.batch_graph_edit(*dev, 0.5, (SEED[0], SEED[1] + 1))
    assert not torch.equal(other.ncol, T(want["ncol"]))


# ---- broken graphs -------------------------------------------------------------------------------------------------------------------
GUARD = 64


def broken_graphs():
    """n = 130; the random graph with one thing wrong in row 70 (or in the last row's range)"""
    rowptr, col, values = R.graph("random", 130)
    p0 = int(rowptr[70])
    desc, big, equal, past = col.copy(), col.copy(), col.copy(), rowptr.copy()
    desc[[p0, p0 + 1]] = desc[[p0 + 1, p0]]                               # a descending pair
    equal[p0 + 1] = equal[p0]                                             # ... an equal pair: not STRICTLY ascending
    big[int(rowptr[71]) - 1] = 130                                        # a column equal to n
    past[-1] += 5                                                         # a rowptr past E
    neg = rowptr.copy()
    neg[70] = -1
    return dict(descending=(rowptr, desc, values), equal=(rowptr, equal, values), column_n=(rowptr, big, values), rowptr_past_E=(past, col, values),
                rowptr_negative=(neg, col, values))


def guarded(count, dtype, fill):
    buf = torch.full((count + 2 * GUARD,), fill, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + count]


def guards_intact(buf, count, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + count:] == fill).all())


@pytest.mark.parametrize("name", ["descending", "equal", "column_n", "rowptr_past_E", "rowptr_negative"])
def test_a_broken_graph_is_refused_and_nothing_is_written_outside_the_outputs(name):
    """through ops: ValueError after the one read-back.  Through the entry itself, both phases on the broken graph with the prefix sums
    of the intact one: the status word is set, the broken row counts 0 and every word around every output array keeps its value"""
    import dgg_amd
    from dgg_amd import ops
    rowptr, col, values = broken_graphs()[name]
    good = R.graph("random", 130)
    n, E, p = 130, col.size, 0.5
    lab = T(R.labels("three", n).astype(np.int32))
    cbuf, dcol = guarded(E, torch.int32, 0)                               # (col itself sits between guard words: a row range past E stays inside)
    dcol.copy_(T(col))
    drp, dval = T(rowptr), T(values)
    with pytest.raises(ValueError, match="batch_graph_edit"):
        ops.batch_graph_edit(drp, dcol, dval, p, SEED, lab)
    with pytest.raises(ValueError, match="batch_graph_edit"):
        ops.batch_graph_edit(drp, dcol, dval, 0.0, SEED)
    ok = ops.batch_graph_edit(T(good[0]), T(good[1]), T(good[2]), p, SEED, lab)            # the intact graph: its prefix sums and sizes
    L = dgg_amd._lib.lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    FILLS = dict(ndeg=-7, tdeg=-7, ncol=-7, nrow=-7, nval=-7.0, nsrc=-7, tcol=-7, trow=-7, status=0)
    bufs = {k_: guarded(c_, dt, FILLS[k_]) for k_, c_, dt in (
        ("ndeg", n, torch.int32), ("tdeg", n, torch.int32), ("ncol", ok.e, torch.int32), ("nrow", ok.e, torch.int32), ("nval", ok.e, torch.float32),
        ("nsrc", ok.e, torch.int64), ("tcol", ok.e_t, torch.int32), ("trow", ok.e_t, torch.int32), ("status", 1, torch.int32))}
    v = {k_: b[1] for k_, b in bufs.items()}
    thr = ops.noise_threshold(p)

    def call(phase):
        return L.dgg_batch_graph_edit(phase, ptr(drp), ptr(dcol), ptr(dval), n, E, ptr(lab), SEED[0], SEED[1], thr, ptr(v["ndeg"]), ptr(v["tdeg"]),
                                      ptr(ok.nrowptr), ok.e, ptr(v["ncol"]), ptr(v["nrow"]), ptr(v["nval"]), ptr(v["nsrc"]), ptr(ok.trowptr), ok.e_t,
                                      ptr(v["tcol"]), ptr(v["trow"]), ptr(v["status"]), st)
    assert call(ops.BATCH_EDIT_COUNT) == 0
    torch.cuda.synchronize()
    assert int(v["status"]) == 1
    bad_row = 129 if name == "rowptr_past_E" else (69 if name == "rowptr_negative" else 70)
    assert int(v["ndeg"][bad_row]) == 0 and int(v["tdeg"][bad_row]) == 0
    if name == "rowptr_negative":                                         # rows 69 and 70 both have a bound that is no position
        assert int(v["ndeg"][70]) == 0
    rest = [i for i in range(n) if i not in (bad_row, 70)]
    assert torch.equal(v["ndeg"][rest].long(), (ok.nrowptr[1:] - ok.nrowptr[:-1])[rest])   # every other row counts what it counted
    v["status"].zero_()
    assert call(ops.BATCH_EDIT_FILL) == 0
    torch.cuda.synchronize()
    assert int(v["status"]) == 1
    for k_, (buf, view) in bufs.items():
        assert guards_intact(buf, view.shape[0], FILLS[k_]), k_
    assert guards_intact(cbuf, E, 0)
    q0, q1 = int(ok.nrowptr[bad_row]), int(ok.nrowptr[bad_row + 1])
    assert (v["ncol"][q0:q1] == -7).all() and (v["nsrc"][q0:q1] == -7).all()                # the skipped row's slots were left alone
    r0 = 0 if bad_row != 0 else 1
    assert torch.equal(v["ncol"][int(ok.nrowptr[r0]):int(ok.nrowptr[r0 + 1])], ok.ncol[int(ok.nrowptr[r0]):int(ok.nrowptr[r0 + 1])])


def test_prefix_sums_of_another_seed_are_reported_and_stay_inside_the_outputs():
    import dgg_amd
    from dgg_amd import ops
    rowptr, col, values = R.graph("random", 130)
    n, E, p = 130, col.size, 0.5
    drp, dcol, dval = T(rowptr), T(col), T(values)
    ok = ops.batch_graph_edit(drp, dcol, dval, p, SEED)
    L = dgg_amd._lib.lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    bufs = {k_: guarded(ok.e, dt, -7) for k_, dt in (("ncol", torch.int32), ("nrow", torch.int32), ("nval", torch.float32), ("nsrc", torch.int64))}
    status = torch.zeros(1, device=DEV, dtype=torch.int32)
    rc = L.dgg_batch_graph_edit(ops.BATCH_EDIT_FILL, ptr(drp), ptr(dcol), ptr(dval), n, E, None, SEED[0], SEED[1] + 1, ops.noise_threshold(p), None, None,
                                ptr(ok.nrowptr), ok.e, ptr(bufs["ncol"][1]), ptr(bufs["nrow"][1]), ptr(bufs["nval"][1]), ptr(bufs["nsrc"][1]), None, 0,
                                None, None, ptr(status), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and int(status) == 1
    assert all(guards_intact(buf, ok.e, -7) for buf, _ in bufs.values())
    rp = ok.nrowptr.cpu().numpy()
    nrow = bufs["nrow"][1].cpu().numpy()
    for i in range(n):                                                   # what was written landed in its own row's slots
        assert set(nrow[rp[i]:rp[i + 1]].tolist()) <= {i, -7}


# ---- with_noise ----------------------------------------------------------------------------------------------------------------------
def whole_graph_batch(name, n):
    from dgg_amd import ops
    from dgg_amd.sampling import SubgraphBatch
    rowptr, col, values = R.graph(name, n)
    dv = T(values)
    return SubgraphBatch(ops.induced_subgraph(T(rowptr), T(col), torch.arange(n, device=DEV, dtype=torch.int32), dv), dv, step=0), (rowptr, col, values)


@pytest.mark.parametrize("name,n", [("random", 300), ("selfloops", 130), ("edges", 300), ("empty", 65)])
def test_with_noise_dresses_the_edit(name, n, monkeypatch):
    import dgg_amd
    import dgg_amd.data as D
    from dgg_amd import adjacency
    batch, (rowptr, col, values) = whole_graph_batch(name, n)
    level = 0.03                                                         # p = 0.3
    thr = R.threshold(10 * level)
    lab = R.labels("three", n)
    noisy, pattern, target = R.dense(rowptr, col, values, thr, SEED, lab)
    calls = []
    real_coalesce, real_convert = torch.Tensor.coalesce, torch._convert_indices_from_coo_to_csr
    monkeypatch.setattr(torch.Tensor, "coalesce", lambda self: (calls.append("coalesce"), real_coalesce(self))[1])
    monkeypatch.setattr(torch, "_convert_indices_from_coo_to_csr", lambda *a, **k: (calls.append("coo->csr"), real_convert(*a, **k))[1])
    ed = batch.with_noise(level, SEED, labels=T(lab))
    rp, cc, deg = dgg_amd.csr_candidates(ed.adj)
    rp2, cc2, er2 = dgg_amd.csr_pattern(ed.adj)
    assert calls == [], calls                                            # the first use of adj coalesced and converted nothing
    assert rp is ed.edit.nrowptr and cc is ed.edit.ncol and rp2 is ed.edit.nrowptr and cc2 is ed.edit.ncol and er2 is ed.edit.nrow
    assert adjacency._cached("values_f32", ed.adj, lambda: None) is ed.edit.nval
    fresh = torch.sparse_coo_tensor(ed.edge_index.clone(), ed.adj.values().clone(), ed.adj.shape)     # the unseeded functions on a fresh copy
    frp, fcc, fdeg = dgg_amd.csr_candidates(fresh)
    assert "coalesce" in calls and "coo->csr" in calls
    monkeypatch.undo()
    assert torch.equal(frp, rp) and torch.equal(fcc, cc) and torch.equal(fdeg, deg) and deg.dtype == torch.float32
    fp = dgg_amd.csr_pattern(fresh)
    assert all(torch.equal(a, b) for a, b in zip(fp, (rp2, cc2, er2)))
    # the tensors
    assert ed.adj.is_coalesced() and ed.adj.dtype == torch.float32 and tuple(ed.adj.shape) == (n, n)
    assert np.array_equal(ed.adj.to_dense().cpu().numpy(), noisy)
    co = fresh.coalesce()                                                # the flag does not lie
    assert torch.equal(co.indices(), ed.adj.indices()) and torch.equal(co.values(), ed.adj.values())
    assert torch.equal(ed.edge_index, ed.adj.indices()) and ed.num_edges == int(pattern.sum()) and ed.num_nodes == n and ed.step == 0
    assert torch.equal(ed.nodes, batch.nodes) and torch.equal(ed.take(T(lab)), T(lab))
    want_t = D.remove_interclass_edges(ed.adj, T(lab)).to_dense()
    assert torch.equal(ed.target.to_dense(), want_t) and np.array_equal(want_t.cpu().numpy(), target)
    assert isinstance(ed.target, dgg_amd.CsrAdjacency) and (ed.target.values() == 1).all() and ed.target.values().dtype == torch.float32
    # eid / is_noise against the source batch
    assert ed.is_noise.dtype == torch.bool and int((~ed.is_noise).sum()) == batch.num_edges
    assert torch.equal(ed.eid[~ed.is_noise], batch.eid) and (ed.eid[ed.is_noise] == -1).all()
    assert torch.equal(ed.edge_index[:, ~ed.is_noise], batch.edge_index) and torch.equal(ed.adj.values()[~ed.is_noise], batch.adj.values())
    assert (ed.adj.values()[ed.is_noise] == 1).all() and int(ed.is_noise.sum()) == int(pattern.sum()) - col.size
    assert batch.with_noise(level, SEED).target is None


# ---- the harness -----------------------------------------------------------------------------------------------------------------------
ARGS = ["--data", "toy", "--model", "GCN_DGG", "--hidden", "16", "--epochs", "2", "--graphsaint_bs", "64", "--graphsaint_wl", "2", "--num_steps", "3",
        "--cluster_parts", "7", "--cluster_bs", "2", "--print_batches", "true"]


def run_device(monkeypatch, capsys, data_dir, extra):
    """the harness with --batch_noise device -> dict(hist, batch lines, [(printed-term source, dense float64)] per loss call, the edits
    seen [(labels given, target built, cut read-backs, edit read-backs before / after)], generator gradients at the first step)"""
    import dgg_amd
    import dgg_amd.data as D
    from dgg_amd import ops
    from dgg_amd import train_large_graphs as H
    from dgg_amd.sampling import SubgraphBatch
    state = dict(training=False, last=None)
    seen, edits, made, reach, grads = [], [], [], [], []
    real_remove, real_noisy = D.remove_interclass_edges, D.add_noisy_edges

    def host_only(real, what):
        def f(*a, **k):
            if state["training"]:
                raise AssertionError(f"{what} was called for a training batch")
            return real(*a, **k)
        return f
    monkeypatch.setattr(D, "add_noisy_edges", host_only(real_noisy, "data.add_noisy_edges"))
    monkeypatch.setattr(D, "remove_interclass_edges", host_only(real_remove, "data.remove_interclass_edges"))
    real_train = H.train_gcn_dgg

    def train(*a, **k):
        state["training"] = True
        try:
            return real_train(*a, **k)
        finally:
            state["training"] = False
    monkeypatch.setattr(H, "train_gcn_dgg", train)
    real_with_noise = SubgraphBatch.with_noise
    base = (ops.SUBGRAPH_READBACKS, ops.BATCH_EDIT_READBACKS)

    def with_noise(self, noise_level, seed, labels=None):
        before = ops.BATCH_EDIT_READBACKS - base[1]
        ed = real_with_noise(self, noise_level, seed, labels=labels)
        edits.append(dict(labels=labels is not None, target=ed.target is not None, cuts=ops.SUBGRAPH_READBACKS - base[0], before=before,
                          after=ops.BATCH_EDIT_READBACKS - base[1], level=noise_level, seed=seed, step=self.step))
        state["last"] = (ed, labels)
        return ed
    monkeypatch.setattr(SubgraphBatch, "with_noise", with_noise)
    real_loss = H.adjacency_mse_loss

    def loss_spy(out_adj, gt, *a, **k):
        ed, labels = state["last"]
        assert gt is ed.target
        if not reach:
            reach.append(graph_leaves(out_adj.values().grad_fn))
        term = real_loss(out_adj, gt, *a, **k)
        with torch.no_grad():
            dense = torch.nn.functional.mse_loss(out_adj.to_dense().double(), real_remove(ed.adj, labels).to_dense().double())
        seen.append((float(term.detach()), float(dense)))
        return term
    monkeypatch.setattr(H, "adjacency_mse_loss", loss_spy)
    real_init = dgg_amd.GCN_DGG.__init__
    monkeypatch.setattr(dgg_amd.GCN_DGG, "__init__", lambda self, *a_, **k_: (real_init(self, *a_, **k_), made.append(self))[0])
    real_step = torch.optim.Adam.step

    def step_spy(self, *a, **k):
        if made and not grads:
            grads.append({n_: (id(p_) in reach[0] if reach else None, None if p_.grad is None else float(p_.grad.abs().max()))
                          for n_, p_ in made[0].dggs[0].named_parameters()})
        return real_step(self, *a, **k)
    monkeypatch.setattr(torch.optim.Adam, "step", step_spy)
    capsys.readouterr()
    hist = H.main(ARGS + ["--data_dir", data_dir, "--batch_noise", "device"] + extra)
    out = capsys.readouterr().out.splitlines()
    return dict(hist=hist, batches=[ln for ln in out if ln.lstrip().startswith("batch:")], epochs=[ln for ln in out if ln.startswith("Epoch:")],
                seen=seen, edits=edits, made=made, grads=grads)


@pytest.mark.parametrize("loader", ["SAINT", "Cluster"])
def test_harness_trains_with_the_device_edit(monkeypatch, capsys, planetoid_dir, loader):  # noqa: F811
    r = run_device(monkeypatch, capsys, planetoid_dir, ["--dataloader", loader])
    n_batches = 2 * (3 if loader == "SAINT" else 4)
    print("\n".join(r["batches"] + r["epochs"]))
    assert len(r["hist"]) == 2 and all(np.isfinite(r["hist"])) and len(r["epochs"]) == 2
    assert len(r["batches"]) == n_batches and len(r["seen"]) == n_batches and len(r["edits"]) == n_batches
    assert all(np.isfinite(float(re.search(r" loss:(\S+)", ln).group(1))) for ln in r["batches"])
    # one cut read-back and one edit read-back per batch, labels given, a target built, the default noise level, each step its own seed
    for k_, e in enumerate(r["edits"]):
        assert (e["cuts"], e["before"], e["after"]) == (k_ + 1, k_, k_ + 1), (k_, e)
        assert e["labels"] and e["target"] and e["level"] == 0.00014 and e["step"] == k_ % (n_batches // 2)
    assert len({e["seed"] for e in r["edits"]}) == n_batches
    # the printed adjacency term of the first batch is the dense float64 mse_loss against remove_interclass_edges(batch_adj, y_b)
    printed = float(re.search(r"adj loss:(\S+)", r["batches"][0]).group(1))
    sparse, dense = r["seen"][0]
    print(f"{loader}: first batch adjacency term printed {printed!r} sparse {sparse!r} dense float64 {dense!r} rel {abs(printed - dense) / dense:.3e} "
          f"(bar {adj_loss_ref.RTOL:.3e})")
    assert dense > 0 and abs(printed - dense) <= adj_loss_ref.RTOL * dense, (printed, dense)
    # the generator's used parameters got non-zero gradients on the first step
    assert r["made"] and r["made"][0].differentiable_adj and r["grads"] and r["grads"][0], "no optimiser step was seen"
    g = r["grads"][0]
    assert all(g[n_][0] for n_ in USED), [n_ for n_ in USED if not g[n_][0]]
    for n_, (used, g_) in g.items():
        assert (g_ is not None and g_ > 0 and np.isfinite(g_)) if used else g_ is None, (n_, used, g_)


@pytest.mark.parametrize("loader", ["SAINT", "Cluster"])
def test_harness_device_edit_without_the_adjacency_term_builds_no_target(monkeypatch, capsys, planetoid_dir, loader):  # noqa: F811
    r = run_device(monkeypatch, capsys, planetoid_dir, ["--dataloader", loader, "--adj_loss_weight", "0"])
    assert len(r["hist"]) == 2 and all(np.isfinite(r["hist"])) and not r["seen"] and "adj loss" not in " ".join(r["batches"] + r["epochs"])
    assert r["edits"] and all(not e["labels"] and not e["target"] for e in r["edits"])
    assert r["made"] and not r["made"][0].differentiable_adj


# the per-epoch training losses of the UNCHANGED host path: recorded from the parent commit's package (the code before --batch_noise
# existed) in the session that added the flag, on an MI355X; two runs of the parent's code and two of this tree's default path in fresh
# processes gave these same bits.  The step is NOT bit-reproducible from one process state to another, though (inside the whole suite the
# second epoch of the Cluster run came out 2e-9 away: sums of float32 terms whose order is not fixed), so the bar is a float32 one,
# written down before the comparison: every batch loss is a float32 value (one rounding: 2^-24 relative), an epoch's figure is a mean of
# 3 or 4 of them, and the second epoch sits behind at most 4 optimiser steps whose reordered sums each move it by a few units of that
# rounding -- HOST_RTOL = 2^-17 = 128 such units.  Anything the flag could break (another noise realisation, another target, a missed
# edge) moves the loss in its third digit: the adjacency term, weighted 10 000, is 65 of the 67.
HOST_RTOL = 2.0 ** -17
HOST_RECORDED = {
    "SAINT": [67.6829776763916, 66.20014230828536],
    "Cluster": [44.17157005541252, 54.446934671112984],
}


@pytest.mark.parametrize("flag", [[], ["--batch_noise", "host"]], ids=["default", "host"])
@pytest.mark.parametrize("loader", ["SAINT", "Cluster"])
def test_harness_host_path_gives_the_parent_commits_losses(capsys, planetoid_dir, loader, flag):  # noqa: F811
    from dgg_amd import train_large_graphs as H
    hist = H.main(ARGS + ["--data_dir", planetoid_dir, "--dataloader", loader] + flag)
    capsys.readouterr()
    print(loader, [repr(v) for v in hist])
    want = HOST_RECORDED[loader]
    print(loader, [abs(h - w) / w for h, w in zip(hist, want)], "bar", HOST_RTOL)
    assert len(hist) == len(want) and all(abs(h - w) <= HOST_RTOL * w for h, w in zip(hist, want)), (hist, want)
