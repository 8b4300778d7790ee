"""train_stats/* on the GPU: dgg_adj_diff_stats (ops.adj_diff_stats) against the float64 restatement of get_adj_diff_stats
(tests/adj_stats_ref.py, itself held against the reference's scalars by tests/test_adj_stats_host.py), against the scalars the reference
wrote (fixtures adj_stats_{a,b,c}.npz), and the modules that log through it: DGG_LearnableK_debug / GCN_DGG with a recording writer,
on the fused layer (args.dgg_writer_fused) and on the separate modules.

Tolerance: adj_stats_ref.RTOL = 2^-22 relative per scalar (derived there: double accumulation leaves the one float32 rounding of the
stored result, 2^-24, and a square root taken in double), NaN matching NaN; against the reference's scalars the fixture's recorded
|reference - float64| is added.  Shapes: 130 rows (not a multiple of the 4 rows of a workgroup), graph rows of 0, 1, 63, 64, 65 and 130
entries (both sides of the 64-entry walk of the input row), K = 64 and 32, chunked rows of 1, 2 and 3 chunks with trailing empty chunks."""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

import adj_stats_ref as R
from helpers import load_fixture

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROWS = 130
GRAPH_LENS = (0, 1, 63, 64, 65, 130)          # entries of the first six graph rows


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr_of(A_stored, vals):
    """A_stored [n,n] bool: which pairs the graph stores; vals [n,n] float32 -> (rowptr int64, col int32, aval float32) on the device"""
    n = A_stored.shape[0]
    r, c = np.nonzero(A_stored)                                    # row-major: columns ascending within a row
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    col, av = c.astype(np.int32), vals[r, c].astype(np.float32)
    if col.size == 0:
        col, av = np.zeros(1, np.int32), np.zeros(1, np.float32)
    return T(rowptr), T(col), T(av)


@functools.lru_cache(maxsize=None)
def problem(K, chunked=False, seed=0):
    """-> dict(stored, A, slots = per-row list of (column, w) in slot order with column -1 for an empty slot, k): the awkward cases of the
    module docstring.  Row widths: K slots (list) or 64 * (1, 2, 3 cycling) slots (chunked)."""
    rng = np.random.default_rng(100 + seed + K + 7 * chunked)
    n = ROWS
    lens = np.concatenate([GRAPH_LENS, rng.integers(0, 24, n - len(GRAPH_LENS))])
    stored = np.zeros((n, n), bool)
    for i, L in enumerate(lens):
        stored[i, rng.choice(n, L, replace=False)] = True
    A = np.where(stored, (2.0 * (1.0 - rng.random((n, n)))).astype(np.float32), np.float32(0))       # (0, 2]
    # stored zeros (the same as absent) and stored negatives (in neither population), some under learned entries (forced below)
    A[4, np.nonzero(stored[4])[0][:3]] = 0.0
    A[5, np.nonzero(stored[5])[0][10:13]] = 0.0
    A[3, np.nonzero(stored[3])[0][5]] = -0.5
    A[5, np.nonzero(stored[5])[0][20]] = -1.25
    slots = []
    for i in range(n):
        width = 64 * (1 + i % 3) if chunked else K
        m = int(rng.integers(0, width + 1)) if i >= 8 else width - 3                # learned entries of the row
        m = min(m, n)
        in_graph = np.nonzero(stored[i])[0]
        take = in_graph[rng.random(in_graph.size) < 0.6][:m]                         # part of the input row is selected, part is not
        if i == 4:
            take = np.union1d(take, in_graph[:3])[:m]                                # the stored zeros of row 4 under learned entries
        if i == 3:
            take = np.union1d(take, in_graph[5:6])[:m]                               # ... and its stored negative
        rest = np.setdiff1d(np.arange(n), take)
        cols = np.concatenate([take, rng.choice(rest, m - take.size, replace=False)]).astype(np.int64)
        w = rng.random(m).astype(np.float32)
        w[rng.random(m) < 0.1] = 0.0                                                 # selected with weight exactly 0
        if i == 2 and take.size:                                                     # a == w exactly: d == 0, in no population
            w[0] = A[i, cols[0]]
        row = [(-1, np.float32(7.0))] * width                                        # empty slots hold a value nobody may read
        for s_, c_, w_ in zip(rng.choice(width, m, replace=False), cols, w):
            row[s_] = (int(c_), w_)
        slots.append(row)
    k = (1.0 + 30.0 * rng.random(n)).astype(np.float32)
    W = np.zeros((n, n), np.float32)                               # the learned adjacency, dense
    for i, row in enumerate(slots):
        for c_, w_ in row:
            if c_ >= 0:
                W[i, c_] = w_
    return dict(stored=stored, A=A, slots=slots, k=k, n=n, W=W)


def arrays(p, K, chunked, trailing=2):
    """the problem as the kernel takes it -> (idx, w, layout or None), W dense"""
    from dgg_amd import ops
    n, W = p["n"], p["W"]
    flat = [np.array(row, dtype=[("c", np.int32), ("w", np.float32)]) for row in p["slots"]]
    if not chunked:
        idx = np.stack([f["c"] for f in flat])
        w = np.stack([f["w"] for f in flat])
        assert idx.shape == (n, K)
        return (T(idx), T(w)), W
    cnt = np.array([len(f) // 64 for f in flat])
    cptr = np.zeros(n + 1, np.int32)
    np.cumsum(cnt, out=cptr[1:])
    idx = np.concatenate([f["c"] for f in flat] + [np.arange(64 * trailing, dtype=np.int32) % n]).reshape(-1, 64)      # trailing chunks: nobody's
    w = np.concatenate([f["w"] for f in flat] + [np.full(64 * trailing, 3.0, np.float32)]).reshape(-1, 64)
    cnode = np.concatenate([np.repeat(np.arange(n), cnt), np.full(trailing, n - 1)]).astype(np.int32)
    lay = ops.ChunkLayout(T(cptr), T(cnode), None, idx.shape[0], int(cnt.max()), n)
    assert lay.wide
    return (T(idx), T(w), lay), W


def run(arrs, graph, k):
    from dgg_amd import ops
    out = ops.adj_diff_stats(arrs, graph, T(k))
    torch.cuda.synchronize()
    return out


def as_dict(out):
    return dict(zip(R.FIELDS, out.cpu().numpy().astype(np.float64)))


@pytest.mark.parametrize("K,chunked", [(64, False), (32, False), (64, True)], ids=["K64", "K32", "chunked"])
def test_kernel_matches_the_float64_restatement(K, chunked):
    p = problem(K, chunked)
    arrs, W = arrays(p, K, chunked)
    # the awkward cases are really there
    assert tuple(p["stored"][:6].sum(1)) == GRAPH_LENS
    assert ((p["A"] == 0) & p["stored"] & (W != 0)).any(), "a stored zero under a learned entry"
    assert ((p["A"] < 0) & (W != 0)).any() and ((p["A"] > 0) & (p["A"] == W)).any()
    assert any(c_ >= 0 and w_ == 0 for row in p["slots"] for c_, w_ in row) and any(c_ < 0 for row in p["slots"] for c_, w_ in row)
    assert ((p["A"] > 0) & (W == 0)).any(), "input edges the generator did not select"
    out = run(arrs, csr_of(p["stored"], p["A"]), p["k"])
    want = R.stats_dense(p["A"], W, p["k"])
    assert want["on_n"] > 100 and want["off_n"] > 100
    R.assert_fields(as_dict(out), want, what=f"K={K} chunked={chunked}")
    assert as_dict(out)["on_n"] == want["on_n"] and as_dict(out)["off_n"] == want["off_n"]


def test_two_launches_give_the_same_bits():
    for K, chunked in ((64, False), (64, True)):
        p = problem(K, chunked)
        arrs, _ = arrays(p, K, chunked)
        g = csr_of(p["stored"], p["A"])
        a, b = run(arrs, g, p["k"]), run(arrs, g, p["k"])
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n_off", [0, 1])
def test_degenerate_off_edge_populations(n_off):
    n = ROWS
    rng = np.random.default_rng(5)
    stored = rng.random((n, n)) < 0.1
    A = np.where(stored, np.float32(1.0), np.float32(0))
    idx = np.full((n, 64), -1, np.int32)
    w = np.zeros((n, 64), np.float32)
    for i in range(n):
        c = np.nonzero(stored[i])[0][:40:2]                        # every learned entry is an input edge
        idx[i, :c.size], w[i, :c.size] = c, 0.25 + 0.5 * rng.random(c.size)
    if n_off:
        j = int(np.nonzero(~stored[77])[0][0])
        idx[77, 63], w[77, 63] = j, 0.375
    W = np.zeros((n, n), np.float32)
    r_, s_ = np.nonzero(idx >= 0)
    W[r_, idx[r_, s_]] = w[r_, s_]
    k = (2.0 + rng.random(n)).astype(np.float32)
    got = as_dict(run((T(idx), T(w)), csr_of(stored, A), k))
    want = R.stats_dense(A, W, k)
    assert want["off_n"] == n_off and np.isnan(want["off_std"]) and np.isnan(want["off_mean"]) == (n_off == 0)
    R.assert_fields(got, want, what=f"off-edge population of {n_off}")
    if n_off:
        assert got["off_mean"] == -0.375


def test_no_rows():
    from dgg_amd import ops
    e = lambda dt, *s: torch.empty(s, device=DEV, dtype=dt)  # noqa: E731
    out = ops.adj_diff_stats((e(torch.int32, 0, 64), e(torch.float32, 0, 64)), (torch.zeros(1, device=DEV, dtype=torch.int64), e(torch.int32, 0), e(torch.float32, 0)),
                             e(torch.float32, 0))
    got = as_dict(out)
    assert got["on_n"] == 0 and got["off_n"] == 0
    assert all(np.isnan(got[f]) for f in R.FIELDS if f not in ("on_n", "off_n")), got


def test_tiny_spread_keeps_the_std():
    """every d = 1 - eps_i with eps_i ~ 1e-4: a float32 accumulation, or sum / sum of squares in any precision short of double, loses
    the std (spread ~3e-5 on a mean of 1: the squares agree to 9 digits)"""
    n = ROWS
    rng = np.random.default_rng(9)
    stored = np.zeros((n, n), bool)
    idx = np.full((n, 64), -1, np.int32)
    w = np.zeros((n, 64), np.float32)
    for i in range(n):
        c = np.sort(rng.choice(n, 48, replace=False))
        stored[i, c] = True
        idx[i, :48], w[i, :48] = c, (1e-4 * rng.random(48)).astype(np.float32) + np.float32(1e-6)
    A = stored.astype(np.float32)
    W = np.zeros((n, n), np.float32)
    W[np.repeat(np.arange(n), 48), idx[:, :48].reshape(-1)] = w[:, :48].reshape(-1)
    k = np.full(n, 48.0, np.float32)
    want = R.stats_dense(A, W, k)
    assert want["on_n"] == 48 * n and 1e-5 < want["on_std"] < 1e-4 and want["off_n"] == 0
    d32 = (A - W)[stored]
    naive = np.sqrt(max(0.0, float((np.sum(d32 * d32, dtype=np.float32) - np.sum(d32, dtype=np.float32) ** 2 / d32.size) / (d32.size - 1))))
    print("float32 sum / sum of squares would give", naive, "for", want["on_std"])
    assert not R.close(naive, want["on_std"]), "the case does not separate a float32 accumulation from the double one"
    R.assert_fields(as_dict(run((T(idx), T(w)), csr_of(stored, A), k)), want, what="tiny spread")


def test_refusals_write_nothing():
    from dgg_amd import _lib, ops
    L = _lib.lib()
    p = problem(64)
    (idx, w), _ = arrays(p, 64, False)
    rowptr, col, aval = csr_of(p["stored"], p["A"])
    k = T(p["k"])
    ws = torch.empty(8 * ROWS, device=DEV, dtype=torch.float64)
    out = torch.full((10,), -5.0, device=DEV)
    P = ops._ptr
    good = [P(idx), P(w), ROWS, 64, None, 0, P(rowptr), P(col), P(aval), P(k), P(ws), P(out), ops._stream()]
    for pos, val in ((3, 65), (3, 0), (2, -1), (2, 2 ** 31), (0, None), (6, None), (9, None), (10, None), (11, None)):
        args = list(good)
        args[pos] = val
        assert L.dgg_adj_diff_stats(*args) == 1, (pos, val)              # DGG_ERR_ARG
    lay_args = list(good)
    lay_args[3], lay_args[4], lay_args[5] = 32, P(torch.zeros(ROWS + 1, device=DEV, dtype=torch.int32)), 4
    assert L.dgg_adj_diff_stats(*lay_args) == 1                          # chunked rows are 64 wide
    torch.cuda.synchronize()
    assert bool((out == -5.0).all())
    with pytest.raises(_lib.DggHipError):
        ops.adj_diff_stats((torch.full((ROWS, 65), -1, device=DEV, dtype=torch.int32), torch.zeros(ROWS, 65, device=DEV)), (rowptr, col, aval), k)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_kernel_reproduces_the_reference_scalars(case):
    fx = load_fixture("adj_stats_" + case)
    n = fx["meta"]["N"]
    stored = np.zeros((n, n), bool)
    stored[fx["rows"], fx["cols"]] = True
    A = R.dense_from_triplets(n, fx["rows"], fx["cols"], fx["adj_vals"])
    idx = np.full((n, 64), -1, np.int32)
    w = np.zeros((n, 64), np.float32)
    fill = np.zeros(n, np.int64)
    for r_, c_, v_ in zip(fx["out_rows"], fx["out_cols"], fx["out_vals"]):
        idx[r_, fill[r_]], w[r_, fill[r_]] = c_, v_
        fill[r_] += 1
    got = as_dict(run((T(idx), T(w)), csr_of(stored, A), fx["k"]))
    ref = {R.TAG_FIELD[t]: fx["ref"][i] for i, t in enumerate(R.TAGS)}
    extra = {R.TAG_FIELD[t]: fx["dist"][i] for i, t in enumerate(R.TAGS)}
    R.assert_fields(got, ref, fields=tuple(ref), extra=extra, what=f"fixture {case} (reference)")
    assert got["on_n"] == fx["meta"]["n_on"] and got["off_n"] == fx["meta"]["n_off"]


# ---- the modules -----------------------------------------------------------------------------------------------------------------
N_MOD, NFEAT, NHID = 300, 64, 32
ALL_TAGS = ("values/first_k_std", "values/first_k_mean") + tuple("train_stats/" + t for t in R.TAGS)


class Recorder:
    def __init__(self):
        self.scalars, self.hist = [], []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, value, step))

    def add_histogram(self, tag, values, step):
        self.hist.append((tag, step))

    def train_stats(self):
        return {R.TAG_FIELD[t[len("train_stats/"):]]: v for t, v, _ in self.scalars if t.startswith("train_stats/")}


def model_args(**kw):
    base = dict(extra_edge_dim=0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288, dgg_mode_edge_net="u-v-dist", dgg_mode_k_net="x",
                dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=True, symmetric_noise=False, stochastic_k=False,
                dgg_adj_input="input_adj", n_dgg_layers=1)
    base.update(kw)
    return Namespace(**base)


def graph(wide_row=None):
    """random symmetric graph WITHOUT self loops (the model adds them), ~8 neighbours a node; wide_row: one row of 100 neighbours"""
    g = torch.Generator().manual_seed(3)
    A = (torch.rand(N_MOD, N_MOD, generator=g) < 4.0 / N_MOD).float()
    A = ((A + A.T) > 0).float()
    if wide_row is not None:
        A[wide_row, torch.randperm(N_MOD, generator=g)[:100]] = 1.0
    A.fill_diagonal_(0)
    return A.to_sparse().coalesce()


def build(wide_row=None, degree_k=False, **kw):
    import dgg_amd
    torch.manual_seed(0)
    m = dgg_amd.GCN_DGG(nfeat=NFEAT, nhidden=NHID, nclass=7, args=model_args(**kw))
    if degree_k:                                                   # k = deg + 1: the wide row needs a second chunk
        dgg = m.dggs[0]
        with torch.no_grad():
            for lin in (dgg.k_embed[0], dgg.k_net.k_mu, dgg.k_net.k_project):
                lin.weight.zero_()
                lin.bias.zero_()
            dgg.k_embed[0].weight[0, NHID] = 1.0
            dgg.k_net.k_mu.weight[0, 0] = 1.0
            dgg.k_net.k_project.weight[0, 0] = 1.0
    m = m.to(DEV)
    m.dggs[0].set_seed(1234, 5)
    x = torch.randn(N_MOD, NFEAT, generator=torch.Generator().manual_seed(1)).to(DEV)
    return m, x, graph(wide_row).to(DEV)


def forward(m, x, A, writer, epoch=11):
    torch.manual_seed(7)                                           # (the dropout between the layers)
    out = m(x, A, epoch=epoch, writer=writer)
    torch.cuda.synchronize()
    return out


def check_logged(rec, unnorm_adj, A_in, k, epoch=11, off_finite=None):
    """all nine tags once, at step `epoch`, Python floats; train_stats/* = the restatement on the returned adjacency against A_in"""
    tags = [t for t, _, _ in rec.scalars]
    assert sorted(tags) == sorted(ALL_TAGS), tags
    assert all(s == epoch for _, _, s in rec.scalars)
    assert all(isinstance(v, float) for t, v, _ in rec.scalars if t.startswith("train_stats/"))
    want = R.stats_dense(A_in, unnorm_adj.to_dense().detach().cpu().numpy(), k.detach().cpu().numpy())
    got = rec.train_stats()
    R.assert_fields(got, want, fields=tuple(got), what="module")
    if off_finite is not None:
        assert np.isfinite(got["off_mean"]) == off_finite and np.isfinite(got["off_std"]) == off_finite


def dense_plus_eye(A):
    return (A.to_dense() + torch.eye(N_MOD, device=A.device)).cpu().numpy()


def test_gcn_dgg_logs_from_the_fused_layer():
    from dgg_amd import ops
    m, x, A = build(dgg_writer_fused=True)
    m.train()
    dgg = m.dggs[0]
    calls = ops.ADJ_STATS_CALLS
    out0, adj0, _ = forward(m, x, A, None)                          # before any writer was involved
    assert ops.ADJ_STATS_CALLS == calls, "writer=None launched the stats kernel"
    rec = Recorder()
    out1, adj1, _ = forward(m, x, A, rec)
    assert ops.ADJ_STATS_CALLS == calls + 1
    assert not dgg.__dict__.get("fused_fallback") and adj1.idx is dgg._fused_layer.saved["idx"] and not adj1.values().requires_grad
    check_logged(rec, adj1, dense_plus_eye(A), adj1.k, off_finite=False)
    assert [h for h in rec.hist] == [("gcn_conv1_dist", 11), ("gcn_conv2_dist", 11)]
    out2, adj2, _ = forward(m, x, A, None)
    assert ops.ADJ_STATS_CALLS == calls + 1
    for a, b in ((out0, out1), (out0, out2), (adj0.values(), adj1.values()), (adj0.values(), adj2.values())):
        assert torch.equal(a, b), "the writer changed the forward"
    assert torch.equal(adj0.idx, adj1.idx)
    m.eval()                                                       # the reference computes the numbers in eval and writes nothing
    rec2 = Recorder()
    forward(m, x, A, rec2)
    assert rec2.scalars == [] and ops.ADJ_STATS_CALLS == calls + 1


def test_gcn_dgg_all_pairs_with_a_prior_has_off_edge_pairs():
    import dgg_amd
    m, x, A = build(dgg_writer_fused=True)
    m.train()
    ap = dgg_amd.AllPairs.from_graph(A, self_loops=True)
    rec = Recorder()
    _, adj, _ = forward(m, x, ap, rec)
    assert not m.dggs[0].__dict__.get("fused_fallback") and adj.idx is m.dggs[0]._fused_layer.saved["idx"]
    check_logged(rec, adj, dense_plus_eye(A), adj.k, off_finite=True)
    # without a prior there are no stored values: the three degree scalars only
    rec3 = Recorder()
    _, adj3, _ = forward(m, x, dgg_amd.AllPairs(ap.prior_degree), rec3)
    tags = sorted(t for t, _, _ in rec3.scalars)
    assert tags == sorted(("values/first_k_std", "values/first_k_mean", "train_stats/in_deg_mean", "train_stats/k_diff_mean", "train_stats/k_mean"))
    deg, k = ap.prior_degree.double().cpu().numpy(), adj3.k.double().cpu().numpy()
    got = rec3.train_stats()
    assert R.close(got["in_deg_mean"], deg.mean()) and R.close(got["k_diff_mean"], (k - deg).mean()) and R.close(got["k_mean"], k.mean())


def test_gcn_dgg_chunked_edge_list_rows():
    m, x, A = build(wide_row=17, degree_k=True, dgg_writer_fused=True, dgg_edgelist_rows="chunked")
    m.train()
    rec = Recorder()
    _, adj, _ = forward(m, x, A, rec)
    assert not m.dggs[0].__dict__.get("fused_fallback") and adj.layout is not None and adj.layout.wide
    assert int(adj.layout.cptr[18] - adj.layout.cptr[17]) >= 2
    check_logged(rec, adj, dense_plus_eye(A), adj.k, off_finite=False)
    # the same graph without the opt-in: the separate modules, whose wide rows take the CSR form -- the same tags, elementwise
    m2, _, _ = build(wide_row=17, degree_k=True, dgg_edgelist_rows="chunked")
    m2.train()
    rec2 = Recorder()
    _, adj2, _ = forward(m2, x, A, rec2)
    assert "_fused_layer" not in m2.dggs[0].__dict__ and type(adj2).__name__ == "CsrAdjacency"
    tags = sorted(t for t, _, _ in rec2.scalars)
    assert tags == sorted("train_stats/" + t for t in R.TAGS), tags     # (the CSR form never logged values/first_k_*)
    want = R.stats_dense(dense_plus_eye(A), adj2.to_dense().detach().cpu().numpy(), adj2.k.cpu().numpy())
    R.assert_fields(rec2.train_stats(), want, fields=tuple(rec2.train_stats()), what="CSR form")


def test_without_the_opt_in_the_separate_modules_write_the_same_tags():
    from dgg_amd import ops
    m, x, A = build()
    m.train()
    calls = ops.ADJ_STATS_CALLS
    rec = Recorder()
    _, adj, _ = forward(m, x, A, rec)
    assert "_fused_layer" not in m.dggs[0].__dict__ and adj.values().requires_grad, "a writer without the opt-in keeps the separate modules"
    assert ops.ADJ_STATS_CALLS == calls + 1
    check_logged(rec, adj, dense_plus_eye(A), adj.k, off_finite=False)
    m.eval()
    rec2 = Recorder()
    forward(m, x, A, rec2)
    assert [t for t, _, _ in rec2.scalars if t.startswith("train_stats/")] == []


def test_a_capture_refuses_the_writer():
    m, x, A = build(dgg_writer_fused=True)
    m.train()
    forward(m, x, A, None)                                         # (everything cached and allocated before the capture)
    dgg = m.dggs[0]
    import dgg_amd.dgm as dgm_mod
    real = dgm_mod._capturing
    dgm_mod._capturing = lambda: True                              # what a capture looks like to the module, without starting one
    try:
        with pytest.raises(RuntimeError, match="read-back"):
            dgg._log_adj_stats(Recorder(), 0, None, None, None, None, None)
        with pytest.raises(RuntimeError, match="read-back"):
            dgg.forward_conv(x, A, m.conv1.W, writer=Recorder(), epoch=0)
    finally:
        dgm_mod._capturing = real


@pytest.mark.parametrize("fused", ["false", "true"])
def test_the_harness_logs_the_training_forward(tmp_path, fused, monkeypatch):
    """train_small_graphs --log_dir on the Cora fixture, two epochs: the training forward of each epoch writes the nine scalars and the
    two histograms at its epoch, the evaluation forward nothing -- with and without the fused layer under the writer"""
    import os
    from dgg_amd import ScalarLog, train_small_graphs as H
    monkeypatch.setattr(H, "make_writer", ScalarLog)               # (whichever writer this machine has: the tags are read back from the JSON log)
    planetoid = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planetoid")
    H.main(["--data", "cora", "--data_dir", planetoid, "--epochs", "2", "--hidden", "64", "--log_dir", str(tmp_path / "run"), "--dgg_writer_fused", fused])
    recs = ScalarLog.read(tmp_path / "run" / "scalars.jsonl")
    for epoch in (0, 1):
        mine = [r for r in recs if r["step"] == epoch]
        assert sorted(r["tag"] for r in mine if "value" in r) == sorted(ALL_TAGS), (epoch, mine)
        assert sorted(r["tag"] for r in mine if "count" in r) == ["gcn_conv1_dist", "gcn_conv2_dist"]
        vals = {r["tag"]: r["value"] for r in mine if "value" in r}
        assert all(np.isfinite(vals["train_stats/" + t]) for t in ("on_edge_mean", "on_edge_std", "in_deg_mean", "k_diff_mean", "k_mean"))
        assert np.isnan(vals["train_stats/off_edge_mean"]) and np.isnan(vals["train_stats/off_edge_std"])      # (edge list, no perturbation)
    assert len(recs) == 2 * 11
