"""Edge-list rows of any width inside the fused layer: args.dgg_edgelist_rows = "chunked" on one GPU (GCN_DGG) and on two ranks sharing
one MI355X over gloo (ShardedGCN_DGG; this process is rank 0, one spawned child rank 1).

Graph and k-net of tests/test_sharded_edgelist_csr.py at N = 601 (shards of 301 and 300 rows): rows of 1-60 candidates and three rows of
100 in rank 1's half only; the k-net weights make k = deg + 1, so those rows need 2 chunks and every other row one.  Rank 0 therefore owns
no wide row and stays on the list kernels while rank 1 runs the chunked ones: each rank decides from its own rows.

One GPU, reference = the same model as separate modules in CSR form (dgg_fused_layer = False, dgg_wide_rows = "csr"), which is what the
argument's absence leads to: nothing leaves the fused layer, the adjacency is an EllAdjacency with a wide layout, the weighted entries of
every row are the same set, values 1e-6, log-probabilities 1e-5, every parameter gradient 3e-4 of its maximum (the bars of
test_gcn_dgg_fused_first_layer_matches_the_separate_modules).  A graph whose rows all fit gives the same bits with and without the argument.
Two ranks under "chunked" and the default dgg_wide_rows: log-probabilities and each rank's rows equal the single-process fused model bit
for bit, gradients meet the bar of test_two_ranks_match_single_process (1e-5 of the maximum, 1e-4 for dggs.0.edge_*, or twice the single
process's own call-to-call spread), five Adam steps keep the ranks bit-identical; under "list" the same forward raises NotImplementedError.
Without the feature the argument is ignored: the one-GPU forward leaves for the CSR form and the two-rank forward raises.

Measured on an MI355X: gradients at most 3.3e-6 of their maximum on one GPU (bar 3e-4) and 0.06 of their bar on two ranks;
log-probabilities at most 0.53 of the bar.  The classifier is scaled as the test these bars come from scales it (conv2.W x 0.2, setup):
unscaled (logits up to 22) one log-probability of 9 616 sat at 1.01 of the bar in one case (u-v-deg-dist, no noise, 3.6e-5 apart), and
against a float64 evaluation of the two layers on the adjacency each form produced the fused chunked form was off by 1.4e-5, the CSR
reference by 3.2e-5 (the two float64 results identical): the reference's own rounding, at a scale the absolute bar was not set for."""
import copy
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sharded_edgelist_csr import ROOT, _rank_job, degree_knet, grads, synthetic_graph  # noqa: E402

pytestmark = pytest.mark.gpu
N_SYN = 601
WIDE = (N_SYN - 7, N_SYN - 100, N_SYN - 250)                  # rank 1's half only (rows 301 ..)
SCORERS = ("u-v-dist", "u-v-deg", "u-v-A_uv", "u-v-deg-dist")


def model_args(scorer, noise, **kw):
    base = dict(extra_edge_dim={"u-v-deg": 2, "u-v-deg-dist": 3, "u-v-A_uv": 1}.get(scorer, 0), extra_k_dim=1, dgg_hard=False, deg_mean=3.899,
                deg_std=5.288, dgg_mode_edge_net=scorer, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3,
                perturb_edge_prob=noise != "none", symmetric_noise=noise == "sym", stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
    base.update(kw)
    return Namespace(**base)


def setup(scorer, noise, wide=WIDE, d=64, h=64, nclass=16, conv2_scale=0.2, **kw):
    """the set-up of tests/test_sharded_edgelist_csr.py at N_SYN nodes, with the classifier scaled as
    test_gcn_dgg_fused_first_layer_matches_the_separate_modules scales it (conv2.W x 0.2: GCNConv draws W ~ U[0, 1), and the absolute
    1e-5 on log-probabilities that this file takes from that test is a bar for logits of its size)"""
    import dgg_amd
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = dgg_amd.GCN_DGG(nfeat=d, nhidden=h, nclass=nclass, args=model_args(scorer, noise, **kw))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N_SYN, d, generator=g)
    A = synthetic_graph(N_SYN, wide)
    degree_knet(m.dggs[0], h, 1.0)
    with torch.no_grad():
        m.conv2.W.mul_(conv2_scale)
    m = m.to(dev)
    m.dggs[0].set_seed(1234, 5)
    labels = torch.randint(0, nclass, (N_SYN,), generator=g)
    idx = torch.randperm(N_SYN, generator=g)[: N_SYN // 5]
    return m, x.to(dev), A.to(dev), labels.to(dev), idx.to(dev)


def Nn(t):
    return t.detach().cpu().numpy()


def dense_of(adj):
    """the adjacency's weights as a dense [rows, N] float32 array (entries are unique per row)"""
    rows, ncol = adj.shape
    out = np.zeros((rows, ncol), np.float32)
    if type(adj).__name__ == "CsrAdjacency":
        rp = Nn(adj.rowptr)
        r = np.repeat(np.arange(rows), rp[1:] - rp[:-1])
        out[r, Nn(adj.col)] = Nn(adj.values())
        return out
    idx, val = Nn(adj.idx), Nn(adj.values())
    node = Nn(adj.layout.cnode)[:idx.shape[0]] if adj.layout is not None else np.arange(rows)
    keep = idx >= 0
    out[np.broadcast_to(node[:, None], idx.shape)[keep], idx[keep]] = val[keep]
    return out


def rows_form(idx, val, cptr):
    """(idx, val) of a [rows,64] list (cptr None) or of chunked rows -> per-row lists of the kept (column, value bits) in rank order"""
    rows = idx.shape[0] if cptr is None else len(cptr) - 1
    out = []
    for i in range(rows):
        c0, c1 = (i, i + 1) if cptr is None else (cptr[i], cptr[i + 1])
        ii, vv = idx[c0:c1].reshape(-1), val[c0:c1].reshape(-1)
        out.append((ii[ii >= 0].tolist(), vv[ii >= 0].view(np.int32).tolist()))
    return out


def adj_arrays(adj):
    return Nn(adj.idx), Nn(adj.values()), (None if adj.layout is None else Nn(adj.layout.cptr).astype(np.int64))


# ---- one GPU: the fused layer on chunked rows against the separate modules in CSR form ----------------------------------------------
@pytest.mark.parametrize("noise", ["none", "asym"])
@pytest.mark.parametrize("scorer", SCORERS)
def test_fused_chunked_rows_match_the_separate_modules_in_csr_form(scorer, noise):
    m1, x, A, labels, _ = setup(scorer, noise, dgg_edgelist_rows="chunked")
    m1.eval()
    m2 = copy.deepcopy(m1)
    m2.dggs[0].args = Namespace(**dict(vars(m1.dggs[0].args), dgg_fused_layer=False, dgg_wide_rows="csr", dgg_edgelist_rows="list"))
    m2.dggs[0].set_seed(1234, 5)
    outs = []
    for m in (m1, m2):
        logp, adj, _ = m(x, A)
        F.nll_loss(logp, labels).backward()
        outs.append((logp, adj))
    torch.cuda.synchronize()
    (lp1, adj1), (lp2, adj2) = outs
    assert not m1.dggs[0].__dict__.get("fused_fallback"), m1.dggs[0].__dict__.get("fused_fallback")
    assert type(adj1).__name__ == "EllAdjacency" and adj1.layout is not None and adj1.layout.wide
    assert type(adj2).__name__ == "CsrAdjacency"
    cptr = Nn(adj1.layout.cptr)
    M = cptr[1:] - cptr[:-1]
    assert sorted(np.where(M == 2)[0].tolist()) == sorted(WIDE) and ((M == 1) | (M == 2)).all()
    m1.dggs[0].check_ell_bound()                             # quiet: no weighted rank was dropped, no flag was raised
    d1, d2 = dense_of(adj1), dense_of(adj2)
    assert np.array_equal(d1 != 0, d2 != 0), "the weighted entries of a row differ"
    assert (d1[list(WIDE)] != 0).sum(1).min() > 64, "the wide rows carry weight beyond the list"
    np.testing.assert_allclose(d1, d2, rtol=0, atol=1e-6)
    np.testing.assert_allclose(Nn(lp1), Nn(lp2), rtol=1e-5, atol=1e-5)
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        if p2.grad is None:
            assert p1.grad is None or float(p1.grad.abs().max()) == 0.0, n1
            continue
        ref = Nn(p2.grad)
        assert p1.grad is not None, n1
        err = np.abs(Nn(p1.grad) - ref).max() / max(np.abs(ref).max(), 1e-30)
        print("  %-44s err/max %.3e  max %.3e" % (n1, err, np.abs(ref).max()))
        assert err <= 3e-4, f"{n1}: {err:.2e}"


@pytest.mark.parametrize("scorer", ["u-v-dist", "u-v-deg"])
def test_rows_that_all_fit_give_the_same_bits_with_and_without_the_argument(scorer):
    res = []
    for kw in ({}, {"dgg_edgelist_rows": "chunked"}):
        m, x, A, labels, _ = setup(scorer, "asym", wide=(), **kw)
        m.eval()
        logp, adj, _ = m(x, A)
        F.nll_loss(logp, labels).backward()
        torch.cuda.synchronize()
        assert type(adj).__name__ == "EllAdjacency" and adj.layout is None and not m.dggs[0].__dict__.get("fused_fallback")
        res.append((Nn(logp), Nn(adj.idx), Nn(adj.values())))
    for a, b in zip(*res):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- two ranks on one GPU -------------------------------------------------------------------------------------------------------------
def _child(job_name, args, port, ret):
    sys.path.insert(0, ROOT)
    job = globals()[job_name]
    try:
        ret[1] = _rank_job(lambda r: job(r, *args), 1, port)
    except Exception as e:  # noqa: BLE001
        ret[1] = ("error", repr(e))
        raise


_CALLS = [0]


def two_ranks(job_name, *args):
    # (a port of its own per call, away from the other files' ranges: see test_sharded_edgelist_csr.two_ranks)
    _CALLS[0] += 1
    port = 33900 + (os.getpid() % 2000) * 8 % 16000 + _CALLS[0]
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    p = ctx.Process(target=_child, args=(job_name, args, port, ret))
    p.start()
    try:
        r0 = _rank_job(lambda r: globals()[job_name](r, *args), 0, port)
    finally:
        p.join(240)
        if p.is_alive():
            p.kill()
    assert p.exitcode == 0, ret.get(1)
    return r0, ret[1]


def _eval_job(rank, scorer, noise):
    from dgg_amd.distributed import ShardedGCN_DGG, global_nll_loss
    m, x, A, labels, idx = setup(scorer, noise, dgg_edgelist_rows="chunked")
    net = ShardedGCN_DGG(m).eval()
    out, adj, _ = net(x, A)
    global_nll_loss(out, labels, idx, net.rows).backward()
    torch.cuda.synchronize()
    assert not m.dggs[0].__dict__.get("fused_fallback")
    return net.rows, Nn(out), adj_arrays(adj), {k: v.cpu().numpy() for k, v in grads(m).items()}


@pytest.mark.parametrize("scorer,noise", [("u-v-dist", "asym"), ("u-v-A_uv", "sym"), ("u-v-deg-dist", "asym")])
def test_two_ranks_on_chunked_rows_match_the_single_process(scorer, noise):
    (rows0, o0, a0, ga), (rows1, o1, a1, gb) = two_ranks("_eval_job", scorer, noise)
    m, x, A, labels, idx = setup(scorer, noise, dgg_edgelist_rows="chunked")
    m.eval()
    spread = {}
    for rep in range(2):                                     # (twice: how far the single process's own gradients move between calls)
        for p_ in m.parameters():
            p_.grad = None
        out, adj, _ = m(x, A)
        F.nll_loss(out[idx], labels[idx]).backward()
        torch.cuda.synchronize()
        spread = {k: v for k, v in grads(m).items()} if rep == 0 else {k: float((v - spread[k]).abs().max()) for k, v in grads(m).items()}
    assert not m.dggs[0].__dict__.get("fused_fallback")
    assert rows0 == (0, 301) and rows1 == (301, N_SYN)
    assert a0[2] is None and a1[2] is not None and adj.layout.wide, "rank 0 owns no wide row and keeps the list; rank 1 lays its rows out"
    assert np.array_equal(np.concatenate([o0, o1]).view(np.int32), Nn(out).view(np.int32))
    whole = rows_form(*adj_arrays(adj))
    for (r0, r1), arr in ((rows0, a0), (rows1, a1)):
        assert rows_form(*arr) == whole[r0:r1], f"rows [{r0}, {r1}) differ from the single process's"
    g1 = grads(m)
    assert set(g1) == set(ga) == set(gb)
    if scorer != "u-v-dist":
        assert any("edge" in k for k in g1)
    for k, v in g1.items():
        v = v.cpu().numpy()
        assert np.array_equal(ga[k], gb[k]), k
        rel = 1e-4 if k.startswith("dggs.0.edge_") else 1e-5
        bar = max(rel * max(np.abs(v).max(), 1e-30), 2 * spread[k])
        print("  %-44s err %.3e  max %.3e  spread %.3e  bar %.3e" % (k, np.abs(ga[k] - v).max(), np.abs(v).max(), spread[k], bar))
        assert np.abs(ga[k] - v).max() <= bar, (k, np.abs(ga[k] - v).max(), np.abs(v).max(), spread[k])


def _adam_job(rank, steps):
    from dgg_amd.distributed import ShardedGCN_DGG, global_nll_loss
    m, x, A, labels, idx = setup("u-v-deg", "asym", dgg_edgelist_rows="chunked")
    net = ShardedGCN_DGG(m).train()
    opt = torch.optim.Adam([{"params": net.params1, "weight_decay": 5e-4}, {"params": net.params2, "weight_decay": 0.0}], lr=0.01)
    torch.cuda.manual_seed(100 + rank)                        # (each rank's own dropout masks)
    hist = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        out, adj, _ = net(x, A)
        loss = global_nll_loss(out, labels, idx, net.rows)
        loss.backward()
        opt.step()
        flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()
        hist.append((float(loss.detach()), flat, type(adj).__name__))
    assert not m.dggs[0].__dict__.get("fused_fallback")
    return hist


def test_adam_on_chunked_rows_keeps_the_ranks_bit_identical():
    h0, h1 = two_ranks("_adam_job", 5)
    assert len(h0) == len(h1) == 5
    for (l0, p0, t0), (l1, p1, t1) in zip(h0, h1):
        assert np.isfinite(l0) and l0 == l1 and t0 == t1 == "EllAdjacency"
        assert np.array_equal(p0, p1)
    assert not np.array_equal(h0[0][1], h0[-1][1])           # (the parameters moved)


def _list_job(rank):
    from dgg_amd.distributed import ShardedGCN_DGG
    m, x, A, _, _ = setup("u-v-dist", "asym", dgg_edgelist_rows="list")
    net = ShardedGCN_DGG(m).eval()
    try:
        with torch.no_grad():
            net(x, A)
    except NotImplementedError as e:
        return "NotImplementedError", str(e)
    return "ran", ""


def test_under_list_the_same_forward_still_raises_on_both_ranks():
    (k0, msg0), (k1, msg1) = two_ranks("_list_job")
    assert k0 == k1 == "NotImplementedError" and "dgg_wide_rows" in msg0 and "dgg_edgelist_rows" in msg0 and msg0 == msg1
