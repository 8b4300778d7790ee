"""ShardedGCN_DGG with u-v-A_uv on ALL-PAIRS candidates that carry a prior graph (AllPairs(prior_degree, prior=P); opt-in
args.dgg_allpairs_prior_fused = True, alone) on two ranks sharing one MI355X over gloo (this process is rank 0, one spawned child rank 1;
the harness and the bars of tests/test_sharded_allpairs_mlp.py): the concatenated log-probabilities and each rank's adjacency rows equal
the single-process GCN_DGG bit for bit -- on the 64-rank list and on chunked rows --, the gradients are identical on both ranks and match
the single process, and Adam keeps the ranks bit-identical.  (Before this feature every test here fails with NotImplementedError.)

N = 1001: shard_bounds puts the boundary at row 501 -- odd, inside a 64-column tile and inside a row block of either blocking.  The prior
(test_allpairs_prior_fused.make_prior) stores, in rows 500 and 501, the columns 499 .. 502: entries that cross the boundary both ways;
every rank gets the whole prior.  Column 2h of edge_encode.0.weight keeps its initialisation here (at this width no scale of it raises
a prior edge's score -- CPU emulation with the oracle, as in tests/test_allpairs_prior_fused.py, which holds the share of prior edges to
a bar): in that emulation about 0.4 % of the entries with rank below k + 9 are prior edges, some hundred of them, and the test asserts
that kept prior edges cross the boundary in both directions, so both ranks look up entries of the other's half.

Gradient bars: 1e-5 of a parameter's largest entry, 1e-4 for dggs.0.edge_* (the scorer's parameter sums group the rows by workgroup, and
a shard groups them differently; cancelling sums such as an output bias), or twice the single process's own call-to-call spread,
whichever is larger."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_sharded_allpairs_mlp import _rank_job, grads, sparse_rows  # noqa: E402

pytestmark = pytest.mark.gpu
N_NODES = 1001
BOUNDARY = 501


def setup(noise, chunked=False, N=N_NODES, d=64, h=64, nclass=16, dev=None):
    """-> model, x, AllPairs(prior degrees, prior=P), labels, train index (on cuda:0 unless dev says otherwise).  chunked:
    args.dgg_allpairs_mlp_rows = "chunked" and the degree-following k-net: every eighth row near 200 ranks -- on both ranks' halves --,
    the others under 40"""
    import dgg_amd
    from test_allpairs_mlp import module_args
    from test_allpairs_mlp_fused import NOISES, degree_following_knet
    from test_allpairs_prior_fused import make_prior
    dev = torch.device("cuda", 0) if dev is None else dev
    torch.manual_seed(0)
    kw = dict(dgg_allpairs_mlp_rows="chunked") if chunked else {}
    m = dgg_amd.GCN_DGG(nfeat=d, nhidden=h, nclass=nclass, args=module_args("u-v-A_uv", dgg_wide_rows="auto", dgg_allpairs_prior_fused=True,
                                                                             **NOISES[noise], **kw))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, d, generator=g)
    prior = torch.randint(6, 31, (N,), generator=g).float()
    dgg = m.dggs[0]
    if chunked:
        prior[::8] = torch.randint(150, 200, (len(prior[::8]),), generator=g).float()
        degree_following_knet(dgg)
    else:
        with torch.no_grad():
            dgg.k_net.k_project.weight.mul_(0.1)
    m = m.to(dev)
    dgg.set_seed(1234, 5)
    labels = torch.randint(0, nclass, (N,), generator=g)
    idx = torch.randperm(N, generator=g)[: N // 5]
    return m, x.to(dev), dgg_amd.AllPairs(prior.to(dev), prior=make_prior(N, cross=(BOUNDARY,)).to(dev)), labels.to(dev), idx.to(dev)


# ---- two ranks on one GPU (the harness of test_sharded_allpairs_mlp; the jobs are looked up in THIS module) ------------------------
def _child(job_name, args, port, ret):
    sys.path.insert(0, ROOT)
    job = globals()[job_name]
    try:
        ret[1] = _rank_job(lambda r: job(r, *args), 1, port)
    except Exception as e:  # noqa: BLE001
        ret[1] = ("error", repr(e))
        raise


def two_ranks(job_name, *args):
    port = 33800 + os.getpid() % 2000
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


def _eval_job(rank, noise, chunked):
    from dgg_amd.distributed import ShardedGCN_DGG, global_nll_loss
    m, x, A, labels, idx = setup(noise, chunked)
    net = ShardedGCN_DGG(m).eval()
    out, adj, _ = net(x, A)
    global_nll_loss(out, labels, idx, net.rows).backward()
    torch.cuda.synchronize()
    assert m.dggs[0].__dict__.get("fused_fallback") is None
    m.dggs[0].check_ell_bound()
    assert (adj.layout is not None) == chunked and adj.shape == (net.rows[1] - net.rows[0], x.shape[0])
    lists = (adj.idx.cpu().numpy(), adj.values().detach().cpu().numpy()) if not chunked else None
    return (net.rows, out.detach().cpu().numpy(), lists, sparse_rows(adj), {k: v.cpu().numpy() for k, v in grads(m).items()})


def compare_with_single_process(noise, chunked):
    (rows0, o0, l0, s0, ga), (rows1, o1, l1, s1, gb) = two_ranks("_eval_job", noise, chunked)
    m, x, A, labels, idx = setup(noise, chunked)
    m.eval()
    spread = {}
    for rep in range(2):                                     # (twice: how far the single process's own gradients move between calls)
        for p_ in m.parameters():
            p_.grad = None
        out, adj, _ = m(x, A)
        F.nll_loss(out[idx], labels[idx]).backward()
        torch.cuda.synchronize()
        spread = {k: v for k, v in grads(m).items()} if rep == 0 else {k: float((v - spread[k]).abs().max()) for k, v in grads(m).items()}
    dgg = m.dggs[0]
    assert dgg.__dict__.get("fused_fallback") is None and dgg.__dict__.get("_fused_layer") is not None
    assert (adj.layout is not None) == chunked
    if chunked:
        print(f"k in {float(adj.k.min()):.1f} .. {float(adj.k.max()):.1f}, {adj.layout.chunks} chunks")
        assert float(adj.k.max()) > 150 and float(adj.k.min()) < 40
    assert rows0 == (0, BOUNDARY) and rows1 == (BOUNDARY, N_NODES)
    assert np.array_equal(np.concatenate([o0, o1]), out.detach().cpu().numpy()), "log-probabilities"
    wr, wc, wv = sparse_rows(adj)
    # kept prior edges on both sides of the boundary and across it
    Pd = A.prior.to_dense().cpu().numpy()
    on = Pd[wr, wc] != 0
    print(f"{noise} / {'chunked' if chunked else 'list'}: {100 * on.mean():.1f} % of the weighted entries are prior edges; "
          f"across the boundary: {int((on & (wr < BOUNDARY) & (wc >= BOUNDARY)).sum())} from below, {int((on & (wr >= BOUNDARY) & (wc < BOUNDARY)).sum())} from above")
    assert (on & (wr < BOUNDARY) & (wc >= BOUNDARY)).any() and (on & (wr >= BOUNDARY) & (wc < BOUNDARY)).any()
    for (r0, r1), ll, (sr, sc, sv) in ((rows0, l0, s0), (rows1, l1, s1)):
        if not chunked:
            assert np.array_equal(ll[0], adj.idx[r0:r1].cpu().numpy()) and np.array_equal(ll[1], adj.values()[r0:r1].detach().cpu().numpy())
        own = (wr >= r0) & (wr < r1)
        assert np.array_equal(sr + r0, wr[own]) and np.array_equal(sc, wc[own]) and np.array_equal(sv.view(np.int32), wv[own].view(np.int32))
    g1 = grads(m)
    assert set(g1) == set(ga) == set(gb)
    h = dgg.latent_dim
    assert float(g1["dggs.0.edge_encode.0.weight"][:, 2 * h].abs().max()) > 0, "the prior column's gradient"
    for k, v in g1.items():
        v = v.cpu().numpy()
        assert np.array_equal(ga[k], gb[k]), k
        rel = 1e-4 if k.startswith("dggs.0.edge_") else 1e-5
        bar = max(rel * max(np.abs(v).max(), 1e-30), 2 * spread[k])
        assert np.abs(ga[k] - v).max() <= bar, (k, np.abs(ga[k] - v).max(), np.abs(v).max(), spread[k])


@pytest.mark.parametrize("noise", ["hash", "sym"])
def test_two_ranks_match_single_process(noise):
    compare_with_single_process(noise, False)


def test_two_ranks_match_single_process_on_chunked_rows():
    compare_with_single_process("hash", True)


def _adam_job(rank, steps):
    from dgg_amd.distributed import ShardedGCN_DGG, global_nll_loss
    m, x, A, labels, idx = setup("hash")
    net = ShardedGCN_DGG(m).train()
    opt = torch.optim.Adam([{"params": net.params1, "weight_decay": 5e-4}, {"params": net.params2, "weight_decay": 0.0}], lr=0.01)
    torch.cuda.manual_seed(100 + rank)                        # (each rank's own dropout masks)
    hist = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        out, _, _ = net(x, A)
        loss = global_nll_loss(out, labels, idx, net.rows)
        loss.backward()
        opt.step()
        flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()
        hist.append((float(loss.detach()), flat))
    return hist


def test_adam_keeps_the_ranks_bit_identical():
    h0, h1 = two_ranks("_adam_job", 3)
    assert len(h0) == len(h1) == 3
    for (l0, p0), (l1, p1) in zip(h0, h1):
        assert np.isfinite(l0) and l0 == l1
        assert np.array_equal(p0, p1)
    assert not np.array_equal(h0[0][1], h0[-1][1])           # (the parameters moved)
