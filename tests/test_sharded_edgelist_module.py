"""ShardedGCN_DGG with edge-list candidates (a sparse in_adj) on two ranks sharing one MI355X over gloo (this process is rank 0, one
spawned child rank 1): the concatenated log-probabilities and each rank's adjacency rows equal the single-process GCN_DGG bit for bit,
the gradients are identical on both ranks and match the single process, Cora's reference fixture runs through two ranks, a wide row
on one rank only makes both ranks refuse in the same forward, and Adam keeps the ranks bit-identical."""
import os
import sys
from argparse import Namespace
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
N_SYN = 20000


def model_args(scorer, noise):
    return Namespace(extra_edge_dim=2 if scorer == "u-v-deg" else 0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288,
                     dgg_mode_edge_net=scorer, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3,
                     perturb_edge_prob=noise != "none", symmetric_noise=noise == "sym", stochastic_k=False, dgg_adj_input="input_adj",
                     n_dgg_layers=1)


def synthetic_graph(N, wide_rows, seed=2):
    """sparse [N, N] graph (no self loops: the model adds them): 1-60 neighbours a row, `wide_rows` with 100"""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 61, N)
    n[list(wide_rows)] = 100
    rows = np.repeat(np.arange(N), n)
    cols = np.concatenate([rng.choice(N, c, replace=False) for c in n])
    keep = rows != cols
    ind = torch.from_numpy(np.stack([rows[keep], cols[keep]]))
    return torch.sparse_coo_tensor(ind, torch.ones(ind.shape[1]), (N, N)).coalesce()


def setup(scorer, noise, N=N_SYN, d=64, h=64, nclass=16, wide_rank1=False):
    """-> model (cuda:0), x, sparse in_adj, labels, train index.  wide_rank1: the wide rows lie in rank 1's half only and the k-net
    weights make k = deg + 1, so those rows need more ranks than the list holds"""
    import dgg_amd
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = dgg_amd.GCN_DGG(nfeat=d, nhidden=h, nclass=nclass, args=model_args(scorer, noise))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, d, generator=g)
    wide = (N - 7, N - 300, N - 4000) if wide_rank1 else (3, 5000, 12000, N - 2)
    A = synthetic_graph(N, wide)
    dgg = m.dggs[0]
    with torch.no_grad():
        dgg.k_net.k_project.weight.mul_(0.1)
        if wide_rank1:
            for lin in (dgg.k_embed[0], dgg.k_net.k_mu, dgg.k_net.k_project):
                lin.weight.zero_()
                lin.bias.zero_()
            dgg.k_embed[0].weight[0, h] = 1.0            # the normalised-degree input
            dgg.k_net.k_mu.weight[0, 0] = 1.0
            dgg.k_net.k_project.weight[0, 0] = 1.0
    m = m.to(dev)
    dgg.set_seed(1234, 5)
    labels = torch.randint(0, nclass, (N,), generator=g)
    idx = torch.randperm(N, generator=g)[: N // 5]
    return m, x.to(dev), A.to(dev), labels.to(dev), idx.to(dev)


def grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


# ---- two ranks on one GPU (the harness of test_sharded_module) ---------------------------------------------------------------------
def _rank_job(job, rank, port):
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2, timeout=timedelta(seconds=180))
    try:
        return job(rank)
    finally:
        dist.destroy_process_group()


def _child(job_name, args, port, ret):
    sys.path.insert(0, ROOT)
    job = globals()[job_name]
    try:
        ret[1] = _rank_job(lambda r: job(r, *args), 1, port)
    except Exception as e:  # noqa: BLE001
        ret[1] = ("error", repr(e))
        raise


def two_ranks(job_name, *args):
    port = 29800 + os.getpid() % 2000
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
    m, x, A, labels, idx = setup(scorer, noise)
    net = ShardedGCN_DGG(m).eval()
    out, adj, _ = net(x, A)
    global_nll_loss(out, labels, idx, net.rows).backward()
    torch.cuda.synchronize()
    assert m.dggs[0].__dict__.get("fused_fallback") is None
    return (net.rows, out.detach().cpu().numpy(), adj.idx.cpu().numpy(), adj.values().detach().cpu().numpy(),
            {k: v.cpu().numpy() for k, v in grads(m).items()})


@pytest.mark.parametrize("scorer,noise", [("u-v-dist", "none"), ("u-v-dist", "asym"), ("u-v-dist", "sym"), ("u-v-deg", "asym"),
                                          ("edge_conv", "sym")])
def test_two_ranks_match_single_process(scorer, noise):
    (rows0, o0, i0, v0, ga), (rows1, o1, i1, v1, gb) = two_ranks("_eval_job", scorer, noise)
    m, x, A, labels, idx = setup(scorer, noise)
    m.eval()
    spread = {}
    for rep in range(2):                                     # (twice: how far the single process's own gradients move between calls)
        for p_ in m.parameters():
            p_.grad = None
        out, adj, _ = m(x, A)
        F.nll_loss(out[idx], labels[idx]).backward()
        torch.cuda.synchronize()
        spread = {k: v for k, v in grads(m).items()} if rep == 0 else {k: float((v - spread[k]).abs().max()) for k, v in grads(m).items()}
    assert m.dggs[0].__dict__.get("fused_fallback") is None
    assert rows0 == (0, rows1[0]) and rows1[1] == N_SYN
    assert np.array_equal(np.concatenate([o0, o1]), out.detach().cpu().numpy())
    for (r0, r1), ii, vv in (((rows0), i0, v0), ((rows1), i1, v1)):
        assert np.array_equal(ii, adj.idx[r0:r1].cpu().numpy()) and np.array_equal(vv, adj.values()[r0:r1].detach().cpu().numpy())
    g1 = grads(m)
    assert set(g1) == set(ga) == set(gb)
    if scorer != "u-v-dist":
        assert any("edge" in k for k in g1)                      # (the scorer's own parameters got their gradient)
    # (the edge-MLP scorer's parameter sums are float atomics over every selected edge -- ~6e5 here -- grouped by workgroup rows, and a
    #  shard groups its rows differently; edge_conv's have no activation, so e.g. its output bias gradient is sum(ds), a cancelling sum:
    #  measured 2.9e-5 of its max between the shards and the single process.  Those parameters get 1e-4, the others 1e-5 of their max,
    #  or twice the single process's own call-to-call spread)
    for k, v in g1.items():
        v = v.cpu().numpy()
        assert np.array_equal(ga[k], gb[k]), k
        rel = 1e-4 if k.startswith("dggs.0.edge_") else 1e-5
        bar = max(rel * max(np.abs(v).max(), 1e-30), 2 * spread[k])
        assert np.abs(ga[k] - v).max() <= bar, (k, np.abs(ga[k] - v).max(), np.abs(v).max(), spread[k])


def cora():
    import dgg_amd
    from dgg_amd.train_small_graphs import make_adjacency
    from helpers import load_fixture
    dev = torch.device("cuda", 0)
    fx, inp = load_fixture("cora_gcn_dgg"), load_fixture("cora_gcn_dgg_00")
    meta = fx["meta"]
    N, d, h, C = meta["N"], meta["d"], meta["h"], meta["C"]
    x = np.zeros((N, d), np.float32)
    x[inp["feat_rows"].astype(np.int64), inp["feat_cols"].astype(np.int64)] = inp["feat_vals"]
    A = make_adjacency({"x": x, "rows": inp["rows"], "cols": inp["cols"]}, inp["meta"]["edge_noise_level"], dev)
    m = dgg_amd.GCN_DGG(nfeat=d, nlayers=2, nhidden=h, nclass=C, args=Namespace(**meta["args"]))
    m.load_state_dict({k_[2:]: torch.from_numpy(v) for k_, v in fx.items() if k_.startswith("p.")}, strict=True)
    m = m.to(dev).eval()
    m.dggs[0].set_seed(11, 12)
    return m, torch.from_numpy(x).to(dev), A, fx


def _cora_job(rank):
    from dgg_amd.distributed import ShardedGCN_DGG
    m, x, A, _ = cora()
    net = ShardedGCN_DGG(m).eval()
    outs = []
    with torch.no_grad():
        for _ in range(2):                                       # (the undecided graph's collective flag on every forward)
            outs.append(net(x, A)[0].cpu().numpy())
    assert m.dggs[0].__dict__.get("fused_fallback") is None
    return net.rows, outs


def test_cora_through_two_ranks_is_the_one_process_model():
    (rows0, o0), (rows1, o1) = two_ranks("_cora_job")
    m, x, A, fx = cora()
    with torch.no_grad():
        ref = m(x, A)[0].cpu().numpy()
    assert m.dggs[0].__dict__.get("fused_fallback") is None
    for a, b in zip(o0, o1):
        assert np.array_equal(np.concatenate([a, b]), ref)
    err = np.abs(ref - fx["out"]) / (np.abs(fx["out"]) + 2.0)     # (the bar of test_cora_named_models_match_reference)
    assert err.max() <= 2e-3 and (err > 1e-5).any(1).sum() <= 0.05 * ref.shape[0]


def _refuse_job(rank):
    from dgg_amd.distributed import ShardedGCN_DGG
    m, x, A, _, _ = setup("u-v-dist", "asym", wide_rank1=True)
    net = ShardedGCN_DGG(m).eval()
    try:
        net(x, A)
    except NotImplementedError as e:
        return "NotImplementedError", str(e)
    return "no error", ""


def test_a_wide_row_on_one_rank_refuses_on_both():
    r0, r1 = two_ranks("_refuse_job")
    assert r0[0] == r1[0] == "NotImplementedError", (r0, r1)
    assert r0[1] == r1[1] and "edge-list candidates" in r0[1]


def _adam_job(rank, steps):
    from dgg_amd.distributed import ShardedGCN_DGG, global_nll_loss
    m, x, A, labels, idx = setup("u-v-deg", "asym")
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


def test_adam_on_an_edge_list_keeps_the_ranks_bit_identical():
    h0, h1 = two_ranks("_adam_job", 5)
    assert len(h0) == len(h1) == 5
    for (l0, p0), (l1, p1) in zip(h0, h1):
        assert np.isfinite(l0) and l0 == l1
        assert np.array_equal(p0, p1)
    assert not np.array_equal(h0[0][1], h0[-1][1])           # (the parameters moved)
