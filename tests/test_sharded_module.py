"""ShardedGCN_DGG on the MI355X: at one rank it is GCN_DGG's fused path (same kernels, same bits); with two ranks sharing one GPU
over gloo (this process is rank 0, one spawned child rank 1: two processes hold the GPU) the concatenated rows and the summed
gradients reproduce the single-process model, the symmetric-noise generator is chosen collectively when only one rank has chunked
rows, and Adam keeps the ranks' parameters bit-identical."""
import os
import sys
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NOISES = ("none", "asym", "sym")


def model_args(noise):
    from argparse import Namespace
    return Namespace(extra_edge_dim=0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288, dgg_mode_edge_net="u-v-dist",
                     dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=noise != "none",
                     symmetric_noise=noise == "sym", stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1,
                     dgg_sym_generator="ranked")


def setup(N, noise, nclass=16, d=128, h=64, wide_rank0=False):
    """-> model (cuda:0), x, AllPairs, labels, train index.  wide_rank0: prior degrees and k-net weights such that k = deg + 1 on the
    high-degree rows: the first 64 rows (rank 0's) need more than 64 ranks, every other row about 14"""
    sys.path.insert(0, ROOT)
    import dgg_amd
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = dgg_amd.GCN_DGG(nfeat=d, nhidden=h, nclass=nclass, args=model_args(noise))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, d, generator=g)
    deg = 24 + 16 * torch.rand(N, generator=g)
    dgg = m.dggs[0]
    with torch.no_grad():
        dgg.k_net.k_project.weight.mul_(0.1)
        if wide_rank0:
            deg = torch.full((N,), 10.0)
            deg[:64] = 120.0
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
    return m, x.to(dev), dgg_amd.AllPairs(deg.to(dev)), labels.to(dev), idx.to(dev)


def grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def single_step(m, x, cand, labels, idx):
    for p in m.parameters():
        p.grad = None
    out, adj, _ = m(x, cand)
    F.nll_loss(out[idx], labels[idx]).backward()
    torch.cuda.synchronize()
    return out.detach(), adj, grads(getattr(m, "module", m))


# ---- one rank, no process group ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,noise,nclass", [(4096, n, 16) for n in NOISES] + [(4096, "asym", 7)] + [(20000, n, 16) for n in NOISES])
def test_world_one_is_the_fused_path_bit_for_bit(N, noise, nclass):
    from dgg_amd.distributed import ShardedGCN_DGG
    m, x, cand, labels, idx = setup(N, noise, nclass)
    m.eval()
    out1, adj1, g1 = single_step(m, x, cand, labels, idx)
    _, _, g1b = single_step(m, x, cand, labels, idx)
    assert m.dggs[0].__dict__.get("fused_fallback") is None
    net = ShardedGCN_DGG(m)
    out2, adj2, g2 = single_step(net, x, cand, labels, idx)
    assert net.rows == (0, N)
    assert torch.equal(out1, out2)
    assert torch.equal(adj1.idx, adj2.idx) and torch.equal(adj1.values(), adj2.values())
    assert g1.keys() == g2.keys() and "convs.0.W" in g2 and "convs.1.W" in g2          # (conv1 / conv2)
    # the weight gradients of the fused path do not repeat their last bits from one call to the next (measured: up to 2e-6 of their
    # max between two identical calls of the model); the wrapper's differ from the model's by as little
    for k in g1:
        spread = float((g1[k] - g1b[k]).abs().max())
        assert float((g1[k] - g2[k]).abs().max()) <= max(1e-5 * float(g1[k].abs().max()), 2 * spread), k


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------
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
    """runs job(rank, *args) as rank 0 here and rank 1 in a spawned child -> (result 0, result 1)"""
    port = 29700 + os.getpid() % 2000
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


def _sharded_eval_job(rank, N, noise, wide_rank0):
    from dgg_amd.distributed import ShardedGCN_DGG, global_nll_loss
    m, x, cand, labels, idx = setup(N, noise, wide_rank0=wide_rank0)
    net = ShardedGCN_DGG(m).eval()
    out, adj, _ = net(x, cand)
    global_nll_loss(out, labels, idx, net.rows).backward()
    torch.cuda.synchronize()
    return (net.rows, out.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in grads(m).items()}, adj.layout is not None)


def _compare_with_single(res, N, noise, wide_rank0, exact):
    m, x, cand, labels, idx = setup(N, noise, wide_rank0=wide_rank0)
    m.eval()
    out1, adj1, g1 = single_step(m, x, cand, labels, idx)
    out1 = out1.cpu().numpy()
    (rows0, o0, ga, w0), (rows1, o1, gb, w1) = res
    assert rows0 == (0, rows1[0]) and rows1[1] == N
    cat = np.concatenate([o0, o1])
    if exact:
        assert np.array_equal(cat, out1), float(np.abs(cat - out1).max())
    else:
        np.testing.assert_allclose(cat, out1, rtol=0, atol=1e-5)
    for k, v in g1.items():
        v = v.cpu().numpy()
        assert np.array_equal(ga[k], gb[k]), k                 # (summed inside the autograd nodes: the same on both ranks)
        assert np.abs(ga[k] - v).max() <= 1e-5 * max(np.abs(v).max(), 1e-30), (k, np.abs(ga[k] - v).max(), np.abs(v).max())
    return adj1, (w0, w1)


@pytest.mark.parametrize("noise", NOISES)
def test_two_ranks_match_single_process(noise):
    N = 4096
    res = two_ranks("_sharded_eval_job", N, noise, False)
    _compare_with_single(res, N, noise, False, exact=True)


def test_symmetric_noise_with_chunked_rows_on_one_rank_only():
    """some of rank 0's rows need more than 64 ranks, none of rank 1's: both ranks must evaluate the symmetric per-pair hash (the
    generator of the chunked rows), as the single process does for every row"""
    N = 4096
    res = two_ranks("_sharded_eval_job", N, "sym", True)
    adj1, (w0, w1) = _compare_with_single(res, N, "sym", True, exact=False)
    assert adj1.layout is not None and w0 and not w1


def _adam_job(rank, N, steps):
    from dgg_amd.distributed import ShardedGCN_DGG, global_nll_loss
    m, x, cand, labels, idx = setup(N, "asym")
    net = ShardedGCN_DGG(m).train()
    opt = torch.optim.Adam([{"params": net.params1, "weight_decay": 5e-4}, {"params": net.params2, "weight_decay": 0.0}], lr=0.01)
    torch.cuda.manual_seed(100 + rank)                        # (each rank's own dropout masks)
    hist = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        out, _, _ = net(x, cand)
        loss = global_nll_loss(out, labels, idx, net.rows)
        loss.backward()
        opt.step()
        flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()
        hist.append((float(loss.detach()), flat))
    return hist


def test_adam_keeps_the_ranks_bit_identical():
    h0, h1 = two_ranks("_adam_job", 4096, 5)
    assert len(h0) == len(h1) == 5
    for (l0, p0), (l1, p1) in zip(h0, h1):
        assert np.isfinite(l0) and l0 == l1
        assert np.array_equal(p0, p1)
    assert not np.array_equal(h0[0][1], h0[-1][1])           # (the parameters moved)
