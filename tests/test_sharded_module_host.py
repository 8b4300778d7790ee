"""dgg_amd.distributed without a GPU: global_nll_loss under gloo worlds of 2 and 3 on CPU tensors reproduces the whole graph's
F.nll_loss (value and gradient of the log-probabilities), and ShardedGCN_DGG refuses what it does not cover instead of falling back."""
import os
import sys
from argparse import Namespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model_args(**kw):
    a = dict(extra_edge_dim=0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288, dgg_mode_edge_net="u-v-dist",
             dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=True, symmetric_noise=False,
             stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
    a.update(kw)
    return Namespace(**a)


def loss_inputs(N=37, C=5):
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(N, C, generator=g)
    labels = torch.randint(0, C, (N,), generator=g)
    idx = torch.cat([torch.randperm(N, generator=g)[:15], torch.tensor([4, 4])])      # (a repeated index counts twice, as in nll_loss)
    mask = torch.rand(N, generator=g) < 0.4
    return logits, labels, idx, mask


def _loss_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from dgg_amd.distributed import global_nll_loss
    from dgg_amd.parallel import shard_bounds
    logits, labels, idx, mask = loss_inputs()
    r0, r1, _ = shard_bounds(logits.shape[0], world, rank)
    out = {}
    for name, sel in (("index", idx), ("mask", mask)):
        lp = F.log_softmax(logits, -1)[r0:r1].clone().requires_grad_(True)
        loss = global_nll_loss(lp, labels, sel, (r0, r1))
        loss.backward()
        out[name] = (float(loss.detach()), lp.grad.clone())
    ret[rank] = (r0, r1, out)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_global_nll_loss_matches_whole_graph_nll_loss(world):
    port = 29600 + (os.getpid() + 7 * world) % 2000
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_loss_worker, args=(r, world, port, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        if p.is_alive():
            p.kill()
            pytest.fail("a rank did not finish")
    assert all(p.exitcode == 0 for p in procs) and len(ret) == world
    logits, labels, idx, mask = loss_inputs()
    for name, sel in (("index", idx), ("mask", mask)):
        lp = F.log_softmax(logits, -1).clone().requires_grad_(True)
        ref = F.nll_loss(lp[sel], labels[sel])
        ref.backward()
        grad = torch.zeros_like(lp)
        for r in range(world):
            r0, r1, out = ret[r]
            val, g = out[name]
            assert abs(val - float(ref.detach())) <= 1e-6 * max(1.0, abs(float(ref.detach()))), (name, r, val)
            grad[r0:r1] = g
        torch.testing.assert_close(grad, lp.grad, rtol=0, atol=1e-7)


def test_global_nll_loss_without_a_process_group_is_nll_loss():
    sys.path.insert(0, ROOT)
    from dgg_amd.distributed import global_nll_loss
    logits, labels, idx, _ = loss_inputs()
    lp = F.log_softmax(logits, -1)
    torch.testing.assert_close(global_nll_loss(lp, labels, idx, (0, lp.shape[0])), F.nll_loss(lp[idx], labels[idx]), rtol=1e-6, atol=1e-7)


def _model(**kw):
    sys.path.insert(0, ROOT)
    import dgg_amd
    torch.manual_seed(0)
    return dgg_amd.GCN_DGG(nfeat=16, nhidden=16, nclass=16, args=model_args(**kw))


def test_wrapper_shares_the_models_parameters_and_state_dict():
    from dgg_amd.distributed import ShardedGCN_DGG
    m = _model()
    net = ShardedGCN_DGG(m)
    assert list(net.state_dict().keys()) == list(m.state_dict().keys())
    assert net.params1 is m.params1 and net.params2 is m.params2
    assert {id(p) for p in net.parameters()} == {id(p) for p in m.parameters()}
    sd = {k: v + 1 for k, v in m.state_dict().items()}
    net.load_state_dict(sd)
    assert torch.equal(m.conv2.W, sd["conv2.W"])
    with pytest.raises(RuntimeError, match="first forward"):
        net.rows


def test_wrapper_refuses_what_it_does_not_cover():
    import dgg_amd
    from dgg_amd.distributed import ShardedGCN_DGG
    N = 64
    x = torch.randn(N, 16)
    cand = dgg_amd.AllPairs(torch.full((N,), 8.0))
    net = ShardedGCN_DGG(_model())
    with pytest.raises(NotImplementedError, match="writer"):
        net(x, cand, writer=object())
    with pytest.raises(ValueError, match="gradient"):
        net(x.requires_grad_(True), cand)
    x = x.detach()
    with pytest.raises(NotImplementedError, match="not on the GPU"):            # (a configuration forward_conv declines)
        net(x, cand)
    with pytest.raises(NotImplementedError, match="dgg_hard_literal"):
        ShardedGCN_DGG(_model(dgg_hard_literal=True))(x, cand)
    with pytest.raises(NotImplementedError, match="dgg_differentiable_adj"):
        ShardedGCN_DGG(_model(dgg_differentiable_adj=True))(x, cand)
    with pytest.raises(NotImplementedError, match="dgg_wide_rows"):
        ShardedGCN_DGG(_model(dgg_wide_rows="csr"))(x, cand)
    with pytest.raises(TypeError):
        ShardedGCN_DGG(torch.nn.Linear(2, 2))


def _refuse_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    import dgg_amd
    from dgg_amd.distributed import ShardedGCN_DGG
    N = 40
    x = torch.randn(N, 16)
    A = torch.sparse_coo_tensor(torch.stack([torch.arange(N), (torch.arange(N) + 1) % N]), torch.ones(N), (N, N)).coalesce()
    got = []
    net = ShardedGCN_DGG(_model())
    try:
        net(x, A)
    except NotImplementedError as e:
        got.append(str(e))
    try:
        ShardedGCN_DGG(_model(symmetric_noise=True, dgg_sym_generator="auto"))(x, dgg_amd.AllPairs(torch.full((N,), 8.0)))
    except NotImplementedError as e:
        got.append(str(e))
    ret[rank] = got
    dist.destroy_process_group()


def test_wrapper_refuses_edge_lists_and_a_per_rank_generator_switch_on_two_ranks():
    port = 29650 + os.getpid() % 2000
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_refuse_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        if p.is_alive():
            p.kill()
            pytest.fail("a rank did not finish")
    assert all(p.exitcode == 0 for p in procs)
    for r in range(2):
        assert len(ret[r]) == 2, ret[r]
        assert "edge-list candidates" in ret[r][0]
        assert "dgg_sym_generator" in ret[r][1]
