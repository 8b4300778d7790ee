"""ShardedGCN_DGG's CSR form of wide edge-list rows (args.dgg_wide_rows = "csr" / "csr_auto") on two ranks sharing one MI355X over gloo
(this process is rank 0, one spawned child rank 1; the harness of test_sharded_edgelist_module.py).

Graph: N = 2001 (shards of 1001 and 1000 rows), d = h = 64, 16 classes, rows of 1-60 candidates and three rows of 100 in rank 1's half
only; the k-net weights make k = deg + 1, so those rows need more ranks than the 64-rank list holds and rank 0 owns no wide row.
Forward: the concatenated log-probabilities and each rank's adjacency rows equal the single-process model under the same policy bit
for bit.  Gradients: the same keys everywhere, bit-equal between the ranks, and against the single process the bar of
test_two_ranks_match_single_process (1e-5 of the maximum, 1e-4 for dggs.0.edge_*, or twice the single process's own call-to-call
spread).  "csr_auto": the fused layer until the collective flag fires, then the CSR form, sticky.  Five Adam steps keep the ranks
bit-identical.  Cora's reference fixture through two ranks in CSR form is the one-process CSR model and meets the golden's bar.
On the parent commit every test of this file raises NotImplementedError (args.dgg_wide_rows)."""
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
N_SYN = 2001
WIDE = (N_SYN - 7, N_SYN - 300, N_SYN - 900)                  # rank 1's half only (rows 1001 ..)
CASES = [("u-v-dist", "none"), ("u-v-dist", "asym"), ("u-v-dist", "sym"), ("u-v-deg", "asym"), ("edge_conv", "sym")]


def model_args(scorer, noise, policy):
    return Namespace(extra_edge_dim=2 if scorer == "u-v-deg" else 0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288,
                     dgg_mode_edge_net=scorer, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3,
                     perturb_edge_prob=noise != "none", symmetric_noise=noise == "sym", stochastic_k=False, dgg_adj_input="input_adj",
                     n_dgg_layers=1, dgg_wide_rows=policy)


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


def degree_knet(dgg, h, scale=1.0):
    """k-net weights that make k = relu(scale * (deg - mean) + mean) + 1 (k = deg + 1 at scale 1): in place, the same on every rank"""
    with torch.no_grad():
        for lin in (dgg.k_embed[0], dgg.k_net.k_mu, dgg.k_net.k_project):
            lin.weight.zero_()
            lin.bias.zero_()
        dgg.k_embed[0].weight[0, h] = 1.0                    # the normalised-degree input
        dgg.k_net.k_mu.weight[0, 0] = 1.0
        dgg.k_net.k_project.weight[0, 0] = scale


def setup(scorer, noise, policy="csr", d=64, h=64, nclass=16, knet_scale=1.0):
    import dgg_amd
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = dgg_amd.GCN_DGG(nfeat=d, nhidden=h, nclass=nclass, args=model_args(scorer, noise, policy))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N_SYN, d, generator=g)
    A = synthetic_graph(N_SYN, WIDE)
    degree_knet(m.dggs[0], h, knet_scale)
    m = m.to(dev)
    m.dggs[0].set_seed(1234, 5)
    labels = torch.randint(0, nclass, (N_SYN,), generator=g)
    idx = torch.randperm(N_SYN, generator=g)[: N_SYN // 5]
    return m, x.to(dev), A.to(dev), labels.to(dev), idx.to(dev)


def grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def adj_arrays(adj):
    return type(adj).__name__, tuple(adj.shape), adj.col.cpu().numpy(), adj.values().detach().cpu().numpy()


# ---- two ranks on one GPU (the harness of test_sharded_edgelist_module) ------------------------------------------------------------
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


_CALLS = [0]


def two_ranks(job_name, *args):
    # (a port of its own per call: rank 0 hosts the rendezvous store in this process, and a store of an earlier call that is still
    #  alive on the same port would be reused with the dead child's address in it)
    _CALLS[0] += 1
    port = 31800 + (os.getpid() % 2000) * 8 % 16000 + _CALLS[0]
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
    return net.rows, out.detach().cpu().numpy(), adj_arrays(adj), {k: v.cpu().numpy() for k, v in grads(m).items()}


@pytest.mark.parametrize("scorer,noise", CASES)
def test_two_ranks_in_csr_form_match_the_single_process(scorer, noise):
    (rows0, o0, a0, ga), (rows1, o1, a1, gb) = two_ranks("_eval_job", scorer, noise)
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
    assert rows0 == (0, 1001) and rows1 == (1001, N_SYN)
    assert np.array_equal(np.concatenate([o0, o1]), out.detach().cpu().numpy())
    assert type(adj).__name__ == "CsrAdjacency"
    rowptr = adj.rowptr.cpu().numpy()
    for (r0, r1), (kind, shape, col, val) in ((rows0, a0), (rows1, a1)):
        e0, e1 = rowptr[r0], rowptr[r1]
        assert kind == "CsrAdjacency" and shape == (r1 - r0, N_SYN)
        assert np.array_equal(col, adj.col[e0:e1].cpu().numpy()) and np.array_equal(val, adj.values()[e0:e1].detach().cpu().numpy())
    g1 = grads(m)
    assert set(g1) == set(ga) == set(gb)
    if scorer != "u-v-dist":
        assert any("edge" in k for k in g1)                      # (the scorer's own parameters got their gradient)
    for k, v in g1.items():
        v = v.cpu().numpy()
        assert np.array_equal(ga[k], gb[k]), k
        rel = 1e-4 if k.startswith("dggs.0.edge_") else 1e-5
        bar = max(rel * max(np.abs(v).max(), 1e-30), 2 * spread[k])
        print("  %-44s err %.3e  max %.3e  spread %.3e  bar %.3e" % (k, np.abs(ga[k] - v).max(), np.abs(v).max(), spread[k], bar))
        assert np.abs(ga[k] - v).max() <= bar, (k, np.abs(ga[k] - v).max(), np.abs(v).max(), spread[k])


def _switch_sequence(net, m, x, A):
    """small degrees -> the fused layer; then k = deg + 1 in place -> the CSR form, twice"""
    outs = []
    with torch.no_grad():
        out, adj, _ = net(x, A)
        outs.append((type(adj).__name__, out.cpu().numpy(), m.dggs[0].__dict__.get("fused_fallback")))
        degree_knet(m.dggs[0], 64, 1.0)
        for _ in range(2):
            out, adj, _ = net(x, A)
            outs.append((type(adj).__name__, out.cpu().numpy(), tuple(adj.shape)))
    return outs


def _switch_job_outs(rank):
    from dgg_amd.distributed import ShardedGCN_DGG
    m, x, A, _, _ = setup("u-v-dist", "asym", policy="csr_auto", knet_scale=0.05)
    net = ShardedGCN_DGG(m).eval()
    return net.__class__.__name__, _switch_sequence(net, m, x, A)


def test_csr_auto_switches_on_both_ranks_in_the_same_forward_and_stays():
    (_, s0), (_, s1) = two_ranks("_switch_job_outs")
    m, x, A, _, _ = setup("u-v-dist", "asym", policy="csr_auto", knet_scale=0.05)
    ref = _switch_sequence(m.eval(), m, x, A)
    assert s0[0][0] == s1[0][0] == ref[0][0] == "EllAdjacency" and s0[0][2] is None and s1[0][2] is None
    for q in (1, 2):
        assert s0[q][0] == s1[q][0] == ref[q][0] == "CsrAdjacency"
        assert s0[q][2] == (1001, N_SYN) and s1[q][2] == (1000, N_SYN)
    for q in range(3):
        assert np.array_equal(np.concatenate([s0[q][1], s1[q][1]]), ref[q][1]), q
    assert not np.array_equal(ref[0][1], ref[1][1])


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


def test_adam_in_csr_form_keeps_the_ranks_bit_identical():
    h0, h1 = two_ranks("_adam_job", 5)
    assert len(h0) == len(h1) == 5
    for (l0, p0), (l1, p1) in zip(h0, h1):
        assert np.isfinite(l0) and l0 == l1
        assert np.array_equal(p0, p1)
    assert not np.array_equal(h0[0][1], h0[-1][1])           # (the parameters moved)


def cora():
    """the fixture set-up of test_cora_through_two_ranks_is_the_one_process_model under the CSR policy (its args: u-v-deg scorer, k-net
    x, k_times_edge_prob, no noise -- inside _fused_outside's coverage, checked on the CPU by tests/test_sharded_csr_host.py)"""
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
    m = dgg_amd.GCN_DGG(nfeat=d, nlayers=2, nhidden=h, nclass=C, args=Namespace(dgg_wide_rows="csr", **meta["args"]))
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
        for _ in range(2):
            out, adj, _ = net(x, A)
            assert type(adj).__name__ == "CsrAdjacency"
            outs.append(out.cpu().numpy())
    return net.rows, outs


def test_cora_through_two_ranks_in_csr_form_is_the_one_process_csr_model():
    (rows0, o0), (rows1, o1) = two_ranks("_cora_job")
    m, x, A, fx = cora()
    with torch.no_grad():
        ref, adj, _ = m(x, A)
    ref = ref.cpu().numpy()
    assert type(adj).__name__ == "CsrAdjacency"
    for a, b in zip(o0, o1):
        assert np.array_equal(np.concatenate([a, b]), ref)
    err = np.abs(ref - fx["out"]) / (np.abs(fx["out"]) + 2.0)     # (the bar of test_cora_named_models_match_reference)
    assert err.max() <= 2e-3 and (err > 1e-5).any(1).sum() <= 0.05 * ref.shape[0]
