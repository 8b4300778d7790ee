#!/usr/bin/env python3
"""ms per training step (forward, nll loss on a fifth of the nodes, backward) of GCN_DGG on its fused path and of the same model
through dgg_amd.distributed.ShardedGCN_DGG at one rank (no process group: the wrapper's own overhead), one GPU, all-pairs candidates
at N = 100 000, d = 128, h = 64, k ~ 32, asymmetric noise.  The two are timed in alternating windows.
python tools/time_sharded_module.py [N] [steps per window] [windows]"""
import json
import os
import sys
import time
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import dgg_amd  # noqa: E402
from dgg_amd.distributed import ShardedGCN_DGG, global_nll_loss  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
windows = int(sys.argv[3]) if len(sys.argv) > 3 else 5
d, h, C = 128, 64, 16
dev = torch.device("cuda", 0)
args = Namespace(extra_edge_dim=0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288, dgg_mode_edge_net="u-v-dist",
                 dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=True,
                 symmetric_noise=False, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
torch.manual_seed(0)
m = dgg_amd.GCN_DGG(nfeat=d, nhidden=h, nclass=C, args=args)
with torch.no_grad():
    m.dggs[0].k_net.k_project.weight.mul_(0.1)
m = m.to(dev).train()
m.dggs[0].set_seed(1234, 0)
g = torch.Generator().manual_seed(1000)
x = torch.randn(N, d, generator=g).to(dev)
cand = dgg_amd.AllPairs((24 + 16 * torch.rand(N, generator=g)).to(dev))
labels = torch.randint(0, C, (N,), generator=g).to(dev)
idx = torch.randperm(N, generator=g)[: N // 5].to(dev)
net = ShardedGCN_DGG(m)
params = list(m.parameters())


def step_model():
    for p in params:
        p.grad = None
    out, adj, _ = m(x, cand)
    F.nll_loss(out[idx], labels[idx]).backward()
    return adj


def step_wrapper():
    for p in params:
        p.grad = None
    out, adj, _ = net(x, cand)
    F.nll_loss(out[idx], labels[idx]).backward()
    return adj


def step_wrapper_global_loss():
    for p in params:
        p.grad = None
    out, adj, _ = net(x, cand)
    global_nll_loss(out, labels, idx, net.rows).backward()
    return adj


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        adj = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, adj


fns = {"model": step_model, "wrapper": step_wrapper, "wrapper_global_loss": step_wrapper_global_loss}
for fn in fns.values():
    for _ in range(5):
        fn()
res = {k: [] for k in fns}
for _ in range(windows):
    for k, fn in fns.items():
        ms, adj = window(fn)
        res[k].append(ms)
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
print(json.dumps({"N": N, "d": d, "h": h, "k_mean": round(float(adj.k.mean()), 2), "fused_path_ms": round(med["model"], 4),
                  "wrapper_world1_ms": round(med["wrapper"], 4), "wrapper_over_fused": round(med["wrapper"] / med["model"] - 1, 4),
                  "wrapper_world1_global_nll_loss_ms": round(med["wrapper_global_loss"], 4),
                  "windows_ms": {k: [round(v_, 4) for v_ in v] for k, v in res.items()}}))
