#!/usr/bin/env python3
"""Times one training step (forward + backward) of GCN_DGG on a Pubmed-SHAPED synthetic edge-list graph whose wide rows are live, on one
GPU (diagnostic): the fused layer on chunked rows (args.dgg_edgelist_rows = "chunked") against the CSR form as separate modules, which is
where the same model goes without the argument (args.dgg_wide_rows = "auto": sticky from the first forward that needs it).

    python tools/time_edgelist_chunked.py [--scorer u-v-dist u-v-deg] [--windows 7]

Graph: N = 19 717 nodes, d = 500 features, h = 64, 3 classes; 1-30 candidates a row with a mean near 4.5 (+ the self loop the model
adds) and 40 rows of 65 .. 171 candidates (Pubmed's widest row has 171).  The k-net weights make k = deg + 1 (the helper of
tests/test_sharded_edgelist_csr.py), so every row wider than the list has a learned degree beyond it.  Synthetic features and graph:
the step's kernel sequence and sizes are Pubmed's, its numbers are not.

Each figure is the median over `windows` timed windows (device events around `reps` back-to-back steps, reps chosen so that a window
lasts about a quarter of a second), with the smallest and largest window next to it; the two variants alternate window by window, and
their losses are compared before anything is timed.  One JSON line per figure."""
import argparse
import copy
import json
import os
import statistics
import sys
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dgg_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scorer", nargs="*", default=["u-v-dist", "u-v-deg"], choices=["u-v-dist", "u-v-deg", "u-v-A_uv", "u-v-deg-dist", "edge_conv"])
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--nodes", type=int, default=19717)
a = ap.parse_args()
assert torch.cuda.is_available(), "time_edgelist_chunked.py needs a GPU"
dev = torch.device("cuda", 0)
D, H, C = 500, 64, 3


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps                       # ms per step


def reps_for(fn):
    fn()
    fn()                                                    # (warm: code objects loaded, allocator settled, the CSR decision taken)
    torch.cuda.synchronize()
    t1 = max(window(fn, 1), 1e-3)
    return max(1, min(500, int(250.0 / t1)))


def pubmed_shaped_graph(N):
    rng = np.random.default_rng(N)
    n = np.minimum(1 + rng.geometric(1.0 / 3.5, N), 30)
    wide = rng.choice(N, 40, replace=False)
    n[wide] = np.linspace(65, 171, 40).astype(np.int64)
    rows = np.repeat(np.arange(N), n)
    cols = np.concatenate([rng.choice(N, c, replace=False) for c in n])
    keep = rows != cols                                     # (the model adds the self loops)
    ind = torch.from_numpy(np.stack([rows[keep], cols[keep]]))
    return torch.sparse_coo_tensor(ind, torch.ones(ind.shape[1]), (N, N)).coalesce(), int(n.max()), float(n.mean())


def degree_knet(dgg, h):
    """k-net weights that make k = deg + 1"""
    with torch.no_grad():
        for lin in (dgg.k_embed[0], dgg.k_net.k_mu, dgg.k_net.k_project):
            lin.weight.zero_()
            lin.bias.zero_()
        dgg.k_embed[0].weight[0, h] = 1.0                    # the normalised-degree input
        dgg.k_net.k_mu.weight[0, 0] = 1.0
        dgg.k_net.k_project.weight[0, 0] = 1.0


def case(scorer, N):
    args = Namespace(extra_edge_dim={"u-v-deg": 2, "u-v-deg-dist": 3, "u-v-A_uv": 1}.get(scorer, 0), extra_k_dim=1, dgg_hard=False, deg_mean=3.899,
                     deg_std=5.288, dgg_mode_edge_net=scorer, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3,
                     perturb_edge_prob=True, symmetric_noise=False, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1,
                     dgg_edgelist_rows="chunked")
    torch.manual_seed(3)
    chunked = dgg_amd.GCN_DGG(nfeat=D, nhidden=H, nclass=C, args=args)
    degree_knet(chunked.dggs[0], H)
    with torch.no_grad():
        chunked.conv1.W.mul_(0.05)                           # (W ~ U[0, 1) over 500 features: keeps the activations of order one)
    chunked = chunked.to(dev).eval()                         # (eval: no dropout, the two models compare)
    csr = copy.deepcopy(chunked)
    csr.dggs[0].args = Namespace(**dict(vars(args), dgg_edgelist_rows="list"))
    g = torch.Generator().manual_seed(N)
    x = torch.randn(N, D, generator=g).to(dev)
    y = torch.randint(0, C, (N,), generator=g).to(dev)
    A, widest, mean = pubmed_shaped_graph(N)
    A = A.to(dev)

    def step(m):
        def run():
            m.dggs[0].set_seed(9, 4)
            for p_ in m.parameters():
                p_.grad = None
            logp, adj, _ = m(x, A)
            loss = torch.nn.functional.nll_loss(logp, y)
            loss.backward()
            return loss.detach(), adj
        return run

    paths = {"CSR form, separate modules": step(csr), "fused layer, chunked rows": step(chunked)}
    step(csr)()                                              # (the first forward discovers the wide rows and leaves the fused layer for good)
    (l1, a1), (l2, a2) = paths["fused layer, chunked rows"](), paths["CSR form, separate modules"]()
    assert type(a1).__name__ == "EllAdjacency" and a1.layout is not None and a1.layout.wide and not chunked.dggs[0].__dict__.get("fused_fallback")
    assert type(a2).__name__ == "CsrAdjacency", "the case does not run the form it names"
    assert abs(float(l1) - float(l2)) <= 1e-4 * abs(float(l2)), f"the two forms disagree: {float(l1)} vs {float(l2)}"
    tags = dict(scorer=scorer, N=N, d=D, h=H, candidates_mean=round(mean + 1, 2), widest_row=widest + 1, k_max=round(float(a1.k.max()), 1),
                chunks=a1.layout.chunks, chunks_widest_row=a1.layout.maxm)
    reps = {name: reps_for(fn) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(a.windows):
        for name, fn in paths.items():
            times[name].append(window(fn, reps[name]))
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        print(json.dumps(dict(tags, what=name, median_ms=round(med[name], 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), reps=reps[name],
                              windows=a.windows)), flush=True)
    print(json.dumps(dict(tags, chunked_over_csr=round(med["fused layer, chunked rows"] / med["CSR form, separate modules"], 3))), flush=True)


for scorer in a.scorer:
    case(scorer, a.nodes)
