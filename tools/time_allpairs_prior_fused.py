#!/usr/bin/env python3
"""Times the scorer u-v-A_uv on all-pairs candidates that carry a prior graph through the module API on one GPU (diagnostic): forward +
backward of GCN_DGG with the fused layer (DGG_LearnableK_debug.forward_conv on ShardedDGGConv; opt-in args.dgg_allpairs_prior_fused = True)
against the separate modules (args.dgg_fused_layer = False), h = hw = 64, per-pair hash noise.  The prior: 4 random entries per row of
weight 1 plus the self loops; the prior degrees are set apart from it, so that the learned degrees land where the part says.
(After tools/time_allpairs_mlp_fused.py, which times u-v-deg at the same four points.)

    python tools/time_allpairs_prior_fused.py [--part list|chunked|rank8 ...] [--windows 7]

    list     N = 4096 and 20000, learned degrees ~ 32: the 64-rank list (dgg_allpairs_mlp_topk_prior)
    chunked  N = 4096 and 20000, learned degrees ~ 130 under args.dgg_allpairs_mlp_rows = "chunked": three chunks per row
             (dgg_allpairs_mlp_topk_wide_prior); the separate modules convert the chunked adjacency to CSR on every forward
    rank8    N = 100000, list form, the engine step alone: the whole graph on one GPU against ONE EMULATED rank of eight
             (ShardedDGGConv.emulate_rank(8, r): the rank's 12 500 rows against all N columns and the whole prior, replicated features,
             the collectives left out, the other ranks' row sums faked).  An emulation of one rank's compute on one GPU -- no run on
             several GPUs exists.

Each figure is the median over `windows` timed windows (device events around `reps` back-to-back steps, reps chosen so that a window
lasts about a quarter of a second), with the smallest and largest window next to it; the variants of a part alternate window by window,
and their losses are compared before anything is timed.  One JSON line per figure."""
import argparse
import copy
import json
import os
import statistics
import sys
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dgg_amd  # noqa: E402
from dgg_amd import ops  # noqa: E402
from dgg_amd.parallel import ShardedDGGConv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", nargs="*", default=["list", "chunked", "rank8"], choices=["list", "chunked", "rank8"])
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 20000])
a = ap.parse_args()
assert torch.cuda.is_available(), "time_allpairs_prior_fused.py needs a GPU"
dev = torch.device("cuda", 0)
H = 64


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
    fn()                                                    # (warm: code objects loaded, allocator settled)
    torch.cuda.synchronize()
    t1 = max(window(fn, 1), 1e-3)
    return max(1, min(500, int(250.0 / t1)))


def timed(paths, **tags):
    """alternates the paths window by window -> {name: median ms}; prints one JSON line per path"""
    reps = {name: reps_for(fn) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(a.windows):
        for name, fn in paths.items():
            times[name].append(window(fn, reps[name]))
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        print(json.dumps(dict(tags, what=name, median_ms=round(med[name], 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                              reps=reps[name], windows=a.windows)), flush=True)
    return med


def prior_graph(N, g):
    """4 random entries per row of weight 1 plus the self loops -> sparse COO [N, N] on the device (duplicates summed by AllPairs)"""
    rows = torch.arange(N).repeat_interleave(5)
    cols = torch.randint(0, N, (N, 5), generator=g)
    cols[:, 0] = torch.arange(N)
    return torch.sparse_coo_tensor(torch.stack([rows, cols.reshape(-1)]), torch.ones(5 * N), (N, N)).to(dev)


def module_case(N, k_about, chunked):
    args = Namespace(extra_edge_dim=1, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288, dgg_mode_edge_net="u-v-A_uv",
                     dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=True, symmetric_noise=False,
                     stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1, dgg_wide_rows="auto", dgg_allpairs_prior_fused=True,
                     dgg_allpairs_mlp_rows="chunked" if chunked else "list")
    torch.manual_seed(3)
    fused = dgg_amd.GCN_DGG(nfeat=H, nhidden=H, nclass=16, args=args).to(dev).eval()        # (eval: no dropout, the two models compare)
    with torch.no_grad():
        fused.dggs[0].k_net.k_project.weight.mul_(0.1)      # (the learned degree stays near the priors' mean + 1)
    separate = copy.deepcopy(fused)
    separate.dggs[0].args = Namespace(**dict(vars(args), dgg_fused_layer=False))
    g = torch.Generator().manual_seed(N)
    x = torch.randn(N, H, generator=g).to(dev)
    y = torch.randint(0, 16, (N,), generator=g).to(dev)
    A = dgg_amd.AllPairs((k_about - 4.0 + 6.0 * torch.rand(N, generator=g)).round().to(dev), prior=prior_graph(N, g))

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

    (l1, a1), (l2, a2) = step(fused)(), step(separate)()
    assert fused.dggs[0].__dict__.get("_fused_layer") is not None and not fused.dggs[0].__dict__.get("fused_fallback")
    assert (a1.layout is not None) == chunked and (a2.layout is not None) == chunked, "the case does not run the form it names"
    assert abs(float(l1) - float(l2)) <= 1e-4 * abs(float(l2)), f"fused and separate modules disagree: {float(l1)} vs {float(l2)}"
    tags = dict(part="chunked" if chunked else "list", N=N, k_mean=round(float(a1.k.mean()), 1), k_max=round(float(a1.k.max()), 1))
    if chunked:
        tags["chunks_per_row"] = a1.layout.maxm
    m = timed({"separate modules": step(separate), "fused layer": step(fused)}, **tags)
    print(json.dumps(dict(tags, fused_over_separate=round(m["fused layer"] / m["separate modules"], 3))), flush=True)


def engine_case(N):
    g = torch.Generator().manual_seed(N)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev)  # noqa: E731
    x = r(N, H)
    deg = torch.randint(28, 35, (N,), generator=g).float().to(dev)
    P = dict(We=r(H, H, sc=0.1), be=r(H, sc=0.1), Wk=r(H, H, sc=0.1), bk=r(H, sc=0.1), W1=r(H // 2, H + 1, sc=0.1), b1=r(H // 2, sc=0.1),
             Wmu=r(H // 4, H // 2, sc=0.1), bmu=r(H // 4, sc=0.1), Wp=r(1, H // 4, sc=0.03), bp=torch.tensor([0.05], device=dev), Wc=r(H, H, sc=0.1))
    prior = dgg_amd.AllPairs(deg, prior=prior_graph(N, g)).prior_csr()[:3]
    sc = dict(Wcat=r(2 * H, H, sc=0.3), wdu=None, wdv=None, wex=r(H, sc=0.05), b1=r(H, sc=0.1), w2=r(H, sc=0.4),
              b2=torch.tensor([0.1], device=dev), erow=None, ex_in=None, ex_mode=1, t_ex=0.0, act=ops.ACT_LEAKY, prior=prior)

    def engine(rank_of_8):
        lay = ShardedDGGConv(ops, N, K=64, t=ops.T_DIST, noise_mode=ops.NOISE_HASH, seed=(9, 4), x_full=x, hybrid=True)
        lay.scorer = sc
        if rank_of_8 is not None:
            lay.emulate_rank(8, rank_of_8)
        xl = x[lay.r0:lay.r1].contiguous()
        cot = torch.ones((lay.r1 - lay.r0, H), device=dev)

        def run():
            lay.forward(xl, deg, P)
            return lay.backward(cot, xl, P)
        return run

    m = timed({"whole graph, one GPU": engine(None), "emulated rank 3 of 8": engine(3)}, part="rank8", N=N, form="list", k="~32")
    print(json.dumps(dict(part="rank8", N=N, whole_over_rank=round(m["whole graph, one GPU"] / m["emulated rank 3 of 8"], 2),
                          note="one rank's compute emulated on one GPU, collectives left out; not a multi-GPU run")), flush=True)


for part in a.part:
    if part == "rank8":
        engine_case(100000)
    else:
        for N in a.sizes:
            module_case(N, 130.0 if part == "chunked" else 32.0, part == "chunked")
