#!/usr/bin/env python3
"""Times u-v-A_uv on all-pairs candidates against a sparse prior (ops.allpairs_mlp_topk(..., prior=)) beside u-v-deg on the same shapes
(diagnostic, one GPU): h = hw = 64, per-pair hash noise, a prior of --per-row random entries per row plus self loops; the same kernel
on an EMPTY prior (no tile ever holds an entry) is timed next to it: the difference is what the lookup costs.

    python tools/time_allpairs_prior.py [N ...] [--hw 64] [--per-row 4] [--windows 7] [--baseline-lib PATH/libdgg_hip.so] [--dist]

--baseline-lib: a second build of the library (for instance the parent commit's); its dgg_allpairs_mlp_topk (u-v-deg) and
dgg_allpairs_mlp_topk_prior (u-v-A_uv with the prior) are timed in the same process, alternating with the others, after their outputs
were found bit-equal to the tree's, so that "the kernels did not move" is read off one run under the same clocks (tools/baseline_lib.py).
--dist: u-v-deg-dist (the distance extra) as well.
Each figure is the median over `windows` timed windows (device events around `reps` back-to-back calls, a window lasts about a quarter
of a second), with the smallest and largest window next to it: that spread is what a difference has to exceed."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dgg_amd  # noqa: E402
from dgg_amd import ops  # noqa: E402
from baseline_lib import Baseline, compare, same_bits  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int, default=[100000])
ap.add_argument("--hw", type=int, default=64)
ap.add_argument("--per-row", type=int, default=4)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--baseline-lib", default=None)
ap.add_argument("--dist", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_allpairs_prior.py needs a GPU"
dev = torch.device("cuda", 0)
hw = h = a.hw
base = Baseline(a.baseline_lib) if a.baseline_lib else None


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps                       # ms per call


def reps_for(fn):
    fn()
    fn()                                                    # (warm: code objects loaded, allocator settled)
    torch.cuda.synchronize()
    t1 = max(window(fn, 1), 1e-3)
    return max(1, min(500, int(250.0 / t1)))


for N in a.sizes:
    g = torch.Generator().manual_seed(N)
    xp = (torch.randn(N, h, generator=g) * 0.3).to(dev)
    Wcat = (torch.randn(2 * hw, h, generator=g) * 0.3).to(dev)
    AB = ops.linear_fwd(xp, Wcat, None, ops.ACT_NONE)
    v = lambda s: (torch.randn(hw, generator=g) * s).to(dev)  # noqa: E731
    wdu, wdv, wex, b1, w2, b2 = v(0.05), v(0.05), v(0.5), v(0.1), v(0.4), torch.tensor([0.1], device=dev)
    rows = torch.arange(N).repeat_interleave(a.per_row)
    cols = torch.randint(0, N, (N * a.per_row,), generator=g)
    G = torch.sparse_coo_tensor(torch.stack([rows, cols]), torch.ones(N * a.per_row), (N, N)).coalesce().to(dev)
    A = dgg_amd.AllPairs.from_graph(G, self_loops=True)
    deg, prior = A.prior_degree, A.prior_csr()[:3]
    idx = torch.empty((N, 64), device=dev, dtype=torch.int32)
    val = torch.empty((N, 64), device=dev, dtype=torch.float32)
    ex = torch.empty((N, 64), device=dev, dtype=torch.float32)

    def uvdeg():
        return ops.allpairs_mlp_topk(AB, xp, deg, 0, 0.0, wdu, wdv, None, b1, w2, b2, ops.ACT_LEAKY, 64, ops.NOISE_HASH, None, (9, 4),
                                     out=(idx, val, None))

    def uvauv():
        return ops.allpairs_mlp_topk(AB, xp, None, 1, 0.0, None, None, wex, b1, w2, b2, ops.ACT_LEAKY, 64, ops.NOISE_HASH, None, (9, 4),
                                     out=(idx, val, ex), prior=prior)

    empty = (torch.zeros_like(prior[0]), prior[1][:1], prior[2][:1])     # (no row points into the arrays: the same kernel, never a hit)

    def uvauv_empty():
        return ops.allpairs_mlp_topk(AB, xp, None, 1, 0.0, None, None, wex, b1, w2, b2, ops.ACT_LEAKY, 64, ops.NOISE_HASH, None, (9, 4),
                                     out=(idx, val, ex), prior=empty)

    def uvdist():
        return ops.allpairs_mlp_topk(AB, xp, deg, 2, -1.0, wdu, wdv, wex, b1, w2, b2, ops.ACT_LEAKY, 64, ops.NOISE_HASH, None, (9, 4),
                                     out=(idx, val, ex))

    paths = {"u-v-A_uv with the prior": uvauv, "u-v-A_uv, empty prior": uvauv_empty, "u-v-deg": uvdeg}
    if a.dist:
        paths["u-v-deg-dist"] = uvdist
    both = [name for name in paths if name != "u-v-A_uv, empty prior"] if base is not None else []
    for name in both:
        fn_base = base.calls(paths[name])
        r_tree = tuple(None if t_ is None else t_.clone() for t_ in paths[name]())
        assert same_bits(r_tree, fn_base()), f"the two builds disagree on {name}"
        paths[name + ", baseline build"] = fn_base
    uvauv()
    torch.cuda.synchronize()
    kept_edges = int((ex != 0).sum())
    reps = {name: reps_for(fn) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(a.windows):                              # alternate the paths window by window
        for name, fn in paths.items():
            times[name].append(window(fn, reps[name]))
    out = dict(N=N, hw=hw, h=h, noise="hash", prior_nnz=int(prior[1].shape[0]), kept_prior_edges=kept_edges, windows=a.windows)
    for name, ts in times.items():
        med = statistics.median(ts)
        print(f"N={N:7d} hw={hw}  {name:41s} median {med:10.3f} ms  (windows {min(ts):.3f} .. {max(ts):.3f} ms, {reps[name]} calls each)", flush=True)
        out[name.replace(",", "").replace(" ", "_") + "_ms"] = dict(median=med, min=min(ts), max=max(ts), reps=reps[name])
    out["ratio_prior_over_empty_prior"] = statistics.median(times["u-v-A_uv with the prior"]) / statistics.median(times["u-v-A_uv, empty prior"])
    out["ratio_prior_over_uvdeg"] = statistics.median(times["u-v-A_uv with the prior"]) / statistics.median(times["u-v-deg"])
    for name in both:
        out["vs_baseline_" + name.replace(" ", "_")] = compare(times[name], times[name + ", baseline build"])
    print(json.dumps(out), flush=True)
