#!/usr/bin/env python3
"""Times the edge-MLP scorer on all-pairs candidates on one GPU (diagnostic): the one-kernel path (ops.allpairs_mlp_topk) and, up to
--compose-max nodes, the composed path it replaces (ops.edge_mlp_fwd + ops.edgelist_topk_p on the complete pattern, whose per-entry
arrays have N^2 elements).  Scorer u-v-deg, per-pair hash noise, h = hw = 64 unless told otherwise.

    python tools/time_allpairs_mlp.py [N ...] [--hw 64] [--scorer u-v-deg] [--noise hash] [--windows 7] [--compose-max 4096]

Each figure is the median over `windows` timed windows (device events around `reps` back-to-back calls, reps chosen so that a window lasts
about a quarter of a second), with the smallest and largest window next to it: that spread is what a difference has to exceed.  The two
paths alternate window by window, and their results are compared bit for bit before anything is timed."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgg_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int, default=[4096, 20000, 100000])
ap.add_argument("--hw", type=int, default=64)
ap.add_argument("--scorer", default="u-v-deg", choices=["u-v-deg", "u-v-deg-dist", "edge_conv"])
ap.add_argument("--noise", default="hash", choices=["none", "hash", "sym"])
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--compose-max", type=int, default=4096)
a = ap.parse_args()
assert torch.cuda.is_available(), "time_allpairs_mlp.py needs a GPU"
dev = torch.device("cuda", 0)
noise_mode = {"none": ops.NOISE_NONE, "hash": ops.NOISE_HASH, "sym": ops.NOISE_HASH_SYM}[a.noise]
hw = h = a.hw
ex_mode = 2 if a.scorer == "u-v-deg-dist" else 0
act = ops.ACT_NONE if a.scorer == "edge_conv" else ops.ACT_LEAKY


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
    deg = None if a.scorer == "edge_conv" else torch.randint(3, 20, (N,), generator=g).float().to(dev)
    v = lambda s: (torch.randn(hw, generator=g) * s).to(dev)  # noqa: E731
    wdu, wdv = (None, None) if deg is None else (v(0.05), v(0.05))
    wex = v(0.5) if ex_mode else None
    b1, w2, b2 = v(0.1), v(0.4), torch.tensor([0.1], device=dev)

    def fused():
        return ops.allpairs_mlp_topk(AB, xp, deg, ex_mode, -1.0, wdu, wdv, wex, b1, w2, b2, act, 64, noise_mode, None, (9, 4))

    paths = {"one kernel": fused}
    if N <= a.compose_max:
        ar = torch.arange(N, device=dev, dtype=torch.int32)
        rowptr, col, erow = torch.arange(N + 1, device=dev, dtype=torch.int64) * N, ar.repeat(N), ar.repeat_interleave(N)

        def composed():
            p, _ = ops.edge_mlp_fwd(AB, xp, erow, col, deg, None, ex_mode, -1.0, wdu, wdv, wex, b1, w2, b2, act)
            return ops.edgelist_topk_p(p, N, rowptr, col, 64, noise_mode, None, (9, 4))

        i1, v1, _ = fused()
        i2, v2, _ = composed()
        assert torch.equal(i1, i2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32)), "the two paths disagree"
        paths["composed (edge_mlp_fwd + edgelist_topk_p)"] = composed
    reps = {name: reps_for(fn) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(a.windows):                              # alternate the paths window by window
        for name, fn in paths.items():
            times[name].append(window(fn, reps[name]))
    out = dict(N=N, scorer=a.scorer, noise=a.noise, hw=hw, h=h, windows=a.windows)
    for name, ts in times.items():
        med = statistics.median(ts)
        print(f"N={N:7d} {a.scorer} {a.noise} hw={hw}  {name:42s} median {med:10.3f} ms  (windows {min(ts):.3f} .. {max(ts):.3f} ms, {reps[name]} calls each)",
              flush=True)
        out[name.split(" (")[0].replace(" ", "_") + "_ms"] = dict(median=med, min=min(ts), max=max(ts), reps=reps[name])
    if len(times) == 2:
        f_, c_ = times["one kernel"], times["composed (edge_mlp_fwd + edgelist_topk_p)"]
        out["speedup_median"] = statistics.median(c_) / statistics.median(f_)
        out["not_slower_beyond_spread"] = statistics.median(f_) <= statistics.median(c_) + (max(c_) - min(c_)) + (max(f_) - min(f_))
    print(json.dumps(out), flush=True)
