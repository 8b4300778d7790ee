#!/usr/bin/env python3
"""Times the wide-row form of the edge-MLP scorers on all-pairs candidates on one GPU (diagnostic): ops.allpairs_mlp_topk_wide and the
autograd node on chunked rows.  Scorer u-v-deg, per-pair hash noise, h = hw = 64.

    python tools/time_allpairs_mlp_wide.py [--part list|csr|passes|baseline ...] [--windows 7] [--baseline-lib PATH/libdgg_hip.so]

    list    N = 4096 and 20000, k ~ 30 (every row one chunk): the wide kernel against dgg_allpairs_mlp_topk (alone, and followed by
            softk_fwd, which the wide kernel fuses) on the same inputs -- the cost of the cascade and of two rows per wavefront
    csr     N = 4096, k ~ 130 (three chunks per row): the node on chunked rows, forward and forward + backward, against the only way to
            this result without it: the CSR form on the complete pattern (_DGGScoresFn + ops.CsrSoftkFn: N^2-sized arrays)
    passes  N = 20000, k ~ 30 / 130 / 600: one sweep settles ops.APMLP_WIDE_REG_CHUNKS chunks of a row; time, sweeps, time per sweep
            relative to the one-chunk sweep
    baseline  (with --baseline-lib: a second build of the library, for instance the parent commit's; tools/baseline_lib.py)
            dgg_allpairs_mlp_topk_wide (u-v-deg) and dgg_allpairs_mlp_topk_wide_prior (u-v-A_uv, 4 random entries per row plus self loops)
            of both builds at N = 20000 with k ~ 32 (one chunk) and ~ 130 (three chunks) and at N = 4096 with k ~ 600 (ten chunks: a
            continuation sweep), outputs bit-equal before anything is timed; the verdict is baseline_lib.compare's

Each figure is the median over `windows` timed windows (device events around `reps` back-to-back calls, reps chosen so that a window
lasts about a quarter of a second), with the smallest and largest window next to it.  The variants of a part alternate window by
window; where two variants compute the same thing their results are compared before anything is timed.  One JSON line per figure."""
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
from dgg_amd.dgm import _DGGAllPairsMlpWideAdjFn, _DGGScoresFn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", nargs="*", default=["list", "csr", "passes"], choices=["list", "csr", "passes", "baseline"])
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--baseline-lib", default=None)
a = ap.parse_args()
assert ("baseline" in a.part) == (a.baseline_lib is not None), "--part baseline and --baseline-lib go together"
assert torch.cuda.is_available(), "time_allpairs_mlp_wide.py needs a GPU"
dev = torch.device("cuda", 0)
H = HW = 64
SEED = (9, 4)


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


def timed(paths, **tags):
    """alternates the paths window by window -> {name: median ms}; prints one JSON line per path (with the verdict against its
    "..., baseline build" twin, if it has one)"""
    reps = {name: reps_for(fn) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(a.windows):
        for name, fn in paths.items():
            times[name].append(window(fn, reps[name]))
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        twin = times.get(name + ", baseline build")
        print(json.dumps(dict(tags, what=name, median_ms=round(med[name], 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                              reps=reps[name], windows=a.windows, **(compare(ts, twin) if twin else {}))), flush=True)
    return med


def inputs(N):
    g = torch.Generator().manual_seed(N)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev)  # noqa: E731
    t = dict(x=r(N, H), We=r(H, H, sc=0.1), be=r(H, sc=0.1), Wcat=r(2 * HW, H, sc=0.3), wdu=r(HW, sc=0.05), wdv=r(HW, sc=0.05), eb1=r(HW, sc=0.1),
             w2=r(HW, sc=0.4), b2=torch.tensor([0.1], device=dev))
    t["deg"] = torch.randint(3, 20, (N,), generator=g).float().to(dev)
    t["u"] = torch.rand(N, generator=g).to(dev)
    t["xp"] = ops.linear_fwd(t["x"], t["We"], t["be"], ops.ACT_LEAKY)
    t["AB"] = ops.linear_fwd(t["xp"], t["Wcat"], None, ops.ACT_NONE)
    return t


def wide_call(t, k, lay):
    return lambda: ops.allpairs_mlp_topk_wide(t["AB"], t["xp"], t["deg"], 0, -1.0, t["wdu"], t["wdv"], None, t["eb1"], t["w2"], t["b2"], ops.ACT_LEAKY,
                                              k, lay, ops.MODE_K_TIMES_EDGE_PROB, ops.NOISE_HASH, None, SEED)


one_chunk_ms = {}
if "list" in a.part or "passes" in a.part:
    for N in (4096, 20000):
        if N == 4096 and "list" not in a.part:
            continue
        t = inputs(N)
        k = (25.0 + 10.0 * t["u"]).contiguous()
        lay = ops.chunk_layout(k, ncols=N)
        assert lay.maxm == 1
        wide = wide_call(t, k, lay)

        def lst():
            return ops.allpairs_mlp_topk(t["AB"], t["xp"], t["deg"], 0, -1.0, t["wdu"], t["wdv"], None, t["eb1"], t["w2"], t["b2"], ops.ACT_LEAKY, 64,
                                         ops.NOISE_HASH, None, SEED)

        def lst_ramp():
            i_, v_, _ = lst()
            return ops.softk_fwd(i_, v_, k, ops.MODE_K_TIMES_EDGE_PROB)

        i1, v1, _, w1, _ = wide()
        i2, v2, _ = lst()
        live = i1 >= 0
        assert torch.equal(i1[live], i2[live]) and torch.equal(v1[live], v2[live]), "the wide kernel and the list kernel disagree"
        m = timed({"wide, one chunk per row": wide, "list kernel": lst, "list kernel + softk_fwd": lst_ramp}, part="list", N=N, k="~30")
        one_chunk_ms[N] = m["wide, one chunk per row"]
        print(json.dumps(dict(part="list", N=N, wide_over_list=round(m["wide, one chunk per row"] / m["list kernel"], 3),
                              wide_over_list_plus_ramp=round(m["wide, one chunk per row"] / m["list kernel + softk_fwd"], 3))), flush=True)

if "csr" in a.part:
    N = 4096
    t = inputs(N)
    k0 = (120.0 + 20.0 * t["u"]).contiguous()
    lay = ops.chunk_layout(k0, ncols=N)
    assert lay.maxm == 3
    ar = torch.arange(N, device=dev, dtype=torch.int32)
    pattern = (torch.arange(N + 1, device=dev, dtype=torch.int64) * N, ar.repeat(N), ar.repeat_interleave(N))
    names = ("x", "We", "be", "Wcat", "wdu", "wdv", "eb1", "w2", "b2")

    def leaves(grad):
        lf = {n: t[n].detach().clone().requires_grad_(grad) for n in names}
        lf["k"] = k0.detach().clone().requires_grad_(grad)
        return lf

    def chunked(grad):
        lf = leaves(grad)
        cfg = dict(K=64, noise_mode=ops.NOISE_HASH, G=None, seed=SEED, mode=ops.MODE_K_TIMES_EDGE_PROB, ex_mode=0, t_ex=-1.0, act=ops.ACT_LEAKY, layout=lay)
        w = _DGGAllPairsMlpWideAdjFn.apply(lf["x"], lf["k"], t["deg"], lf["We"], lf["be"], lf["Wcat"], lf["wdu"], lf["wdv"], None, lf["eb1"], lf["w2"],
                                           lf["b2"], cfg)[0]
        if grad:
            w.sum().backward()
        return w

    def csr(grad):
        lf = leaves(grad)
        cfg = dict(cand=pattern, t=ops.T_DIST, rows=None, ex_mode=0, t_ex=-1.0, act=ops.ACT_LEAKY)
        p = _DGGScoresFn.apply(lf["x"], t["deg"], None, lf["We"], lf["be"], lf["Wcat"], lf["wdu"], lf["wdv"], None, lf["eb1"], lf["w2"], lf["b2"], cfg)
        w = ops.CsrSoftkFn.apply(p, lf["k"], pattern[0], pattern[1], ops.NOISE_HASH, None, SEED, ops.MODE_K_TIMES_EDGE_PROB)
        if grad:
            w.sum().backward()
        return w

    with torch.no_grad():
        s1, s2 = float(chunked(False).sum()), float(csr(False).sum())
    assert abs(s1 - s2) <= 1e-4 * abs(s2), f"the chunked node and the CSR form disagree: {s1} vs {s2}"

    def fwd_only(f):
        def run():
            with torch.no_grad():
                return f(False)
        return run

    timed({"wide kernel alone": wide_call(t, k0, lay), "chunked node, forward": fwd_only(chunked), "CSR form, forward": fwd_only(csr),
           "chunked node, forward + backward": lambda: chunked(True), "CSR form, forward + backward": lambda: csr(True)}, part="csr", N=N, k="~130")

if "passes" in a.part:
    N = 20000
    t = inputs(N)
    for what, lo, hi in (("~130", 120.0, 140.0), ("~600", 590.0, 610.0)):
        k = (lo + (hi - lo) * t["u"]).contiguous()
        lay = ops.chunk_layout(k, ncols=N)
        sweeps = -(-lay.maxm // ops.APMLP_WIDE_REG_CHUNKS)
        m = timed({"wide": wide_call(t, k, lay)}, part="passes", N=N, k=what, chunks_per_row=lay.maxm, sweeps=sweeps)
        print(json.dumps(dict(part="passes", N=N, k=what, sweeps=sweeps, ms_per_sweep=round(m["wide"] / sweeps, 4),
                              per_sweep_over_one_chunk_sweep=round(m["wide"] / sweeps / one_chunk_ms[N], 3))), flush=True)

if "baseline" in a.part:
    base = Baseline(a.baseline_lib)
    for N, what, lo, hi in ((20000, "~32", 27.0, 37.0), (20000, "~130", 120.0, 140.0), (4096, "~600", 590.0, 610.0)):
        t = inputs(N)
        g = torch.Generator().manual_seed(N + 1)
        graph = torch.sparse_coo_tensor(torch.stack([torch.arange(N).repeat_interleave(4), torch.randint(0, N, (4 * N,), generator=g)]),
                                        torch.ones(4 * N), (N, N)).coalesce().to(dev)
        prior = dgg_amd.AllPairs.from_graph(graph, self_loops=True).prior_csr()[:3]
        wex = (torch.randn(HW, generator=g) * 0.5).to(dev)
        k = (lo + (hi - lo) * t["u"]).contiguous()
        lay = ops.chunk_layout(k, ncols=N)

        def uvauv():
            return ops.allpairs_mlp_topk_wide(t["AB"], t["xp"], None, 1, 0.0, None, None, wex, t["eb1"], t["w2"], t["b2"], ops.ACT_LEAKY, k, lay,
                                              ops.MODE_K_TIMES_EDGE_PROB, ops.NOISE_HASH, None, SEED, prior=prior)

        paths = {"wide, u-v-deg": wide_call(t, k, lay), "wide, u-v-A_uv with the prior": uvauv}
        for name in list(paths):
            paths[name + ", baseline build"] = base.calls(paths[name])
            assert same_bits(paths[name](), paths[name + ", baseline build"]()), f"the two builds disagree on {name}"
        timed(paths, part="baseline", N=N, k=what, chunks_per_row=lay.maxm, sweeps=-(-lay.maxm // ops.APMLP_WIDE_REG_CHUNKS))
