#!/usr/bin/env python3
"""Times one training step (forward, nll_loss, backward, Adam) of GCN_DGG with a WRITER on a Pubmed-SHAPED synthetic edge-list graph, on
one GPU (diagnostic), and the train_stats kernel pair (ops.adj_diff_stats) alone.

    python tools/time_adj_stats.py [--scorer u-v-deg] [--windows 9] [--tree DIR]

Configurations, alternating window by window in one process:
    fused, no writer                       the step nobody logs (the baseline the writer's overhead is reported against)
    separate modules, writer, no stats     a writer as it ran before train_stats/* existed: the separate modules, values/first_k_* only
                                           (this tree with _log_adj_stats switched off; --tree DIR runs the step of ANOTHER checkout, e.g. the
                                           parent commit, in the same way -- in a process of its own, so not alternating with the others)
    separate modules, writer               this tree without args.dgg_writer_fused: the same route + train_stats/*
    fused, writer (dgg_writer_fused)       the opt-in: the fused node + values/first_k_* + train_stats/*
The writer converts every scalar to a Python float, as a SummaryWriter does (a tensor scalar costs a read-back of its own), and drops
histograms.  Graph: N = 19 717 nodes, d = 500 features, h = 64, 3 classes, 1-30 candidates a row with a mean near 4.5 (+ the self loop
the model adds); harness defaults otherwise (scorer u-v-deg, no perturbation).  Synthetic features and graph: the step's kernel sequence
and sizes are Pubmed's, its numbers are not.

Each figure is the median over `windows` timed windows (device events around `reps` back-to-back steps, reps chosen so that a window
lasts about a third of a second), with the smallest and largest window next to it.  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys
from argparse import Namespace

ap = argparse.ArgumentParser()
ap.add_argument("--scorer", default="u-v-deg", choices=["u-v-dist", "u-v-deg", "u-v-A_uv", "u-v-deg-dist", "edge_conv"])
ap.add_argument("--windows", type=int, default=9)
ap.add_argument("--nodes", type=int, default=19717)
ap.add_argument("--tree", default=None, help="time the writer step of the dgg_amd package of this checkout instead (one configuration)")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dgg_amd  # noqa: E402
from dgg_amd import ops  # noqa: E402

assert torch.cuda.is_available(), "time_adj_stats.py needs a GPU"
dev = torch.device("cuda", 0)
D, H, C = 500, 64, 3


class FloatWriter:
    """what a SummaryWriter costs the step: every scalar becomes a Python float; histograms are dropped"""
    n = 0

    def add_scalar(self, tag, value, step):
        float(value)
        self.n += 1

    def add_histogram(self, tag, values, step):
        pass


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
    fn()                                                    # (warm: code objects loaded, allocator settled, the graph's conversions cached)
    torch.cuda.synchronize()
    t1 = max(window(fn, 1), 1e-3)
    return max(1, min(500, int(330.0 / t1)))


def pubmed_shaped_graph(N):
    rng = np.random.default_rng(N)
    n = np.minimum(1 + rng.geometric(1.0 / 3.5, N), 30)
    rows = np.repeat(np.arange(N), n)
    cols = np.concatenate([rng.choice(N, c, replace=False) for c in n])
    keep = rows != cols                                     # (the model adds the self loops)
    ind = torch.from_numpy(np.stack([rows[keep], cols[keep]]))
    return torch.sparse_coo_tensor(ind, torch.ones(ind.shape[1]), (N, N)).coalesce(), float(n.mean())


def model(**kw):
    args = Namespace(extra_edge_dim={"u-v-deg": 2, "u-v-deg-dist": 3, "u-v-A_uv": 1}.get(a.scorer, 0), extra_k_dim=1, dgg_hard=False, deg_mean=3.899,
                     deg_std=5.288, dgg_mode_edge_net=a.scorer, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3,
                     perturb_edge_prob=False, symmetric_noise=True, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1, **kw)
    torch.manual_seed(3)
    m = dgg_amd.GCN_DGG(nfeat=D, nhidden=H, nclass=C, args=args)
    with torch.no_grad():
        m.conv1.W.mul_(0.05)                                 # (W ~ U[0, 1) over 500 features: keeps the activations of order one)
    return m.to(dev).train()


N = a.nodes
g = torch.Generator().manual_seed(N)
x = torch.randn(N, D, generator=g).to(dev)
y = torch.randint(0, C, (N,), generator=g).to(dev)
A, mean = pubmed_shaped_graph(N)
A = A.to(dev)


def step(m, writer):
    opt = torch.optim.Adam([dict(params=m.params1, weight_decay=5e-4), dict(params=m.params2, weight_decay=0)], lr=0.01)
    state = {"epoch": 0}

    def run():
        opt.zero_grad(set_to_none=True)
        logp, adj, _ = m(x, A, epoch=state["epoch"], writer=writer)
        loss = torch.nn.functional.nll_loss(logp, y)
        loss.backward()
        opt.step()
        state["epoch"] += 1
        return adj
    return run


tags = dict(scorer=a.scorer, N=N, d=D, h=H, candidates_mean=round(mean + 1, 2))


def report(name, ts, reps, **more):
    print(json.dumps(dict(tags, what=name, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), reps=reps,
                          windows=len(ts), **more)), flush=True)


if a.tree:
    m = model()
    fn = step(m, FloatWriter())
    reps = reps_for(fn)
    report("separate modules, writer (--tree)", [window(fn, reps) for _ in range(a.windows)], reps, tree=os.path.abspath(a.tree),
           has_train_stats=hasattr(ops, "adj_diff_stats"))
    sys.exit(0)

m_plain, m_nostats, m_sep, m_fused = model(), model(), model(), model(dgg_writer_fused=True)
m_nostats.dggs[0]._log_adj_stats = lambda *args_, **kw_: None              # a writer as it ran before train_stats/* existed
w_sep, w_fused = FloatWriter(), FloatWriter()
paths = {"fused, no writer": step(m_plain, None), "separate modules, writer, no stats": step(m_nostats, FloatWriter()),
         "separate modules, writer": step(m_sep, w_sep), "fused, writer (dgg_writer_fused)": step(m_fused, w_fused)}
adjs = {name: fn() for name, fn in paths.items()}
assert not m_plain.dggs[0].__dict__.get("fused_fallback") and not m_fused.dggs[0].__dict__.get("fused_fallback"), "the fused cases left the fused layer"
assert "_fused_layer" in m_fused.dggs[0].__dict__ and "_fused_layer" not in m_sep.dggs[0].__dict__ and "_fused_layer" not in m_nostats.dggs[0].__dict__
assert w_sep.n == 9 and w_fused.n == 9, "the case does not write the nine scalars it names"
reps = {name: reps_for(fn) for name, fn in paths.items()}
times = {name: [] for name in paths}
for _ in range(a.windows):
    for name, fn in paths.items():
        times[name].append(window(fn, reps[name]))
med = {name: statistics.median(ts) for name, ts in times.items()}
for name, ts in times.items():
    report(name, ts, reps[name])

# the kernel pair alone, on what the fused layer's last forward holds
dgg = m_fused.dggs[0]
st = dgg._fused_layer.saved
in_adj, cand, deg, prior, _, _ = dgg._candidates(dgg_amd.model._with_self_loops(A))
graph = dgg._stats_graph(in_adj, cand, deg, prior)
lay = st.get("layout")
arrs = (st["idx"], st["w"], lay)
pair = lambda: ops.adj_diff_stats(arrs, graph, st["k"])  # noqa: E731
rp = reps_for(pair)
rp = max(rp, 200)
ts = [window(pair, rp) for _ in range(a.windows)]
report("adj_diff_stats (row kernel + fold, no read-back)", ts, rp, graph_entries=int(graph[1].shape[0]))
print(json.dumps(dict(tags, fused_writer_over_separate_writer_no_stats=round(med["fused, writer (dgg_writer_fused)"] / med["separate modules, writer, no stats"], 3),
                      separate_writer_over_no_stats=round(med["separate modules, writer"] / med["separate modules, writer, no stats"], 3),
                      fused_writer_minus_fused_ms=round(med["fused, writer (dgg_writer_fused)"] - med["fused, no writer"], 4),
                      fused_writer_over_fused=round(med["fused, writer (dgg_writer_fused)"] / med["fused, no writer"], 3))), flush=True)
