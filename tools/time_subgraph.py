#!/usr/bin/env python3
"""Times the mini-batch sampling (dgg_amd.sampling: kernels dgg_random_walk_nodes + dgg_induced_subgraph) on one GPU (diagnostic), against
the route a caller has without them: torch ops only.

    python tools/time_subgraph.py [--windows 9] [--batch_size 2000] [--walk_length 2]

Shapes (synthetic: the sizes are the point, not the numbers):
    Pubmed shape   N = 19 717, 88 648 stored entries (a random symmetric graph of Pubmed's size)
    N = 100 000    1 000 000 stored entries
A batch: batch_size roots, walk_length steps (the reference's defaults, train_large_graphs.py:195-204), the sub-graph induced by the visited
nodes, as a coalesced sparse COO tensor PLUS the CSR arrays and prior degrees the generator asks for (csr_candidates).

Per shape, the same roots on both sides:
    walk           ops.random_walk_nodes   |  torch: L rounds of (rowptr gathers, a torch.rand pick, a col gather, a where)
    cut            ops.induced_subgraph + SubgraphBatch (CSR arrays and degrees come with it)
                                           |  torch: a node mask, the COO entries with both ends in it (mask gathers + nonzero), a cumsum for
                                              the new ids, index_select of indices and values, sparse_coo_tensor, csr_candidates of the result
    batch          RandomWalkSampler.batch |  the two torch steps above
Both routes read the device once or more per batch (the output shapes depend on the data), so a figure is WALL time per call with a
synchronize at the end of each window: the median over `windows` windows of `reps` calls (reps chosen so that a window lasts about a
third of a second), with the smallest and largest window next to it.  One JSON line per figure.  The torch walk draws other random numbers
than the kernel's law; the cut is checked to give the same sub-graph on both routes before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=9)
ap.add_argument("--batch_size", type=int, default=2000)
ap.add_argument("--walk_length", type=int, default=2)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dgg_amd  # noqa: E402
from dgg_amd import ops  # noqa: E402
from dgg_amd.sampling import SubgraphBatch  # noqa: E402

assert torch.cuda.is_available(), "time_subgraph.py needs a GPU"
dev = torch.device("cuda", 0)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps          # ms per call


def report(tags, name, fn):
    fn()
    fn()                                                    # (warm: code objects loaded, allocator settled, the graph's conversion cached)
    reps = max(1, min(2000, int(330.0 / max(window(fn, 1), 1e-3))))
    ts = [window(fn, reps) for _ in range(a.windows)]
    print(json.dumps(dict(tags, what=name, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), reps=reps,
                          windows=len(ts))), flush=True)


def random_graph(N, half_edges, gen):
    """symmetric, no self loops, coalesced sparse COO float32"""
    r = torch.randint(0, N, (half_edges,), generator=gen, device=dev)
    c = torch.randint(0, N, (half_edges,), generator=gen, device=dev)
    keep = r != c
    r, c = r[keep], c[keep]
    ind = torch.stack([torch.cat([r, c]), torch.cat([c, r])])
    g = torch.sparse_coo_tensor(ind, torch.ones(ind.shape[1], device=dev), (N, N)).coalesce()
    return torch.sparse_coo_tensor(g.indices(), torch.ones_like(g.values()), (N, N), is_coalesced=True)


# ---- the torch route -------------------------------------------------------------------------------------------------------------------
def torch_walk(rowptr, col, roots, L, gen):
    v = roots.long()
    out = [v]
    for _ in range(L):
        p0 = rowptr[v]
        d = rowptr[v + 1] - p0
        pick = (torch.rand(v.shape, generator=gen, device=dev, dtype=torch.float64) * d).long()
        v = torch.where(d > 0, col[(p0 + pick).clamp(max=col.shape[0] - 1)].long(), v)
        out.append(v)
    return torch.stack(out, 1)


def torch_cut(graph, nodes):
    """-> (batch adj coalesced COO, original ids, csr_candidates(adj))"""
    N = graph.shape[0]
    ind, val = graph.indices(), graph.values()
    mask = torch.zeros(N, dtype=torch.bool, device=dev)
    mask[nodes.long()] = True
    newid = torch.cumsum(mask, 0) - 1
    orig = mask.nonzero().squeeze(1)
    e = (mask[ind[0]] & mask[ind[1]]).nonzero().squeeze(1)
    sub = newid[ind.index_select(1, e)]
    adj = torch.sparse_coo_tensor(sub, val.index_select(0, e), (orig.shape[0], orig.shape[0]), is_coalesced=True)
    return adj, orig, dgg_amd.csr_candidates(adj)


def shape(name, N, half_edges, gen):
    graph = random_graph(N, half_edges, gen)
    s = dgg_amd.RandomWalkSampler(graph, a.batch_size, a.walk_length, num_steps=1, seed=0)
    rowptr, col, values = s.rowptr, s.col, s.values
    roots = s.roots(0).to(dev)
    walk = ops.random_walk_nodes(rowptr, col, roots, a.walk_length, s.walk_seed(0), check=True)
    nodes = walk.reshape(-1)
    # the same sub-graph on both routes
    b = SubgraphBatch(ops.induced_subgraph(rowptr, col, nodes, values), values)
    adj_t, orig_t, (rp_t, col_t, deg_t) = torch_cut(graph, nodes)
    assert torch.equal(b.nodes, orig_t) and torch.equal(b.adj.indices(), adj_t.indices()) and torch.equal(b.adj.values(), adj_t.values())
    assert torch.equal(b.sub.browptr, rp_t) and torch.equal(b.sub.bcol, col_t) and torch.equal(b.sub.bdeg, deg_t)
    tags = dict(shape=name, N=N, entries=int(graph._nnz()), roots=a.batch_size, walk_length=a.walk_length, batch_nodes=b.num_nodes, batch_entries=b.num_edges)
    tg = torch.Generator(device=dev).manual_seed(1)
    report(tags, "walk: kernel", lambda: ops.random_walk_nodes(rowptr, col, roots, a.walk_length, s.walk_seed(0)))
    report(tags, "walk: torch ops", lambda: torch_walk(rowptr, col, roots, a.walk_length, tg))
    report(tags, "cut: kernels (induced_subgraph + SubgraphBatch, CSR arrays and degrees included)",
           lambda: SubgraphBatch(ops.induced_subgraph(rowptr, col, nodes, values), values))
    report(tags, "cut: torch ops (masks + index_select + csr_candidates)", lambda: torch_cut(graph, nodes))
    report(tags, "batch: RandomWalkSampler.batch", lambda: s.batch(0))
    report(tags, "batch: torch ops", lambda: torch_cut(graph, torch_walk(rowptr, col, roots, a.walk_length, tg).reshape(-1)))


gen = torch.Generator(device=dev).manual_seed(0)
shape("Pubmed shape", 19717, 44324, gen)
shape("N = 100 000", 100000, 500000, gen)
