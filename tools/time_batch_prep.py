#!/usr/bin/env python3
"""Times the preparation of one training batch of dgg_amd.train_large_graphs on one GPU (diagnostic): the batch's noisy graph plus its
same-class target, on the two routes of --batch_noise.

    python tools/time_batch_prep.py [--windows 9] [--nodes 100000] [--half_edges 500000]

    host     train_large_graphs.noisy_batch_adj (edge list to the host, data.add_noisy_edges in numpy, COO back to the device, coalesce)
             + data.remove_interclass_edges (the parent path, and the reference's)
    device   SubgraphBatch.with_noise (ops.batch_graph_edit: two kernels, two cumsum, one read-back; CSR caches seeded)
on a synthetic graph (the sizes are the point, not the numbers) at the reference's default sampler settings: GraphSAINT roots 2000, walk
length 2, edge noise level 0.00014 (train_large_graphs.py:77-81, 195-204), and on one Cluster batch (500 contiguous parts, 5 a batch).
The batch itself (walks + cut) is drawn once, outside the timed region: it is the same on both routes.

Both routes read the device back (the output shapes depend on the data), so a figure is WALL time per call with a synchronize at the end
of each window: the median over `windows` windows of `reps` calls, with the smallest and largest window next to it.  The edit's kernels
alone (COUNT + FILL, no allocation, no read-back) are timed with device events around `reps` back-to-back pairs.  One JSON line per
figure."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=9)
ap.add_argument("--nodes", type=int, default=100000)
ap.add_argument("--half_edges", type=int, default=500000)
ap.add_argument("--batch_size", type=int, default=2000)
ap.add_argument("--walk_length", type=int, default=2)
ap.add_argument("--noise_level", type=float, default=0.00014)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dgg_amd  # noqa: E402
import dgg_amd.data as D  # noqa: E402
from dgg_amd import _lib, ops  # noqa: E402
from dgg_amd import train_large_graphs as H  # noqa: E402

assert torch.cuda.is_available(), "time_batch_prep.py needs a GPU"
dev = torch.device("cuda", 0)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps          # ms per call


def report(tags, name, fn, budget_ms=330.0):
    fn()
    fn()                                                    # (warm: code objects loaded, allocator settled)
    reps = max(1, min(2000, int(budget_ms / max(window(fn, 1), 1e-3))))
    ts = [window(fn, reps) for _ in range(a.windows)]
    print(json.dumps(dict(tags, what=name, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), reps=reps,
                          windows=len(ts))), flush=True)
    return statistics.median(ts)


def kernels_only(tags, batch, seed, labels):
    """COUNT + FILL on preallocated outputs, device events around `reps` pairs"""
    sub = batch.sub
    ed = ops.batch_graph_edit(sub.browptr, sub.bcol, batch.adj.values(), 10 * a.noise_level, seed, labels)
    lab = labels.to(torch.int32)
    n, E = sub.n, sub.e
    thr = ops.noise_threshold(10 * a.noise_level)
    ndeg, tdeg = (torch.empty(n, device=dev, dtype=torch.int32) for _ in range(2))
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    L, p, st = _lib.lib(), ops._ptr, ops._stream()
    values = batch.adj.values()

    def pair():
        for ph in (ops.BATCH_EDIT_COUNT, ops.BATCH_EDIT_FILL):
            fill = ph == ops.BATCH_EDIT_FILL
            _lib.check(L.dgg_batch_graph_edit(ph, p(sub.browptr), p(sub.bcol), p(values), n, E, p(lab), seed[0], seed[1], thr, p(ndeg), p(tdeg),
                                              p(ed.nrowptr) if fill else None, ed.e, p(ed.ncol), p(ed.nrow), p(ed.nval), p(ed.nsrc),
                                              p(ed.trowptr) if fill else None, ed.e_t, p(ed.tcol), p(ed.trow), p(status), st), "batch_graph_edit")
    pair()
    torch.cuda.synchronize()
    assert int(status) == 0
    reps, ts = 50, []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            pair()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    print(json.dumps(dict(tags, what="device: the edit's two kernels alone (COUNT + FILL, device events)", median_ms=round(statistics.median(ts), 4),
                          min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), reps=reps, windows=len(ts))), flush=True)


def one_batch(name, loader, batch, y):
    y_b = batch.take(y)
    seed = loader.noise_seed(batch.step)
    ed = batch.with_noise(a.noise_level, seed, labels=y_b)
    tags = dict(batch=name, batch_nodes=batch.num_nodes, batch_entries=batch.num_edges, noisy_entries=int(ed.is_noise.sum()), target_entries=ed.edit.e_t,
                noise_level=a.noise_level)

    def host():
        adj = H.noisy_batch_adj(batch, a.noise_level)
        return adj, D.remove_interclass_edges(adj, y_b)

    def device():
        return batch.with_noise(a.noise_level, seed, labels=y_b)
    adj_h, gt_h = host()
    tags["host_noisy_entries"] = int(adj_h._nnz()) - batch.num_edges
    t_h = report(tags, "host: noisy_batch_adj + remove_interclass_edges", host, budget_ms=1000.0)
    t_d = report(tags, "device: SubgraphBatch.with_noise", device)
    kernels_only(tags, batch, seed, y_b)
    print(json.dumps(dict(tags, what="host / device", ratio=round(t_h / t_d, 1))), flush=True)


gen = torch.Generator(device=dev).manual_seed(0)
r = torch.randint(0, a.nodes, (a.half_edges,), generator=gen, device=dev)
c = torch.randint(0, a.nodes, (a.half_edges,), generator=gen, device=dev)
ind = torch.stack([torch.cat([r[r != c], c[r != c]]), torch.cat([c[r != c], r[r != c]])])
graph = torch.sparse_coo_tensor(ind, torch.ones(ind.shape[1], device=dev), (a.nodes, a.nodes)).coalesce()
y = torch.randint(0, 7, (a.nodes,), generator=gen, device=dev)
saint = dgg_amd.RandomWalkSampler(graph, a.batch_size, a.walk_length, num_steps=1, seed=0)
one_batch("GraphSAINT roots %d walk %d" % (a.batch_size, a.walk_length), saint, saint.batch(0), y)
cluster = dgg_amd.ClusterSampler(graph, dgg_amd.contiguous_parts(a.nodes, 500), batch_size=5, seed=0)
one_batch("Cluster 5 of 500 parts", cluster, next(iter(cluster)), y)
