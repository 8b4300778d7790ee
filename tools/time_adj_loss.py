#!/usr/bin/env python3
"""Times the adjacency supervision loss (dgg_amd.adjacency_mse_loss; kernel pair dgg_adj_mse_loss) alone, on one GPU (diagnostic), and at
the Pubmed shape the dense route it replaces (out_adj.to_dense() + F.mse_loss, forward + backward), with the peak device memory of each.

    python tools/time_adj_loss.py [--windows 9] [--skip_dense]

Shapes (synthetic: the sizes are the point, not the numbers):
    Pubmed shape   N = 19 717; CSR learned rows (1-31 entries a row, mean near 5.5: an edge-list generator keeps every candidate) and
                   64-rank list rows with ~41 live slots
    N = 100 000    64-rank list rows with ~41 live slots (k ~ 32 + the ramp's margin) and chunked rows of 3 chunks with ~140 live slots
                   (k ~ 130)
The target holds about half of the first eight learned columns of every row with value 1 and three columns the row does not hold (what
remove_interclass_edges leaves of a graph the generator follows), through the public path: a sparse COO tensor converted once.

Per shape: the kernel pair without and with the gradient output (ops.adj_mse_loss: row kernel + fold, nothing read back), and forward +
backward through adjacency_mse_loss (the pair + one elementwise product).  Each figure is the median over `windows` timed windows (device
events around `reps` back-to-back calls, reps chosen so that a window lasts about a third of a second), with the smallest and largest
window next to it; peak_mb is torch.cuda.max_memory_allocated over one call, above what was allocated before it.  One JSON line per
figure."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=9)
ap.add_argument("--skip_dense", action="store_true", help="do not run the dense route at the Pubmed shape (2 x 1.6 GB operands + gradients)")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dgg_amd  # noqa: E402
from dgg_amd import ops  # noqa: E402

assert torch.cuda.is_available(), "time_adj_loss.py needs a GPU"
dev = torch.device("cuda", 0)
STEP = 7919                                                 # prime, divides neither N: start + r * STEP (mod N) are distinct columns for r < N


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
    fn()                                                    # (warm: code objects loaded, allocator settled, the target's conversion cached)
    torch.cuda.synchronize()
    t1 = max(window(fn, 1), 1e-3)
    return max(1, min(2000, int(330.0 / t1)))


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def columns(N, width, gen):
    """[N, width] distinct columns per row"""
    start = torch.randint(0, N, (N, 1), generator=gen, device=dev)
    return (start + torch.arange(width, device=dev)[None, :] * STEP) % N


def target_of(cols, N, gen):
    """about half of the first eight columns of every row, value 1, + three columns the row does not hold -> sparse COO int64 values"""
    rows = torch.arange(N, device=dev)[:, None]
    first = cols[:, :8]
    keep = torch.rand(first.shape, generator=gen, device=dev) < 0.5
    other = (cols[:, :1] - torch.arange(1, 4, device=dev)[None, :] * STEP) % N
    r = torch.cat([rows.expand_as(first)[keep], rows.expand_as(other).reshape(-1)])
    c = torch.cat([first[keep], other.reshape(-1)])
    return torch.sparse_coo_tensor(torch.stack([r, c]), torch.ones(r.shape[0], device=dev, dtype=torch.int64), (N, N)).coalesce()


def list_rows(N, live, gen):
    cols = columns(N, 64, gen)
    idx = torch.where(torch.arange(64, device=dev)[None, :] < live, cols, torch.full_like(cols, -1)).to(torch.int32)
    val = torch.rand(N, 64, generator=gen, device=dev)
    return dgg_amd.EllAdjacency(idx, val.requires_grad_(), N), cols


def chunked_rows(N, k, gen):
    kk = torch.full((N,), float(k), device=dev)
    lay = ops.chunk_layout(kk)
    m = lay.chunks // N
    assert lay.wide and lay.chunks == m * N
    cols = columns(N, 64 * m, gen)
    live = int(k) + 10
    idx = torch.where(torch.arange(64 * m, device=dev)[None, :] < live, cols, torch.full_like(cols, -1)).to(torch.int32).reshape(lay.chunks, 64)
    val = torch.rand(lay.chunks, 64, generator=gen, device=dev)
    return dgg_amd.EllAdjacency(idx, val.requires_grad_(), N, layout=lay), cols


def csr_rows(N, gen):
    n = torch.clamp(1 + torch.distributions.Geometric(torch.tensor(1.0 / 4.5)).sample((N,)).long(), max=31).to(dev)
    cols = columns(N, 31, gen)
    live = torch.arange(31, device=dev)[None, :] < n[:, None]
    erow = torch.arange(N, device=dev)[:, None].expand_as(cols)[live]
    rowptr = torch.zeros(N + 1, device=dev, dtype=torch.int64)
    rowptr[1:] = n.cumsum(0)
    val = torch.rand(int(live.sum()), generator=gen, device=dev)
    return dgg_amd.CsrAdjacency(rowptr, cols[live].to(torch.int32).contiguous(), erow.to(torch.int32).contiguous(), val.requires_grad_(), N), cols


def arrays_of(A):
    if isinstance(A, dgg_amd.CsrAdjacency):
        return (A.rowptr, A.col, A.values())
    return (A.idx, A.values()) + ((A.layout,) if A.layout is not None else ())


def report(tags, name, fn, **more):
    reps = reps_for(fn)
    ts = [window(fn, reps) for _ in range(a.windows)]
    print(json.dumps(dict(tags, what=name, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), reps=reps,
                          windows=len(ts), peak_mb=peak_mb(fn), **more)), flush=True)


def fwd_bwd(loss_fn, values):
    def run():
        values.grad = None
        loss = loss_fn()
        loss.backward()
        return loss
    return run


def shape(N, name, A, cols, gen, dense):
    target = target_of(cols, N, gen)
    graph = dgg_amd.adjacency._target_csr(target)[:3]
    tags = dict(N=N, rows=name, learned_entries=int((arrays_of(A)[1 if isinstance(A, dgg_amd.CsrAdjacency) else 0] >= 0).sum()), target_entries=int(target._nnz()))
    arrs = arrays_of(A)
    report(tags, "kernel pair, no gradient output", lambda: ops.adj_mse_loss(arrs, graph, "mean"))
    report(tags, "kernel pair + gradient output", lambda: ops.adj_mse_loss(arrs, graph, "mean", want_grad=True))
    sparse = fwd_bwd(lambda: dgg_amd.adjacency_mse_loss(A, target), A.values())
    report(tags, "adjacency_mse_loss forward + backward", sparse)
    if dense:
        gt = target.to_dense().float()                      # (held outside the timed region: the reference densifies it every step)
        route = fwd_bwd(lambda: torch.nn.functional.mse_loss(A.to_dense(), gt), A.values())
        ls, ld = float(sparse().detach()), float(route().detach())
        report(tags, "dense route: to_dense() + F.mse_loss forward + backward", route, dense_target_mb=round(gt.numel() * 4 / 2 ** 20, 2),
               loss_sparse=ls, loss_dense=ld)
        del gt


gen = torch.Generator(device=dev).manual_seed(0)
for N, name, make, dense in ((19717, "csr", lambda: csr_rows(19717, gen), True), (19717, "list K=64", lambda: list_rows(19717, 41, gen), True),
                             (100000, "list K=64", lambda: list_rows(100000, 41, gen), False),
                             (100000, "chunked, 3 chunks", lambda: chunked_rows(100000, 130.0, gen), False)):
    A, cols = make()
    shape(N, name, A, cols, gen, dense and not a.skip_dense)
    del A, cols
    torch.cuda.empty_cache()
