#!/usr/bin/env python3
"""Golden fixtures of the train_stats/* scalars: get_adj_diff_stats (dgm.py:1288, 1313-1350) of DGG_LearnableK_debug in TRAINING mode
with a recording writer.

Companion of make_golden.py (runs only where the reference is available, on the CPU): the reference is imported through make_golden's
own shims, unmodified, and only data is stored --
    rows / cols / adj_vals   the input graph as a sparse matrix (stored zeros and a negative value included where a case has them)
    k                        the learned degrees the reference handed to get_adj_diff_stats [N]
    out_rows / out_cols / out_vals   the reference's SOFT output (topk_edge_p of dgm.py:1288) as the triplets of its non-zeros
    ref [7]                  the seven scalars the reference wrote, in the order of `tags` (float32 tensors -> float)
    f64 [7]                  a float64 two-pass evaluation of the same formula on the stored data (stats_f64)
    dist [7]                 |ref - f64| (0 where both are NaN): the reference's own float32 error, the bound of the parity tests
Cases (N = 160, u-v-dist, k-net x, k_times_edge_prob):
    a   edge-list graph with self loops, perturb_edge_prob=False: the output stays inside the graph, both off-edge tags are NaN
    b   a COMPLETE in_adj that stores a sparse graph's values and 0 elsewhere (the reference form of AllPairs.from_graph), captured
        asymmetric noise; every row's non-zeros fit 64, both populations hold at least two pairs (asserted)
    c   as b with a weighted graph: values in (0, 2], a few stored zeros and one negative value

    python tests/golden/make_golden_adj_stats.py      # writes tests/golden/adj_stats_*.npz
"""
import json
import os

import numpy as np

# importing make_golden imports the reference behind its shims (torch_geometric stubs, .cuda() no-op, np.float)
from make_golden import HERE, base_args, dgm, grid_gumbel, random_graph, torch

TAGS = ("on_edge_mean", "on_edge_std", "off_edge_mean", "off_edge_std", "in_deg_mean", "k_diff_mean", "k_mean")
N, D, H = 160, 24, 16


class Recorder:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        assert tag not in self.scalars, tag
        self.scalars[tag] = (float(value), step)

    def add_histogram(self, *a, **k):
        pass


def moments(v):
    """two-pass mean and unbiased std in float64; NaN where torch.mean / torch.std give NaN"""
    v = np.asarray(v, np.float64)
    n = v.size
    mean = v.sum() / n if n else np.nan
    std = np.sqrt(((v - mean) ** 2).sum() / (n - 1)) if n > 1 else np.nan
    return mean, std


def stats_f64(n, grows, gcols, gvals, orows, ocols, ovals, k):
    """the formula of dgm.py:1321-1348 on the stored data: float32 differences (as the reference subtracts), float64 moments"""
    A = np.zeros((n, n), np.float32)
    A[grows, gcols] = gvals
    W = np.zeros((n, n), np.float32)
    W[orows, ocols] = ovals
    d = A - W
    on_mean, on_std = moments(d[(A > 0) & (d != 0)])
    off_mean, off_std = moments(d[(A == 0) & (d != 0)])
    deg = A.astype(np.float64).sum(1)
    kd = np.asarray(k, np.float64) - deg
    return np.array([on_mean, on_std, off_mean, off_std, deg.mean(), kd.mean(), np.asarray(k, np.float64).mean()]), \
        int(((A > 0) & (d != 0)).sum()), int(((A == 0) & (d != 0)).sum())


def run_case(tag, graph, complete, noise, k_scale, x):
    """graph: coalesced sparse COO [N,N] (what the fixture stores); complete: hand the reference the complete in_adj holding its values"""
    a = base_args(perturb_edge_prob=noise is not None, symmetric_noise=False)
    torch.manual_seed(1234)
    m = dgm.DGG_LearnableK_debug(in_dim=D, latent_dim=H, args=a)
    with torch.no_grad():
        m.k_net.k_project.weight.mul_(k_scale)
    m.train()
    if noise is not None:
        Gt = torch.from_numpy(noise)
        m.gumbel.sample = lambda shape: Gt.reshape(shape)       # dgm.py:1226 draws [1,N,N]
    in_adj = graph
    if complete:
        ar = torch.arange(N)
        ind = torch.stack([ar.repeat_interleave(N), ar.repeat(N)])
        in_adj = torch.sparse_coo_tensor(ind, graph.to_dense().reshape(-1), (N, N)).coalesce()
        assert in_adj._nnz() == N * N
    cap = {}
    _stats = m.get_adj_diff_stats

    def stats(in_adj_, topk_edge_p=None, k=None, writer=None, epoch=None):
        cap["soft"] = topk_edge_p.detach().squeeze(0).clone()
        cap["k"] = k.detach().flatten().clone()
        return _stats(in_adj_, topk_edge_p, k, writer=writer, epoch=epoch)

    m.get_adj_diff_stats = stats
    rec = Recorder()
    m(x, in_adj, writer=rec, epoch=7)
    assert all(rec.scalars["train_stats/" + t][1] == 7 for t in TAGS)
    ref = np.array([rec.scalars["train_stats/" + t][0] for t in TAGS], np.float64)
    soft = cap["soft"]
    nnz = (soft != 0).sum(-1)
    assert int(nnz.max()) <= 64, f"{tag}: a row of the reference output has {int(nnz.max())} non-zeros (k_scale {k_scale})"
    orows, ocols = (t.numpy().astype(np.int32) for t in torch.nonzero(soft, as_tuple=True))
    ovals = soft[soft != 0].numpy()
    gi = graph.indices().numpy().astype(np.int32)
    gv = graph.values().numpy().astype(np.float32)
    k = cap["k"].numpy().astype(np.float32)
    f64, n_on, n_off = stats_f64(N, gi[0], gi[1], gv, orows, ocols, ovals, k)
    if complete:
        assert n_on >= 2 and n_off >= 2, f"{tag}: populations of {n_on} on-edge / {n_off} off-edge pairs"
    else:
        assert n_off == 0 and np.isnan(ref[2]) and np.isnan(ref[3]), f"{tag}: the off-edge population should be empty"
    assert np.array_equal(np.isnan(ref), np.isnan(f64)), (tag, ref, f64)
    dist = np.where(np.isnan(ref), 0.0, np.abs(ref - f64))
    assert np.all(dist <= 1e-4 * np.maximum(1.0, np.abs(np.nan_to_num(f64)))), (tag, ref, f64)      # (float32 sums over <= N^2 terms)
    meta = dict(name="adj_stats_" + tag, N=N, d=D, h=H, torch=torch.__version__, args=vars(a), k_scale=k_scale, tags=list(TAGS),
                complete=bool(complete), n_on=n_on, n_off=n_off, max_row_nnz=int(nnz.max()),
                reference="dgm.py:1288, 1313-1350 DGG_LearnableK_debug.get_adj_diff_stats, training mode")
    fx = {"rows": gi[0], "cols": gi[1], "adj_vals": gv, "k": k, "out_rows": orows, "out_cols": ocols, "out_vals": ovals,
          "ref": ref, "f64": f64, "dist": dist, "meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)}
    path = os.path.join(HERE, f"adj_stats_{tag}.npz")
    np.savez_compressed(path, **fx)
    print(f"adj_stats_{tag}: on {n_on} off {n_off} max row nnz {int(nnz.max())} k [{k.min():.2f}, {k.max():.2f}] {os.path.getsize(path)} bytes")
    for t, r, f in zip(TAGS, ref, f64):
        print(f"    {t:14s} ref {r:+.9e}  f64 {f:+.9e}")


def main():
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(N, D, generator=gen)
    ga = random_graph(N, 12, gen)                               # symmetric, unit weights, self loops
    gb = random_graph(N, 8, gen)
    wt = (2.0 * (1.0 - torch.rand(N, N, generator=gen))).clamp(min=1e-3)          # (0, 2]
    dense = gb.to_dense() * wt
    ii = gb.indices()
    vals = dense[ii[0], ii[1]].clone()
    off_diag = torch.nonzero(ii[0] != ii[1]).flatten()
    vals[off_diag[[3, 57, 211]]] = 0.0                          # stored zeros: the same as absent entries
    vals[off_diag[101]] = -0.75                                 # a stored negative value: in neither population
    gc = torch.sparse_coo_tensor(ii, vals, (N, N)).coalesce()   # (coalesce keeps explicit zeros)
    assert gc._nnz() == gb._nnz()
    G = grid_gumbel(171, (N, N))
    run_case("a", ga, False, None, 1.0, x)
    run_case("b", gb, True, G, 1.0, x)
    run_case("c", gc, True, G, 1.0, x)


if __name__ == "__main__":
    main()
