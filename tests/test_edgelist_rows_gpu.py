"""Row-range forms of the edge-list entries on the MI355X (include/dgg_hip.h, dgg_edgelist_topk_softk_rows and its kin): for every cut
[r0, r1) -- empty, a single row, rows of at most 16 candidates (the pack-4 kernel), rows wider than 64 -- the shard's rebased CSR slice
gives the matching rows of the full-range entry bit for bit (idx, val, w, rs, the ELL-bound flag, eid mapped back), and the row-range
scorer backward summed over a partition of the rows gives the full-range dAB / dpar."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
K = 64


@pytest.fixture(scope="module")
def dev():
    sys.path.insert(0, ROOT)
    import dgg_amd  # noqa: F401
    return torch.device("cuda", 0)


def graph(N=3000, seed=5):
    """CSR with self loops: rows 0..999 hold 1-16 candidates (pack-4 rows), 1000..2499 17-60, a few hubs of 100-300 (wider than the
    list), the rest 1-8"""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 16, N)
    n[1000:2500] = rng.integers(16, 60, 1500)
    for r in (5, 1003, 1777, 2600, 2999):
        n[r] = rng.integers(100, 300)
    n[2500:] = np.minimum(n[2500:], 7)
    for r in (2600, 2999):
        n[r] = 200
    cols = [np.unique(np.append(rng.choice(N, n[i], replace=False), i)).astype(np.int32) for i in range(N)]
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum([len(c) for c in cols])
    return torch.from_numpy(rowptr), torch.from_numpy(np.concatenate(cols))


CUTS = [(1234, 1234), (0, 0), (5, 6), (7, 8), (0, 1000), (40, 300), (1000, 2500), (990, 1010), (2500, 3000), (2999, 3000), (0, 3000)]


def _bound_flag(rowptr, k, r0, r1):
    lens = (rowptr[1:] - rowptr[:-1])[r0:r1]
    return bool(((lens > K) & (k[r0:r1] + 8.5 > K)).any())


@pytest.mark.parametrize("h", [32, 64])
@pytest.mark.parametrize("noise_mode", [0, 2, 3])
def test_topk_softk_rows_match_full_range(dev, h, noise_mode):
    from dgg_amd import ops
    from dgg_amd.parallel import csr_rows
    N = 3000
    rowptr, col = graph(N)
    rowptr, col = rowptr.to(dev), col.to(dev)
    g = torch.Generator().manual_seed(h + noise_mode)
    xp = torch.randn(N, h, generator=g).to(dev)
    k = (3 + 70 * torch.rand(N, generator=g)).to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    full = ops.edgelist_topk_softk(xp, rowptr, col, k, ops.MODE_K_TIMES_EDGE_PROB, K, ops.T_DIST, noise_mode, None, (7, 9), overflow=flag)
    assert int(flag.item()) == int(_bound_flag(rowptr, k, 0, N))
    for r0, r1 in CUTS:
        rp, cl, _ = csr_rows(rowptr, col, (r0, r1))
        fl = torch.zeros(1, dtype=torch.int32, device=dev)
        got = ops.edgelist_topk_softk(xp, rp, cl, k[r0:r1].contiguous(), ops.MODE_K_TIMES_EDGE_PROB, K, ops.T_DIST, noise_mode, None, (7, 9),
                                      overflow=fl, rows=(r0, r1))
        for name, a, b in zip(("idx", "val", "w", "rs"), got, full):
            assert a.shape[0] == r1 - r0
            assert torch.equal(a, b[r0:r1]), (name, r0, r1)
        assert int(fl.item()) == int(_bound_flag(rowptr, k, r0, r1)), (r0, r1)


@pytest.mark.parametrize("noise_mode", [0, 2, 3])
def test_topk_p_and_scorer_backward_rows_match_full_range(dev, noise_mode):
    from dgg_amd import ops
    from dgg_amd.parallel import csr_rows
    N, hw = 3000, 16
    rowptr, col = graph(N, seed=8)
    rowptr, col = rowptr.to(dev), col.to(dev)
    E = col.shape[0]
    g = torch.Generator().manual_seed(30 + noise_mode)
    p = (0.02 + 0.96 * torch.rand(E, generator=g)).to(dev)
    full = ops.edgelist_topk_p(p, N, rowptr, col, K, noise_mode, None, (3, 4))
    for r0, r1 in CUTS:
        rp, cl, (e0, e1) = csr_rows(rowptr, col, (r0, r1))
        idx, val, eid = ops.edgelist_topk_p(p[e0:e1].contiguous(), N, rp, cl, K, noise_mode, None, (3, 4), rows=(r0, r1))
        assert torch.equal(idx, full[0][r0:r1]) and torch.equal(val, full[1][r0:r1]), (r0, r1)
        assert torch.equal(torch.where(eid >= 0, eid + e0, eid), full[2][r0:r1]), (r0, r1)          # (eid: the slice's own edge ids)
    # the scorer backward (u-v-A_uv-like: degrees and a per-edge extra read through eid) summed over a partition of the rows
    idx, val, eid = full
    rnd = lambda *sh: (0.3 * torch.randn(*sh, generator=g)).to(dev)  # noqa: E731
    AB, deg, ex = rnd(N, 2 * hw), (1 + 30 * torch.rand(N, generator=g)).to(dev), torch.rand(E, generator=g).to(dev)
    # (positive cotangents and pre-activations: the parameter sums then add terms of one sign each, so the comparison measures the row
    #  decomposition and not the conditioning of a cancelling fp32 sum over ~10^5 atomically accumulated terms)
    wdu, wdv, wex, b1, w2, b2 = rnd(hw), rnd(hw), rnd(hw), 1.0 + rnd(hw), rnd(hw), rnd(1)
    dval = torch.where(idx >= 0, rnd(N, K).abs(), torch.zeros(N, K, device=dev))
    args = (deg, ex, wdu, wdv, wex, b1, w2, b2, ops.ACT_LEAKY, noise_mode != 0)
    dAB_f, dpar_f, _ = ops.edge_mlp_bwd(AB, idx, eid, val, dval, *args)
    dAB_s, dpar_s = torch.zeros_like(dAB_f), torch.zeros_like(dpar_f)
    for r0, r1 in [(0, 0), (0, 1), (1, 16), (16, 1000), (1000, 1000), (1000, 2999), (2999, N)]:
        _, _, (e0, e1) = csr_rows(rowptr, col, (r0, r1))
        sl = slice(r0, r1)
        el = torch.where(eid[sl] >= 0, eid[sl] - e0, eid[sl]).contiguous()
        a, b, _ = ops.edge_mlp_bwd(AB, idx[sl].contiguous(), el, val[sl].contiguous(), dval[sl].contiguous(), deg, ex[e0:e1].contiguous(),
                                   *args[2:], rows=(r0, r1))
        dAB_s += a
        dpar_s += b
    torch.cuda.synchronize()
    for a, b in ((dAB_s, dAB_f), (dpar_s, dpar_f)):
        assert float(b.abs().max()) > 0
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), float((a - b).abs().max())
