"""Edge-list candidates ranked into CHUNKED rows: dgg_edgelist_topk_chunked (u-v-dist) and dgg_edgelist_topk_p_chunked (given edge
probabilities: the edge-MLP scorers' path), include/dgg_hip_next.h, against the CPU oracle.

Definition under test: row i keeps its first L_i = min(n_i, ceil(k_i + 8.5) + 1) ranks of oracle.edgelist_topk / oracle.edgelist_topk_p
called with K = 64 * maxm (every candidate of every row, score descending, lower column first) in the chunks of
ops.chunk_layout(min(k_i, n_i - 9.5)), with the weights of oracle.softk on the WHOLE ranked row and the true k.

Graph: N = 704, h = 64 (one case at h = 16), rows of {0, 1, 16, 17, 63, 64, 65, 128, 129, 511, 512, 513, 704} candidates, the rest 1-12;
four duplicated feature rows (exact score ties inside the widest rows).  Degrees {1, 54.5, 54.6, 118.49, n_i - 9.5, 503, 1e6}: the chunk
boundaries of L, the clamp by n_i, rows of 9 and 11 chunks (a pass settles 8: the continuation pass runs) and a row without candidates
whose degree is 1e6 (one chunk, not 15 626).

Bars: idx / val / w of the ranks below L_i and ex / eid of the _p form bit for bit; every oracle weight at a rank >= L_i exactly 0;
the rest of a row's chunks and the spare chunks empty; rs_i within n_i 2^-24 relative of the float64 sum of the oracle's weights (positive
terms: the bound of float32 summation in ANY order), and with the bits of ops.edgelist_topk_softk on one-chunk rows; two runs identical;
NaN / -7 canaries around every output intact; the row ranges cut at {0, 1, 350, 703, 704} equal the whole graph's rows bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_chunked_rows import Nn, chunked_to_rows

pytestmark = pytest.mark.gpu

N = 704
SEED = (1234, 5)
PAD = 256
WIDTHS = {3: 0, 50: 1, 100: 16, 150: 17, 200: 63, 250: 64, 300: 65, 349: 128, 350: 129, 351: 511, 500: 512, 702: 513, 703: 704}
#           row -> k (None: n_i - 9.5)
DEGREES = {3: 1e6, 50: 1e6, 100: 54.5, 150: 1.0, 200: 54.5, 250: 54.6, 300: 54.6, 349: 118.49, 350: None, 351: 503.0, 500: None, 702: 503.0,
           703: 1e6}
CUTS = (0, 1, 350, 703, 704)
NOISE = {"none": 0, "hash": 2, "sym": 3}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def graph():
    """-> rowptr int64 [N+1], col int32 [E] (columns of a row ascending, no duplicates), n [N], k float32 [N]"""
    rng = np.random.default_rng(5)
    n = rng.integers(1, 13, N)
    for i, w in WIDTHS.items():
        n[i] = w
    col = np.concatenate([np.sort(rng.choice(N, c, replace=False)) for c in n]).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    k = np.array([1.0, 54.5, 54.6, 118.49, 503.0, 1e6], np.float32)[rng.integers(0, 6, N)]
    small = rng.random(N) < 0.5
    k[small] = (1.0 + 10.0 * rng.random(N)).astype(np.float32)[small]
    for i, kk in DEGREES.items():
        k[i] = np.float32(n[i] - 9.5) if kk is None else np.float32(kk)
    for a in (rowptr, col, n, k):
        a.setflags(write=False)
    return rowptr, col, n, k


@functools.lru_cache(maxsize=None)
def features(h):
    g = torch.Generator().manual_seed(40 + h)
    xp = (torch.randn(N, h, generator=g) * 0.7).numpy()
    for a, b in ((10, 11), (20, 400), (333, 334), (600, 601)):       # duplicated rows: exact ties wherever both are candidates
        xp[b] = xp[a]
    xp.setflags(write=False)
    return xp


@functools.lru_cache(maxsize=None)
def edge_inputs():
    """p_edge [E] in (0, 1) with exact ties inside the rows, ex_edge [E]"""
    rowptr, col, n, _ = graph()
    rng = np.random.default_rng(9)
    p = rng.random(col.shape[0]).astype(np.float32) * np.float32(0.98) + np.float32(0.01)
    for i in WIDTHS:
        e0, e1 = rowptr[i], rowptr[i + 1]
        if e1 - e0 >= 16:
            p[e0 + 3:e1:5] = p[e0 + 3]                             # every fifth candidate of a wide row carries one probability
    ex = rng.standard_normal(col.shape[0]).astype(np.float32)
    p.setflags(write=False)
    ex.setflags(write=False)
    return p, ex


def limits(n, k):
    """L_i = min(n_i, ceil(k_i + 8.5) + 1) in float32, at least 1 rank (a row always owns a chunk) -> L, M"""
    L = np.minimum(np.ceil(k.astype(np.float32) + np.float32(8.5)) + 1, np.maximum(n, 1)).astype(np.int64)
    return L, (L + 63) // 64


@functools.lru_cache(maxsize=None)
def reference(kind, h, noise, mode):
    """the oracle's whole ranked rows (computed once per case, shared, never modified) -> idx, val, w [N, 64 maxm], eid or None"""
    rowptr, col, n, k = graph()
    K = 64 * int(limits(n, k)[1].max())
    assert K >= n.max()
    if kind == "dist":
        idx, val = O.edgelist_topk(features(h), rowptr, col, K, -0.05, NOISE[noise], None, SEED)
        eid = None
    else:
        idx, val, eid = O.edgelist_topk_p(edge_inputs()[0], N, rowptr, col, K, NOISE[noise], None, SEED)
    w, _ = O.softk(idx, val, k, mode)
    for a in (idx, val, w) + (() if eid is None else (eid,)):
        a.setflags(write=False)
    return idx, val, w, eid


class Canaried:
    """[ccap, 64] int32 / float32 outputs and rs [rows] handed to the kernel as views between canary words, filled with -7 / NaN"""

    def __init__(self, ccap, rows, dev, nint, nflt):
        self.n, self.rows = ccap * 64, rows
        self.bi = [torch.full((self.n + 2 * PAD,), -7, dtype=torch.int32, device=dev) for _ in range(nint)]
        self.bf = [torch.full((self.n + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev) for _ in range(nflt)]
        self.br = torch.full((rows + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)

    def view(self, b):
        return b[PAD:PAD + self.n].view(-1, 64)

    def rs(self):
        return self.br[PAD:PAD + self.rows]

    def canaries_intact(self):
        ok = all(bool((b[:PAD] == -7).all()) and bool((b[PAD + self.n:] == -7).all()) for b in self.bi)
        ok = ok and all(bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[PAD + self.n:]).all()) for b in self.bf)
        return ok and bool(torch.isnan(self.br[:PAD]).all()) and bool(torch.isnan(self.br[PAD + self.rows:]).all())


def layout_of(ops, kd, rowptr_d):
    return ops.chunk_layout(ops.edgelist_clamped_degrees(kd, rowptr_d), ncols=N)


def check_rows(lay, got, ref, n, k, r0=0):
    """got: {name: [>= chunks, 64] tensor} + "rs"; ref: the oracle's ranked rows of the whole graph; rows [r0, r0 + lay.rows)"""
    rows = lay.rows
    n, k = n[r0:r0 + rows], k[r0:r0 + rows]
    L, M = limits(n, k)
    cptr = Nn(lay.cptr).astype(np.int64)
    assert np.array_equal(cptr[1:] - cptr[:-1], M), "the layout of the clamped degrees gives ceil(L_i / 64) chunks per row"
    keep = np.arange(64 * int(M.max()))[None, :] < L[:, None]
    fills = {"idx": -1, "val": 0.0, "w": 0.0, "ex": 0.0, "eid": -1}
    for name, fill in fills.items():
        if name not in got:
            continue
        g = chunked_to_rows(lay, got[name], fill)
        r = ref[name][r0:r0 + rows]
        want = np.where(keep, r[:, :g.shape[1]], fill).astype(r.dtype)
        assert np.array_equal(bits(g), bits(want)), f"{name} differs from the oracle below L_i, or a slot beyond L_i is not empty"
    beyond = np.arange(ref["w"].shape[1])[None, :] >= L[:, None]
    assert (ref["w"][r0:r0 + rows][beyond] == 0).all(), "an oracle weight at a rank >= L_i is not exactly 0"
    rs = Nn(got["rs"]).astype(np.float64)
    want = ref["w"][r0:r0 + rows].astype(np.float64).sum(1)
    assert (np.abs(rs - want) <= n * 2.0 ** -24 * want).all(), "rs beyond n_i 2^-24 of the float64 sum of the oracle's weights"
    return M


def ref_dict(kind, h, noise, mode):
    idx, val, w, eid = reference(kind, h, noise, mode)
    ref = {"idx": idx, "val": val, "w": w}
    if eid is not None:
        ref["eid"] = eid
        ref["ex"] = np.where(eid >= 0, edge_inputs()[1][np.maximum(eid, 0)], 0.0).astype(np.float32)
    return ref


def run_dist(ops, dev, h, noise, mode, rows=None, spare=0):
    """-> layout, outputs, the canaried buffers"""
    rowptr, col, n, k = graph()
    r0, r1 = (0, N) if rows is None else rows
    e0, e1 = rowptr[r0], rowptr[r1]
    rp = torch.from_numpy(rowptr[r0:r1 + 1] - e0).to(dev)
    cd = torch.from_numpy(col[e0:e1].copy()).to(dev)
    kd = torch.from_numpy(k[r0:r1].copy()).to(dev)
    lay = layout_of(ops, kd, rp)
    buf = Canaried(lay.chunks + spare, r1 - r0, dev, 1, 2)
    out = (buf.view(buf.bi[0]), buf.view(buf.bf[0]), buf.view(buf.bf[1]), buf.rs())
    got = ops.edgelist_topk_chunked(torch.from_numpy(features(h).copy()).to(dev), rp, cd, kd, lay, mode, -0.05, NOISE[noise], SEED,
                                    rows=rows, out=out)
    return lay, dict(zip(("idx", "val", "w", "rs"), got)), buf


def run_p(ops, dev, noise, mode, rows=None, spare=0, with_ex=True):
    rowptr, col, n, k = graph()
    p, ex = edge_inputs()
    r0, r1 = (0, N) if rows is None else rows
    e0, e1 = rowptr[r0], rowptr[r1]
    rp = torch.from_numpy(rowptr[r0:r1 + 1] - e0).to(dev)
    cd = torch.from_numpy(col[e0:e1].copy()).to(dev)
    kd = torch.from_numpy(k[r0:r1].copy()).to(dev)
    lay = layout_of(ops, kd, rp)
    buf = Canaried(lay.chunks + spare, r1 - r0, dev, 2, 3)
    out = (buf.view(buf.bi[0]), buf.view(buf.bf[0]), buf.view(buf.bf[1]) if with_ex else None, buf.view(buf.bf[2]), buf.rs(), buf.view(buf.bi[1]))
    got = ops.edgelist_topk_p_chunked(torch.from_numpy(p[e0:e1].copy()).to(dev), N, rp, cd, kd, lay, mode, NOISE[noise], SEED,
                                      ex_edge=torch.from_numpy(ex[e0:e1].copy()).to(dev) if with_ex else None, rows=rows, out=out)
    d = dict(zip(("idx", "val", "ex", "w", "rs"), got))
    if not with_ex:
        assert d.pop("ex") is None
    d["eid"] = out[5] + int(e0)                                    # (the slice's index -> the whole graph's; empty slots checked below)
    d["eid"] = torch.where(out[5] < 0, out[5], d["eid"])
    return lay, d, buf


def check_spare_and_canaries(lay, got, buf, spare):
    sp = slice(lay.chunks, lay.chunks + spare)
    for name, g in got.items():
        if name != "rs":
            assert bool((g[sp] == (-1 if name in ("idx", "eid") else 0)).all()), f"{name}: spare chunks not empty"
    assert buf.canaries_intact(), "written outside the outputs"


def test_the_cases_hit_every_branch():
    rowptr, col, n, k = graph()
    L, M = limits(n, k)
    assert sorted(n[list(WIDTHS)]) == sorted(WIDTHS.values()) and n[[i for i in range(N) if i not in WIDTHS]].max() <= 12
    assert M.max() == 11 and (M == 9).any() and (M == 8).any() and ((M > 1) & (M < 8)).any(), "rows of one pass and of two"
    assert M[3] == 1 and n[3] == 0 and k[3] == 1e6, "no candidate, k = 1e6: one chunk"
    assert (L[150], n[150]) == (11, 17) and (L[250], L[300]) == (64, 65) and (L[349], L[350]) == (128, 129) and L[702] == 513
    assert set(np.float32([1.0, 54.5, 54.6, 118.49, 503.0, 1e6])) <= set(k)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("noise", ["none", "hash", "sym"])
def test_dist_kernel_matches_the_oracle(dev, noise, mode):
    from dgg_amd import ops
    rowptr, col, n, k = graph()
    ref = ref_dict("dist", 64, noise, mode)
    if noise == "none":                                                # the duplicated feature rows tie exactly in the widest row
        v = ref["val"][703]
        assert (v[:-1] == v[1:]).sum() >= 4
    lay, got, buf = run_dist(ops, dev, 64, noise, mode, spare=37)
    M = check_rows(lay, got, ref, n, k)
    check_spare_and_canaries(lay, got, buf, 37)
    # a one-chunk row sums as the list kernel does
    rp, cd, kd = (torch.from_numpy(a.copy()).to(dev) for a in (rowptr, col, k))
    lst = ops.edgelist_topk_softk(torch.from_numpy(features(64).copy()).to(dev), rp, cd, kd, mode, 64, -0.05, NOISE[noise], None, SEED)
    one = M == 1
    assert one.sum() > 600 and np.array_equal(bits(Nn(got["rs"])[one]), bits(Nn(lst[3])[one])), "rs of one-chunk rows: the list kernel's bits"
    # two runs, identical bits
    _, again, _ = run_dist(ops, dev, 64, noise, mode, spare=37)
    for name in got:
        assert np.array_equal(bits(Nn(got[name])), bits(Nn(again[name]))), f"{name}: two runs differ"


def test_dist_kernel_at_latent_width_16(dev):
    from dgg_amd import ops
    _, _, n, k = graph()
    lay, got, buf = run_dist(ops, dev, 16, "hash", 0, spare=5)
    check_rows(lay, got, ref_dict("dist", 16, "hash", 0), n, k)
    check_spare_and_canaries(lay, got, buf, 5)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("noise", ["none", "hash", "sym"])
def test_p_kernel_matches_the_oracle(dev, noise, mode):
    from dgg_amd import ops
    _, _, n, k = graph()
    ref = ref_dict("p", 0, noise, mode)
    if noise == "none":
        v = ref["val"][703]
        assert (v[:-1] == v[1:]).sum() >= 100, "the tied probabilities of the widest row"
    lay, got, buf = run_p(ops, dev, noise, mode, spare=37)
    check_rows(lay, got, ref, n, k)
    check_spare_and_canaries(lay, got, buf, 37)
    _, again, _ = run_p(ops, dev, noise, mode, spare=37)
    for name in got:
        assert np.array_equal(bits(Nn(got[name])), bits(Nn(again[name]))), f"{name}: two runs differ"
    # without the extras: the same rows, ex untouched
    lay2, got2, buf2 = run_p(ops, dev, noise, mode, with_ex=False)
    check_rows(lay2, got2, ref, n, k)
    assert bool(torch.isnan(buf2.bf[1]).all()) and buf2.canaries_intact()


@pytest.mark.parametrize("kind", ["dist", "p"])
def test_row_ranges_give_the_whole_graphs_rows(dev, kind):
    from dgg_amd import ops
    _, _, n, k = graph()
    ref = ref_dict(kind, 64 if kind == "dist" else 0, "hash", 0)
    run = (lambda rows: run_dist(ops, dev, 64, "hash", 0, rows=rows, spare=3)) if kind == "dist" else (lambda rows: run_p(ops, dev, "hash", 0, rows=rows, spare=3))
    _, whole, _ = run(None)
    rs_whole = Nn(whole["rs"])
    for r0, r1 in zip(CUTS[:-1], CUTS[1:]):
        lay, got, buf = run((r0, r1))
        check_rows(lay, got, ref, n, k, r0)
        check_spare_and_canaries(lay, got, buf, 3)
        assert np.array_equal(bits(Nn(got["rs"])), bits(rs_whole[r0:r1])), f"rows [{r0}, {r1}): rs differs from the whole graph's"


def test_refusals_and_the_empty_range(dev):
    from dgg_amd import _lib, ops
    rowptr, col, n, k = graph()
    rp, cd, kd = (torch.from_numpy(a.copy()).to(dev) for a in (rowptr, col, k))
    lay = layout_of(ops, kd, rp)
    xp = torch.from_numpy(features(64).copy()).to(dev)
    with pytest.raises(_lib.DggHipError, match="noise_mode"):
        ops.edgelist_topk_chunked(xp, rp, cd, kd, lay, 0, -0.05, 4, SEED)
    with pytest.raises(_lib.DggHipError, match="mode must be"):
        ops.edgelist_topk_chunked(xp, rp, cd, kd, lay, 2, -0.05, 0, SEED)
    with pytest.raises(_lib.DggHipError, match="noise_mode"):
        ops.edgelist_topk_p_chunked(torch.from_numpy(edge_inputs()[0].copy()).to(dev), N, rp, cd, kd, lay, 0, 1, SEED)
    assert ops.edgelist_topk_chunked(xp[:, :24].contiguous(), rp, cd, kd, lay) is None
    # row0 == row1: success without a launch, nothing written
    L = _lib.lib()
    buf = Canaried(4, 1, dev, 1, 2)
    rc = L.dgg_edgelist_topk_chunked(xp.data_ptr(), N, 64, 5, 5, rp.data_ptr(), cd.data_ptr(), -0.05, 0, 0, 0, kd.data_ptr(), 0, 1, lay.cptr.data_ptr(),
                                     4, buf.bi[0].data_ptr(), buf.bf[0].data_ptr(), buf.bf[1].data_ptr(), buf.br.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and bool((buf.bi[0] == -7).all()) and bool(torch.isnan(buf.bf[0]).all())
    for maxm, ccap in ((0, 4), ((1 << 20) + 1, 4), (1, -1), (1, 1 << 25)):
        rc = L.dgg_edgelist_topk_chunked(xp.data_ptr(), N, 64, 0, N, rp.data_ptr(), cd.data_ptr(), -0.05, 0, 0, 0, kd.data_ptr(), 0, maxm,
                                         lay.cptr.data_ptr(), ccap, buf.bi[0].data_ptr(), buf.bf[0].data_ptr(), buf.bf[1].data_ptr(), buf.br.data_ptr(), None)
        assert rc == 1 and b"maxm in 1..2^20" in L.dgg_last_error(), (maxm, ccap)
