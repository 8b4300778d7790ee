"""The CSR adjacency kernels of csrc/dgg_csr.hip against exact and float64 references.

These kernels run whenever the adjacency keeps the pattern of in_adj: the `DGG` class and the *_DGG_00 wrappers, DGG_Ablations,
GATConv_DGG's background softmax and attention dropout, the u-v-dist scorer on stored entries, and the fallback of
DGG_LearnableK_debug when a learned degree exceeds the 64-wide list (ops.CsrSoftkFn).  This module calls every one of them through the C
ABI (dgg_csr_perturb_fwd / _bwd are held by tests/test_perturbed_scores.py).

Graph (build_graph): seeded, unique ascending columns per row, N = 270 nodes and rows of EVERY length in {0, 1, 2, 63, 64, 65, 127,
128, 129, 200} placed in the first, a middle and the last block of four rows (one wavefront per row, four per block), a row with a
self loop, a hub column that every non-empty row lists.  A row that lists every column and a node that no row lists exclude each
other, so the builder has two forms: `full` (the `all` row has cnt == N) and `unlisted` (the `all` row lists every column except the
nodes of the empty and the 1-long row, which nobody lists).  Every row-per-wavefront kernel runs at N, N + 1, N + 2, N + 3 (1, 2, 3,
4 live wavefronts in the last block; the last four rows are named rows) and at N = 1.  Every output is handed in NaN-filled (int32:
-7777) between canary words, every input sits between NaN guards (Guard of test_partitioned_backward.py); N == 0 / E == 0 and every
refusal return their documented code and write nothing.  64-bit offsets (E >= 2^31) cannot be reached at test sizes and are not tested.

Tier 1, bit for bit
  canonical forwards against the oracle (oracle/dgg_oracle.c): row_sum, normalize_fwd, spmm_fwd (F in 1, 63, 64, 65, 130),
    rank_ramp_fwd (out, S, k, pos), rank_cut_fwd (kcut in 0, 1, 63, 64, 65, 200, 1000), noisy_sigmoid_fwd, uvdist_fwd (h in 1, 16,
    128, 129, 192: both branches of pair_d2_thread).  Values to rank: positive normal floats and +0.0, exact ties across a chunk
    boundary (entries 60..70 of the 129-long row), the 65-long row entirely tied, first entry of the 200-long row tied with its last.
    normalize: the empty row and a zero-sum row (the 1-long row with weight +0.0) have rs = 0 and are listed by nobody; the zero-sum
    row's own entry is 0 * inf = NaN on both sides.
  dgg_csr_softk_fwd against a reference composed from oracle primitives (softk_reference): pp = O.exp(O.log(p + 1e-8) + g) rounded
    step by step, g from an explicit matrix (ldG = N + 3, NaN in the padding columns) or ora_noise, pos by a stable sort on (pp
    descending, column ascending), ramp = 1 - 0.5 (1 + O.tanh(pos - k)); four noise modes x two k-select modes; k below 0, near the
    row's length and beyond it; some p exactly 0.  w, pp, pos equal bit for bit.
  integer-exact backwards and sums: spmm_bwd (a, X, dY integers |.| <= 3; dX starts at a non-zero integer pattern; dX = NULL; a == 0
    entries), norm_bwd (rs in {1, 4, 16}, w in {1, 2}: every factor a power of two), masked_dense_sum (integer X against the numpy
    restatement of the pair mask, F in 1, 7, 8, 9, 16, 17, 32, 33, 64, both transposes, p in 0, 0.3, 0.9, N in 1, 7, 8, 9, 130),
    rank_cut_bwd / noisy_sigmoid_bwd at E in 1, 255, 256, 257.  test_exactness_premises_hold_for_every_case proves per case that
    every term is a multiple of the unit and every sum of magnitudes stays below 2^24 units.

Tier 2, float64.  Reference: restate_*(np.float64, ...) = the oracle's formula in numpy float64 (checked on the CPU against the float32
oracle function where one exists, against a dense softmax / torch autograd in float64 where none does).  pos, pp, S, k, p, att and bg come
from the bit-exact or forward side and are inputs of BOTH sides, so no rank can swap and no element is left out: the excluded share is
0 and every test asserts it.  Statistic: max|got - ref| / max|ref| per output.  Bar: 4 x the larger error of the same arithmetic in
float32 on the CPU (restate_*(np.float32, ...), tanh / exp as the kernel takes them: ora_tanh, and for bg_softmax's __expf a float32
product with log2 e followed by exp2) in two summation orders, row order and a seeded shuffle -- the margin test_weight_gradients.py
established.  bg_softmax: logits 3 N(0,1), one row all negative, one row with an outlier of +60, the full row (bg == 0 exactly), the
empty row (bg = 1/N exactly), and sum att + (N - cnt) bg = 1 within the bar of the identity's own CPU error.  uvdist_bwd: twin nodes
joined by an entry and a self loop contribute exactly 0, an entry with dp == 0, dxp starts non-zero, untouched rows come back bit for
bit.  softk_bwd with perturb = 1: some p exactly 0.

Measured on an MI355X (err / max|ref| per output; the bar is computed in the test from the two CPU columns, nothing is fixed here; N = 1:
a single self loop).  `identity` is max_i |sum att + (N - cnt) bg - 1| with its own CPU figures.  mode 1 of softk_bwd has dp == 0 on both
sides.  Every MI355X figure is under its bar; the 79 GPU tests of this module take 4 s.

  output                                    CPU row   CPU shuf   bar = 4x     MI355X
  rank_ramp_bwd dp N=270                  6.89e-08   6.89e-08   2.76e-07   6.89e-08
  rank_ramp_bwd dkz N=270                 9.64e-08   1.56e-07   6.24e-07   1.31e-07
  rank_ramp_bwd dp N=271                  1.02e-07   1.02e-07   4.06e-07   1.02e-07
  rank_ramp_bwd dkz N=271                 1.46e-07   1.38e-07   5.83e-07   1.79e-07
  rank_ramp_bwd dp N=272                  8.45e-08   8.45e-08   3.38e-07   8.42e-08
  rank_ramp_bwd dkz N=272                 1.58e-07   1.58e-07   6.32e-07   1.21e-07
  rank_ramp_bwd dp N=273                  5.51e-08   5.51e-08   2.20e-07   5.51e-08
  rank_ramp_bwd dkz N=273                 1.54e-07   1.30e-07   6.16e-07   1.85e-07
  rank_ramp_bwd dp N=1                    2.03e-08   2.03e-08   8.12e-08   2.03e-08
  rank_ramp_bwd dkz N=1                   3.37e-08   3.37e-08   1.35e-07   3.37e-08
  softk_bwd perturb=0 mode=0 N=270 dp     4.34e-08   4.34e-08   1.74e-07   4.34e-08
  softk_bwd perturb=0 mode=0 N=270 dk     1.17e-07   1.27e-07   5.06e-07   1.03e-07
  softk_bwd perturb=0 mode=1 N=271 dp     0.00e+00   0.00e+00   0.00e+00   0.00e+00
  softk_bwd perturb=0 mode=1 N=271 dk     1.31e-07   1.69e-07   6.77e-07   1.69e-07
  softk_bwd perturb=1 mode=0 N=272 dp     2.73e-08   2.73e-08   1.09e-07   2.73e-08
  softk_bwd perturb=1 mode=0 N=272 dk     2.22e-07   2.22e-07   8.89e-07   2.22e-07
  softk_bwd perturb=1 mode=1 N=273 dp     0.00e+00   0.00e+00   0.00e+00   0.00e+00
  softk_bwd perturb=1 mode=1 N=273 dk     1.62e-07   1.23e-07   6.48e-07   1.21e-07
  softk_bwd perturb=1 mode=0 N=1 dp       1.43e-07   1.43e-07   5.73e-07   1.43e-07
  softk_bwd perturb=1 mode=0 N=1 dk       2.95e-08   2.95e-08   1.18e-07   2.95e-08
  uvdist_bwd dxp h=1 N=270                2.48e-07   3.39e-07   1.36e-06   2.00e-07
  uvdist_bwd dxp h=63 N=271               4.78e-07   4.78e-07   1.91e-06   5.07e-07
  uvdist_bwd dxp h=64 N=272               3.71e-07   3.71e-07   1.48e-06   3.71e-07
  uvdist_bwd dxp h=65 N=273               8.64e-07   8.64e-07   3.46e-06   8.64e-07
  uvdist_bwd dxp h=130 N=270              5.89e-07   5.89e-07   2.36e-06   5.89e-07
  uvdist_bwd dxp h=16 N=1                 0.00e+00   0.00e+00   0.00e+00   0.00e+00
  spmm_bwd dA F=1 N=270                   3.53e-08   3.53e-08   1.41e-07   3.53e-08
  spmm_bwd dX F=1 N=270                   7.08e-08   1.46e-07   5.82e-07   7.20e-08
  norm_bwd dw N=270                       1.80e-07   3.45e-07   1.38e-06   1.03e-07
  spmm_bwd dA F=63 N=271                  2.04e-07   2.50e-07   1.00e-06   8.55e-08
  spmm_bwd dX F=63 N=271                  3.41e-07   2.69e-07   1.36e-06   2.88e-07
  norm_bwd dw N=271                       2.68e-07   9.16e-08   1.07e-06   9.16e-08
  spmm_bwd dA F=64 N=272                  3.02e-07   2.82e-07   1.21e-06   7.71e-08
  spmm_bwd dX F=64 N=272                  3.56e-07   2.73e-07   1.42e-06   4.51e-07
  norm_bwd dw N=272                       1.71e-07   1.71e-07   6.83e-07   1.32e-07
  spmm_bwd dA F=65 N=273                  2.41e-07   2.73e-07   1.09e-06   8.68e-08
  spmm_bwd dX F=65 N=273                  3.41e-07   4.06e-07   1.62e-06   4.15e-07
  norm_bwd dw N=273                       8.29e-08   1.15e-07   4.59e-07   1.16e-07
  spmm_bwd dA F=130 N=270                 4.84e-07   4.60e-07   1.94e-06   8.30e-08
  spmm_bwd dX F=130 N=270                 2.97e-07   3.71e-07   1.49e-06   5.08e-07
  norm_bwd dw N=270                       1.97e-07   1.08e-07   7.87e-07   1.04e-07
  bg_softmax_fwd att N=270                2.47e-07   4.26e-07   1.70e-06   1.21e-07
  bg_softmax_fwd bg N=270                 6.17e-08   6.17e-08   2.47e-07   6.17e-08
  bg_softmax_fwd identity N=270           2.92e-07   4.94e-07   1.97e-06   1.92e-07
  bg_softmax_bwd dL N=270                 4.99e-07   3.51e-07   2.00e-06   3.03e-07
  bg_softmax_fwd att N=271                4.47e-07   4.47e-07   1.79e-06   1.48e-07
  bg_softmax_fwd bg N=271                 8.06e-08   6.75e-08   3.22e-07   8.06e-08
  bg_softmax_fwd identity N=271           6.85e-07   6.85e-07   2.74e-06   1.88e-07
  bg_softmax_bwd dL N=271                 1.81e-07   2.43e-07   9.73e-07   2.16e-07
  bg_softmax_fwd att N=272                2.24e-07   1.85e-07   8.96e-07   1.22e-07
  bg_softmax_fwd bg N=272                 7.41e-08   7.76e-08   3.10e-07   6.44e-08
  bg_softmax_fwd identity N=272           2.25e-07   3.01e-07   1.21e-06   1.92e-07
  bg_softmax_bwd dL N=272                 3.14e-07   4.72e-07   1.89e-06   1.97e-07
  bg_softmax_fwd att N=273                1.98e-07   2.10e-07   8.40e-07   1.19e-07
  bg_softmax_fwd bg N=273                 6.85e-08   8.75e-08   3.50e-07   6.53e-08
  bg_softmax_fwd identity N=273           3.56e-07   2.23e-07   1.42e-06   1.41e-07
  bg_softmax_bwd dL N=273                 1.87e-07   3.04e-07   1.22e-06   1.56e-07
  bg_softmax_fwd att N=1                  0.00e+00   0.00e+00   0.00e+00   0.00e+00
  bg_softmax_fwd bg N=1                   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  bg_softmax_fwd identity N=1             0.00e+00   0.00e+00   0.00e+00   0.00e+00
  bg_softmax_bwd dL N=1                   0.00e+00   0.00e+00   0.00e+00   0.00e+00
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from test_partitioned_backward import CANARY, Guard, nans, rel_max

ERR_ARG, ERR_UNSUPPORTED = 1, 2
EXACT_LIMIT = 1 << 24
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
N0 = 270
SIZES = (N0, N0 + 1, N0 + 2, N0 + 3, 1)
T_DIST = float(np.float32(-0.05))
ICANARY, IFILL = np.int32(-24680), np.int32(-7777)
F32 = np.float32
EPS = np.float32(1e-8)
LEAKY = np.float32(0.01)
LOG2E = np.float32(1.4426950408889634)
SPMM_F = (1, 63, 64, 65, 130)
UV_H = (1, 16, 128, 129, 192)
UVB_H = (1, 63, 64, 65, 130)
KCUTS = (0, 1, 63, 64, 65, 200, 1000)
MDS_F = (1, 7, 8, 9, 16, 17, 32, 33, 64)
MDS_P = (0.0, 0.3, 0.9)
MDS_N = (1, 7, 8, 9, 130)
MDS_SEED = (12345, 678)
ELEM_E = (1, 255, 256, 257)
SPMM_BWD = [(F, (N0, N0 + 1, N0 + 2, N0 + 3)[q % 4]) for q, F in enumerate(SPMM_F)] + [(65, 1)]          # (F, N)
UV_BWD = [(h, (N0, N0 + 1, N0 + 2, N0 + 3)[q % 4]) for q, h in enumerate(UVB_H)] + [(16, 1)]             # (h, N)


# ---------------------------------------------------------------------------------------------------------------
# one graph builder with prescribed row lengths
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build_graph(N, full=True, seed=0):
    """-> dict: rowptr int64 [N+1], col int32 [E], erow int64 [E], N, E, named {length or 'all' or 'self': row}, hub, unlisted (nodes no
    row lists; empty when `full`).  N = 1: the single row is a self loop."""
    if N == 1:
        return dict(rowptr=np.array([0, 1], np.int64), col=np.zeros(1, np.int32), erow=np.zeros(1, np.int64), N=1, E=1, named={"self": 0},
                    hub=0, unlisted=[], full=True)
    assert N >= 203
    rng = np.random.default_rng(9000 + 7 * N + seed)
    mid = (N // 2) // 4 * 4
    place = {129: 0, 0: 1, 200: 2, 64: 3, "all": mid, 65: mid + 1, 1: mid + 2, 127: mid + 3, 63: N - 4, 128: N - 3, 2: N - 2, "self": N - 1}
    length = rng.integers(1, 25, N)
    for name, row in place.items():
        length[row] = {"all": N, "self": 9}.get(name, name)
    unlisted = [] if full else [place[0], place[1]]
    hub = int(mid + 9)
    allowed = np.setdiff1d(np.arange(N), unlisted)
    length = np.minimum(length, len(allowed))
    cols = []
    for i in range(N):
        n = int(length[i])
        must = ([hub] if n >= 1 else []) + ([i] if i == place["self"] else [])
        rest = rng.permutation(np.setdiff1d(allowed, must))[:n - len(must)]
        cols.append(np.sort(np.concatenate([np.array(must, np.int64), rest]).astype(np.int64)))
    rowptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    col = np.concatenate(cols).astype(np.int32)
    erow = np.repeat(np.arange(N), length)
    return dict(rowptr=rowptr, col=col, erow=erow, N=N, E=int(rowptr[-1]), named=place, hub=hub, unlisted=unlisted, full=full)


def check_graph(g):
    N, rowptr, col = g["N"], g["rowptr"], g["col"]
    cnt = np.diff(rowptr)
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == g["E"] and np.array_equal(g["erow"], np.repeat(np.arange(N), cnt))
    for i in range(N):
        c = col[rowptr[i]:rowptr[i + 1]]
        assert (np.diff(c) > 0).all() and (len(c) == 0 or (0 <= c[0] and c[-1] < N)), "row %d: columns not unique ascending" % i
        assert len(c) == 0 or g["hub"] in c, "row %d does not list the hub" % i
    if N == 1:
        return
    for L in LENGTHS:
        assert cnt[g["named"][L]] == L, "no row of length %d" % L
    assert cnt[g["named"]["all"]] == N - len(g["unlisted"]) and (cnt[g["named"]["all"]] == N) == g["full"]
    s = g["named"]["self"]
    assert s in col[rowptr[s]:rowptr[s + 1]]
    listed = np.bincount(col, minlength=N)
    assert all(listed[u] == 0 for u in g["unlisted"]) and (g["full"] or len(g["unlisted"]) == 2)
    assert listed[g["hub"]] == (cnt > 0).sum()
    blocks = {r // 4 for r in g["named"].values()}
    assert 0 in blocks and (N - 1) // 4 in blocks and ((N // 2) // 4) in blocks
    assert all(r in g["named"].values() for r in range(N - 4, N))          # every live wavefront of the last block is a named row


def test_graph_builder_prescribes_every_row_length():
    for N in SIZES:
        for full in (True, False):
            g = build_graph(N, full)
            check_graph(g)
    g = build_graph(N0, False)
    assert g["E"] <= 25000 and sorted(g["unlisted"]) == sorted([g["named"][0], g["named"][1]])
    # ... and the check notices a row that lost its hub or a length that is missing
    bad = dict(g)
    bad["col"] = np.where(g["col"] == g["hub"], (g["hub"] + 1) % N0, g["col"]).astype(np.int32)
    with pytest.raises(AssertionError):
        check_graph(bad)


def seg(g, name):
    r = g["named"][name]
    return int(g["rowptr"][r]), int(g["rowptr"][r + 1])


def rank_values(g, seed=0, zeros=True):
    """values to rank: positive normal floats, some +0.0, and the prescribed exact ties"""
    rng = np.random.default_rng(100 + seed + g["N"])
    p = (0.05 + 0.9 * rng.random(g["E"])).astype(F32)
    if zeros:
        p[rng.random(g["E"]) < 0.03] = 0.0
    if g["N"] > 1:
        a, _ = seg(g, 129)
        p[a + 60:a + 71] = F32(0.625)                               # a run of ties across the 64-entry chunk boundary
        a, b = seg(g, 65)
        p[a:b] = F32(0.3)                                           # one row entirely tied
        a, b = seg(g, 200)
        p[a] = p[b - 1] = F32(0.97)                                 # first and last entry tied (the row's best two)
    assert not np.signbit(p).any() and (p[p > 0] >= np.finfo(F32).tiny).all()
    return p


def vec(fn):
    return np.vectorize(fn, otypes=[np.float32])


def tanh32(x):
    from oracle import oracle as O
    return vec(O.tanh)(np.asarray(x, F32)) if np.size(x) else np.zeros(np.shape(x), F32)


# ---------------------------------------------------------------------------------------------------------------
# dgg_csr_softk_fwd: reference composed from oracle primitives
# ---------------------------------------------------------------------------------------------------------------
def entry_noise(g, noise_mode, Gm, seed):
    from oracle import oracle as O
    if noise_mode == 1:
        return Gm[g["erow"], g["col"]].astype(F32)
    L = O.lib()
    return np.array([L.ora_noise(seed[0], seed[1], int(i), int(j), int(noise_mode == 3)) for i, j in zip(g["erow"], g["col"])], F32)


def positions_by_sort(g, v):
    """pos [E]: place of every entry in its row's stable sort on (v descending, column ascending)"""
    pos = np.empty(g["E"], np.int32)
    for i in range(g["N"]):
        a, b = int(g["rowptr"][i]), int(g["rowptr"][i + 1])
        order = np.argsort(-v[a:b].astype(np.float64), kind="stable")          # columns ascend within a row: stable = lower column first
        pos[a + order] = np.arange(b - a, dtype=np.int32)
    return pos


def ramp32(pos, k_e):
    th = tanh32(pos.astype(F32) - k_e)
    a = F32(1) + th
    a = F32(0.5) * a
    return (F32(1) - a).astype(F32)


def softk_reference(g, p, k, noise_mode, Gm, seed, mode):
    from oracle import oracle as O
    if noise_mode == 0:
        pp = p.copy()
    else:
        lp = vec(O.log)((p + EPS).astype(F32))
        pp = vec(O.exp)((lp + entry_noise(g, noise_mode, Gm, seed)).astype(F32))
    pos = positions_by_sort(g, pp)
    r = ramp32(pos, k[g["erow"]])
    w = (pp * r).astype(F32) if mode == 0 else r
    return w, pp, pos


def softk_inputs(g, noise_mode, seed=0):
    rng = np.random.default_rng(300 + g["N"] + noise_mode + seed)
    N, cnt = g["N"], np.diff(g["rowptr"]).astype(np.float64)
    p = rank_values(g, seed=noise_mode)
    kinds = rng.integers(0, 4, N)
    k = np.select([kinds == 0, kinds == 1, kinds == 2], [np.full(N, -3.5), cnt - 0.5, cnt + 20.0], rng.random(N) * (cnt + 1)).astype(F32)
    for name, kv in ((129, 64.25), (200, 199.5), (64, -1.0), ("all", 300.0)):
        if name in g["named"]:
            k[g["named"][name]] = kv
    Gm = None
    if noise_mode == 1:
        Gm = np.full((N, N + 3), np.nan, F32)
        Gm[:, :N] = (0.3 * rng.gumbel(size=(N, N))).astype(F32)
    return p, k, Gm


SOFTK_SEED = (4321, 99)
SOFTK_CASES = [(nm, mode, SIZES[(2 * nm + mode) % 4]) for nm in range(4) for mode in (0, 1)] + [(2, 0, 1), (1, 1, 1), (0, 0, N0 + 3)]


def test_composed_positions_equal_the_oracles_rank_cut():
    from oracle import oracle as O
    for N in (N0, N0 + 1, 1):
        g = build_graph(N)
        p = rank_values(g)
        _, pos_o = O.csr_rank_cut(p, g["rowptr"], g["col"], 5)
        assert np.array_equal(positions_by_sort(g, p), pos_o)
        _, _, _, pos_r = O.csr_rank_ramp(p, g["rowptr"], g["col"], 0.4, -0.3)
        assert np.array_equal(pos_o, pos_r)
    # the ramp composed from O.tanh is the oracle's own: rank_ramp's out = p * (ramp + 1)
    g = build_graph(N0)
    p = rank_values(g)
    out, S, k, pos = O.csr_rank_ramp(p, g["rowptr"], g["col"], 0.4, -0.3)
    assert np.array_equal(out, (p * (ramp32(pos, k[g["erow"]]) + F32(1)).astype(F32)).astype(F32))
    # ordering by bit pattern (the kernels' make_key) agrees with float comparison exactly on non-negative values without -0.0
    v = np.array([0.0, 1e-38, 0.3, 0.97, 3e38], F32)
    assert (np.diff(v.view(np.uint32).astype(np.int64)) > 0).all()
    assert np.array([-0.0], F32).view(np.uint32)[0] > np.array([3e38], F32).view(np.uint32)[0]        # -0.0 would outrank everything


# ---------------------------------------------------------------------------------------------------------------
# tier 1: integer-exact cases and their premises
# ---------------------------------------------------------------------------------------------------------------
def ints(rng, shape, lim=3):
    return rng.integers(-lim, lim + 1, shape).astype(F32)


@functools.lru_cache(maxsize=None)
def spmm_bwd_case(F, N):
    g = build_graph(N, False)
    rng = np.random.default_rng(500 + F + N)
    a = ints(rng, g["E"])
    return dict(g=g, a=a, X=ints(rng, (N, F)), dY=ints(rng, (N, F)), dX0=ints(rng, (N, F), 5))


def spmm_bwd_exact(c):
    g = c["g"]
    i, j = g["erow"], g["col"].astype(np.int64)
    dA = (c["dY"].astype(np.float64)[i] * c["X"].astype(np.float64)[j]).sum(1)
    dX = c["dX0"].astype(np.float64)
    np.add.at(dX, j, c["a"].astype(np.float64)[:, None] * c["dY"].astype(np.float64)[i])
    absA = (np.abs(c["dY"]).astype(np.float64)[i] * np.abs(c["X"]).astype(np.float64)[j]).sum(1)
    absX = np.abs(c["dX0"]).astype(np.float64)
    np.add.at(absX, j, np.abs(c["a"]).astype(np.float64)[:, None] * np.abs(c["dY"]).astype(np.float64)[i])
    whole = all(np.array_equal(v, np.round(v)) for v in (c["a"], c["X"], c["dY"], c["dX0"]))
    return dA, dX, whole and max(absA.max(initial=0), absX.max(initial=0)) < EXACT_LIMIT


@functools.lru_cache(maxsize=None)
def norm_bwd_case(N):
    g = build_graph(N, True)
    rng = np.random.default_rng(600 + N)
    return dict(g=g, rs=rng.choice(np.array([1.0, 4.0, 16.0], F32), N), w=rng.integers(1, 3, g["E"]).astype(F32), dA=ints(rng, g["E"]))


NORM_UNIT = 2.0 ** -11          # a in {1, 1/2, 1/4}: g a in 1/4 units, drs = -da a / (2 rs) in 1/4 * 1/8 * 1/16 = 2^-9 units; 2^-11 leaves room


def norm_bwd_exact(c, da0=None):
    g = c["g"]
    i, j = g["erow"], g["col"].astype(np.int64)
    a = 1.0 / np.sqrt(c["rs"].astype(np.float64))
    gg = c["dA"].astype(np.float64) * c["w"].astype(np.float64)
    da = np.zeros(g["N"]) if da0 is None else da0.astype(np.float64)
    ab = np.abs(da)
    np.add.at(da, i, gg * a[j])
    np.add.at(da, j, gg * a[i])
    np.add.at(ab, i, np.abs(gg) * a[j])
    np.add.at(ab, j, np.abs(gg) * a[i])
    drs = -0.5 * da * a / c["rs"].astype(np.float64)
    dw = c["dA"].astype(np.float64) * a[i] * a[j] + drs[i]
    units = [v / NORM_UNIT for v in (da, drs, dw, gg * a[j], gg * a[i])]
    ok = set(np.unique(c["rs"])) <= {1.0, 4.0, 16.0} and all(np.array_equal(u, np.round(u)) for u in units)
    worst = max(ab.max() / NORM_UNIT, (np.abs(drs).max() + 3.0) / NORM_UNIT)
    return da, dw, ok and worst < EXACT_LIMIT


@functools.lru_cache(maxsize=None)
def pair_mask(N, p):
    from test_hip_parity import _np_pair_keep
    return _np_pair_keep(MDS_SEED[0], MDS_SEED[1], N, float(F32(p)))          # the library takes p as a float32: threshold (uint32)(p 2^24)


def mds_case(N, F):
    return ints(np.random.default_rng(700 + 131 * N + F), (N, F))


def test_exactness_premises_hold_for_every_case():
    for F, N in SPMM_BWD:
        c = spmm_bwd_case(F, N)
        dA, dX, ok = spmm_bwd_exact(c)
        assert ok and np.array_equal(dA.astype(F32), dA) and np.array_equal(dX.astype(F32), dX), F
        assert N == 1 or ((c["a"] == 0).any() and (c["dX0"] != 0).any())
    for N in SIZES:
        c = norm_bwd_case(N)
        da, dw, ok = norm_bwd_exact(c)
        assert ok and np.array_equal(da.astype(F32), da) and np.array_equal(dw.astype(F32), dw), N
    for N in MDS_N:
        for F in MDS_F:
            X = mds_case(N, F)
            assert np.array_equal(X, np.round(X)) and np.abs(X).sum(0).max() < EXACT_LIMIT
    # ... and the checks do fail outside the exact range
    c = dict(spmm_bwd_case(64, N0 + 2))
    c["dY"] = c["dY"] * F32(1 << 20)
    assert not spmm_bwd_exact(c)[2]
    c = dict(norm_bwd_case(N0))
    c["rs"] = np.where(c["rs"] == 4.0, F32(3.0), c["rs"])
    assert not norm_bwd_exact(c)[2]
    # the float32 threshold of the pair mask: p = 0.3 rounds UP in float32, so the double product would be one too small
    assert int(float(F32(0.3)) * 16777216.0) == 5033165 and int(0.3 * 16777216.0) == 5033164
    M = pair_mask(130, 0.3)
    assert M.shape == (130, 130) and abs(M.mean() - 0.7) < 0.02 and pair_mask(9, 0.0).all() and not np.array_equal(M, M.T)


# ---------------------------------------------------------------------------------------------------------------
# tier 2: float64 / float32 restatements
# ---------------------------------------------------------------------------------------------------------------
def seg_sum(keys, terms, n, init=None):
    """out[key] = init[key] + the terms of that key, added ONE BY ONE in the order given, in the dtype of `terms`"""
    order = np.argsort(keys, kind="stable")
    ks, t = keys[order], terms[order]
    cnt = np.bincount(ks, minlength=n)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    out = np.zeros((n,) + t.shape[1:], t.dtype) if init is None else init.astype(t.dtype).copy()
    for q in range(int(cnt.max()) if len(ks) else 0):
        nodes = np.flatnonzero(cnt > q)
        out[nodes] = out[nodes] + t[starts[nodes] + q]
    return out


def orders(E, seed):
    return [np.arange(E), np.random.default_rng(seed + E).permutation(E)]


def tanh_of(T, d32):
    return tanh32(d32) if T == np.float32 else np.tanh(d32.astype(np.float64))


def restate_rank_ramp_bwd(T, g, p, S, k, pos, gr, w, b, perm):
    i = g["erow"]
    th = tanh_of(T, pos.astype(F32) - k[i])
    term = gr.astype(T) * p.astype(T) * T(0.5) * (T(1) - th * th)
    dk = seg_sum(i[perm], term[perm], g["N"])
    z = S.astype(T) * T(F32(w)) + T(F32(b))
    dz = np.where(z > 0, dk, T(LEAKY) * dk)
    f = T(1) - T(0.5) * (T(1) + th) + T(1)
    return gr.astype(T) * f + dz[i] * T(F32(w)), dz


def restate_softk_bwd(T, g, p, pp, k, pos, gr, perturb, mode, perm):
    i = g["erow"]
    th = tanh_of(T, pos.astype(F32) - k[i])
    f, dfdk = T(1) - T(0.5) * (T(1) + th), T(0.5) * (T(1) - th * th)
    gr, pp = gr.astype(T), pp.astype(T)
    if mode == 0:
        dpp, term = gr * f, gr * pp * dfdk
    else:
        dpp, term = np.zeros_like(gr), gr * dfdk
    dp = dpp * pp / (p.astype(T) + T(EPS)) if perturb else dpp
    return dp, seg_sum(i[perm], term[perm], g["N"])


def restate_uvdist_bwd(T, g, xp, p, dp, dxp0, perm):
    i, j = g["erow"], g["col"].astype(np.int64)
    x = xp.astype(T)
    d = x[i] - x[j]
    d2 = (d * d).sum(1, dtype=T)
    gg = dp.astype(T) * p.astype(T) * T(F32(T_DIST))
    ok = (gg != 0) & (d2 > 0)
    coef = np.where(ok, gg / np.sqrt(np.where(ok, d2, T(1))), T(0))
    v = (coef[:, None] * d)[perm]
    both, keys = np.empty((2 * len(perm), x.shape[1]), T), np.empty(2 * len(perm), np.int64)
    both[0::2], both[1::2], keys[0::2], keys[1::2] = v, -v, i[perm], j[perm]
    return seg_sum(keys, both, g["N"], dxp0)


def restate_spmm_bwd(T, g, a, X, dY, dX0, perm):
    i, j = g["erow"], g["col"].astype(np.int64)
    fperm = np.arange(X.shape[1]) if np.array_equal(perm, np.arange(len(perm))) else np.random.default_rng(3).permutation(X.shape[1])
    prod = dY.astype(T)[i][:, fperm] * X.astype(T)[j][:, fperm]
    dA = np.zeros(g["E"], T)
    for c in range(prod.shape[1]):
        dA = dA + prod[:, c]
    dX = seg_sum(j[perm], (a.astype(T)[:, None] * dY.astype(T)[i])[perm], g["N"], dX0)
    return dA, dX


def restate_norm_bwd(T, g, w, rs, dA, perm):
    i, j = g["erow"], g["col"].astype(np.int64)
    rs = rs.astype(T)
    a = T(1) / np.sqrt(rs)
    gg = dA.astype(T) * w.astype(T)
    both, keys = np.empty(2 * len(perm), T), np.empty(2 * len(perm), np.int64)
    both[0::2], both[1::2], keys[0::2], keys[1::2] = (gg * a[j])[perm], (gg * a[i])[perm], i[perm], j[perm]
    da = seg_sum(keys, both, g["N"])
    drs = T(-0.5) * da * a / rs
    return dA.astype(T) * a[i] * a[j] + drs[i]


def fast_exp(T, x):
    """float64: exp.  float32: what bounds __expf -- a float32 product with log2 e, then exp2 (not a correctly rounded exp)"""
    if T == np.float64:
        return np.exp(x)
    return np.exp2((x.astype(F32) * LOG2E).astype(F32)).astype(F32)


def restate_bg_softmax_fwd(T, g, L, perm):
    i, N = g["erow"], g["N"]
    nbg = (N - np.diff(g["rowptr"])).astype(T)
    m = np.where(nbg > 0, T(0), T(-np.inf))
    np.maximum.at(m, i, L.astype(T))
    ex = fast_exp(T, L.astype(T) - m[i])
    z = seg_sum(i[perm], ex[perm], N)
    eb = np.where(nbg > 0, fast_exp(T, -m), T(0)).astype(T)
    z = z + nbg * eb
    iz = T(1) / z
    return (ex * iz[i]).astype(T), (eb * iz).astype(T)


def restate_bg_softmax_bwd(T, g, att, bg, datt, dbg, perm):
    i = g["erow"]
    s = seg_sum(i[perm], (att.astype(T) * datt.astype(T))[perm], g["N"]) + bg.astype(T) * dbg.astype(T)
    return att.astype(T) * (datt.astype(T) - s[i])


def identity_error(g, att, bg):
    """max_i |sum att + (N - cnt) bg - 1|, the sums taken in float64 from the values given"""
    s = np.zeros(g["N"])
    np.add.at(s, g["erow"], att.astype(np.float64))
    return float(np.abs(s + (g["N"] - np.diff(g["rowptr"])) * bg.astype(np.float64) - 1.0).max())


def bg_logits(g):
    rng = np.random.default_rng(800 + g["N"])
    L = (3.0 * rng.standard_normal(g["E"])).astype(F32)
    if g["N"] > 1:
        a, b = seg(g, 127)
        L[a:b] = -np.abs(L[a:b]) - F32(0.5)                            # all negative: the background is the maximum
        a, b = seg(g, 128)
        L[a + 70] = F32(60.0)                                          # an outlier
    return L


def tier2_inputs(g, h=16, seed=0):
    """everything the tier-2 kernels read, with the forward side taken from the oracle (bit-exact side)"""
    from oracle import oracle as O
    rng = np.random.default_rng(900 + g["N"] + h + seed)
    N, E = g["N"], g["E"]
    p = rank_values(g, seed=1)
    w_, b_ = 0.4, -0.3
    _, S, k, pos = O.csr_rank_ramp(p, g["rowptr"], g["col"], w_, b_)
    xp = (0.6 * rng.standard_normal((N, h))).astype(F32)
    twins = None
    if N > 1:
        a, _ = seg(g, 2)                                               # the 2-long row: make its first neighbour its twin
        r, j = g["named"][2], int(g["col"][a])
        if j != r:
            xp[j] = xp[r]
            twins = (r, j)
    pe = O.csr_uvdist(xp, g["rowptr"], g["col"], T_DIST)
    dp = rng.standard_normal(E).astype(F32)
    dp[rng.integers(0, E, 5)] = 0.0
    return dict(p=p, S=S, k=k, pos=pos, w=w_, b=b_, gr=rng.standard_normal(E).astype(F32), xp=xp, pe=pe, dp=dp, twins=twins,
                dxp0=rng.standard_normal((N, h)).astype(F32))


def figures(name, gpu, ref, cpus):
    """one row of the measured table; gpu may be None (CPU run)"""
    row = dict(out=name, cpu_row=rel_max(cpus[0], ref), cpu_shuf=rel_max(cpus[1], ref))
    row["bar"] = 4 * max(row["cpu_row"], row["cpu_shuf"])
    if gpu is not None:
        row["gpu"] = rel_max(gpu, ref)
    return row


def test_float64_restatements_match_the_oracle():
    """each float64 restatement against the float32 oracle function (which accumulates in double but takes tanh / the distance terms in
    float32 and rounds its results: 64 * 2^-24 of max bounds the difference), bg_softmax against a dense softmax, softk_bwd against
    torch autograd in float64; the float32 restatements stay within 1e-4 in both orders"""
    import torch
    from oracle import oracle as O
    tol = 64 * 2.0 ** -24
    g = build_graph(N0 + 1, False)
    x = tier2_inputs(g)
    E, N = g["E"], g["N"]
    o = orders(E, 1)
    dp_o, dkz_o = O.csr_rank_ramp_bwd(x["p"], g["rowptr"], x["w"], x["b"], x["S"], x["k"], x["pos"], x["gr"])
    dp, dkz = restate_rank_ramp_bwd(np.float64, g, x["p"], x["S"], x["k"], x["pos"], x["gr"], x["w"], x["b"], o[0])
    assert rel_max(dp_o, dp) < tol and rel_max(dkz_o, dkz) < tol
    for perm in o:
        a, b = restate_rank_ramp_bwd(np.float32, g, x["p"], x["S"], x["k"], x["pos"], x["gr"], x["w"], x["b"], perm)
        assert a.dtype == np.float32 and rel_max(a, dp) < 1e-4 and rel_max(b, dkz) < 1e-4
    zero = np.zeros_like(x["xp"])
    dxp_o = O.csr_uvdist_bwd(x["xp"], g["rowptr"], g["col"], x["pe"], x["dp"], T_DIST)
    dxp = restate_uvdist_bwd(np.float64, g, x["xp"], x["pe"], x["dp"], zero, o[0])
    assert rel_max(dxp_o, dxp) < tol
    for perm in o:
        assert rel_max(restate_uvdist_bwd(np.float32, g, x["xp"], x["pe"], x["dp"], zero, perm), dxp) < 1e-4
    rng = np.random.default_rng(2)
    F = 65
    a_, X, dY = (rng.standard_normal(s).astype(F32) for s in (E, (N, F), (N, F)))
    dA_o, dX_o = O.csr_spmm_bwd(g["rowptr"], g["col"], a_, X, dY)
    dA, dX = restate_spmm_bwd(np.float64, g, a_, X, dY, np.zeros((N, F), F32), o[0])
    assert rel_max(dA_o, dA) < tol and rel_max(dX_o, dX) < tol
    for perm in o:
        u, v = restate_spmm_bwd(np.float32, g, a_, X, dY, np.zeros((N, F), F32), perm)
        assert rel_max(u, dA) < 1e-4 and rel_max(v, dX) < 1e-4
    w_ = (0.1 + rng.random(E)).astype(F32)
    rs = (1.0 + 10 * rng.random(N)).astype(F32)
    dw_o = O.csr_norm_bwd(g["rowptr"], g["col"], w_, rs, dA_o)
    dw = restate_norm_bwd(np.float64, g, w_, rs, dA_o, o[0])
    assert rel_max(dw_o, dw) < tol
    for perm in o:
        assert rel_max(restate_norm_bwd(np.float32, g, w_, rs, dA_o, perm), dw) < 1e-4
    # bg_softmax: the dense [N,N] softmax the reference takes, logit 0 on every non-listed pair
    gf = build_graph(N0 + 1, True)
    L = bg_logits(gf)
    of = orders(gf["E"], 1)
    att, bg = restate_bg_softmax_fwd(np.float64, gf, L, of[0])
    D = torch.zeros(N, N, dtype=torch.float64)
    ii, jj = torch.from_numpy(gf["erow"]), torch.from_numpy(gf["col"].astype(np.int64))
    D[ii, jj] = torch.from_numpy(L.astype(np.float64))
    D.requires_grad_(True)
    sm = torch.softmax(D, 1)
    listed = torch.zeros(N, N, dtype=torch.bool)
    listed[ii, jj] = True
    assert np.abs(sm[ii, jj].detach().numpy() - att).max() < 1e-14
    full, empty = gf["named"]["all"], gf["named"][0]
    other = np.flatnonzero(~listed[:, 0].numpy())
    assert bg[full] == 0.0 and bg[empty] == 1.0 / N and abs(float(sm.detach()[other[0], 0]) - bg[other[0]]) < 1e-15 and identity_error(gf, att, bg) < 1e-14
    datt, dbg = rng.standard_normal(gf["E"]), rng.standard_normal(N)
    cot = torch.zeros(N, N, dtype=torch.float64)
    cot[ii, jj] = torch.from_numpy(datt)
    nb = (~listed).sum(1).clamp(min=1).double()
    cot = torch.where(listed, cot, (torch.from_numpy(dbg) / nb)[:, None].expand(N, N))          # bg_i = mean of the row's non-listed weights
    (sm * cot).sum().backward()
    dL = restate_bg_softmax_bwd(np.float64, gf, att, bg, datt, np.where(np.diff(gf["rowptr"]) < N, dbg, 0.0), of[0])
    assert np.abs(D.grad[ii, jj].numpy() - dL).max() < 1e-13
    for perm in of:
        a32, b32 = restate_bg_softmax_fwd(np.float32, gf, L, perm)
        assert a32.dtype == np.float32 and rel_max(a32, att) < 1e-4 and rel_max(b32, bg) < 1e-4 and b32[full] == 0.0 and b32[empty] == F32(1) / F32(N)
    # softk_bwd: autograd of w = pp * ramp(pos - k), pp = exp(log(p + 1e-8) + noise), in float64 (k on a 1/8 grid: pos - k exact)
    ps = rank_values(g, seed=2)
    k8 = (np.round(8 * rng.random(N) * 30) / 8).astype(F32)
    nz = torch.from_numpy(0.3 * rng.gumbel(size=E))
    pt = torch.from_numpy(ps.astype(np.float64)).requires_grad_(True)
    kt = torch.from_numpy(k8.astype(np.float64)).requires_grad_(True)
    ppt = torch.exp(torch.log(pt + float(EPS)) + nz)
    pos = positions_by_sort(g, ppt.detach().numpy())
    ramp = 1 - 0.5 * (1 + torch.tanh(torch.from_numpy(pos.astype(np.float64)) - kt[torch.from_numpy(g["erow"])]))
    gr = rng.standard_normal(E)
    for mode in (0, 1):
        pt.grad = kt.grad = None
        (((ppt * ramp) if mode == 0 else ramp) * torch.from_numpy(gr)).sum().backward(retain_graph=True)
        dp, dk = restate_softk_bwd(np.float64, g, ps, ppt.detach().numpy(), k8, pos, gr, 1, mode, o[0])
        gp = np.zeros(E) if pt.grad is None else pt.grad.numpy()
        assert np.abs(gp - dp).max() <= 1e-12 * max(np.abs(gp).max(), 1.0) and np.abs(kt.grad.numpy() - dk).max() < 1e-12 * np.abs(dk).max()
    # seg_sum is a sequential sum in the order given, on top of `init`
    keys, terms = np.array([2, 0, 2, 2, 0]), np.array([1e8, 1.0, 1.0, -1e8, 2.0], F32)
    assert np.array_equal(seg_sum(keys, terms, 3), np.array([3.0, 0.0, 0.0], F32))
    assert np.array_equal(seg_sum(keys[[0, 3, 2, 1, 4]], terms[[0, 3, 2, 1, 4]], 3, np.array([1, 1, 1], F32)), np.array([4.0, 1.0, 1.0], F32))
    assert np.array_equal(fast_exp(np.float32, np.array([0.0, 1.0], F32)), np.array([1.0, np.exp2(LOG2E)], F32))


# ---------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


class Ctx:
    """uploads between guards and calls through the C ABI"""

    def __init__(self, dev):
        self.dev, self.ins, self.outs = dev, [], []

    def inp(self, a):
        a = np.asarray(a)
        gd = Guard(self.dev, a, np.nan if a.dtype.kind == "f" else a.dtype.type(-1))
        self.ins.append((gd, a.copy()))
        return gd

    def out(self, shape, dtype=np.float32, start=None):
        """an output: NaN-filled (int32: -7777), or holding `start`, between canary words"""
        if start is None:
            start = nans(shape) if dtype == np.float32 else np.full(shape, IFILL, np.int32)
        gd = Guard(self.dev, start, CANARY if dtype == np.float32 else ICANARY)
        self.outs.append(gd)
        return gd

    def graph(self, g):
        return self.inp(g["rowptr"]), self.inp(g["col"])

    def call(self, name, *args):
        import torch
        from dgg_amd import _lib, ops
        a = [x.addr if isinstance(x, Guard) else x for x in args]
        rc = getattr(_lib.lib(), name)(*a, ops._stream())
        torch.cuda.synchronize()
        return rc

    def inputs_intact(self):
        for gd, a in self.ins:
            assert np.array_equal(gd.read("an input"), a, equal_nan=True), "an input was written"


def untouched(gd):
    h = gd.read("an output")
    return bool(np.isnan(h).all()) if h.dtype == np.float32 else bool((h == IFILL).all())


def same(got, exp):
    """bit for bit (NaN only where the reference has NaN)"""
    exp = np.asarray(exp).astype(got.dtype)
    return got.shape == exp.shape and np.array_equal(got, exp, equal_nan=got.dtype.kind == "f")


def describe(name, got, exp):
    exp = np.asarray(exp).astype(got.dtype)
    bad = np.flatnonzero(~((got == exp) | ((got != got) & (exp != exp))).ravel())
    return "%s differs in %d of %d elements, first at flat index %d: got %r, expected %r" % (name, len(bad), got.size, bad[0], got.ravel()[bad[0]],
                                                                                            exp.ravel()[bad[0]])


def expect(bad, name, gd, exp):
    got = gd.read(name)
    if not same(got, exp):
        bad.append(describe(name, got, exp))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_sum_normalize_spmm_forwards_equal_the_oracle(dev, N):
    from oracle import oracle as O
    g = build_graph(N, False)
    c, bad = Ctx(dev), []
    rp, cl = c.graph(g)
    rng = np.random.default_rng(N)
    w = rank_values(g, zeros=False)
    if N > 1:
        w[seg(g, 1)[0]] = 0.0                                          # the zero-sum row (nobody lists its node)
    gw, rs = c.inp(w), c.out(N)
    assert c.call("dgg_csr_row_sum", gw, rp, N, rs) == 0
    rs_h = expect(bad, "row_sum", rs, O.csr_row_sum(w, g["rowptr"]))
    assert N == 1 or (rs_h[g["unlisted"]] == 0).all() and (rs_h[np.unique(g["col"])] > 0).all()
    grs, ahat = c.inp(rs_h), c.out(g["E"], start=np.full(g["E"], 7.0, F32))
    assert c.call("dgg_csr_normalize_fwd", rp, cl, gw, grs, N, ahat) == 0
    with np.errstate(all="ignore"):
        ah_o = O.csr_normalize(g["rowptr"], g["col"], w, rs_h)
    ah = expect(bad, "normalize_fwd", ahat, ah_o)
    assert int(np.isnan(ah_o).sum()) == (1 if N > 1 else 0) and not (ah == 7.0).any()
    a = rng.standard_normal(g["E"]).astype(F32)
    ga = c.inp(a)
    for F in SPMM_F:
        X = rng.standard_normal((N, F)).astype(F32)
        Y = c.out((N, F))
        assert c.call("dgg_csr_spmm_fwd", rp, cl, ga, c.inp(X), N, F, Y) == 0
        expect(bad, "spmm_fwd F=%d" % F, Y, O.csr_spmm(g["rowptr"], g["col"], a, X))
    c.inputs_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_ranking_and_scoring_forwards_equal_the_oracle(dev, N):
    from oracle import oracle as O
    g = build_graph(N, True)
    c, bad = Ctx(dev), []
    rp, cl = c.graph(g)
    rng = np.random.default_rng(N + 50)
    E = g["E"]
    p = rank_values(g)
    gp = c.inp(p)
    wb, bb = np.array([0.4], F32), np.array([-0.3], F32)
    out, S, k, pos = c.out(E), c.out(N), c.out(N), c.out(E, np.int32)
    assert c.call("dgg_csr_rank_ramp_fwd", gp, rp, cl, N, c.inp(wb), c.inp(bb), out, S, k, pos) == 0
    for nm, gd, ref in zip(("out", "S", "k", "pos"), (out, S, k, pos), O.csr_rank_ramp(p, g["rowptr"], g["col"], wb[0], bb[0])):
        expect(bad, "rank_ramp_fwd " + nm, gd, ref)
    for kcut in KCUTS:
        out, pos = c.out(E), c.out(E, np.int32)
        assert c.call("dgg_csr_rank_cut_fwd", gp, rp, cl, N, kcut, out, pos) == 0
        ro, rpos = O.csr_rank_cut(p, g["rowptr"], g["col"], kcut)
        expect(bad, "rank_cut_fwd kcut=%d out" % kcut, out, ro)
        expect(bad, "rank_cut_fwd kcut=%d pos" % kcut, pos, rpos)
    noise = (2 * rng.random(E) - 1).astype(F32)
    out = c.out(E)
    assert c.call("dgg_csr_noisy_sigmoid_fwd", gp, c.inp(noise), E, out) == 0
    expect(bad, "noisy_sigmoid_fwd", out, O.csr_noisy_sigmoid(p, noise))
    for h in UV_H:
        xp = (0.6 * rng.standard_normal((N, h))).astype(F32)
        pe = c.out(E)
        assert c.call("dgg_csr_uvdist_fwd", c.inp(xp), rp, cl, N, h, T_DIST, pe) == 0
        expect(bad, "uvdist_fwd h=%d" % h, pe, O.csr_uvdist(xp, g["rowptr"], g["col"], T_DIST))
    c.inputs_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("noise_mode,mode,N", SOFTK_CASES, ids=["noise%d-mode%d-N%d" % t for t in SOFTK_CASES])
def test_softk_forward_equals_the_composed_reference(dev, noise_mode, mode, N):
    g = build_graph(N, True)
    p, k, Gm = softk_inputs(g, noise_mode)
    assert (p == 0).any() or N == 1
    c, bad = Ctx(dev), []
    rp, cl = c.graph(g)
    w, pp, pos = c.out(g["E"]), c.out(g["E"]), c.out(g["E"], np.int32)
    gG = c.inp(Gm) if Gm is not None else None
    rc = c.call("dgg_csr_softk_fwd", c.inp(p), rp, cl, N, c.inp(k), noise_mode, gG, N + 3 if Gm is not None else 0, SOFTK_SEED[0], SOFTK_SEED[1], mode,
                w, pp, pos)
    assert rc == 0
    for nm, gd, ref in zip(("w", "pp", "pos"), (w, pp, pos), softk_reference(g, p, k, noise_mode, Gm, SOFTK_SEED, mode)):
        expect(bad, "softk_fwd " + nm, gd, ref)
    c.inputs_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("F,N", SPMM_BWD)
def test_spmm_backward_is_the_integer_reference_bit_for_bit(dev, F, N):
    x = spmm_bwd_case(F, N)
    g = x["g"]
    dA_e, dX_e, ok = spmm_bwd_exact(x)
    assert ok
    c, bad = Ctx(dev), []
    rp, cl = c.graph(g)
    ga, gX, gdY = c.inp(x["a"]), c.inp(x["X"]), c.inp(x["dY"])
    dA, dX = c.out(g["E"]), c.out((N, F), start=x["dX0"])
    assert c.call("dgg_csr_spmm_bwd", rp, cl, ga, gX, gdY, N, F, dA, dX) == 0
    expect(bad, "dA", dA, dA_e)
    got = expect(bad, "dX (accumulated onto its start)", dX, dX_e)
    assert np.array_equal(got[g["unlisted"]], x["dX0"][g["unlisted"]])                     # rows of nodes nobody lists: unchanged
    dA2 = c.out(g["E"])
    assert c.call("dgg_csr_spmm_bwd", rp, cl, ga, gX, gdY, N, F, dA2, None) == 0
    expect(bad, "dA with dX = NULL", dA2, dA_e)
    # entries with a == 0 add nothing: with a = 0 everywhere dX keeps its start, NaN included
    start = x["dX0"].copy()
    start[g["hub"]] = np.nan
    dX3 = c.out((N, F), start=start)
    assert c.call("dgg_csr_spmm_bwd", rp, cl, c.inp(np.zeros(g["E"], F32)), gX, gdY, N, F, c.out(g["E"]), dX3) == 0
    expect(bad, "dX with a == 0", dX3, start)
    c.inputs_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_norm_backward_is_exact_on_powers_of_two(dev, N):
    x = norm_bwd_case(N)
    g = x["g"]
    da_e, dw_e, ok = norm_bwd_exact(x)
    assert ok
    c, bad = Ctx(dev), []
    rp, cl = c.graph(g)
    gw, grs, gdA = c.inp(x["w"]), c.inp(x["rs"]), c.inp(x["dA"])
    da, dw = c.out(N, start=np.zeros(N, F32)), c.out(g["E"])
    assert c.call("dgg_csr_norm_bwd", rp, cl, gw, grs, gdA, N, da, dw) == 0
    expect(bad, "da_ws", da, da_e)
    expect(bad, "dw", dw, dw_e)
    # da_ws is accumulated into and then READ: a non-zero start enters dw (hence `must be zero on entry`)
    da0 = np.zeros(N, F32)
    da0[g["hub"]] = 64.0
    da_s, dw_s, ok = norm_bwd_exact(x, da0)
    assert ok and not np.array_equal(dw_s, dw_e)
    da, dw = c.out(N, start=da0), c.out(g["E"])
    assert c.call("dgg_csr_norm_bwd", rp, cl, gw, grs, gdA, N, da, dw) == 0
    expect(bad, "da_ws from a non-zero start", da, da_s)
    expect(bad, "dw from a non-zero da_ws", dw, dw_s)
    c.inputs_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("N", MDS_N)
def test_masked_dense_sum_is_the_integer_mask_sum(dev, N):
    c, bad = Ctx(dev), []
    for p in MDS_P:
        M = pair_mask(N, p).astype(np.float64)
        for F in MDS_F:
            X = mds_case(N, F)
            gX = c.inp(X)
            for tr in (0, 1):
                out = c.out((N, F))
                assert c.call("dgg_masked_dense_sum", gX, N, F, C.c_float(p), MDS_SEED[0], MDS_SEED[1], tr, out) == 0
                expect(bad, "N=%d F=%d p=%g transpose=%d" % (N, F, p, tr), out, (M.T if tr else M) @ X.astype(np.float64))
        ii, jj = np.nonzero(np.ones((N, N), bool))
        keep = c.out(N * N)
        assert c.call("dgg_pair_keep", c.inp(ii.astype(np.int32)), c.inp(jj.astype(np.int32)), N * N, C.c_float(p), MDS_SEED[0], MDS_SEED[1], keep) == 0
        expect(bad, "pair_keep p=%g" % p, keep, M.ravel())
    c.inputs_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("E", ELEM_E)
def test_elementwise_backwards_at_block_edges(dev, E):
    rng = np.random.default_rng(E)
    c, bad = Ctx(dev), []
    pos = rng.integers(0, 9, E).astype(np.int32)
    gr = ints(rng, E)
    for kcut in (0, 4, 1000):
        dp = c.out(E)
        assert c.call("dgg_csr_rank_cut_bwd", c.inp(pos), c.inp(gr), E, kcut, dp) == 0
        expect(bad, "rank_cut_bwd kcut=%d" % kcut, dp, np.where(pos < kcut, gr, F32(0)))
    out = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], F32), E)          # out (1 - out) and its product with a small integer are exact
    dp = c.out(E)
    assert c.call("dgg_csr_noisy_sigmoid_bwd", c.inp(out), c.inp(gr), E, dp) == 0
    expect(bad, "noisy_sigmoid_bwd", dp, gr.astype(np.float64) * out * (1.0 - out))
    c.inputs_intact()
    assert not bad, "\n".join(bad)


REFUSALS = {
    "softk-noise-4": ERR_ARG, "softk-noise-negative": ERR_ARG, "softk-explicit-without-G": ERR_ARG, "softk-mode-2": ERR_ARG,
    "rank_cut-kcut-negative": ERR_ARG, "uvdist-h-0": ERR_ARG, "masked-F-0": ERR_UNSUPPORTED, "masked-F-65": ERR_UNSUPPORTED,
    "masked-p-1": ERR_UNSUPPORTED, "masked-p-negative": ERR_UNSUPPORTED, "pair_keep-p-1": ERR_ARG,
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_return_their_code_and_write_nothing(dev, name):
    from dgg_amd import _lib
    g = build_graph(N0, True)
    N, E = g["N"], g["E"]
    c = Ctx(dev)
    rp, cl = c.graph(g)
    p, k, Gm = softk_inputs(g, 1)
    gp, gk = c.inp(p), c.inp(k)
    if name.startswith("softk"):
        nm, G, mode = {"softk-noise-4": (4, c.inp(Gm), 0), "softk-noise-negative": (-1, c.inp(Gm), 0), "softk-explicit-without-G": (1, None, 0),
                       "softk-mode-2": (0, None, 2)}[name]
        rc = c.call("dgg_csr_softk_fwd", gp, rp, cl, N, gk, nm, G, N + 3, 1, 2, mode, c.out(E), c.out(E), c.out(E, np.int32))
    elif name == "rank_cut-kcut-negative":
        rc = c.call("dgg_csr_rank_cut_fwd", gp, rp, cl, N, -1, c.out(E), c.out(E, np.int32))
    elif name == "uvdist-h-0":
        rc = c.call("dgg_csr_uvdist_fwd", c.inp(np.zeros((N, 4), F32)), rp, cl, N, 0, T_DIST, c.out(E))
    elif name.startswith("masked"):
        F, pd = {"masked-F-0": (0, 0.3), "masked-F-65": (65, 0.3), "masked-p-1": (8, 1.0), "masked-p-negative": (8, -0.1)}[name]
        rc = c.call("dgg_masked_dense_sum", c.inp(np.zeros((N, 65), F32)), N, F, C.c_float(pd), 1, 2, 0, c.out((N, 65)))
    else:
        rc = c.call("dgg_pair_keep", c.inp(g["erow"].astype(np.int32)), cl, E, C.c_float(1.0), 1, 2, c.out(E))
    assert rc == REFUSALS[name] and _lib.lib().dgg_last_error().decode() != ""
    assert all(untouched(o) for o in c.outs)
    c.inputs_intact()


@pytest.mark.gpu
def test_empty_graphs_return_zero_and_write_nothing(dev):
    """N == 0 (rowptr = [0]) for the row kernels, E == 0 for the elementwise ones"""
    c = Ctx(dev)
    rp, cl, f, one = c.inp(np.zeros(1, np.int64)), c.inp(np.zeros(4, np.int32)), c.inp(np.ones(8, F32)), c.inp(np.ones(1, F32))
    o, oi = (lambda: c.out(8)), (lambda: c.out(8, np.int32))
    calls = [("dgg_csr_row_sum", f, rp, 0, o()), ("dgg_csr_normalize_fwd", rp, cl, f, f, 0, o()), ("dgg_csr_spmm_fwd", rp, cl, f, f, 0, 4, o()),
             ("dgg_csr_spmm_bwd", rp, cl, f, f, f, 0, 4, o(), o()), ("dgg_csr_norm_bwd", rp, cl, f, f, f, 0, o(), o()),
             ("dgg_csr_rank_ramp_fwd", f, rp, cl, 0, one, one, o(), o(), o(), oi()), ("dgg_csr_rank_ramp_bwd", f, rp, 0, one, one, f, f, cl, f, o(), o()),
             ("dgg_csr_softk_fwd", f, rp, cl, 0, f, 2, None, 0, 1, 2, 0, o(), o(), oi()), ("dgg_csr_softk_bwd", f, f, rp, 0, f, cl, 1, 0, f, o(), o()),
             ("dgg_csr_rank_cut_fwd", f, rp, cl, 0, 3, o(), oi()), ("dgg_csr_uvdist_fwd", f, rp, cl, 0, 4, T_DIST, o()),
             ("dgg_csr_uvdist_bwd", f, rp, cl, 0, 4, T_DIST, f, f, o()), ("dgg_csr_bg_softmax_fwd", f, rp, 0, o(), o()),
             ("dgg_csr_bg_softmax_bwd", f, f, rp, 0, f, f, o()), ("dgg_masked_dense_sum", f, 0, 4, C.c_float(0.3), 1, 2, 0, o()),
             ("dgg_csr_noisy_sigmoid_fwd", f, f, 0, o()), ("dgg_csr_noisy_sigmoid_bwd", f, f, 0, o()), ("dgg_csr_rank_cut_bwd", cl, f, 0, 3, o()),
             ("dgg_pair_keep", cl, cl, 0, C.c_float(0.3), 1, 2, o()), ("dgg_csr_spmm_fwd", rp, cl, f, f, 0, 0, o())]
    for call in calls:
        assert c.call(*call) == 0, call[0]
    assert all(untouched(gd) for gd in c.outs)
    c.inputs_intact()


# ---- tier 2 ---------------------------------------------------------------------------------------------------------
def hold(rows, bad):
    for r in rows:
        print("TIER2 " + json.dumps(r))
        if not r["gpu"] <= r["bar"]:
            bad.append("%s: %.3g of max against a bar of %.3g (4 x the float32 restatement on the CPU)" % (r["out"], r["gpu"], r["bar"]))


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_rank_ramp_backward_within_four_times_the_float32_restatement(dev, N):
    g = build_graph(N, True)
    x = tier2_inputs(g)
    c, bad = Ctx(dev), []
    rp, _ = c.graph(g)
    dp, dkz = c.out(g["E"]), c.out(N)
    rc = c.call("dgg_csr_rank_ramp_bwd", c.inp(x["p"]), rp, N, c.inp(np.array([x["w"]], F32)), c.inp(np.array([x["b"]], F32)), c.inp(x["S"]), c.inp(x["k"]),
                c.inp(x["pos"]), c.inp(x["gr"]), dp, dkz)
    assert rc == 0
    dp, dkz = dp.read("dp"), dkz.read("dkz")
    excluded = int((~np.isfinite(dp)).sum() + (~np.isfinite(dkz)).sum())
    assert excluded == 0, "%d elements were not written" % excluded
    args = (g, x["p"], x["S"], x["k"], x["pos"], x["gr"], x["w"], x["b"])
    o = orders(g["E"], N)
    ref = restate_rank_ramp_bwd(np.float64, *args, o[0])
    cpu = [restate_rank_ramp_bwd(np.float32, *args, perm) for perm in o]
    hold([figures("rank_ramp_bwd dp N=%d" % N, dp, ref[0], [q[0] for q in cpu]), figures("rank_ramp_bwd dkz N=%d" % N, dkz, ref[1], [q[1] for q in cpu])], bad)
    c.inputs_intact()
    assert not bad, "\n".join(bad)


SOFTK_BWD = [(perturb, mode, SIZES[(2 * perturb + mode) % 4]) for perturb in (0, 1) for mode in (0, 1)] + [(1, 0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("perturb,mode,N", SOFTK_BWD, ids=["perturb%d-mode%d-N%d" % t for t in SOFTK_BWD])
def test_softk_backward_within_four_times_the_float32_restatement(dev, perturb, mode, N):
    g = build_graph(N, True)
    nm = 2 if perturb else 0
    p, k, _ = softk_inputs(g, nm)
    _, pp, pos = softk_reference(g, p, k, nm, None, SOFTK_SEED, mode)              # the bit-exact side of the forward
    assert N == 1 or (p == 0).any()
    gr = np.random.default_rng(N + mode).standard_normal(g["E"]).astype(F32)
    c, bad = Ctx(dev), []
    rp, _ = c.graph(g)
    dp, dk = c.out(g["E"]), c.out(N)
    assert c.call("dgg_csr_softk_bwd", c.inp(p), c.inp(pp), rp, N, c.inp(k), c.inp(pos), perturb, mode, c.inp(gr), dp, dk) == 0
    dp, dk = dp.read("dp"), dk.read("dk")
    excluded = int((~np.isfinite(dp)).sum() + (~np.isfinite(dk)).sum())
    assert excluded == 0, "%d elements were not written" % excluded
    args = (g, p, pp, k, pos, gr, perturb, mode)
    o = orders(g["E"], N)
    ref = restate_softk_bwd(np.float64, *args, o[0])
    cpu = [restate_softk_bwd(np.float32, *args, perm) for perm in o]
    tag = "softk_bwd perturb=%d mode=%d N=%d " % (perturb, mode, N)
    if mode == 1:
        assert not dp.any() and not ref[0].any(), "k_only: dp is exactly zero"
    hold([figures(tag + "dp", dp, ref[0], [q[0] for q in cpu]), figures(tag + "dk", dk, ref[1], [q[1] for q in cpu])], bad)
    c.inputs_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("h,N", UV_BWD)
def test_uvdist_backward_within_four_times_the_float32_restatement(dev, h, N):
    g = build_graph(N, False)
    x = tier2_inputs(g, h)
    assert N == 1 or (x["twins"] is not None and (x["dp"] == 0).any())
    c, bad = Ctx(dev), []
    rp, cl = c.graph(g)
    dxp = c.out((N, h), start=x["dxp0"])
    assert c.call("dgg_csr_uvdist_bwd", c.inp(x["xp"]), rp, cl, N, h, T_DIST, c.inp(x["pe"]), c.inp(x["dp"]), dxp) == 0
    dxp = dxp.read("dxp")
    excluded = int((~np.isfinite(dxp)).sum())
    assert excluded == 0, "%d elements are not finite (a zero distance must contribute 0, never NaN)" % excluded
    if N > 1:
        lonely = g["named"][0]                                                # empty row, listed by nobody: touched by no entry
        assert np.array_equal(dxp[lonely], x["dxp0"][lonely])
    o = orders(g["E"], h)
    ref = restate_uvdist_bwd(np.float64, g, x["xp"], x["pe"], x["dp"], x["dxp0"], o[0])
    cpu = [restate_uvdist_bwd(np.float32, g, x["xp"], x["pe"], x["dp"], x["dxp0"], perm) for perm in o]
    hold([figures("uvdist_bwd dxp h=%d N=%d" % (h, N), dxp, ref, cpu)], bad)
    # zero distance contributes exactly 0: a graph of twins and self loops only leaves dxp as it was, bit for bit
    N2 = 6
    rowptr, col = np.array([0, 2, 3, 3, 5, 6, 6], np.int64), np.array([0, 1, 0, 3, 4, 3], np.int32)
    xt = np.tile(x["xp"][:1], (N2, 1))
    start = np.random.default_rng(h).standard_normal((N2, h)).astype(F32)
    dxp2 = c.out((N2, h), start=start)
    rc = c.call("dgg_csr_uvdist_bwd", c.inp(xt), c.inp(rowptr), c.inp(col), N2, h, T_DIST, c.inp(np.ones(6, F32)), c.inp(np.full(6, 2.0, F32)), dxp2)
    assert rc == 0
    expect(bad, "dxp of twins and self loops", dxp2, start)
    c.inputs_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("F", SPMM_F)
def test_spmm_and_norm_backward_on_normal_data(dev, F):
    N = SIZES[SPMM_F.index(F) % 4]
    g = build_graph(N, False)
    rng = np.random.default_rng(40 + F)
    E = g["E"]
    a, X, dY, dX0 = (rng.standard_normal(s).astype(F32) for s in (E, (N, F), (N, F), (N, F)))
    c, bad = Ctx(dev), []
    rp, cl = c.graph(g)
    dA, dX = c.out(E), c.out((N, F), start=dX0)
    assert c.call("dgg_csr_spmm_bwd", rp, cl, c.inp(a), c.inp(X), c.inp(dY), N, F, dA, dX) == 0
    dA, dX = dA.read("dA"), dX.read("dX")
    w, rs = (0.1 + rng.random(E)).astype(F32), (1.0 + 10 * rng.random(N)).astype(F32)
    gA = rng.standard_normal(E).astype(F32)
    da, dw = c.out(N, start=np.zeros(N, F32)), c.out(E)
    assert c.call("dgg_csr_norm_bwd", rp, cl, c.inp(w), c.inp(rs), c.inp(gA), N, da, dw) == 0
    dw = dw.read("dw")
    excluded = int(sum((~np.isfinite(v)).sum() for v in (dA, dX, dw)))
    assert excluded == 0, "%d elements were not written" % excluded
    o = orders(E, F)
    ref = restate_spmm_bwd(np.float64, g, a, X, dY, dX0, o[0])
    cpu = [restate_spmm_bwd(np.float32, g, a, X, dY, dX0, perm) for perm in o]
    rows = [figures("spmm_bwd dA F=%d N=%d" % (F, N), dA, ref[0], [q[0] for q in cpu]), figures("spmm_bwd dX F=%d N=%d" % (F, N), dX, ref[1], [q[1] for q in cpu])]
    rows.append(figures("norm_bwd dw N=%d" % N, dw, restate_norm_bwd(np.float64, g, w, rs, gA, o[0]), [restate_norm_bwd(np.float32, g, w, rs, gA, perm) for perm in o]))
    hold(rows, bad)
    c.inputs_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_bg_softmax_within_four_times_the_float32_restatement(dev, N):
    g = build_graph(N, True)
    E = g["E"]
    L = bg_logits(g)
    c, bad = Ctx(dev), []
    rp, _ = c.graph(g)
    att, bg = c.out(E), c.out(N)
    assert c.call("dgg_csr_bg_softmax_fwd", c.inp(L), rp, N, att, bg) == 0
    att, bg = att.read("att"), bg.read("bg")
    o = orders(E, N)
    ref = restate_bg_softmax_fwd(np.float64, g, L, o[0])
    cpu = [restate_bg_softmax_fwd(np.float32, g, L, perm) for perm in o]
    rows = [figures("bg_softmax_fwd att N=%d" % N, att, ref[0], [q[0] for q in cpu]), figures("bg_softmax_fwd bg N=%d" % N, bg, ref[1], [q[1] for q in cpu])]
    ident = dict(out="bg_softmax_fwd identity N=%d" % N, cpu_row=identity_error(g, *cpu[0]), cpu_shuf=identity_error(g, *cpu[1]), gpu=identity_error(g, att, bg))
    ident["bar"] = 4 * max(ident["cpu_row"], ident["cpu_shuf"])
    rows.append(ident)
    if N > 1:
        full, empty = g["named"]["all"], g["named"][0]
        assert bg[full] == 0.0, "a row without background entry has bg == 0 exactly"
        assert bg[empty] == F32(1) / F32(N), "a row without explicit entry has bg = 1/N"
    else:
        assert bg[0] == 0.0 and att[0] == 1.0
    # backward: att and bg of the forward side (the CPU's float32 restatement) feed both sides
    att_in, bg_in = cpu[0]
    rng = np.random.default_rng(N + 7)
    datt, dbg = rng.standard_normal(E).astype(F32), rng.standard_normal(N).astype(F32)
    dL = c.out(E)
    assert c.call("dgg_csr_bg_softmax_bwd", c.inp(att_in), c.inp(bg_in), rp, N, c.inp(datt), c.inp(dbg), dL) == 0
    dL = dL.read("dL")
    excluded = int(sum((~np.isfinite(v)).sum() for v in (att, bg, dL)))
    assert excluded == 0, "%d elements were not written" % excluded
    rows.append(figures("bg_softmax_bwd dL N=%d" % N, dL, restate_bg_softmax_bwd(np.float64, g, att_in, bg_in, datt, dbg, o[0]),
                        [restate_bg_softmax_bwd(np.float32, g, att_in, bg_in, datt, dbg, perm) for perm in o]))
    hold(rows, bad)
    c.inputs_intact()
    assert not bad, "\n".join(bad)
