"""The payload-partition backward of csrc/dgg_scatter.hip against exact and float64 references.

Every training step goes backward through dgg_ell_conv_bwd_partp[_ext] (dA, dA_rec, dH, da of Z = A H), dgg_partp_gather_rec and
dgg_softk_edge_bwd_partp_phase (ramp + normalisation + score backward) -- and their *_chunked forms.  This module calls them through
the C ABI on graphs whose destination IN-DEGREES are prescribed (build_block): in one block a hub that every row selects, nodes with
0, 1, PER-1, PER, PER+1, 127, 128, 129 and 4 PER + 1 records (PER = records per iteration of the walk: 4 * 64 / (F / 4) for the conv
walk, 32 for the score walk; 128 = NODE_LONG), both kinds of inactive entry (idx = -1, w = 0), an entirely inactive row, a self loop
and nodes without a record inside and outside the row range.  In-degrees a block has too few rows for are left out (`grouped`: 100 rows).

Shapes (dispatch of the library itself; K = 64):
  wave     ncols = rows = 700, row0 = 0        wavefront per node, long nodes (> 128 records) in appended workgroups, hub of 699
  shard    ncols = 1100, rows [300, 811)       the same with row0 != 0: dxp rows inside and outside the shard
  grouped  ncols = 700, rows [250, 350)        rows K < 16 ncols: lane group per node (conv_bwd_nodeg / edge_bwd_nodeg); dA_ext
                                               forces conv_bwd_node<F, true>
  unsplit  ncols = 66 000, rows [20 000, 37 000)   ncols > 65536: no appended workgroups, ONE wavefront walks the hub (tier 1 only)
  chunked  300 nodes, degrees up to 130        dgg_partp_build_chunked + *_chunked (the `wide` addressing), long nodes split
The forcing knobs (DGG_NODE_SPLIT, DGG_NODE_GROUPS, DGG_DA_MAP, DGG_PP_THREADS, DGG_PP_WIDTH) are read once per process: one fresh
child process per value runs KNOB_CONV + KNOB_SCORE under it.

Tier 1 (conv backward, bit for bit).  w in {1, 2}, rs in {1, 4}, G / H / dA_ext integers of magnitude <= 2: a_i = rs_i^-1/2, the record
payload w a_i, ahat = w a_i a_j and sqrt(rs_j) are powers of two, every product is exact and every partial sum in ANY order is a
multiple of 1/4 below 2^24 / 4 (test_exactness_premises_hold_for_every_case proves it per case) -- so the wavefront, long-node,
lane-group and EXT kernels must all return exactly  dA_ir = <G_i, H_j> (+ dA_ext_ir),  dH_j = sum ahat_ir G_i,  da_j = sum dA_ir w_ir a_i.
dH, da, dA and dA_rec are handed in filled with NaN between canary words, inputs sit between NaN guards: every element of dH / da comes
back exact (nodes without a record: 0), dA is exact on the active slots and still NaN elsewhere, dA_rec is dA in record order and
untouched beyond the record count.  dA = NULL, phase-1-then-sort builds and partp_gather give the same bits.

Tier 2 (score backward, float64).  Reference: restate(np.float64, ...) below = ora_softk_norm_bwd followed by ora_edge_bwd
(oracle/dgg_oracle.c; validated against them on the CPU), with the LeakyReLU' mask and the normalized = 0 form.  xp = 0.6 N(0, 1), scores
= ora_pair_score of the prescribed pairs, k in [3, 40], row sums from ora_softk (nodes outside the block: stand-ins in [2, 20]); dA,
dA_rec, da and ahat come from the GPU's own conv call on standard-normal G, H and are INPUTS of both sides.  Statistic:
max|got - ref| / max|ref| for dxp and dk.  Bar: 4 x the larger error of the same arithmetic in float32 on the CPU (restate(np.float32)
with ora_tanh / ora_exp) in two summation orders -- row order and a seeded shuffle of the entries; 4 x is the margin
test_weight_gradients.py established for a reordered fp32 sum.

Measured on an MI355X (err / max|ref|; `branch`: node kernel the dispatch took -- W wavefront per node, L + long-node workgroups,
G lane group per node, C chunked; M = dA also read through the slot -> record map):

  case                       branch  hub | dxp CPUrow   CPUshuf    bar=4x    MI355X | dk CPUrow   CPUshuf    bar=4x    MI355X
  wave-h16-m0-p1-n1-a0       W+L+M   699 |  4.33e-07  3.21e-07  1.73e-06  1.97e-07 |  1.66e-07  1.93e-07  7.72e-07  1.77e-07
  shard-h32-m0-p1-n1-a0      W+L+M   510 |  2.24e-07  2.54e-07  1.01e-06  2.43e-07 |  1.11e-06  1.11e-06  4.43e-06  1.11e-06
  wave-h32-m0-p1-n1-a1       W+L+M   699 |  7.86e-07  2.46e-07  3.14e-06  1.81e-07 |  3.01e-07  2.29e-07  1.20e-06  3.01e-07
  grouped-h16-m0-p1-n1-a1    G+M      99 |  2.55e-07  3.56e-07  1.42e-06  2.87e-07 |  1.56e-07  1.56e-07  6.23e-07  1.56e-07
  wave-h64-m0-p1-n0-a0       W+L     699 |  2.40e-07  1.60e-07  9.61e-07  1.67e-07 |  4.62e-08  4.62e-08  1.85e-07  4.62e-08
  shard-h128-m0-p1-n0-a0     W+L     510 |  2.80e-07  4.09e-07  1.64e-06  2.59e-07 |  3.46e-07  3.46e-07  1.38e-06  3.46e-07
  wave-h128-m0-p1-n0-a1      W+L     699 |  6.34e-07  6.10e-07  2.54e-06  3.50e-07 |  5.15e-06  5.13e-06  2.06e-05  5.13e-06
  grouped-h64-m0-p1-n0-a1    G        99 |  8.81e-08  5.72e-08  3.53e-07  6.61e-08 |  1.46e-06  1.47e-06  5.90e-06  1.46e-06
  wave-h16-m0-p0-n1-a0       W+L+M   699 |  5.85e-07  5.82e-07  2.34e-06  1.32e-07 |  1.21e-07  1.51e-07  6.03e-07  1.48e-07
  shard-h32-m0-p0-n1-a0      W+L+M   510 |  2.60e-07  2.62e-07  1.05e-06  1.74e-07 |  2.49e-07  2.49e-07  9.96e-07  2.49e-07
  wave-h32-m0-p0-n1-a1       W+L+M   699 |  5.40e-07  3.22e-07  2.16e-06  4.17e-07 |  1.69e-07  1.72e-07  6.88e-07  1.72e-07
  grouped-h16-m0-p0-n1-a1    G+M      99 |  2.02e-07  1.59e-07  8.09e-07  1.91e-07 |  2.24e-07  1.99e-07  8.96e-07  1.66e-07
  wave-h64-m0-p0-n0-a0       W+L     699 |  4.27e-07  5.90e-07  2.36e-06  1.97e-07 |  1.81e-07  2.26e-07  9.05e-07  1.66e-07
  shard-h128-m0-p0-n0-a0     W+L     510 |  6.63e-07  5.26e-07  2.65e-06  1.88e-07 |  2.04e-07  1.57e-07  8.15e-07  1.57e-07
  wave-h128-m0-p0-n0-a1      W+L     699 |  4.00e-07  5.04e-07  2.02e-06  2.08e-07 |  1.68e-07  2.14e-07  8.57e-07  1.79e-07
  grouped-h64-m0-p0-n0-a1    G        99 |  1.99e-07  1.68e-07  7.95e-07  1.19e-07 |  1.97e-07  1.26e-07  7.90e-07  8.76e-08
  wave-h16-m1-p1-n1-a0       -+M     699 |  0.00e+00  0.00e+00  0.00e+00  0.00e+00 |  1.52e-07  1.53e-07  6.13e-07  1.72e-07
  shard-h32-m1-p1-n1-a0      -+M     510 |  0.00e+00  0.00e+00  0.00e+00  0.00e+00 |  1.61e-07  1.61e-07  6.46e-07  1.62e-07
  wave-h32-m1-p0-n0-a0       -       699 |  0.00e+00  0.00e+00  0.00e+00  0.00e+00 |  1.45e-07  1.28e-07  5.81e-07  1.80e-07
  grouped-h16-m1-p0-n0-a0    -        99 |  0.00e+00  0.00e+00  0.00e+00  0.00e+00 |  1.59e-07  1.90e-07  7.59e-07  1.54e-07
  chunked-h32-m0-p1-n1-a1    C+L     299 |  7.11e-07  7.93e-07  3.17e-06  1.64e-07 |  1.66e-07  1.66e-07  6.65e-07  1.84e-07

(case = shape-h-mode-perturb-normalized-out_act; mode 1 runs no node kernel: dxp is exactly zero on both sides.)

Tier 1 took: wave / shard W+L (EXT where `x`), grouped G (EXT: W), unsplit W without L (hub of 16 999 records by one wavefront).
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K = 64
NODE_LONG = 128
SCORE_PER = 32
T_DIST = float(np.float32(-0.05))
ERR_ARG, ERR_UNSUPPORTED = 1, 2
CANARY = np.float32(-24680.5)
EXACT_LIMIT = 1 << 24
LEAKY = np.float32(0.01)

SHAPES = {
    "wave": dict(ncols=700, row0=0, rows=700),
    "shard": dict(ncols=1100, row0=300, rows=511),
    "grouped": dict(ncols=700, row0=250, rows=100),
    "unsplit": dict(ncols=66000, row0=20000, rows=17000),
    "tiny": dict(ncols=50, row0=10, rows=30),           # CPU checks of the helpers only
    "whole120": dict(ncols=120, row0=0, rows=120),
    "chunked": dict(ncols=300, row0=0, rows=300),
}


def conv_per(F):
    return 4 * (64 // (F // 4))


def named_degrees(per):
    return sorted({1, per - 1, per, per + 1, NODE_LONG - 1, NODE_LONG, NODE_LONG + 1, 4 * per + 1})


def feasible_degrees(per, rows):
    """the named in-degrees a block of `rows` rows can hold (one row is empty, one keeps room for its self loop)"""
    return [d for d in named_degrees(per) if d <= rows - 3]


def chunk_counts(k):
    """M_i of dgg_chunk_layout: L_i = ceil(k_i + 8.5) + 1 ranks in chunks of 64"""
    L = np.ceil(k.astype(np.float32) + np.float32(8.5)) + 1
    return np.ceil(L / 64).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------
# graphs with prescribed in-degrees
# ---------------------------------------------------------------------------------------------------------------
def build_block(shape, per, cap, width=None, seed=0):
    """ELL block (rows [row0, row0 + rows) of `ncols` nodes) whose row i is active on its first cap[i] ranks.  -> idx int32 [rows, W]
    (W = widest row; -1 beyond a row's width), act bool [rows, W], info dict: hub, named {degree: node}, zero_in, zero_out, dead row,
    self-loop row.  Unique columns per row; ranks >= cap[i] hold a few more columns (the w = 0 kind of inactive entry) and then -1."""
    rng = np.random.default_rng(seed)
    ncols, row0, rows = shape["ncols"], shape["row0"], shape["rows"]
    width = np.full(rows, K, np.int64) if width is None else np.asarray(width, np.int64)
    W = int(width.max())
    cap = np.minimum(np.asarray(cap, np.int64), width).copy()
    dead = rows // 3
    cap[dead] = 0
    selfrow = int(np.flatnonzero(cap >= 3)[1])
    zero_in = row0 + dead
    outside = [j for j in (row0 - 1, row0 + rows) if 0 <= j < ncols]
    zero_out = outside[0] if outside else None
    live = np.flatnonzero(cap > 0)
    degs = feasible_degrees(per, rows)
    taken = {zero_in, row0 + selfrow} | ({zero_out} if zero_out is not None else set())
    pool = [int(j) for j in rng.permutation(ncols) if int(j) not in taken][:len(degs) + 1]
    hub, named = pool[0], dict(zip(degs, pool[1:]))
    special = np.zeros(ncols, bool)
    special[pool] = True
    special[[zero_in] + ([zero_out] if zero_out is not None else [])] = True
    chosen = [[] for _ in range(rows)]
    remaining = cap.copy()
    for i in live:
        chosen[i].append(hub)
    remaining[live] -= 1
    for d in sorted(degs, reverse=True):
        elig = np.flatnonzero((remaining > 0) & (np.arange(rows) != selfrow))
        assert len(elig) >= d, "block too small for in-degree %d" % d
        sel = rng.choice(elig, d, replace=False)
        for i in sel:
            chosen[i].append(named[d])
        remaining[sel] -= 1
    idx = np.full((rows, W), -1, np.int32)
    act = np.zeros((rows, W), bool)
    for i in range(rows):
        c, wd = int(cap[i]), int(width[i])
        extra = int(rng.integers(0, min(4, wd - c) + 1)) if i != dead else 0
        need = c - len(chosen[i]) + extra
        assert need + 16 <= ncols - int(special.sum()), "too few nodes for unique columns"
        fill = np.zeros(0, np.int64)
        own = [row0 + i] if i == selfrow else []
        while len(fill) < need:
            cand = np.concatenate([own, fill, rng.integers(0, ncols, need + 8)]).astype(np.int64)
            cand = cand[~special[cand]]
            _, first = np.unique(cand, return_index=True)
            fill = cand[np.sort(first)]
        fill = fill[:need]
        row_act = np.array(chosen[i] + list(fill[:need - extra]), np.int64)
        assert len(row_act) == c and len(set(row_act.tolist()) | set(fill.tolist())) == c + extra
        idx[i, :c] = rng.permutation(row_act)
        idx[i, c:c + extra] = fill[need - extra:]
        act[i, :c] = True
    info = dict(hub=hub, named=named, zero_in=zero_in, zero_out=zero_out, dead=dead, selfrow=selfrow, degs=degs, width=width)
    return idx, act, info


def check_profile(shape, idx, act, info, per):
    """the in-degree profile of the ACTIVE entries is the prescribed one"""
    ncols, row0, rows = shape["ncols"], shape["row0"], shape["rows"]
    indeg = np.bincount(idx[act], minlength=ncols)
    nlive = int((act.sum(1) > 0).sum())
    assert indeg[info["hub"]] == nlive and nlive == rows - 1
    assert info["degs"] == feasible_degrees(per, rows)
    for d in info["degs"]:
        assert indeg[info["named"][d]] == d, "in-degree %d is missing" % d
    assert indeg[info["zero_in"]] == 0 and row0 <= info["zero_in"] < row0 + rows
    if rows < ncols:
        assert info["zero_out"] is not None and indeg[info["zero_out"]] == 0 and not row0 <= info["zero_out"] < row0 + rows
    assert not act[info["dead"]].any()
    sr = info["selfrow"]
    assert (idx[sr][act[sr]] == row0 + sr).sum() == 1
    assert ((idx < 0) & ~act).any() and ((idx >= 0) & ~act).any()          # both kinds of inactive entry
    for i in range(0, rows, max(1, rows // 50)):
        v = idx[i][idx[i] >= 0]
        assert len(np.unique(v)) == len(v)


def positions(width):
    """pos [rows, W]: where rank r of row i sits in the packed [chunks*64] arrays (row i owns ceil(width_i / 64) chunks); -1 beyond"""
    m = (np.asarray(width) + 63) // 64
    cptr = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    W = int(np.max(width))
    pos = cptr[:-1, None] * 64 + np.arange(W)[None, :]
    pos[np.arange(W)[None, :] >= (m * 64)[:, None]] = -1
    return pos, cptr


def pack(wide, pos, fill, dtype):
    out = np.full(int(pos.max()) + 1, fill, dtype)
    out[pos[pos >= 0]] = wide[:, :pos.shape[1]][pos >= 0]
    return out.reshape(-1, 64)


def unpack(packed, pos, fill=0.0):
    out = np.full(pos.shape, fill, packed.dtype)
    out[pos >= 0] = packed.ravel()[pos[pos >= 0]]
    return out


# ---------------------------------------------------------------------------------------------------------------
# tier 1: cases, inputs, integer reference, premises
# ---------------------------------------------------------------------------------------------------------------
def ccase(shape, F, ext=False, phase=0, seed=0):
    return dict(shape=shape, F=F, ext=ext, phase=phase, seed=seed, id="%s-F%d%s%s" % (shape, F, "-x" if ext else "", "-p12" if phase else ""))


CONV = [ccase("wave", 16), ccase("wave", 32, ext=True, phase=1), ccase("wave", 64, ext=True), ccase("wave", 64, phase=1), ccase("wave", 128),
        ccase("shard", 32, ext=True), ccase("shard", 128), ccase("grouped", 64), ccase("grouped", 128, phase=1), ccase("grouped", 64, ext=True),
        ccase("unsplit", 16), ccase("unsplit", 16, ext=True, seed=1), ccase("chunked", 32), ccase("chunked", 64, ext=True)]
KNOB_CONV = [ccase("wave", 16), ccase("wave", 64, ext=True), ccase("shard", 128), ccase("grouped", 64), ccase("grouped", 128, phase=1)]
TINY = ccase("tiny", 128, ext=True)


@functools.lru_cache(maxsize=32)
def conv_inputs(cid):
    c = next(c for c in CONV + KNOB_CONV + [TINY] if c["id"] == cid)
    shape, F = SHAPES[c["shape"]], c["F"]
    ncols, row0, rows = shape["ncols"], shape["row0"], shape["rows"]
    rng = np.random.default_rng(1000 + F + c["seed"])
    width = None
    if c["shape"] == "chunked":
        kdeg = rng.uniform(3.0, 130.0, rows).astype(np.float32)
        width = 64 * chunk_counts(kdeg)
        cap = np.minimum(np.ceil(kdeg + 8.5).astype(np.int64), width)
    elif c["shape"] == "unsplit":
        kdeg, cap = None, rng.integers(1, 9, rows)
    elif c["shape"] == "tiny":
        kdeg, cap = None, rng.integers(1, 21, rows)
    else:
        kdeg, cap = None, rng.integers(1, 65, rows)
    idx, act, info = build_block(shape, conv_per(F), cap, width, seed=c["seed"] + F)
    w = np.where(act, rng.integers(1, 3, idx.shape), 0).astype(np.float32)
    val = rng.integers(1, 9, idx.shape).astype(np.float32)
    rs = rng.choice(np.array([1.0, 4.0], np.float32), ncols)
    G = rng.integers(-2, 3, (rows, F)).astype(np.float32)
    H = rng.integers(-2, 3, (ncols, F)).astype(np.float32)
    ext = np.where(act, rng.integers(-2, 3, idx.shape), np.nan).astype(np.float32) if c["ext"] else None
    pos, cptr = positions(info["width"])
    return dict(c=c, shape=shape, idx=idx, act=act, info=info, w=w, val=val, rs=rs, G=G, H=H, ext=ext, pos=pos, cptr=cptr, kdeg=kdeg)


def conv_reference(x):
    """integer reference on the flat active entries -> ii, rr, jj, dot [E] (float64 integers), dH [ncols,F], da [ncols] (float64)"""
    row0, ncols = x["shape"]["row0"], x["shape"]["ncols"]
    ii, rr = np.nonzero(x["act"])
    jj = x["idx"][ii, rr].astype(np.int64)
    G, H = x["G"].astype(np.int64), x["H"].astype(np.int64)
    dot = (G[ii] * H[jj]).sum(1).astype(np.float64)
    if x["ext"] is not None:
        dot = dot + x["ext"][ii, rr].astype(np.float64)
    a = 1.0 / np.sqrt(x["rs"].astype(np.float64))
    w = x["w"][ii, rr].astype(np.float64)
    ahat = w * a[row0 + ii] * a[jj]
    dH = np.zeros((ncols, G.shape[1]))
    np.add.at(dH, jj, ahat[:, None] * G[ii])
    da = np.zeros(ncols)
    np.add.at(da, jj, dot * w * a[row0 + ii])
    return ii, rr, jj, dot, dH, da


def premises_hold(x):
    """every term is a multiple of 1/4 and (sum of |terms|) * 4 stays below 2^24 for the dot products, dH and da (and da's final
    multiplication by sqrt(rs_j) <= 2) -- whatever the order of the sums"""
    row0, ncols = x["shape"]["row0"], x["shape"]["ncols"]
    ii, rr = np.nonzero(x["act"])
    jj = x["idx"][ii, rr].astype(np.int64)
    a = 1.0 / np.sqrt(x["rs"].astype(np.float64))
    ahat = x["w"][ii, rr].astype(np.float64) * a[row0 + ii] * a[jj]
    vals = [x["G"], x["H"]] + ([x["ext"][x["act"]]] if x["ext"] is not None else [])
    ok = all(np.array_equal(v, np.round(v)) for v in vals) and np.array_equal(ahat * 4, np.round(ahat * 4)) and set(np.unique(x["rs"])) <= {1.0, 4.0}
    absdot = (np.abs(x["G"]).astype(np.float64)[ii] * np.abs(x["H"]).astype(np.float64)[jj]).sum(1)
    if x["ext"] is not None:
        absdot = absdot + np.abs(x["ext"][ii, rr])
    sH, sa = np.zeros(ncols), np.zeros(ncols)
    np.add.at(sH, jj, np.abs(ahat) * np.abs(x["G"]).max(1)[ii])
    np.add.at(sa, jj, absdot * np.abs(ahat))
    worst = dict(dot=float(absdot.max()), dH=float(sH.max() * 4), da=float(sa.max() * 4 * 2))
    return ok and max(worst.values()) < EXACT_LIMIT, worst


def test_exactness_premises_hold_for_every_case():
    seen = set()
    for c in CONV + KNOB_CONV:
        if c["id"] in seen:
            continue
        seen.add(c["id"])
        x = conv_inputs(c["id"])
        ok, worst = premises_hold(x)
        assert ok, "%s: %r" % (c["id"], worst)
        if c["shape"] != "chunked":
            assert np.bincount(x["idx"][x["act"]], minlength=1)[x["info"]["hub"]] == x["shape"]["rows"] - 1
    # ... and the check does fail when the hub's sums leave the exact range
    x = dict(conv_inputs(ccase("unsplit", 16)["id"]))
    x["G"] = x["G"] * 64
    assert not premises_hold(x)[0]
    x = dict(conv_inputs(ccase("wave", 16)["id"]))
    x["rs"] = np.where(x["rs"] == 4.0, np.float32(3.0), x["rs"])
    assert not premises_hold(x)[0]


def test_prescribed_in_degrees_are_present():
    for cid, per in [(ccase("wave", 16)["id"], 64), (ccase("wave", 32, ext=True, phase=1)["id"], 32), (ccase("wave", 64, ext=True)["id"], 16),
                     (ccase("wave", 128)["id"], 8), (ccase("shard", 128)["id"], 8), (ccase("shard", 32, ext=True)["id"], 32),
                     (ccase("grouped", 64)["id"], 16), (ccase("unsplit", 16)["id"], 64), (ccase("chunked", 32)["id"], 32)]:
        x = conv_inputs(cid)
        check_profile(x["shape"], x["idx"], x["act"], x["info"], per)
        present = x["info"]["degs"]
        if x["c"]["shape"] != "grouped":                 # every named boundary is really there
            assert present == named_degrees(per), "%s: %r" % (cid, present)
        else:
            assert present == [d for d in named_degrees(per) if d <= 97]
    for name in ("wave", "shard", "grouped", "chunked"):
        sc = next(c for c in SCORE if c["shape"] == name)
        g = score_graph(sc["shape"], sc["h"], sc["perturb"], sc["mode"], sc["out_act"])
        check_profile(g["shape"], g["idx"], g["act"], g["info"], SCORE_PER)
        assert g["info"]["degs"] == (named_degrees(SCORE_PER) if name != "grouped" else [1, 31, 32, 33])


def test_integer_reference_matches_a_triple_loop():
    x = conv_inputs(TINY["id"])
    ii, rr, jj, dot, dH, da = conv_reference(x)
    row0, (rows, W), F = x["shape"]["row0"], x["idx"].shape, x["G"].shape[1]
    dA2, dH2, da2 = np.zeros((rows, W)), np.zeros_like(dH), np.zeros_like(da)
    for i in range(rows):
        for r in range(W):
            j = int(x["idx"][i, r])
            if j < 0 or x["w"][i, r] == 0:
                continue
            s = 0.0
            for f in range(F):
                s += float(x["G"][i, f]) * float(x["H"][j, f])
            s += float(x["ext"][i, r])
            dA2[i, r] = s
            ai, aj = 1.0 / np.sqrt(float(x["rs"][row0 + i])), 1.0 / np.sqrt(float(x["rs"][j]))
            for f in range(F):
                dH2[j, f] += float(x["w"][i, r]) * ai * aj * float(x["G"][i, f])
            da2[j] += s * float(x["w"][i, r]) * ai
    dA1 = np.zeros((rows, W))
    dA1[ii, rr] = dot
    assert np.array_equal(dA1, dA2) and np.array_equal(dH, dH2) and np.array_equal(da, da2)
    assert np.array_equal(dH.astype(np.float32), dH) and np.array_equal(da.astype(np.float32), da)
    # pack / unpack are inverse on the slots that exist
    width = np.array([64, 128, 64, 192])
    pos, cptr = positions(width)
    wide = np.arange(4 * 192, dtype=np.float32).reshape(4, 192)
    assert list(cptr) == [0, 1, 3, 4, 7] and np.array_equal(unpack(pack(wide, pos, -1.0, np.float32), pos, -1.0)[pos >= 0], wide[pos >= 0])


# ---------------------------------------------------------------------------------------------------------------
# tier 2: graphs, float64 / float32 restatement
# ---------------------------------------------------------------------------------------------------------------
def scase(shape, h, mode=0, perturb=1, normalized=1, out_act=0):
    return dict(shape=shape, h=h, mode=mode, perturb=perturb, normalized=normalized, out_act=out_act,
                id="%s-h%d-m%d-p%d-n%d-a%d" % (shape, h, mode, perturb, normalized, out_act))


def _score_cases():
    combos = [(0, p, n, a) for p in (1, 0) for n in (1, 0) for a in (0, 1)] + [(1, 1, 1, 0), (1, 0, 0, 0)]
    out = []
    for q, (m, p, n, a) in enumerate(combos):
        out.append(scase("wave", (16, 32, 64, 128)[q % 4], m, p, n, a))
        out.append(scase(("shard", "grouped")[q % 2], ((32, 16), (128, 64))[(q // 2) % 2][q % 2], m, p, n, a))
    return out + [scase("chunked", 32, 0, 1, 1, 1)]


SCORE = _score_cases()
KNOB_SCORE = [scase("wave", 16, 0, 1, 1, 0), scase("wave", 64, 0, 1, 0, 0), scase("shard", 32, 0, 1, 1, 0), scase("grouped", 16, 0, 0, 1, 0)]


def ramp_cap(k, W):
    """ranks of a row that carry weight in float32: the ramp 1 - 0.5 (1 + tanh(r - k)) is exactly 0 beyond them"""
    from oracle import oracle as O
    f, _ = O.softk(np.zeros((len(k), W), np.int32), np.ones((len(k), W), np.float32), k, mode=1)
    cap = (f != 0).sum(1)
    assert all((f[i, :cap[i]] != 0).all() for i in range(len(k)))
    return cap


@functools.lru_cache(maxsize=8)
def score_graph(shape_name, h, perturb, mode, out_act):
    from oracle import oracle as O
    shape = SHAPES[shape_name]
    ncols, row0, rows = shape["ncols"], shape["row0"], shape["rows"]
    rng = np.random.default_rng(7000 + 10 * h + 2 * perturb + mode + ncols + rows)
    xp = (rng.standard_normal((ncols, h)) * 0.6).astype(np.float32)
    if out_act:
        xp[rng.integers(0, ncols, 40), rng.integers(0, h, 40)] = 0.0
    chunked = shape_name == "chunked"
    k = rng.uniform(3.0, 130.0 if chunked else 40.0, rows).astype(np.float32)
    width = 64 * chunk_counts(k) if chunked else np.full(rows, K, np.int64)
    cap = np.minimum(ramp_cap(k, int(width.max())), width)
    idx, act, info = build_block(shape, SCORE_PER, cap, width, seed=h + perturb)
    L = O.lib()
    val = np.zeros(idx.shape, np.float32)
    gum = rng.gumbel(size=idx.shape).astype(np.float32)
    base = xp.ctypes.data
    for i, r in zip(*np.nonzero(idx >= 0)):
        val[i, r] = L.ora_pair_score(C.c_void_p(base + 4 * h * (row0 + int(i))), C.c_void_p(base + 4 * h * int(idx[i, r])), C.c_int(h),
                                     C.c_float(T_DIST), C.c_int(perturb), C.c_float(float(gum[i, r])))
    w, rs_rows = O.softk(idx, val, k, mode=mode)
    assert np.array_equal((idx >= 0) & (w != 0), act)
    rs = rng.uniform(2.0, 20.0, ncols).astype(np.float32)           # stand-ins for the nodes whose rows are not in the block
    rs[row0:row0 + rows] = rs_rows
    r32 = np.arange(idx.shape[1], dtype=np.float32)[None, :] - k[:, None]
    th32 = np.vectorize(O.tanh, otypes=[np.float32])(r32)
    F = 32
    pos, cptr = positions(width)
    return dict(shape=shape, idx=idx, act=act, info=info, val=val, w=w, rs=rs, k=k, xp=xp, th32=th32, th64=np.tanh(r32.astype(np.float64)),
                G=rng.standard_normal((rows, F)).astype(np.float32), H=rng.standard_normal((ncols, F)).astype(np.float32),
                dw=rng.standard_normal(idx.shape).astype(np.float32), pos=pos, cptr=cptr, width=width)


def seg_sum(keys, terms, n):
    """out[key] = sum of the terms of that key, accumulated ONE BY ONE in the order given, in the dtype of `terms`"""
    order = np.argsort(keys, kind="stable")
    ks, t = keys[order], terms[order]
    cnt = np.bincount(ks, minlength=n)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    out = np.zeros((n,) + t.shape[1:], t.dtype)
    for p in range(int(cnt.max()) if len(ks) else 0):
        nodes = np.flatnonzero(cnt > p)
        out[nodes] = out[nodes] + t[starts[nodes] + p]
    return out


def restate(T, g, c, dA, da, ahat, perm=None):
    """ora_softk_norm_bwd + ora_edge_bwd for the block of `g` in dtype T (float64: the reference; float32: the CPU figure), sums taken
    entry by entry in row order or in the order `perm`.  dA [rows,W] by rows (normalized = 0: d loss / d w), da [ncols] the neighbour
    side of the normalisation backward (None: formed here from dA), ahat [rows,W] (entries with ahat == 0 carry no dA, as the kernels
    mask them).  -> dxp [ncols,h], dk [rows] in dtype T"""
    shape = g["shape"]
    ncols, row0, rows = shape["ncols"], shape["row0"], shape["rows"]
    f32 = T == np.float32
    ii, rr = np.nonzero(g["idx"] >= 0)
    if perm is not None:
        ii, rr = ii[perm], rr[perm]
    jj = g["idx"][ii, rr].astype(np.int64)
    gi = row0 + ii
    xp, val, dA = g["xp"].astype(T), g["val"][ii, rr].astype(T), dA[ii, rr].astype(T)
    with np.errstate(all="ignore"):
        if c["normalized"]:
            rs = g["rs"].astype(T)
            a = T(1) / np.sqrt(rs)
            w = g["w"][ii, rr].astype(T)
            ah = ahat[ii, rr].astype(T) if ahat is not None else w * a[gi] * a[jj]
            dA = np.where(ah != 0, dA, T(0))
            if da is None:
                da = seg_sum(jj, dA * w * a[gi], ncols)
            rsb, ab = rs[row0:row0 + rows], a[row0:row0 + rows]
            dai = da[row0:row0 + rows].astype(T) + seg_sum(ii, dA * ah, rows) * np.sqrt(rsb)
            drs = T(-0.5) * dai * ab / rsb
            dw = dA * a[gi] * a[jj] + drs[ii]
        else:
            dw = dA
    th = (g["th32"] if f32 else g["th64"])[ii, rr]
    f = T(1) - T(0.5) * (T(1) + th)
    dfdk = T(0.5) * (T(1) - th * th)
    dxp = np.zeros((ncols, xp.shape[1]), T)
    if c["mode"] == 0:
        dk = seg_sum(ii, dw * val * dfdk, rows)
        dval = dw * f
        d = xp[gi] - xp[jj]
        dist = np.sqrt((d * d).sum(1))
        ok = (dval != 0) & (dist != 0)
        t = T(np.float32(T_DIST))
        if f32:
            from oracle import oracle as O
            p = np.vectorize(O.exp, otypes=[np.float32])(t * dist)
        else:
            p = np.exp(t * dist)
        with np.errstate(all="ignore"):
            dp = dval * val / (p + T(np.float32(1e-8))) if c["perturb"] else dval
            dd = np.where(ok, dp * t * p / np.where(ok, dist, T(1)), T(0))
        terms = dd[:, None] * d
        both = np.empty((2 * len(ii),) + terms.shape[1:], T)
        both[0::2], both[1::2] = terms, -terms
        keys = np.empty(2 * len(ii), np.int64)
        keys[0::2], keys[1::2] = gi, jj
        dxp = seg_sum(keys, both, ncols)
        if c["out_act"]:
            dxp = dxp * np.where(g["xp"] > 0, T(1), T(LEAKY))
    else:
        dk = seg_sum(ii, dw * dfdk, rows)
    return dxp, dk


def rel_max(got, ref):
    m = float(np.abs(ref).max())
    return float(np.abs(got.astype(np.float64) - ref).max()) / (m if m > 0 else 1.0)


def test_float64_restatement_matches_the_oracle():
    """restate(float64) against ora_softk_norm_bwd + ora_edge_bwd on a whole 120-node graph (row0 = 0, rows = ncols).  The oracle
    accumulates in double but takes tanh / exp / the distance in float32 and rounds dval, dk and dxp to float32: a few float32 ulps per
    term, so 64 * 2^-24 = 4e-6 of max bounds the difference; the float32 restatement in both orders stays within 1e-4"""
    from oracle import oracle as O
    for mode, perturb in [(0, 1), (0, 0), (1, 1)]:
        g = score_graph("whole120", 16, perturb, mode, 0)
        c = scase("whole120", 16, mode, perturb, 1, 0)
        rng = np.random.default_rng(5)
        dA = np.where(g["act"], rng.standard_normal(g["idx"].shape), 0).astype(np.float32)
        g = dict(g)
        g["rs"] = np.where(g["rs"] > 0, g["rs"], np.float32(1.0)).astype(np.float32)    # (the empty row: the oracle divides by rs_i)
        dval, dk_o = O.softk_norm_bwd(g["idx"], g["val"], g["k"], g["w"], g["rs"], dA, mode)
        dxp_o = O.edge_bwd(g["xp"], g["idx"], g["val"], dval, T_DIST, bool(perturb))
        dxp, dk = restate(np.float64, g, c, dA, None, None)
        assert rel_max(dk_o, dk) < 64 * 2.0 ** -24 and rel_max(dxp_o, dxp) < 64 * 2.0 ** -24, (rel_max(dk_o, dk), rel_max(dxp_o, dxp))
        E = int((g["idx"] >= 0).sum())
        for perm in (None, np.random.default_rng(1).permutation(E)):
            dxp32, dk32 = restate(np.float32, g, c, dA, None, None, perm)
            assert dxp32.dtype == np.float32 and rel_max(dxp32, dxp) < 1e-4 and rel_max(dk32, dk) < 1e-4
        # the mask and the un-normalised form are what they say
        c2 = scase("whole120", 16, mode, perturb, 0, 1)
        dxp2, dk2 = restate(np.float64, g, c2, dA, None, None)
        c3 = scase("whole120", 16, mode, perturb, 0, 0)
        dxp3, dk3 = restate(np.float64, g, c3, dA, None, None)
        assert np.array_equal(dk2, dk3) and np.array_equal(dxp2, dxp3 * np.where(g["xp"] > 0, 1.0, np.float64(LEAKY)))
    # seg_sum is a sequential sum in the order given
    keys = np.array([2, 0, 2, 2, 0])
    terms = np.array([1e8, 1.0, 1.0, -1e8, 2.0], np.float32)
    assert np.array_equal(seg_sum(keys, terms, 3), np.array([3.0, 0.0, 0.0], np.float32))
    assert np.array_equal(seg_sum(keys[[0, 3, 2, 1, 4]], terms[[0, 3, 2, 1, 4]], 3), np.array([3.0, 0.0, 1.0], np.float32))


# ---------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------
class Guard:
    """`body` inside a larger device buffer with `fill` on both sides (NaN around inputs, canary words around outputs); .t is the
    tensor view of the body (16-byte aligned)"""

    def __init__(self, dev, body, fill, guard=256):
        import torch
        body = np.ascontiguousarray(body)
        host = np.full(guard + body.size + guard, fill, body.dtype)
        host[guard:guard + body.size] = body.ravel()
        self.g, self.n, self.shape, self.fill = guard, body.size, body.shape, fill
        self.buf = torch.from_numpy(host).to(dev)
        self.t = self.buf[guard:guard + body.size].view(body.shape)
        self.addr = self.t.data_ptr()
        assert self.addr % 16 == 0

    def read(self, what=""):
        h = self.buf.cpu().numpy()
        gd = np.concatenate([h[:self.g], h[self.g + self.n:]])
        ok = bool(np.isnan(gd).all()) if (isinstance(self.fill, float) and np.isnan(self.fill)) else bool((gd == self.fill).all())
        assert ok, "words around %s were overwritten" % what
        return h[self.g:self.g + self.n].reshape(self.shape).copy()


def nans(shape):
    return np.full(shape, np.nan, np.float32)


def addr(gd):
    return None if gd is None else gd.addr


def build_partition(dev, x, phase=0):
    """uploads idx / w / val / rs between guards and builds the payload partition through ops -> dict of the device operands"""
    import torch
    from dgg_amd import ops
    shape = x["shape"]
    ncols, row0, rows = shape["ncols"], shape["row0"], shape["rows"]
    pos = x["pos"]
    chunked = pos.shape[1] > K
    d = dict(idx=Guard(dev, pack(x["idx"], pos, -1, np.int32), 0), w=Guard(dev, pack(x["w"], pos, 0.0, np.float32), np.nan),
             val=Guard(dev, pack(x["val"], pos, 0.0, np.float32), np.nan), rs=Guard(dev, x["rs"], np.nan),
             rs_rows=Guard(dev, x["rs"][row0:row0 + rows], np.nan), lay=None)
    d["chunks"] = d["idx"].shape[0]
    if chunked:
        lay = ops.chunk_layout(torch.from_numpy(x["kdeg"] if "kdeg" in x else x["k"]).to(dev))
        assert lay.wide and np.array_equal(lay.cptr.cpu().numpy(), x["cptr"]), "dgg_chunk_layout differs from L_i = ceil(k_i + 8.5) + 1"
        d["lay"] = lay
    part, ahat = ops.partp_build(d["idx"].t, d["w"].t, d["val"].t, d["rs_rows"].t, ncols, rs_all=d["rs"].t, phase=phase, layout=d["lay"])
    if phase == 1:
        ops.partp_sort(part)
    d["part"], d["ahat"] = part, ahat
    for k_ in ("idx", "w", "val", "rs", "rs_rows"):
        d[k_].read(k_)
    return d


def conv_call(dev, x, d, G, H, ext, dA, F):
    """one call of the case's conv entry point with NaN-filled outputs between canaries; dA: 'nan' (handed in NaN-filled), 'zero'
    or None (NULL) -> rc, dA (packed [chunks*64] or None), dA_rec, dH, da"""
    import torch
    from dgg_amd import _lib, ops
    L, st = _lib.lib(), ops._stream()
    shape = x["shape"]
    ncols, nslots = shape["ncols"], d["chunks"] * 64
    gdA = None if dA is None else Guard(dev, nans(nslots) if dA == "nan" else np.zeros(nslots, np.float32), CANARY)
    grec, gdH, gda = Guard(dev, nans(nslots), CANARY), Guard(dev, nans((ncols, F)), CANARY), Guard(dev, nans(ncols), CANARY)
    ws = d["part"].ws.data_ptr()
    if d["lay"] is not None:
        rc = L.dgg_ell_conv_bwd_partp_chunked(G.addr, H.addr, d["chunks"], F, ws, ncols, d["rs"].addr, addr(ext), addr(gdA), grec.addr, gdH.addr,
                                              gda.addr, st)
    elif ext is None:
        rc = L.dgg_ell_conv_bwd_partp(G.addr, H.addr, d["chunks"], K, F, ws, ncols, d["rs"].addr, addr(gdA), grec.addr, gdH.addr, gda.addr, st)
    else:
        rc = L.dgg_ell_conv_bwd_partp_ext(G.addr, H.addr, d["chunks"], K, F, ws, ncols, d["rs"].addr, ext.addr, addr(gdA), grec.addr, gdH.addr,
                                          gda.addr, st)
    torch.cuda.synchronize()
    return rc, (None if gdA is None else gdA.read("dA")), grec.read("dA_rec"), gdH.read("dH"), gda.read("da"), gdA


def check_conv(dev, c):
    """runs a tier-1 case; returns a list of mismatch descriptions (empty = exact)"""
    import torch
    from dgg_amd import ops
    x = conv_inputs(c["id"])
    ok, worst = premises_hold(x)
    assert ok, worst
    F, ncols = c["F"], x["shape"]["ncols"]
    d = build_partition(dev, x, c["phase"])
    G, H = Guard(dev, x["G"], np.nan), Guard(dev, x["H"], np.nan)
    ext = Guard(dev, pack(x["ext"], x["pos"], np.nan, np.float32), np.nan) if x["ext"] is not None else None
    ii, rr, jj, dot, dH_e, da_e = conv_reference(x)
    pp = x["pos"][ii, rr]
    nodeptr, recs = ops.partp_records(d["part"])
    recs = recs.cpu().numpy()
    nrec = len(recs)
    bad = []
    if nrec != len(ii) or not np.array_equal(np.sort(recs[:, 0]), np.sort(pp)):
        return ["%s: the partition does not hold the active entries (%d records, %d entries)" % (c["id"], nrec, len(ii))]
    indeg = np.diff(nodeptr.cpu().numpy())
    assert np.array_equal(indeg, np.bincount(jj, minlength=ncols))
    rc, dA, rec, dH, da, gdA = conv_call(dev, x, d, G, H, ext, "nan", F)
    if rc != 0:
        return ["%s: status %d" % (c["id"], rc)]
    dA_e = nans(dA.shape)
    dA_e[pp] = dot
    rec_e = nans(rec.shape)
    rec_e[:nrec] = dA_e[recs[:, 0]]

    def cmp(name, got, exp):
        if not np.array_equal(got, exp.astype(np.float32), equal_nan=True):
            wbad = np.flatnonzero(~((got == exp) | (np.isnan(got) & np.isnan(exp))).ravel())
            bad.append("%s: %s differs in %d of %d elements, first at flat index %d: got %r, expected %r" % (
                c["id"], name, len(wbad), got.size, wbad[0], got.ravel()[wbad[0]], exp.ravel()[wbad[0]]))
    cmp("dA (active slots exact, the others untouched)", dA, dA_e)
    cmp("dA_rec", rec, rec_e)
    cmp("dH", dH, dH_e)
    cmp("da", da, da_e)
    gat = ops.partp_gather(d["part"], gdA.t.view(-1, 64))
    torch.cuda.synchronize()
    cmp("partp_gather(dA)", gat.cpu().numpy()[:nrec], rec_e[:nrec])
    if d["lay"] is None and ops.partp_has_map(d["chunks"]):
        rc, _, rec0, dH0, da0, _ = conv_call(dev, x, d, G, H, ext, None, F)
        if rc != 0:
            return bad + ["%s, dA = NULL: status %d" % (c["id"], rc)]
        cmp("dA_rec with dA = NULL", rec0, rec_e)
        cmp("dH with dA = NULL", dH0, dH_e)
        cmp("da with dA = NULL", da0, da_e)
    for gd, nm in ((G, "G"), (H, "H"), (ext, "dA_ext")):
        if gd is not None:
            gd.read(nm)
    return bad


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("c", CONV, ids=[c["id"] for c in CONV])
def test_conv_backward_is_the_integer_reference_bit_for_bit(dev, c):
    bad = check_conv(dev, c)
    assert not bad, "\n".join(bad)


def edge_call(dev, g, c, d, dA, dA_rec, da, ahat, phase=0, state=None, **over):
    """one call of dgg_softk_edge_bwd_partp_phase / _chunked.  dA / da / ahat: Guards or None; outputs between canaries (dxp handed in
    NaN-filled in mode 0, zeroed in mode 1).  -> rc, dxp, dk, state (the output Guards, for phase 2)"""
    import torch
    from dgg_amd import _lib, ops
    L, st = _lib.lib(), ops._stream()
    shape = g["shape"]
    ncols, row0, rows = shape["ncols"], shape["row0"], shape["rows"]
    h = g["xp"].shape[1]
    a = dict(h=h, mode=c["mode"], normalized=c["normalized"], out_act=c["out_act"], phase=phase, rows=rows)
    a.update(over)
    if state is None:
        gdxp = Guard(dev, nans((ncols, h)) if c["mode"] == 0 else np.zeros((ncols, h), np.float32), CANARY)
        gdk, gri = Guard(dev, nans(rows), CANARY), Guard(dev, nans(4 * d["chunks"]), CANARY)
    else:
        gdxp, gdk, gri = state
    rsa = d["rs"].addr if c["normalized"] or over.get("rs") else None
    if d["lay"] is not None:
        rc = L.dgg_softk_edge_bwd_partp_chunked(d["xp"].addr, a["rows"], d["lay"].cptr.data_ptr(), d["chunks"], a["h"], d["idx"].addr, d["val"].addr,
                                                d["k"].addr, rsa, addr(dA), dA_rec.addr, addr(da), addr(ahat), row0, T_DIST, c["perturb"],
                                                a["mode"], a["normalized"], d["part"].ws.data_ptr(), ncols, gri.addr, gdk.addr, gdxp.addr,
                                                a["out_act"], a["phase"], st)
    else:
        rc = L.dgg_softk_edge_bwd_partp_phase(d["xp"].addr, a["rows"], a["h"], d["idx"].addr, d["val"].addr, d["k"].addr, rsa, addr(dA), dA_rec.addr,
                                              addr(da), addr(ahat), K, row0, T_DIST, c["perturb"], a["mode"], a["normalized"],
                                              d["part"].ws.data_ptr(), ncols, gri.addr, gdk.addr, gdxp.addr, a["out_act"], a["phase"], st)
    torch.cuda.synchronize()
    gri.read("rowinfo_ws")
    return rc, gdxp.read("dxp"), gdk.read("dk"), (gdxp, gdk, gri)


def score_setup(dev, c):
    """graph, partition, and the conv call (standard-normal G, H) whose dA / dA_rec / da feed the score backward"""
    from dgg_amd import ops
    g = score_graph(c["shape"], c["h"], c["perturb"], c["mode"], c["out_act"])
    d = build_partition(dev, g)
    d["xp"], d["k"] = Guard(dev, g["xp"], np.nan), Guard(dev, g["k"], np.nan)
    F = g["G"].shape[1]
    G, H = Guard(dev, g["G"], np.nan), Guard(dev, g["H"], np.nan)
    rc, dA, rec, dH, da, gdA = conv_call(dev, g, d, G, H, None, "zero", F)
    assert rc == 0 and np.isfinite(dH).all() and np.isfinite(da).all()
    if not c["normalized"]:                       # the generator as a separate module: d loss / d w by rows, gathered into record order
        dA = pack(g["dw"], g["pos"], 0.0, np.float32).ravel()
        gdA = Guard(dev, dA, np.nan)
        rec = ops.partp_gather(d["part"], gdA.t.view(-1, 64)).cpu().numpy()
    return g, d, dA, rec, da, gdA


def score_figures(dev, c):
    """-> dict of the measured figures of a tier-2 case, plus a list of contract violations"""
    from dgg_amd import ops
    g, d, dA, rec, da, gdA = score_setup(dev, c)
    norm = bool(c["normalized"])
    grec = Guard(dev, rec, np.nan)
    gda = Guard(dev, da, np.nan) if norm else None
    gah = Guard(dev, d["ahat"].cpu().numpy(), np.nan) if norm else None
    rc, dxp, dk, _ = edge_call(dev, g, c, d, gdA, grec, gda, gah)
    assert rc == 0, "status %d" % rc
    bad = []
    if not (np.isfinite(dxp).all() and np.isfinite(dk).all()):
        bad.append("an element of dxp (%d) or dk (%d) was not written" % (int((~np.isfinite(dxp)).sum()), int((~np.isfinite(dk)).sum())))
    has_map = d["lay"] is None and bool(ops.partp_has_map(d["chunks"]))
    if norm and d["lay"] is None:
        if has_map:
            _, dxp1, dk1, _ = edge_call(dev, g, c, d, None, grec, gda, gah)
            if not (np.array_equal(dxp1, dxp) and np.array_equal(dk1, dk)):
                bad.append("dA = NULL through the slot -> record map differs from dA given")
        dAn = np.where(pack(g["act"], g["pos"], False, bool).ravel(), dA, np.nan).astype(np.float32)
        _, dxp2, dk2, _ = edge_call(dev, g, c, d, Guard(dev, dAn, np.nan), grec, gda, gah)
        if not (np.array_equal(dxp2, dxp) and np.array_equal(dk2, dk)):
            bad.append("dA with NaN on the inactive slots (zero_dA=False) differs from the zeroed dA")
    _, dxp3, dk3, state = edge_call(dev, g, c, d, gdA, grec, gda, gah, phase=1)
    if not np.array_equal(dk3, dk):
        bad.append("dk after phase 1 is not the final dk")
    _, dxp4, dk4, _ = edge_call(dev, g, c, d, gdA, grec, gda, gah, phase=2, state=state)
    if not (np.array_equal(dxp4, dxp) and np.array_equal(dk4, dk)):
        bad.append("phase 1 then 2 differs from phase 0")
    dA_w, ah_w = unpack(dA, g["pos"]), (unpack(d["ahat"].cpu().numpy().ravel(), g["pos"]) if norm else None)
    ref_dxp, ref_dk = restate(np.float64, g, c, dA_w, da if norm else None, ah_w)
    E = int((g["idx"] >= 0).sum())
    cpu = [restate(np.float32, g, c, dA_w, da if norm else None, ah_w, perm) for perm in (None, np.random.default_rng(E).permutation(E))]
    indeg = np.bincount(g["idx"][g["act"]], minlength=g["shape"]["ncols"])
    rows, ncols = d["chunks"], g["shape"]["ncols"]
    branch = "-" if c["mode"] == 1 else ("C+L" if d["lay"] is not None else ("G" if rows * K < 16 * ncols else "W" + ("+L" if ncols <= 65536 and indeg.max() > NODE_LONG else "")))
    row = dict(id=c["id"], branch=branch + ("+M" if norm and has_map else ""), hub=int(indeg.max()),
               dxp_gpu=rel_max(dxp, ref_dxp), dxp_cpu_row=rel_max(cpu[0][0], ref_dxp), dxp_cpu_shuf=rel_max(cpu[1][0], ref_dxp),
               dk_gpu=rel_max(dk, ref_dk), dk_cpu_row=rel_max(cpu[0][1], ref_dk), dk_cpu_shuf=rel_max(cpu[1][1], ref_dk))
    row["dxp_bar"] = 4 * max(row["dxp_cpu_row"], row["dxp_cpu_shuf"])
    row["dk_bar"] = 4 * max(row["dk_cpu_row"], row["dk_cpu_shuf"])
    print("TIER2 " + json.dumps(row))
    for gd, nm in ((d["xp"], "xp"), (d["k"], "k"), (grec, "dA_rec"), (gda, "da"), (gah, "ahat_rows"), (gdA, "dA")):
        if gd is not None and nm != "dA":
            gd.read(nm)
    return row, bad


def check_score(dev, c):
    row, bad = score_figures(dev, c)
    if c["mode"] == 1 and row["dxp_gpu"] != 0.0:
        bad.append("mode 1: dxp is not zero")
    if row["dxp_gpu"] > row["dxp_bar"]:
        bad.append("dxp: %.3g of max against a bar of %.3g (4 x the float32 restatement on the CPU)" % (row["dxp_gpu"], row["dxp_bar"]))
    if row["dk_gpu"] > row["dk_bar"]:
        bad.append("dk: %.3g of max against a bar of %.3g (4 x the float32 restatement on the CPU)" % (row["dk_gpu"], row["dk_bar"]))
    return ["%s: %s" % (c["id"], b) for b in bad]


@pytest.mark.gpu
@pytest.mark.parametrize("c", SCORE, ids=[c["id"] for c in SCORE])
def test_score_backward_within_four_times_the_float32_restatement(dev, c):
    bad = check_score(dev, c)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# forcing knobs: one fresh process per value
# ---------------------------------------------------------------------------------------------------------------
KNOBS = ["DGG_NODE_SPLIT=0", "DGG_NODE_GROUPS=0", "DGG_NODE_GROUPS=1", "DGG_DA_MAP=0", "DGG_PP_THREADS=256", "DGG_PP_WIDTH=32"]


@pytest.mark.gpu
@pytest.mark.parametrize("knob", KNOBS)
def test_both_tiers_under_forcing_knob(dev, knob):
    env = dict(os.environ)
    name, value = knob.split("=")
    env[name] = value
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--knob-child"]
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.exit("the %s child process hung: nothing further is started on the GPU" % knob, returncode=3)
    out = r.stdout.decode(errors="replace")
    if r.returncode not in (0, 1):
        pytest.exit("the %s child process ended abnormally (status %d): nothing further is started on the GPU\n%s" % (knob, r.returncode, out[-2000:]),
                    returncode=3)
    assert r.returncode == 0 and "KNOB_CHILD_OK %d" % (len(KNOB_CONV) + len(KNOB_SCORE)) in out, out[-4000:]


def _knob_child():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import dgg_amd  # noqa: F401
    from dgg_amd import ops
    d = torch.device("cuda:0")
    bad = []
    for c in KNOB_CONV:
        bad += check_conv(d, c)
    for c in KNOB_SCORE:
        bad += check_score(d, c)
    if os.environ.get("DGG_DA_MAP") == "0":
        if ops.partp_has_map(100):
            bad.append("DGG_DA_MAP=0 but dgg_partp_has_map says 1")
        bad += refusal("null-dA-without-map", d)
    if bad:
        print("\n".join(bad))
        return 1
    print("KNOB_CHILD_OK %d" % (len(KNOB_CONV) + len(KNOB_SCORE)))
    return 0


# ---------------------------------------------------------------------------------------------------------------
# refusals and empty blocks: argument checks only, nothing is launched
# ---------------------------------------------------------------------------------------------------------------
REFUSALS = {
    "phase-3": ("edge", dict(phase=3), ERR_ARG),
    "mode-2": ("edge", dict(mode=2), ERR_ARG),
    "out_act-with-mode-1": ("edge", dict(mode=1, out_act=1), ERR_ARG),
    "null-dA-unnormalised": ("edge", dict(normalized=0, dA=None, ahat=None), ERR_ARG),
    "ahat_rows-unnormalised": ("edge", dict(normalized=0), ERR_ARG),
    "h-24": ("edge", dict(h=24), ERR_UNSUPPORTED),
    "F-48": ("conv", dict(F=48), ERR_UNSUPPORTED),
    "missing-rs": ("conv", dict(rs=None), ERR_ARG),
    "rs_all-without-ahat": ("build", {}, ERR_ARG),
    "null-dA-without-map": ("edge", dict(dA=None), ERR_ARG),
    "zero-rows-edge": ("edge", dict(rows=0), 0),
    "zero-rows-conv": ("conv", dict(rows=0), 0),
    "zero-rows-build": ("build", dict(rows=0), 0),
}


def refusal(name, dev):
    """-> list of violations: wrong status, empty error text, or an output that was written"""
    import torch
    from dgg_amd import _lib, ops
    L, st = _lib.lib(), ops._stream()
    kind, over, want = REFUSALS[name]
    c = scase("grouped", 16, 0, 1, 1, 0)
    g = score_graph(c["shape"], c["h"], c["perturb"], c["mode"], c["out_act"])
    d = build_partition(dev, g)
    shape = g["shape"]
    ncols, row0, rows = shape["ncols"], shape["row0"], shape["rows"]
    outs = {}

    def out(nm, n):
        outs[nm] = Guard(dev, np.full(n, 7.0, np.float32), CANARY)
        return outs[nm].addr
    ins = dict(xp=Guard(dev, g["xp"], np.nan), k=Guard(dev, g["k"], np.nan), dA=Guard(dev, np.zeros(rows * K, np.float32), np.nan),
               rec=Guard(dev, np.zeros(rows * K, np.float32), np.nan), da=Guard(dev, np.zeros(ncols, np.float32), np.nan),
               ahat=Guard(dev, d["ahat"].cpu().numpy(), np.nan), G=Guard(dev, g["G"], np.nan), H=Guard(dev, g["H"], np.nan))
    ws = d["part"].ws
    ws_before = ws.clone()
    if kind == "edge":
        a = dict(h=16, mode=0, normalized=1, out_act=0, phase=0, rows=rows, dA=ins["dA"], ahat=ins["ahat"])
        a.update(over)
        rc = L.dgg_softk_edge_bwd_partp_phase(ins["xp"].addr, a["rows"], a["h"], d["idx"].addr, d["val"].addr, ins["k"].addr, d["rs"].addr, addr(a["dA"]),
                                              ins["rec"].addr, ins["da"].addr, addr(a["ahat"]), K, row0, T_DIST, 1, a["mode"], a["normalized"],
                                              ws.data_ptr(), ncols, out("rowinfo", 4 * rows), out("dk", rows), out("dxp", ncols * 16), a["out_act"],
                                              a["phase"], st)
    elif kind == "conv":
        a = dict(F=32, rs=d["rs"], rows=rows)
        a.update(over)
        rc = L.dgg_ell_conv_bwd_partp_ext(ins["G"].addr, ins["H"].addr, a["rows"], K, a["F"], ws.data_ptr(), ncols, addr(a["rs"]), None,
                                          out("dA", rows * K), out("dA_rec", rows * K), out("dH", ncols * 32), out("da", ncols), st)
    else:
        ws2 = torch.full_like(ws, 0x5A)
        rc = L.dgg_partp_build_phase(d["idx"].addr, d["w"].addr, d["val"].addr, d["rs_rows"].addr, over.get("rows", rows), K, ncols, d["rs"].addr,
                                     out("ahat", rows * K) if "rows" in over else None, ws2.data_ptr(), 0, st)
        torch.cuda.synchronize()
        if not bool((ws2 == 0x5A).all().item()):
            return ["%s: the workspace was written" % name]
    torch.cuda.synchronize()
    bad = []
    if rc != want:
        bad.append("%s: status %d, expected %d" % (name, rc, want))
    if want != 0 and L.dgg_last_error().decode() == "":
        bad.append("%s: dgg_last_error() is empty" % name)
    for nm, gd in outs.items():
        if not (gd.read(nm) == 7.0).all():
            bad.append("%s: %s was written" % (name, nm))
    if not torch.equal(ws, ws_before):
        bad.append("%s: the partition was written" % name)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in REFUSALS if n != "null-dA-without-map"])
def test_refusals_and_empty_blocks_write_nothing(dev, name):
    bad = refusal(name, dev)
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    if "--knob-child" in sys.argv:
        sys.exit(_knob_child())
