"""The 64-record blocks of the backward walks of csrc/dgg_scatter.hip (conv_bwd_walk, edge_bwd_walk) and the trimmed second group of
edge_bwd_rows, on graphs whose in-degrees and row lengths sit at the edges of the new loops.

A wavefront of conv_bwd_node / edge_bwd_node loads up to 64 records of its node at once and then works on them in batches of
NPI = 64 / (F / 4) records: conv in gather groups of 4 batches (GROUP = 4 NPI records), the score walk in two groups of 32 records of
which only the batches that hold a record are run.  edge_bwd_rows runs, of each 32-entry group of a row, the batches up to the highest
live lane.  The graphs come from test_partitioned_backward.build_block with these in-degrees instead of its own:

    1, NPI-1, NPI, NPI+1, GROUP-1, GROUP, GROUP+1 (conv: 4 NPI; score: 32), 63, 64, 65, 127, 128, 129 (NODE_LONG), 193, 257 (long nodes
    whose quarters are cut inside a block), a hub that every row selects, and 0 for NODE 0 (the first read of a walk must not happen
    for it: its clamped index would be -1) as well as for a node inside and a node outside the row range

with both kinds of inactive entry, a dead row and a self loop.  Checks, references and bars are those of test_partitioned_backward
(tier 1: the integer construction, bit for bit, outputs between NaN fills and canaries; tier 2: 4 x the float32 restatement against
the float64 one); the score graphs add rows whose highest live lane is 0, 31, 32, 32 + NPI - 1, 32 + NPI and 63 and a row with an
idx = -1 hole below its last live entry.  The row kernel's outputs (row part of dxp, dk, rowinfo) are compared bit for bit with
tests/golden/backward_rows_parent.npz, recorded by tools/record_backward_rows.py from the library before the trim.
"""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_partitioned_backward as tpb  # noqa: E402
from test_partitioned_backward import Guard, K, NODE_LONG, build_block, ccase, check_profile, chunk_counts, positions, scase  # noqa: E402,F401

GOLDEN = os.path.join(tpb.ROOT, "tests", "golden", "backward_rows_parent.npz")
SHAPES = {
    "wave": dict(ncols=700, row0=0, rows=700),            # node 0 inside the row range
    "shard": dict(ncols=1100, row0=300, rows=511),        # node 0 outside it
    "chunked": dict(ncols=300, row0=0, rows=300),
}
SCORE_GROUP = 32


def npi(width):
    return 64 // (width // 4)


def walk_degrees(width, group):
    n = npi(width)
    return sorted(d for d in {1, n - 1, n, n + 1, group - 1, group, group + 1, 63, 64, 65, NODE_LONG - 1, NODE_LONG, NODE_LONG + 1, 193, 257} if d > 0)


@contextlib.contextmanager
def prescribed(degs):
    """build_block / check_profile of test_partitioned_backward with `degs` as the named in-degrees"""
    old = tpb.named_degrees
    tpb.named_degrees = lambda per: list(degs)
    try:
        yield
    finally:
        tpb.named_degrees = old


def block_with_empty_node0(shape, degs, cap, width, seed):
    """build_block with the in-degrees `degs`, then node 0 without a record: its label is exchanged with that of a node the block left
    without one (inside the row range when the rows start at 0, outside otherwise)"""
    with prescribed(degs):
        idx, act, info = build_block(shape, 0, cap, width, seed=seed)
    z = info["zero_in"] if shape["row0"] == 0 else info["zero_out"]
    assert z is not None and not (idx == z).any()
    assert shape["row0"] + info["selfrow"] != 0, "node 0 is the self loop"
    idx = np.where(idx == 0, np.int32(z), idx).astype(np.int32)
    if info["hub"] == 0:
        info["hub"] = z
    info["named"] = {d: (z if j == 0 else j) for d, j in info["named"].items()}
    info["zero_in" if shape["row0"] == 0 else "zero_out"] = 0
    return idx, act, info


# ---------------------------------------------------------------------------------------------------------------
# tier 1: conv backward
# ---------------------------------------------------------------------------------------------------------------
CONV = [ccase("wave", 16), ccase("wave", 16, ext=True, phase=1), ccase("wave", 32, phase=1), ccase("wave", 32, ext=True), ccase("wave", 64),
        ccase("wave", 64, ext=True, phase=1), ccase("wave", 128), ccase("wave", 128, ext=True), ccase("shard", 64, ext=True), ccase("shard", 32),
        ccase("shard", 128, phase=1), ccase("chunked", 64)]


@functools.lru_cache(maxsize=32)
def conv_inputs(cid):
    """test_partitioned_backward.conv_inputs for the cases above: same integer construction, the in-degrees of walk_degrees"""
    c = next(c for c in CONV if c["id"] == cid)
    shape, F = SHAPES[c["shape"]], c["F"]
    ncols, rows = shape["ncols"], shape["rows"]
    rng = np.random.default_rng(2000 + F + c["seed"])
    width, kdeg = None, None
    if c["shape"] == "chunked":
        kdeg = rng.uniform(3.0, 130.0, rows).astype(np.float32)
        width = 64 * chunk_counts(kdeg)
        cap = np.minimum(np.ceil(kdeg + 8.5).astype(np.int64), width)
    else:
        cap = rng.integers(1, 65, rows)
    degs = walk_degrees(F, 4 * npi(F))
    idx, act, info = block_with_empty_node0(shape, degs, cap, width, seed=c["seed"] + F)
    w = np.where(act, rng.integers(1, 3, idx.shape), 0).astype(np.float32)
    val = rng.integers(1, 9, idx.shape).astype(np.float32)
    rs = rng.choice(np.array([1.0, 4.0], np.float32), ncols)
    G = rng.integers(-2, 3, (rows, F)).astype(np.float32)
    H = rng.integers(-2, 3, (ncols, F)).astype(np.float32)
    ext = np.where(act, rng.integers(-2, 3, idx.shape), np.nan).astype(np.float32) if c["ext"] else None
    pos, cptr = positions(info["width"])
    return dict(c=c, shape=shape, idx=idx, act=act, info=info, w=w, val=val, rs=rs, G=G, H=H, ext=ext, pos=pos, cptr=cptr, kdeg=kdeg, degs=degs)


def test_conv_graphs_hold_the_block_edges():
    for c in CONV:
        x = conv_inputs(c["id"])
        ok, worst = tpb.premises_hold(x)
        assert ok, "%s: %r" % (c["id"], worst)
        with prescribed(x["degs"]):
            check_profile(x["shape"], x["idx"], x["act"], x["info"], 0)
        assert x["info"]["degs"] == x["degs"], "%s: an in-degree did not fit the block" % c["id"]
        indeg = np.bincount(x["idx"][x["act"]], minlength=x["shape"]["ncols"])
        assert indeg[0] == 0 and not (x["idx"] == 0).any()
        if c["shape"] == "chunked":
            assert x["pos"].shape[1] > K and x["info"]["width"].max() >= 130


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("c", CONV, ids=[c["id"] for c in CONV])
def test_conv_backward_blocks_bit_for_bit(dev, c, monkeypatch):
    """dA, dA_rec, dH, da (and the dA = NULL form through the map, and partp_gather) are the integer reference exactly"""
    monkeypatch.setattr(tpb, "conv_inputs", conv_inputs)
    bad = tpb.check_conv(dev, c)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# tier 2: score backward
# ---------------------------------------------------------------------------------------------------------------
SCORE = [scase("wave", 16, 0, 1, 1, 0), scase("wave", 32, 0, 0, 1, 1), scase("wave", 64, 0, 1, 0, 0), scase("wave", 128, 0, 0, 0, 1),
         scase("shard", 64, 0, 1, 1, 1), scase("shard", 32, 0, 1, 0, 0), scase("shard", 16, 0, 0, 1, 1), scase("wave", 128, 0, 1, 1, 0),
         scase("wave", 64, 0, 0, 1, 1), scase("chunked", 64, 0, 1, 1, 1)]


def top_lanes(h):
    return [0, 31, 32, 32 + npi(h) - 1, 32 + npi(h), 63]


def degree_with_cap(n):
    """a learned degree k whose ramp 1 - 0.5 (1 + tanh(r - k)) is non-zero in float32 on exactly the ranks r < n"""
    for step in range(0, 200):
        k = np.array([n - 9.5 + 0.01 * step], np.float32)
        if int(tpb.ramp_cap(k, K)[0]) == n:
            return float(k[0])
    raise AssertionError("no degree gives %d ranks" % n)


@functools.lru_cache(maxsize=4)
def score_graph(shape_name, h, perturb, mode, out_act):
    """test_partitioned_backward.score_graph with the in-degrees of walk_degrees, node 0 without a record and, on the plain 64-rank
    list, rows whose highest live lane is one of top_lanes(h) (rows[-8:-2], by their degree) and a row with a hole below its last live
    entry (info['hole'])"""
    import ctypes as C
    from oracle import oracle as O
    shape = SHAPES[shape_name]
    ncols, row0, rows = shape["ncols"], shape["row0"], shape["rows"]
    rng = np.random.default_rng(9000 + 10 * h + 2 * perturb + mode + ncols + rows)
    xp = (rng.standard_normal((ncols, h)) * 0.6).astype(np.float32)
    if out_act:
        xp[rng.integers(0, ncols, 40), rng.integers(0, h, 40)] = 0.0
    chunked = shape_name == "chunked"
    k = rng.uniform(3.0, 130.0 if chunked else 40.0, rows).astype(np.float32)
    tops = {}
    if not chunked:
        for q, lane in enumerate(top_lanes(h)):
            tops[rows - 8 + q] = lane
            k[rows - 8 + q] = degree_with_cap(lane + 1)
    width = 64 * chunk_counts(k) if chunked else np.full(rows, K, np.int64)
    cap = np.minimum(tpb.ramp_cap(k, int(width.max())), width)
    degs = walk_degrees(h, SCORE_GROUP)
    idx, act, info = block_with_empty_node0(shape, degs, cap, width, seed=h + perturb)
    # a hole: an active entry of an ordinary column, below the row's last live entry, becomes idx = -1
    named = set([info["hub"]] + list(info["named"].values()))
    hole = None
    for i in range(rows):
        if cap[i] >= 12 and i not in tops and i not in (info["dead"], info["selfrow"]) and int(idx[i, 5]) not in named:
            hole = (i, 5)
            break
    assert hole is not None
    idx[hole] = -1
    L = O.lib()
    val = np.zeros(idx.shape, np.float32)
    gum = rng.gumbel(size=idx.shape).astype(np.float32)
    base = xp.ctypes.data
    for i, r in zip(*np.nonzero(idx >= 0)):
        val[i, r] = L.ora_pair_score(C.c_void_p(base + 4 * h * (row0 + int(i))), C.c_void_p(base + 4 * h * int(idx[i, r])), C.c_int(h),
                                     C.c_float(tpb.T_DIST), C.c_int(perturb), C.c_float(float(gum[i, r])))
    w, rs_rows = O.softk(idx, val, k, mode=mode)
    act[hole] = False
    assert np.array_equal((idx >= 0) & (w != 0), act)
    rs = rng.uniform(2.0, 20.0, ncols).astype(np.float32)
    rs[row0:row0 + rows] = rs_rows
    if row0 == 0:
        # the dead row's node took over the records of node 0 (block_with_empty_node0): as a DESTINATION it needs a row sum, and its
        # own row has none -- a stand-in like those of the nodes outside the block (both sides of the comparison read the same rs)
        assert rs[info["dead"]] == 0
        rs[info["dead"]] = np.float32(5.0)
    r32 = np.arange(idx.shape[1], dtype=np.float32)[None, :] - k[:, None]
    th32 = np.vectorize(O.tanh, otypes=[np.float32])(r32)
    F = 32
    pos, cptr = positions(width)
    info = dict(info, hole=hole, tops=tops)
    return dict(shape=shape, idx=idx, act=act, info=info, val=val, w=w, rs=rs, k=k, xp=xp, th32=th32, th64=np.tanh(r32.astype(np.float64)),
                G=rng.standard_normal((rows, F)).astype(np.float32), H=rng.standard_normal((ncols, F)).astype(np.float32),
                dw=rng.standard_normal(idx.shape).astype(np.float32), pos=pos, cptr=cptr, width=width, degs=degs)


def test_score_graphs_hold_the_block_edges_and_row_lengths():
    for c in (SCORE[2], SCORE[4], SCORE[9]):
        g = score_graph(c["shape"], c["h"], c["perturb"], c["mode"], c["out_act"])
        with prescribed(g["degs"]):
            check_profile(g["shape"], g["idx"], g["act"], g["info"], 0)
        assert g["info"]["degs"] == g["degs"]
        assert np.bincount(g["idx"][g["act"]], minlength=g["shape"]["ncols"])[0] == 0
        i, r = g["info"]["hole"]
        assert g["idx"][i, r] == -1 and g["act"][i, r + 1:].any()
        live_top = np.where(g["act"].any(1), g["act"].shape[1] - 1 - np.argmax(g["act"][:, ::-1], axis=1), -1)
        for row, lane in g["info"]["tops"].items():
            assert live_top[row] == lane, "row %d: highest live lane %d, wanted %d" % (row, live_top[row], lane)
        assert live_top[g["info"]["dead"]] == -1
        if c["shape"] != "chunked":
            assert sorted(g["info"]["tops"].values()) == sorted(top_lanes(c["h"]))


@pytest.mark.gpu
@pytest.mark.parametrize("c", SCORE, ids=[c["id"] for c in SCORE])
def test_score_backward_blocks_within_four_times_the_float32_restatement(dev, c, monkeypatch):
    """max|got - ref| / max|ref| of dxp and dk <= 4 x the larger error of restate(np.float32) in row order and in shuffled order,
    both against restate(np.float64); phases, dA = NULL and NaN-masked dA give the same bits (check_score)"""
    monkeypatch.setattr(tpb, "score_graph", score_graph)
    bad = tpb.check_score(dev, c)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# the row kernel, bit for bit against the library before the trim
# ---------------------------------------------------------------------------------------------------------------
ROWS_CASE = scase("whole120", 64, 0, 1, 1, 0)


def rows_phase_outputs(dev):
    """phase 1 of the score backward (edge_bwd_rows) on the seeded whole120 graph, h = 64, with HOST-made cotangents (dA by rows, the
    neighbour-side da): nothing the row kernel reads depends on the record order of the partition -> dict(dxp_rows, dk, rowinfo)"""
    c = ROWS_CASE
    g = tpb.score_graph(c["shape"], c["h"], c["perturb"], c["mode"], c["out_act"])
    d = tpb.build_partition(dev, g)
    d["xp"], d["k"] = Guard(dev, g["xp"], np.nan), Guard(dev, g["k"], np.nan)
    rng = np.random.default_rng(64)
    rows, ncols, row0 = g["shape"]["rows"], g["shape"]["ncols"], g["shape"]["row0"]
    dA = np.where(g["act"], rng.standard_normal(g["idx"].shape), np.nan).astype(np.float32)      # (inactive slots: never written by the conv kernel)
    da = rng.standard_normal(ncols).astype(np.float32)
    gdA, gda = Guard(dev, dA.ravel(), np.nan), Guard(dev, da, np.nan)
    grec, gah = Guard(dev, np.zeros(rows * K, np.float32), np.nan), Guard(dev, d["ahat"].cpu().numpy(), np.nan)
    rc, dxp, dk, state = tpb.edge_call(dev, g, c, d, gdA, grec, gda, gah, phase=1)
    assert rc == 0
    rowinfo = state[2].read("rowinfo").reshape(rows, 4)
    live = int((g["act"].sum(1) > 32).sum())
    assert live >= 10 and (g["act"].sum(1) <= 32).sum() >= 10, "the graph must hold rows on both sides of the second group"
    return dict(dxp_rows=dxp[row0:row0 + rows], dk=dk, rowinfo=rowinfo)


@pytest.mark.gpu
def test_row_kernel_outputs_are_the_recorded_ones_bit_for_bit(dev):
    got = rows_phase_outputs(dev)
    ref = np.load(GOLDEN)
    for name in ("dxp_rows", "dk", "rowinfo"):
        a, b = got[name], ref[name]
        assert a.shape == b.shape and a.dtype == b.dtype, name
        same = a.view(np.uint32) == b.view(np.uint32)
        assert same.all(), "%s: %d of %d words differ from the recording, first at flat index %d" % (
            name, int((~same).sum()), same.size, int(np.flatnonzero(~same.ravel())[0]))
