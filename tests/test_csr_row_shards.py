"""The row-range (_rows) forms of the CSR adjacency kernels (csrc/dgg_csr.hip) against the full-graph entries they slice.

A row shard owns rows [r0, r1) of an [N, N] pattern and hands them in as a rebased slice (rowptr from 0, global columns); local row i is
node r0 + i, and that id indexes the per-node tables and keys the hash noise.  Everything here goes through the C ABI in one process.

Graph (shard_graph): seeded, N = 517, unique ascending columns, rows of 1, 2, 63, 64, 65, 127, 128, 129, 200 and `all` candidates placed
on both sides of every cut of the ranges below, a hub column every row lists, a self loop on every third row.  A row that lists all N
columns and a node that no row lists exclude each other, so the one seed has the two forms of tests/test_csr_adjacency.py: `full` (the
`all` row has N candidates; used for every overwritten output) and `unlisted` (node 300 is listed by nobody and the `all` row has N - 1;
used for the accumulated outputs, where that node's row of dX must keep its bits).
Ranges: (0, N), (0, 1), (N-1, N), (130, 131), (64, 259), the empty (259, 259) and the partition (0, 173), (173, 346), (346, N).
Outputs are NaN-filled (int32: -7777) between canary words, inputs and per-node tables sit between guards (Ctx / Guard of the sibling).

Overwritten outputs (p, w, pp, pos, ahat, dw, and through the reused entries rs, Y, dA, dp, dk): every range equals the matching slice of
the full-graph entry bit for bit -- HASH and HASH_SYM noise with a fixed seed included, which is what proves that the noise is keyed on
the global pair.  dgg_csr_norm_bwd_apply_rows reads the SUMMED workspace: the one the full-graph dgg_csr_norm_bwd leaves behind.
Accumulated outputs (dxp, dX, da_ws), tier 1: operands on a power-of-two grid, so every partial sum is exact
(test_exactness_premises_hold proves it on the CPU): the three-way partition accumulated into one buffer equals the full-graph call and
the float64 sum bit for bit.  Tier 2: standard-normal data against the float64 restatements of the sibling; the partition's error may be
at most 4 x the error of the existing full-graph entry on the same data.  Both are float atomics over the same terms in an order the
hardware chooses, so the entry's error is not one number: its worst element is the hub (517 terms of mixed sign in one word), and two
runs of the SAME full-graph call on the same data gave 1.03e-07 and 1.84e-07 for da_ws.  The test therefore calls the full-graph entry
three times and takes the largest of the three errors as "the error of the full-graph entry"; the partition is measured once.

Measured on an MI355X (max|got - ref| / max|ref|; nothing is fixed here, the bar is computed in the test from the `full` column; two
runs with ONE call of the full-graph entry each, before the three calls were introduced -- in the first the partition's da_ws missed the
single-call bar, 4.70e-07 against 4.11e-07, with both worst elements at the hub):

  output                      full entry   bar = 4x    partition
  uvdist_bwd dxp h=16           4.56e-07   1.82e-06    4.01e-07
  spmm_bwd dX F=65              1.10e-06   4.40e-06    5.46e-07
  norm_bwd da_ws                1.84e-07   7.38e-07    3.88e-07
  norm_bwd da_ws (other run)    1.03e-07   4.11e-07    4.70e-07
  with three calls of the full-graph entry (their errors; the largest sets the bar):
  uvdist_bwd dxp h=16           4.56e-07 4.56e-07 3.69e-07   1.82e-06    3.92e-07
  spmm_bwd dX F=65              6.97e-07 7.65e-07 4.13e-07   3.06e-06    4.46e-07
  norm_bwd da_ws                1.84e-07 2.66e-07 1.84e-07   1.07e-06    6.34e-07
The 12 GPU tests of this module take 3 s.
"""
import functools

import numpy as np
import pytest

from test_csr_adjacency import (ERR_ARG, EXACT_LIMIT, F32, Ctx, dev, expect, norm_bwd_exact, orders, rel_max, restate_spmm_bwd,  # noqa: F401
                                restate_uvdist_bwd, same, spmm_bwd_exact, untouched)

N = 517
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
PARTITION = ((0, 173), (173, 346), (346, N))
RANGES = ((0, N), (0, 1), (N - 1, N), (130, 131), (64, 259), (259, 259)) + PARTITION
UNLISTED = 300
SEED = (20240607, 99)
T_DIST = float(F32(-0.05))
NOISE_NONE, NOISE_EXPLICIT, NOISE_HASH, NOISE_HASH_SYM = 0, 1, 2, 3
UV_H = (16, 129)                      # both branches of the canonical distance
F_SPMM = 65


@functools.lru_cache(maxsize=None)
def shard_graph(full=True):
    rng = np.random.default_rng(517)
    place = {129: 0, 1: 1, 63: 63, 64: 64, 200: 130, 2: 172, 65: 173, 127: 258, "all": 259, 128: 345, "1b": 346, "64b": N - 1}
    length = rng.integers(1, 25, N)
    for name, row in place.items():
        length[row] = {"all": N, "1b": 1, "64b": 64}.get(name, name)
    hub = 261
    allowed = np.arange(N) if full else np.setdiff1d(np.arange(N), [UNLISTED])
    length = np.minimum(length, len(allowed))
    cols = []
    for i in range(N):
        n = int(length[i])
        must = [hub] + ([i] if (i % 3 == 0 and n >= 2 and i in allowed and i != hub) else [])
        rest = rng.permutation(np.setdiff1d(allowed, must))[:n - len(must)]
        cols.append(np.sort(np.concatenate([np.array(must, np.int64), rest]).astype(np.int64)))
    rowptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    return dict(rowptr=rowptr, col=np.concatenate(cols).astype(np.int32), erow=np.repeat(np.arange(N), length), N=N, E=int(rowptr[-1]),
                named=place, hub=hub, full=full)


def cut(g, r0, r1):
    """the rebased slice a row shard passes -> (rowptr_loc, col_loc, e0, e1)"""
    e0, e1 = int(g["rowptr"][r0]), int(g["rowptr"][r1])
    return (g["rowptr"][r0:r1 + 1] - e0).astype(np.int64), g["col"][e0:e1], e0, e1


def test_graph_has_every_row_length_and_the_ranges_cut_between_named_rows():
    for full in (True, False):
        g = shard_graph(full)
        cnt = np.diff(g["rowptr"])
        for L in LENGTHS:
            assert cnt[g["named"][L]] == L
        assert cnt[g["named"]["all"]] == (N if full else N - 1)
        for i in range(N):
            c = g["col"][g["rowptr"][i]:g["rowptr"][i + 1]]
            assert (np.diff(c) > 0).all() and 0 <= c[0] and c[-1] < N and g["hub"] in c
        listed = np.bincount(g["col"], minlength=N)
        assert (listed[UNLISTED] == 0) == (not full) and (np.delete(listed, UNLISTED) > 0).all()
        assert sum(int(i in g["col"][g["rowptr"][i]:g["rowptr"][i + 1]]) for i in range(N)) > 100          # self loops
    # a named row on each side of every cut, single-row ranges on named rows, the partition covers every row once
    rows = set(shard_graph()["named"].values())
    for r0, r1 in RANGES:
        assert r0 == r1 or (r0 in rows and r1 - 1 in rows), (r0, r1)
    assert PARTITION[0][0] == 0 and PARTITION[-1][1] == N and all(a[1] == b[0] for a, b in zip(PARTITION, PARTITION[1:]))
    rp, cl, e0, e1 = cut(shard_graph(), 259, 259)
    assert rp.tolist() == [0] and len(cl) == 0 and e0 == e1


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_inputs():
    g = shard_graph(True)
    rng = np.random.default_rng(1)
    E = g["E"]
    p = (0.05 + 0.9 * rng.random(E)).astype(F32)
    p[rng.random(E) < 0.03] = 0.0
    a = int(g["rowptr"][g["named"][129]])
    p[a + 60:a + 71] = F32(0.625)                                       # ties across the 64-entry chunk boundary
    k = rng.uniform(-2.0, 40.0, N).astype(F32)
    for name in (200, "all", 129, 65):
        k[g["named"][name]] = F32(rng.uniform(60.0, 220.0))             # learned degrees beyond the 64-rank list
    w = (0.05 + rng.random(E)).astype(F32)
    dA = rng.standard_normal(E).astype(F32)
    X = rng.standard_normal((N, F_SPMM)).astype(F32)
    dY = rng.standard_normal((N, F_SPMM)).astype(F32)
    gr = rng.standard_normal(E).astype(F32)
    xp = {h: (0.6 * rng.standard_normal((N, h))).astype(F32) for h in UV_H}
    assert (p >= 0).all() and not np.signbit(p).any()                   # the ranking precondition: values >= +0.0
    return dict(g=g, p=p, k=k, w=w, dA=dA, X=X, dY=dY, gr=gr, xp=xp)


@pytest.fixture(scope="module")
def full_outputs(dev):
    """every full-graph entry once: the bits the slices must reproduce"""
    x = forward_inputs()
    g, E = x["g"], x["g"]["E"]
    c = Ctx(dev)
    rp, cl = c.graph(g)
    out = {}
    for h in UV_H:
        pe = c.out(E)
        assert c.call("dgg_csr_uvdist_fwd", c.inp(x["xp"][h]), rp, cl, N, h, T_DIST, pe) == 0
        out["p", h] = pe.read()
    gp, gk = c.inp(x["p"]), c.inp(x["k"])
    for nm in (NOISE_NONE, NOISE_HASH, NOISE_HASH_SYM):
        for mode in (0, 1):
            w, pp, pos = c.out(E), c.out(E), c.out(E, np.int32)
            assert c.call("dgg_csr_softk_fwd", gp, rp, cl, N, gk, nm, None, 0, SEED[0], SEED[1], mode, w, pp, pos) == 0
            out["softk", nm, mode] = (w.read(), pp.read(), pos.read())
            dp, dk = c.out(E), c.out(N)
            assert c.call("dgg_csr_softk_bwd", gp, c.inp(out["softk", nm, mode][1]), rp, N, gk, c.inp(out["softk", nm, mode][2]), int(nm != 0),
                          mode, c.inp(x["gr"]), dp, dk) == 0
            out["softk_bwd", nm, mode] = (dp.read(), dk.read())
    gw = c.inp(x["w"])
    rs = c.out(N)
    assert c.call("dgg_csr_row_sum", gw, rp, N, rs) == 0
    out["rs"] = rs.read()
    assert (out["rs"] > 0).all()                                         # the normalisation's precondition: positive on every named node
    grs, ahat = c.inp(out["rs"]), c.out(E)
    assert c.call("dgg_csr_normalize_fwd", rp, cl, gw, grs, N, ahat) == 0
    out["ahat"] = ahat.read()
    da, dw = c.out(N, start=np.zeros(N, F32)), c.out(E)
    assert c.call("dgg_csr_norm_bwd", rp, cl, gw, grs, c.inp(x["dA"]), N, da, dw) == 0
    out["da"], out["dw"] = da.read(), dw.read()
    Y, dAo = c.out((N, F_SPMM)), c.out(E)
    ga, gX = c.inp(out["ahat"]), c.inp(x["X"])
    assert c.call("dgg_csr_spmm_fwd", rp, cl, ga, gX, N, F_SPMM, Y) == 0
    assert c.call("dgg_csr_spmm_bwd", rp, cl, ga, gX, c.inp(x["dY"]), N, F_SPMM, dAo, None) == 0
    out["Y"], out["spmm_dA"] = Y.read(), dAo.read()
    c.inputs_intact()
    return out


# ---------------------------------------------------------------------------------------------------------------
# overwritten outputs: every range is the slice of the full-graph entry, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r0,r1", RANGES, ids=["rows%d-%d" % r for r in RANGES])
def test_every_range_is_the_slice_of_the_full_graph_entry(dev, full_outputs, r0, r1):
    x, full = forward_inputs(), full_outputs
    g = x["g"]
    rp_h, cl_h, e0, e1 = cut(g, r0, r1)
    n, El = r1 - r0, e1 - e0
    c, bad = Ctx(dev), []
    rp, cl = c.inp(rp_h), c.inp(cl_h)
    for h in UV_H:
        pe = c.out(El)
        assert c.call("dgg_csr_uvdist_fwd_rows", c.inp(x["xp"][h]), rp, cl, r0, n, N, h, T_DIST, pe) == 0
        expect(bad, "uvdist_fwd_rows h=%d" % h, pe, full["p", h][e0:e1])
    gp, gk, ggr = c.inp(x["p"][e0:e1]), c.inp(x["k"][r0:r1]), c.inp(x["gr"][e0:e1])
    for nm in (NOISE_NONE, NOISE_HASH, NOISE_HASH_SYM):
        for mode in (0, 1):
            w, pp, pos = c.out(El), c.out(El), c.out(El, np.int32)
            assert c.call("dgg_csr_softk_fwd_rows", gp, rp, cl, r0, n, N, gk, nm, SEED[0], SEED[1], mode, w, pp, pos) == 0
            fw, fpp, fpos = full["softk", nm, mode]
            for name, gd, ref in (("w", w, fw), ("pp", pp, fpp), ("pos", pos, fpos)):
                expect(bad, "softk_fwd_rows noise=%d mode=%d %s" % (nm, mode, name), gd, ref[e0:e1])
            # the reused entry on the slice (no row index reaches a table or a hash in it): N = n
            dp, dk = c.out(El), c.out(n)
            assert c.call("dgg_csr_softk_bwd", gp, c.inp(fpp[e0:e1]), rp, n, gk, c.inp(fpos[e0:e1]), int(nm != 0), mode, ggr, dp, dk) == 0
            expect(bad, "softk_bwd on the slice noise=%d mode=%d dp" % (nm, mode), dp, full["softk_bwd", nm, mode][0][e0:e1])
            expect(bad, "softk_bwd on the slice noise=%d mode=%d dk" % (nm, mode), dk, full["softk_bwd", nm, mode][1][r0:r1])
    gw, grs, gdA = c.inp(x["w"][e0:e1]), c.inp(full["rs"]), c.inp(x["dA"][e0:e1])
    rs = c.out(n)
    assert c.call("dgg_csr_row_sum", gw, rp, n, rs) == 0                 # (reused on the slice)
    expect(bad, "row_sum on the slice", rs, full["rs"][r0:r1])
    ahat = c.out(El)
    assert c.call("dgg_csr_normalize_fwd_rows", rp, cl, gw, grs, r0, n, N, ahat) == 0
    expect(bad, "normalize_fwd_rows", ahat, full["ahat"][e0:e1])
    dw = c.out(El)
    assert c.call("dgg_csr_norm_bwd_apply_rows", rp, cl, grs, gdA, c.inp(full["da"]), r0, n, N, dw) == 0      # (the SUMMED workspace)
    expect(bad, "norm_bwd_apply_rows", dw, full["dw"][e0:e1])
    ga, gX = c.inp(full["ahat"][e0:e1]), c.inp(x["X"])
    Y, dAo = c.out((n, F_SPMM)), c.out(El)
    assert c.call("dgg_csr_spmm_fwd", rp, cl, ga, gX, n, F_SPMM, Y) == 0                                       # (reused on the slice)
    assert c.call("dgg_csr_spmm_bwd", rp, cl, ga, gX, c.inp(x["dY"][r0:r1]), n, F_SPMM, dAo, None) == 0
    expect(bad, "spmm_fwd on the slice", Y, full["Y"][r0:r1])
    expect(bad, "spmm_bwd dA on the slice", dAo, full["spmm_dA"][e0:e1])
    c.inputs_intact()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# accumulated outputs
# ---------------------------------------------------------------------------------------------------------------
UV_UNIT = 2.0 ** -6
T_EXACT = -0.5


@functools.lru_cache(maxsize=None)
def exact_case():
    """operands on a power-of-two grid: xp_i = s_i u with s_i in {0, 1, 2} and ||u||^2 = 16, so a distance is 0, 4 or 8; p in {1, 1/2},
    dp small integers, t = -1/2: g = dp p t in 1/4 units, coef = g / dist in 2^-5 units, every term coef (x_i - x_j) in 2^-4 units"""
    g = shard_graph(False)
    rng = np.random.default_rng(7)
    E, h = g["E"], 16
    u = np.zeros(h, F32)
    u[[0, 5, 10, 15]] = 2.0
    s = rng.integers(0, 3, N).astype(F32)
    uv = dict(xp=s[:, None] * u[None, :], p=rng.choice(np.array([1.0, 0.5], F32), E), dp=rng.integers(-3, 4, E).astype(F32),
              dxp0=rng.integers(-5, 6, (N, h)).astype(F32), h=h)
    sp = dict(g=g, a=rng.integers(-3, 4, E).astype(F32), X=rng.integers(-3, 4, (N, 33)).astype(F32), dY=rng.integers(-3, 4, (N, 33)).astype(F32),
              dX0=rng.integers(-5, 6, (N, 33)).astype(F32))
    nb = dict(g=g, rs=rng.choice(np.array([1.0, 4.0, 16.0], F32), N), w=rng.integers(1, 3, E).astype(F32), dA=rng.integers(-3, 4, E).astype(F32))
    return g, uv, sp, nb


def uvdist_bwd_exact(g, uv):
    """-> dxp in float64, and whether every term is a whole number of units with the sums of magnitudes below 2^24 units"""
    i, j = g["erow"], g["col"].astype(np.int64)
    x = uv["xp"].astype(np.float64)
    d = x[i] - x[j]
    dist = np.sqrt((d * d).sum(1))
    gg = uv["dp"].astype(np.float64) * uv["p"].astype(np.float64) * T_EXACT
    coef = np.where(dist > 0, gg / np.where(dist > 0, dist, 1.0), 0.0)
    v = coef[:, None] * d
    dxp, ab = uv["dxp0"].astype(np.float64), np.abs(uv["dxp0"]).astype(np.float64)
    for keys, sign in ((i, 1.0), (j, -1.0)):
        np.add.at(dxp, keys, sign * v)
        np.add.at(ab, keys, np.abs(v))
    whole = all(np.array_equal(q / UV_UNIT, np.round(q / UV_UNIT)) for q in (gg, coef, v)) and set(np.unique(dist)) <= {0.0, 4.0, 8.0}
    return dxp, whole and ab.max() / UV_UNIT < EXACT_LIMIT


def test_exactness_premises_hold():
    g, uv, sp, nb = exact_case()
    assert uvdist_bwd_exact(g, uv)[1]
    assert spmm_bwd_exact(sp)[2]
    assert norm_bwd_exact(nb)[2]


def accumulate(c, g, ranges, call):
    """runs `call(rp, cl, r0, n, e0, e1)` for every range"""
    for r0, r1 in ranges:
        rp_h, cl_h, e0, e1 = cut(g, r0, r1)
        assert call(c.inp(rp_h), c.inp(cl_h), r0, r1 - r0, e0, e1) == 0


def accumulated_outputs(dev, g, uv, sp, nb, t, full_calls=1):
    """dxp, dX, da_ws by the full-graph entries (`full_calls` times) and by the three-way partition accumulated into one buffer each"""
    c = Ctx(dev)
    E, h, F = g["E"], uv["xp"].shape[1], sp["X"].shape[1]
    gxp, gX, grs = c.inp(uv["xp"]), c.inp(sp["X"]), c.inp(nb["rs"])
    rp, cl = c.graph(g)
    got = {"full_calls": []}
    for _ in range(full_calls):
        dxp, dX, da = c.out((N, h), start=uv["dxp0"]), c.out((N, F), start=sp["dX0"]), c.out(N, start=np.zeros(N, F32))
        assert c.call("dgg_csr_uvdist_bwd", gxp, rp, cl, N, h, t, c.inp(uv["p"]), c.inp(uv["dp"]), dxp) == 0
        assert c.call("dgg_csr_spmm_bwd", rp, cl, c.inp(sp["a"]), gX, c.inp(sp["dY"]), N, F, c.out(E), dX) == 0
        assert c.call("dgg_csr_norm_bwd", rp, cl, c.inp(nb["w"]), grs, c.inp(nb["dA"]), N, da, c.out(E)) == 0
        got["full_calls"].append((dxp.read("dxp"), dX.read("dX"), da.read("da_ws")))
    got["full"] = got["full_calls"][0]
    dxp, dX, da = c.out((N, h), start=uv["dxp0"]), c.out((N, F), start=sp["dX0"]), c.out(N, start=np.zeros(N, F32))
    accumulate(c, g, PARTITION, lambda rp_, cl_, r0, n, e0, e1: c.call(
        "dgg_csr_uvdist_bwd_rows", gxp, rp_, cl_, r0, n, N, h, t, c.inp(uv["p"][e0:e1]), c.inp(uv["dp"][e0:e1]), dxp))
    accumulate(c, g, PARTITION, lambda rp_, cl_, r0, n, e0, e1: c.call(
        "dgg_csr_spmm_bwd", rp_, cl_, c.inp(sp["a"][e0:e1]), gX, c.inp(sp["dY"][r0:r0 + n]), n, F, c.out(e1 - e0), dX))
    accumulate(c, g, PARTITION, lambda rp_, cl_, r0, n, e0, e1: c.call(
        "dgg_csr_norm_bwd_acc_rows", rp_, cl_, c.inp(nb["w"][e0:e1]), grs, c.inp(nb["dA"][e0:e1]), r0, n, N, da))
    got["partition"] = (dxp.read("dxp"), dX.read("dX"), da.read("da_ws"))
    c.inputs_intact()
    return got


@pytest.mark.gpu
def test_the_partition_accumulates_to_the_full_graph_call_exactly(dev):
    g, uv, sp, nb = exact_case()
    got = accumulated_outputs(dev, g, uv, sp, nb, T_EXACT)
    ref = (uvdist_bwd_exact(g, uv)[0], spmm_bwd_exact(sp)[1], norm_bwd_exact(nb)[0])
    bad = []
    for q, name in enumerate(("dxp", "dX", "da_ws")):
        for who in ("full", "partition"):
            if not same(got[who][q], ref[q]):
                bad.append("%s of the %s differs from the exact sum" % (name, who))
        if not np.array_equal(got["full"][q], got["partition"][q]):
            bad.append("%s: partition and full-graph call differ" % name)
    assert not bad, "\n".join(bad)


def restate_norm_da(g, w, rs, dA):
    i, j = g["erow"], g["col"].astype(np.int64)
    a = 1.0 / np.sqrt(rs.astype(np.float64))
    gg = dA.astype(np.float64) * w.astype(np.float64)
    da = np.zeros(g["N"])
    np.add.at(da, i, gg * a[j])
    np.add.at(da, j, gg * a[i])
    return da


@pytest.mark.gpu
def test_the_partition_on_normal_data_within_four_times_the_full_graph_entrys_error(dev):
    g = shard_graph(False)
    rng = np.random.default_rng(11)
    E, h, F = g["E"], 16, 65
    xp = (0.6 * rng.standard_normal((N, h))).astype(F32)
    i, j = g["erow"], g["col"].astype(np.int64)
    pe = np.exp(T_DIST * np.sqrt(((xp[i] - xp[j]).astype(np.float64) ** 2).sum(1))).astype(F32)
    uv = dict(xp=xp, p=pe, dp=rng.standard_normal(E).astype(F32), dxp0=rng.standard_normal((N, h)).astype(F32))
    sp = dict(a=rng.standard_normal(E).astype(F32), X=rng.standard_normal((N, F)).astype(F32), dY=rng.standard_normal((N, F)).astype(F32),
              dX0=rng.standard_normal((N, F)).astype(F32))
    nb = dict(rs=(1.0 + 10 * rng.random(N)).astype(F32), w=(0.1 + rng.random(E)).astype(F32), dA=rng.standard_normal(E).astype(F32))
    assert (nb["rs"] > 0).all()
    got = accumulated_outputs(dev, g, uv, sp, nb, T_DIST, full_calls=3)
    o = orders(E, 5)[0]
    ref = (restate_uvdist_bwd(np.float64, g, uv["xp"], uv["p"], uv["dp"], uv["dxp0"], o),
           restate_spmm_bwd(np.float64, g, sp["a"], sp["X"], sp["dY"], sp["dX0"], o)[1], restate_norm_da(g, nb["w"], nb["rs"], nb["dA"]))
    bad = []
    for q, name in enumerate(("uvdist_bwd dxp h=%d" % h, "spmm_bwd dX F=%d" % F, "norm_bwd da_ws")):
        assert np.isfinite(got["partition"][q]).all() and np.isfinite(got["full"][q]).all()
        efs = [rel_max(f[q], ref[q]) for f in got["full_calls"]]         # (float atomics: the entry's error moves from call to call)
        ef, ep = max(efs), rel_max(got["partition"][q], ref[q])
        worst = [int(np.abs(got[who][q].astype(np.float64) - ref[q]).reshape(N, -1).max(1).argmax()) for who in ("full", "partition")]
        print("  %-28s %10.2e %10.2e %10.2e   (full-graph calls: %s; worst node: full %d, partition %d; hub %d)" % (
            name, ef, 4 * ef, ep, " ".join("%.2e" % e for e in efs), worst[0], worst[1], g["hub"]))
        if ep > 4 * ef:
            bad.append("%s: partition %.3e above 4 x the full-graph entry's %.3e" % (name, ep, ef))
    # the node nobody lists: no entry names it as a column, so its row of dX keeps the start value's bits
    own = sp["dX0"][UNLISTED]
    assert np.array_equal(got["partition"][1][UNLISTED], own) and np.array_equal(got["full"][1][UNLISTED], own)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# refusals and empty ranges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_return_their_code_and_write_nothing(dev):
    x = forward_inputs()
    g, E, h = x["g"], x["g"]["E"], 16
    c = Ctx(dev)
    rp, cl = c.graph(g)
    gp, gk, gw, gdA = c.inp(x["p"]), c.inp(x["k"]), c.inp(x["w"]), c.inp(x["dA"])
    gxp, grs = c.inp(x["xp"][h]), c.inp(np.ones(N, F32))
    o = [c.out(E) for _ in range(4)] + [c.out(E, np.int32), c.out((N, h)), c.out(N)]
    w, pp, p, dw, pos, dxp, da = o
    for nm, mode in ((NOISE_EXPLICIT, 0), (4, 0), (-1, 0), (NOISE_HASH, 2), (NOISE_NONE, -1)):
        assert c.call("dgg_csr_softk_fwd_rows", gp, rp, cl, 0, N, N, gk, nm, 1, 2, mode, w, pp, pos) == ERR_ARG, (nm, mode)
    for r0, n, NN in ((1, N, N), (N, 1, N), (-1, 2, N), (0, -1, N), (0, N + 1, N), (0, 1, 1 << 31)):
        assert c.call("dgg_csr_softk_fwd_rows", gp, rp, cl, r0, n, NN, gk, NOISE_HASH, 1, 2, 0, w, pp, pos) == ERR_ARG, (r0, n, NN)
        assert c.call("dgg_csr_uvdist_fwd_rows", gxp, rp, cl, r0, n, NN, h, T_DIST, p) == ERR_ARG, (r0, n, NN)
        assert c.call("dgg_csr_uvdist_bwd_rows", gxp, rp, cl, r0, n, NN, h, T_DIST, gp, gdA, dxp) == ERR_ARG, (r0, n, NN)
        assert c.call("dgg_csr_normalize_fwd_rows", rp, cl, gw, grs, r0, n, NN, p) == ERR_ARG, (r0, n, NN)
        assert c.call("dgg_csr_norm_bwd_acc_rows", rp, cl, gw, grs, gdA, r0, n, NN, da) == ERR_ARG, (r0, n, NN)
        assert c.call("dgg_csr_norm_bwd_apply_rows", rp, cl, grs, gdA, grs, r0, n, NN, dw) == ERR_ARG, (r0, n, NN)
    assert c.call("dgg_csr_uvdist_fwd_rows", gxp, rp, cl, 0, N, N, 0, T_DIST, p) == ERR_ARG
    assert c.call("dgg_csr_uvdist_bwd_rows", gxp, rp, cl, 0, N, N, 0, T_DIST, gp, gdA, dxp) == ERR_ARG
    # an empty range returns 0 and writes nothing either
    rp0, cl0 = c.inp(np.zeros(1, np.int64)), c.inp(np.zeros(0, np.int32))
    assert c.call("dgg_csr_softk_fwd_rows", gp, rp0, cl0, 259, 0, N, gk, NOISE_HASH, 1, 2, 0, w, pp, pos) == 0
    assert c.call("dgg_csr_uvdist_fwd_rows", gxp, rp0, cl0, N, 0, N, h, T_DIST, p) == 0
    assert c.call("dgg_csr_uvdist_bwd_rows", gxp, rp0, cl0, 259, 0, N, h, T_DIST, gp, gdA, dxp) == 0
    assert c.call("dgg_csr_normalize_fwd_rows", rp0, cl0, gw, grs, 0, 0, N, p) == 0
    assert c.call("dgg_csr_norm_bwd_acc_rows", rp0, cl0, gw, grs, gdA, 259, 0, N, da) == 0
    assert c.call("dgg_csr_norm_bwd_apply_rows", rp0, cl0, grs, gdA, grs, 259, 0, N, dw) == 0
    assert all(untouched(gd) for gd in o)
    c.inputs_intact()
