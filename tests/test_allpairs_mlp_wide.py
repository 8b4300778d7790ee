"""Edge-MLP scorers (u-v-deg / u-v-deg-dist / edge_conv) on ALL-PAIRS candidates with rows of ANY width: dgg_allpairs_mlp_topk_wide,
dgg_softk_bwd_chunked, the autograd node on chunked rows and the module's opt-in args.dgg_allpairs_mlp_rows = "chunked".

Definition under test: row i keeps the L_i = ceil(k_i + 8.5) + 1 best columns (cut to the layout's capacity; all N when L_i > N) of the
composed CPU path oracle.edge_mlp_fwd + oracle.edgelist_topk_p on the COMPLETE candidate pattern (score descending, lower column first),
in the chunks of ops.chunk_layout(k, ncols=N), with the ramp of oracle.softk on the -1-filled top 64 M_max.  Forward checks are bit for
bit.

Gradient check (case 6, N = 200, h = 32, k up to ~150, hash noise): the error of each gradient against a dense float64 restatement with
the GIVEN selection, for the new node and for the two nodes the module's CSR form composes on the complete pattern (_DGGScoresFn +
ops.CsrSoftkFn: the same function for any k).  Both backwards sum with float atomics: each runs 8 times, its largest error counts.
Bar: new <= 4 x existing + one float32 ulp of the gradient's largest magnitude (the bar of tests/test_allpairs_mlp.py).
Measured on an MI355X (largest of 8 runs, max abs error vs float64): gradient maxima 1.4 .. 173, errors 1.2e-07 .. 4.8e-05 on both
sides, ratios new / existing in the paragraph after next.  The module's
dense adjacency against its CSR form (case 7): 0.0 difference for all three scorers.  Ramp backward (case 5): dval off by at most
2.4e-07 of 4.4, dk by 1.2e-07 of 1.1 (mode 0) / of 2.0 (mode 1).
What varies from run to run, and what does not.  Both sides run dgg_edge_mlp_bwd in its CSR form.  Its PARAMETER sums (wdu, wdv, wex,
eb1, w2, b2) used to be added by float atomics, one per workgroup in arrival order; with those, 48 runs of each side (forward bits
identical in all of them) put the error of db2 under edge_conv -- ONE number summed over every entry, with heavy cancellation -- anywhere
between 3.1e-07 (the correctly rounded float) and 1.1e-05 on BOTH sides, so a largest-of-8 of 1.1e-05 could meet a largest-of-8 of
2.4e-06: the bar then failed from time to time, on that leaf only.  The CSR form now adds the workgroups' sums in a fixed order in
double and keeps db2 in double from the entry on (dgg_edge_mlp_bwd_det): the errors of these six leaves are the SAME number in every
run (measured: db2 under edge_conv 3.07e-07 new / 1.26e-06 existing; the largest ratio over these leaves 1.9, dwdv under u-v-deg), so
their part of the bar cannot flip.  x, We, be and Wcat still go through float atomics on the neighbour side of dAB; over 48 runs their
errors stayed within 3x between smallest and largest on either side, and the LARGEST new error of any run was below 4 x the SMALLEST
existing one + ulp for every such leaf (closest: dbe under edge_conv, 1.11e-05 against 4 x 3.08e-06 + 3.8e-06).

Ramp backward (case 5): rtol = 2e-4, atol = 2e-4 x the largest reference entry -- the tolerance of the direct ops.softk_bwd check in
tests/test_hip_parity.py (test_backward_kernels; no test there compares ops.softk_bwd with oracle.softk_bwd alone, the end-to-end
gradient checks that go through oracle.softk_bwd use the wider 3e-4 of the largest entry).
"""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_allpairs_mlp import (NOISE_MODE, NOISES, PAD, SCORERS, SEED, T_EX, Nn, T, complete_in_adj, complete_pattern, make_inputs, module_args,
                               oracle_scores, scorer_args, to_dev, _node_inputs)
from test_chunked_rows import chunked_to_rows, rank_limit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------
# inputs, reference, canaried outputs
# ---------------------------------------------------------------------------------------------------------------
def degrees(N):
    """learned degrees of N rows: mostly narrow, three in ten of 1 .. 4 chunks, the chunk boundaries of L = ceil(k + 8.5) + 1, a row
    with k + 9.5 > N (it keeps every column) and, from N = 600, rows of 9 and of more chunks than the graph has columns for"""
    rng = np.random.default_rng(77 + N)
    k = (3.0 + 40.0 * rng.random(N) ** 2).astype(np.float32)
    wide = rng.random(N) < 0.3
    k[wide] = (40.0 + 160.0 * rng.random(N)).astype(np.float32)[wide]
    edge = np.array([1.0, 54.5, 54.6, 118.49, 118.51], np.float32)
    k[:min(5, N)] = edge[:min(5, N)]
    if N > 5:
        k[5] = N + 3.0
    if N >= 600:
        k[6], k[7] = 560.0, 700.0
    return k


def cap_ranks(N):
    from dgg_amd import ops
    return 64 * ops.chunk_maxm_for(N)


@functools.lru_cache(maxsize=None)
def ranked(N, hw, saturate, scorer, noise):
    """every column of every row in key order (computed once per case, shared, never modified) -> idx, val, ex [N, cap_ranks(N)]"""
    d = make_inputs(N, hw, hw, saturate=saturate)
    p, ex = oracle_scores(d, scorer)
    rowptr, col, _ = complete_pattern(N)
    idx, val, eid = O.edgelist_topk_p(p, N, rowptr, col, cap_ranks(N), NOISE_MODE[noise], d["G"] if noise == "explicit" else None, SEED)
    exo = np.where(eid >= 0, ex[np.maximum(eid, 0)], 0.0).astype(np.float32) if scorer_args(d, scorer)[1] == 2 else np.zeros_like(val)
    for a in (idx, val, exo):
        a.setflags(write=False)
    return idx, val, exo


def cut_to_degrees(full, k, mode, cap):
    """the first L_i ranks of the ranked rows, -1 / 0 beyond, and the ramp on them -> idx, val, ex, w [rows, cap], rs [rows]"""
    ridx, rval, rex = full
    keep = (np.arange(ridx.shape[1])[None, :] < rank_limit(k, cap)[:, None]) & (ridx >= 0)
    idx = np.where(keep, ridx, -1).astype(np.int32)
    val = np.where(keep, rval, 0).astype(np.float32)
    ex = np.where(keep, rex, 0).astype(np.float32)
    w, rs = O.softk(idx, val, k, mode)
    return idx, val, ex, w, rs


class CanariedChunks:
    """idx / val / ex / w [ccap, 64] and rs [rows] handed to the kernel as views between canary words, filled with -7 / NaN"""

    def __init__(self, ccap, rows, dev):
        self.n, self.rows = ccap * 64, rows
        self.bi = torch.full((self.n + 2 * PAD,), -7, dtype=torch.int32, device=dev)
        self.bf = [torch.full((self.n + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev) for _ in range(3)]
        self.br = torch.full((rows + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)

    def views(self):
        v = lambda b: b[PAD:PAD + self.n].view(-1, 64)  # noqa: E731
        return (v(self.bi), v(self.bf[0]), v(self.bf[1]), v(self.bf[2]), self.br[PAD:PAD + self.rows])

    def canaries_intact(self):
        ok = bool((self.bi[:PAD] == -7).all()) and bool((self.bi[PAD + self.n:] == -7).all())
        for b in self.bf:
            ok = ok and bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[PAD + self.n:]).all())
        return ok and bool(torch.isnan(self.br[:PAD]).all()) and bool(torch.isnan(self.br[PAD + self.rows:]).all())

    def untouched(self):
        return bool((self.bi == -7).all()) and all(bool(torch.isnan(b).all()) for b in self.bf + [self.br])


def run_wide(dv, scorer, noise, k, lay, mode, dev, rows=None, out=None):
    from dgg_amd import ops
    deg, ex_mode, wdu, wdv, wex, act = scorer_args(dv, scorer)
    return ops.allpairs_mlp_topk_wide(dv["AB"], dv["xp"], deg, ex_mode, T_EX, wdu, wdv, wex, dv["b1"], dv["w2"], dv["b2"], act, k, lay, mode,
                                      NOISE_MODE[noise], dv["G"] if noise == "explicit" else None, SEED, rows=rows, out=out)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def assert_chunks_equal(lay, got, ref, what):
    """got: idx, val, ex, w [>= chunks, 64], rs; ref: the row forms [rows, >= 64 M_max] and rs.  Everything exact."""
    fills = (-1, 0.0, 0.0, 0.0)
    for g, r, fill, name in zip(got[:4], ref[:4], fills, ("idx", "val", "ex", "w")):
        rows_form = chunked_to_rows(lay, g, fill)
        assert np.array_equal(bits(rows_form), bits(r[:, :rows_form.shape[1]])), f"{what}: {name} differs from the oracle"
        assert (r[:, rows_form.shape[1]:] == fill).all(), f"{what}: the reference has {name} beyond the layout's widest row"
    assert np.array_equal(bits(Nn(got[4])), bits(ref[4])), f"{what}: rs differs from the oracle"


# ---------------------------------------------------------------------------------------------------------------
# 1. the kernel against the CPU oracle, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,hw", [(N, hw) for N in (1, 63, 65, 130, 257, 600) for hw in (16, 64, 128)])
def test_wide_kernel_matches_the_composed_cpu_oracle_bit_for_bit(dev, N, hw):
    """three scorers x four noise settings (mode 1 under symmetric noise, mode 0 otherwise); idx / val / ex / w / rs exact, written into
    NaN / -7 buffers of chunks + 37 chunks between canaries; the spare chunks come back empty"""
    from dgg_amd import ops
    dv = to_dev(make_inputs(N, hw, hw), dev)
    k = degrees(N)
    kd = T(k, dev)
    lay = ops.chunk_layout(kd, ncols=N)
    Mi = (rank_limit(k, cap_ranks(N)) + 63) // 64
    cptr = Nn(lay.cptr).astype(np.int64)
    assert np.array_equal(cptr[1:] - cptr[:-1], Mi) and lay.chunks == int(Mi.sum()) and lay.maxm == int(Mi.max())
    assert (k + 9.5 > N).any(), "a row that keeps every column"
    if N == 600:
        assert Mi.max() > ops.APMLP_WIDE_REG_CHUNKS and ((Mi > 1) & (Mi <= ops.APMLP_WIDE_REG_CHUNKS)).any(), "the continuation pass must run"
    for scorer in SCORERS:
        for noise in NOISES:
            mode = 1 if noise == "sym" else 0
            ref = cut_to_degrees(ranked(N, hw, False, scorer, noise), k, mode, cap_ranks(N))
            assert (ref[0][5] >= 0).sum() == N if N > 5 else True
            buf = CanariedChunks(lay.chunks + 37, N, dev)
            run_wide(dv, scorer, noise, kd, lay, mode, dev, out=buf.views())
            got = buf.views()
            what = f"{scorer} / {noise} / mode {mode}"
            assert_chunks_equal(lay, got, ref, what)
            spare = slice(lay.chunks, lay.chunks + 37)
            assert bool((got[0][spare] == -1).all()) and all(bool((g[spare] == 0).all()) for g in got[1:4]), f"{what}: spare chunks not empty"
            assert buf.canaries_intact(), f"{what}: written outside the outputs"


def test_continuation_ceiling_inside_a_run_of_tied_scores(dev):
    """saturated inputs (many scores of exactly 1.0f), no noise: rows whose rank 64 MR - 1 -- the ceiling of the continuation pass -- and
    rank 64 MR carry the same score get 9 chunks; the pass must continue at exactly the next column of the tie"""
    from dgg_amd import ops
    N, hw = 600, 64
    MR = ops.APMLP_WIDE_REG_CHUNKS
    dv = to_dev(make_inputs(N, hw, hw, saturate=True), dev)
    for scorer in SCORERS:
        full = ranked(N, hw, True, scorer, "none")
        c = 64 * MR - 1
        tied = np.where((full[1][:, c] == np.float32(1.0)) & (full[1][:, c + 1] == np.float32(1.0)))[0]
        assert len(tied) >= 1, "the saturated inputs must hold a row whose ceiling key sits inside a run of scores of exactly 1.0f"
        k = degrees(N)
        k[tied[:4]] = 64.0 * MR + 30.0                                  # L = 64 MR + 40: one chunk beyond the register lists
        kd = T(k, dev)
        lay = ops.chunk_layout(kd, ncols=N)
        ref = cut_to_degrees(full, k, 0, cap_ranks(N))
        for i in tied[:4]:
            assert ref[1][i, c] == ref[1][i, c + 1] == np.float32(1.0) and ref[0][i, c] < ref[0][i, c + 1], "tie: lower column first"
        got = run_wide(dv, scorer, "none", kd, lay, 0, dev)
        got = (got[0], got[1], got[2] if got[2] is not None else torch.zeros_like(got[1]), got[3], got[4])
        assert_chunks_equal(lay, got, ref, f"{scorer} / tied ceiling")


# ---------------------------------------------------------------------------------------------------------------
# 2. the list is a special case
# ---------------------------------------------------------------------------------------------------------------
def test_rows_of_one_chunk_equal_the_list_kernel(dev):
    from dgg_amd import ops
    N, hw = 257, 64
    dv = to_dev(make_inputs(N, hw, hw), dev)
    rng = np.random.default_rng(3)
    k = (1.0 + 53.5 * rng.random(N)).astype(np.float32)
    k[:3] = (1.0, 54.5, 30.0)
    kd = T(k, dev)
    lay = ops.chunk_layout(kd, ncols=N)
    assert lay.chunks == N and lay.maxm == 1 and not lay.wide
    live = torch.arange(64, device=dev)[None, :] < T(rank_limit(k, 64), dev)[:, None]
    for scorer in SCORERS:
        deg, ex_mode, wdu, wdv, wex, act = scorer_args(dv, scorer)
        for noise, mode in (("hash", 0), ("none", 1), ("sym", 3)):
            idx, val, ex, w, rs = run_wide(dv, scorer, noise, kd, lay, mode, dev)
            lidx, lval, lex = ops.allpairs_mlp_topk(dv["AB"], dv["xp"], deg, ex_mode, T_EX, wdu, wdv, wex, dv["b1"], dv["w2"], dv["b2"], act, 64,
                                                    NOISE_MODE[noise], None, SEED)
            lidx, lval = torch.where(live, lidx, torch.full_like(lidx, -1)), torch.where(live, lval, torch.zeros_like(lval))
            what = f"{scorer} / {noise}"
            assert torch.equal(idx, lidx) and torch.equal(val.view(torch.int32), lval.view(torch.int32)), what
            if ex_mode:
                assert torch.equal(ex.view(torch.int32), torch.where(live, lex, torch.zeros_like(lex)).view(torch.int32)), what
            lw, lrs = ops.softk_fwd(lidx, lval, kd, mode)
            assert torch.equal(w.view(torch.int32), lw.view(torch.int32)) and torch.equal(rs.view(torch.int32), lrs.view(torch.int32)), what


# ---------------------------------------------------------------------------------------------------------------
# 3. row ranges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["hash", "sym"])
def test_row_ranges_equal_the_slices_of_the_whole_graph(dev, noise):
    from dgg_amd import ops
    N, hw = 257, 64
    dv = to_dev(make_inputs(N, hw, hw), dev)
    k = degrees(N)
    kd = T(k, dev)
    lay = ops.chunk_layout(kd, ncols=N)
    for scorer in ("u-v-deg", "u-v-deg-dist"):
        full = run_wide(dv, scorer, noise, kd, lay, 0, dev)
        fr = [chunked_to_rows(lay, a, f) for a, f in zip(full[:4], (-1, 0.0, 0.0, 0.0)) if a is not None]
        for r0, r1 in ((0, N), (37, 101), (3, 9), (N - 1, N)):
            ks = kd[r0:r1].contiguous()
            ls = ops.chunk_layout(ks, ncols=N)
            buf = CanariedChunks(ls.chunks, r1 - r0, dev)
            out = buf.views()
            part = run_wide(dv, scorer, noise, ks, ls, 0, dev, rows=(r0, r1), out=out if scorer == "u-v-deg-dist" else (out[0], out[1], None, out[3], out[4]))
            pr = [chunked_to_rows(ls, a, f) for a, f in zip(part[:4], (-1, 0.0, 0.0, 0.0)) if a is not None]
            for a, b, f in zip(pr, fr, (-1, 0.0, 0.0, 0.0)):
                assert np.array_equal(bits(a), bits(b[r0:r1, :a.shape[1]])) and (b[r0:r1, a.shape[1]:] == f).all(), f"{scorer} rows {r0}:{r1}"
            assert torch.equal(part[4].view(torch.int32), full[4][r0:r1].view(torch.int32)), f"{scorer} rows {r0}:{r1}: rs"
            assert buf.canaries_intact(), f"{scorer} rows {r0}:{r1}: written outside the range"


# ---------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["noise=4", "noise=5", "ex_mode=1", "hw=8", "h=256"])
def test_refusals_return_the_code_and_write_nothing(dev, what):
    from dgg_amd import ops
    from dgg_amd._lib import DggHipError
    key, _, v = what.partition("=")
    v = int(v)
    N, hw, h, ex_mode, noise = 70, 64, 64, 2, 2
    if key == "hw":
        hw = v
    elif key == "h":
        h = v
    elif key == "ex_mode":
        ex_mode = v
    else:
        noise = v
    dv = to_dev(make_inputs(N, hw, h), dev)
    kd = T(degrees(N), dev)
    lay = ops.chunk_layout(kd, ncols=N)
    buf = CanariedChunks(lay.chunks, N, dev)
    with pytest.raises(DggHipError, match=r"code 2"):
        ops.allpairs_mlp_topk_wide(dv["AB"], dv["xp"], dv["deg"], ex_mode, T_EX, dv["wdu"], dv["wdv"], dv["wex"], dv["b1"], dv["w2"], dv["b2"], 1, kd,
                                   lay, 0, noise, None, SEED, out=buf.views())
    torch.cuda.synchronize()
    assert buf.untouched()


# ---------------------------------------------------------------------------------------------------------------
# 5. the ramp backward on chunked rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_softk_bwd_chunked_matches_the_float64_oracle(dev, mode):
    from dgg_amd import ops
    rows, ncols = 301, 4096
    rng = np.random.default_rng(5 + mode)
    k = (1.0 + 620.0 * rng.random(rows) ** 2).astype(np.float32)
    k[:5] = (1.0, 54.5, 54.6, 118.49, 620.0)
    kd = T(k, dev)
    lay = ops.chunk_layout(kd, ncols=ncols)
    L = rank_limit(k, 64 * ops.chunk_maxm_for(ncols))
    assert lay.maxm == 10 and int(Nn(lay.cptr)[1]) == 1, "rows of 1 to 10 chunks"
    C = lay.chunks + 3                                                   # (spare chunks: dval comes back 0 there)
    rank = np.full((C, 64), 1 << 30, np.int64)
    rank[:lay.chunks] = Nn(lay.ranks())
    Lc = np.zeros(C, np.int64)
    Lc[:lay.chunks] = L[Nn(lay.cnode).astype(np.int64)]
    live = (rank < Lc[:, None]) & (rng.random((C, 64)) > 0.05)          # empty beyond L_i, and a few empty slots inside
    idx = np.where(live, rng.integers(0, ncols, (C, 64)), -1).astype(np.int32)
    val = np.where(live, rng.random((C, 64)), 0).astype(np.float32)
    dw = rng.standard_normal((C, 64)).astype(np.float32)
    dval, dk = ops.softk_bwd_chunked(T(idx, dev), T(val, dev), kd, T(dw, dev), lay, mode)
    dval2, dk2 = ops.softk_bwd_chunked(T(idx, dev), T(val, dev), kd, T(dw, dev), lay, mode)
    assert torch.equal(dk.view(torch.int32), dk2.view(torch.int32)) and torch.equal(dval.view(torch.int32), dval2.view(torch.int32)), "not deterministic"
    assert bool((dval[torch.from_numpy(~live).to(dev)] == 0).all()), "empty slots must get dval = 0"
    n = lay.chunks
    rdval, rdk = O.softk_bwd(chunked_to_rows(lay, idx[:n], -1), chunked_to_rows(lay, val[:n], 0.0), k, chunked_to_rows(lay, dw[:n], 0.0), mode)
    got = chunked_to_rows(lay, dval, 0.0)
    print(f"mode {mode}: max|dval - ref| = {np.abs(got - rdval).max():.3e} of {np.abs(rdval).max():.3e}, "
          f"max|dk - ref| = {np.abs(Nn(dk) - rdk).max():.3e} of {np.abs(rdk).max():.3e}")
    np.testing.assert_allclose(got, rdval, rtol=2e-4, atol=2e-4 * np.abs(rdval).max())
    np.testing.assert_allclose(Nn(dk), rdk, rtol=2e-4, atol=2e-4 * np.abs(rdk).max())


@pytest.mark.parametrize("hw", [16, 64])
def test_csr_form_parameter_sums_have_the_same_bits_in_every_run(dev, hw):
    """ops.edge_mlp_bwd with rowptr (dgg_edge_mlp_bwd_det): 301 rows = 76 workgroups store their sums, a second kernel adds them in a fixed
    order -> dpar bit-identical between runs; the ELL form of the same rows (float atomics) sums the same terms, so the two agree to
    the tolerance of the direct backward checks in tests/test_hip_parity.py (2e-4, relative and of the largest entry)"""
    from dgg_amd import ops
    N = 301
    dv = to_dev(make_inputs(N, hw, hw), dev)
    rng = np.random.default_rng(9)
    idx = torch.from_numpy(np.where(rng.random((N, 64)) > 0.1, rng.integers(0, N, (N, 64)), -1).astype(np.int32)).to(dev)
    val = torch.from_numpy(rng.random((N, 64)).astype(np.float32)).to(dev)
    dval = torch.from_numpy(rng.standard_normal((N, 64)).astype(np.float32)).to(dev)
    rowptr = torch.arange(N + 1, device=dev, dtype=torch.int64) * 64
    args = (dv["deg"], None, dv["wdu"], dv["wdv"], None, dv["b1"], dv["w2"], dv["b2"])
    runs = [ops.edge_mlp_bwd(dv["AB"], idx.reshape(-1), None, val.reshape(-1), dval.reshape(-1), *args, act=1, perturb=True, rowptr=rowptr)[1]
            for _ in range(4)]
    for r in runs[1:]:
        assert torch.equal(r.view(torch.int32), runs[0].view(torch.int32)), "dpar differs between two runs"
    eid = torch.arange(N * 64, device=dev, dtype=torch.int32).view(N, 64)
    atomic = ops.edge_mlp_bwd(dv["AB"], idx, eid, val, dval, *args, act=1, perturb=True)[1]
    assert float(runs[0].abs().max()) > 0
    diff = float((runs[0] - atomic).abs().max())
    print(f"hw {hw}: max |fixed order - atomics| = {diff:.3e} of {float(atomic.abs().max()):.3e}")
    np.testing.assert_allclose(Nn(runs[0]), Nn(atomic), rtol=2e-4, atol=2e-4 * float(atomic.abs().max()))


# ---------------------------------------------------------------------------------------------------------------
# 6. the autograd node
# ---------------------------------------------------------------------------------------------------------------
def _float64_grads_chunked(t, deg, cot_rows, idx_rows, Gn, scorer):
    """_float64_grads of tests/test_allpairs_mlp.py with the rank taken from the chunk position: dense float64 restatement of the
    definition with the GIVEN selection idx_rows [N, 64 M] (-1 = empty)"""
    leaf = {n: v.double().clone().requires_grad_(True) for n, v in t.items() if v is not None}
    lrelu = torch.nn.functional.leaky_relu
    xp = lrelu(leaf["x"] @ leaf["We"].T + leaf["be"], 0.01)
    AB = xp @ leaf["Wcat"].T
    hw = AB.shape[1] // 2
    z = AB[:, None, :hw] + AB[None, :, hw:] + leaf["eb1"]
    dg = deg.double()
    if "wdu" in leaf:
        z = z + dg[:, None, None] * leaf["wdu"] + dg[None, :, None] * leaf["wdv"]
    if "wex" in leaf:
        d2 = ((xp[:, None, :] - xp[None, :, :]) ** 2).sum(-1)
        dist = torch.where(d2 > 0, d2.clamp_min(1e-300).sqrt(), torch.zeros_like(d2))
        z = z + torch.exp(T_EX * dist)[:, :, None] * leaf["wex"]
    hid = z if scorer == "edge_conv" else lrelu(z, 0.01)
    p = torch.sigmoid(hid @ leaf["w2"] + leaf["b2"])
    v = (p + 1e-8) * torch.exp(Gn.double())
    val = torch.gather(v, 1, idx_rows.long().clamp(min=0))
    ramp = 1.0 - 0.5 * (1.0 + torch.tanh(torch.arange(idx_rows.shape[1], dtype=torch.float64)[None, :] - leaf["k"][:, None]))
    w = torch.where(idx_rows >= 0, val * ramp, torch.zeros_like(val))
    (w * cot_rows.double()).sum().backward()
    return {n: v.grad for n, v in leaf.items()}


@pytest.mark.parametrize("scorer", SCORERS)
def test_autograd_node_forward_bits_and_gradients(dev, scorer):
    from dgg_amd import ops
    from dgg_amd.dgm import _DGGAllPairsMlpWideAdjFn, _DGGScoresFn
    N, d_in, h = 200, 24, 32
    t, deg, _ = _node_inputs(N, d_in, h, scorer, dev)
    g = torch.Generator().manual_seed(12)
    t["k"] = 5.0 + 145.0 * torch.rand(N, generator=g) ** 2
    t["k"][:5] = torch.tensor([1.0, 54.5, 54.6, 118.49, 118.51])
    ex_mode, act = (2 if scorer == "u-v-deg-dist" else 0), (0 if scorer == "edge_conv" else 1)
    names = [n for n in ("x", "k", "We", "be", "Wcat", "wdu", "wdv", "wex", "eb1", "w2", "b2") if t[n] is not None]
    rowptr, col, erow = (T(a, dev) for a in complete_pattern(N))
    lay = ops.chunk_layout(t["k"].to(dev), ncols=N)
    assert lay.wide and lay.maxm >= 3
    cot = torch.randn(lay.chunks, 64, generator=g)
    mode = ops.MODE_K_TIMES_EDGE_PROB
    sel = {}

    def run(new):
        leaf = {n: (None if v is None else v.to(dev).requires_grad_(True)) for n, v in t.items()}
        par = (leaf["We"], leaf["be"], leaf["Wcat"], leaf["wdu"], leaf["wdv"], leaf["wex"], leaf["eb1"], leaf["w2"], leaf["b2"])
        if new:
            cfg = dict(K=64, noise_mode=ops.NOISE_HASH, G=None, seed=SEED, mode=mode, ex_mode=ex_mode, t_ex=T_EX, act=act, layout=lay)
            out = _DGGAllPairsMlpWideAdjFn.apply(leaf["x"], leaf["k"], deg.to(dev), *par, cfg)
            (out[0] * cot.to(dev)).sum().backward()
        else:                                              # the nodes the module's CSR form composes (_csr_soft_adjacency), complete pattern
            cfg = dict(cand=(rowptr, col, erow), t=ops.T_DIST, rows=None, ex_mode=ex_mode, t_ex=T_EX, act=act)
            p = _DGGScoresFn.apply(leaf["x"], deg.to(dev), None, *par, cfg)
            out = ops.CsrSoftkFn.apply(p, leaf["k"], rowptr, col, ops.NOISE_HASH, None, SEED, mode)
            (out * sel["cot_csr"]).sum().backward()
        return out, {n: leaf[n].grad.detach().cpu() for n in names}

    out_new, g_new = run(True)
    w, idx, val, rs = out_new
    # forward: case 1's reference on the node's own projection and first-layer products
    with torch.no_grad():
        xp = ops.linear_fwd(t["x"].to(dev), t["We"].to(dev), t["be"].to(dev), ops.ACT_LEAKY)
        AB = ops.linear_fwd(xp, t["Wcat"].to(dev), None, ops.ACT_NONE)
    o = lambda a: None if a is None else Nn(a)  # noqa: E731
    p_cpu, ex_cpu = O.edge_mlp_fwd(Nn(AB), Nn(xp), Nn(erow), Nn(col), o(deg) if t["wdu"] is not None else None, None, ex_mode, T_EX, o(t["wdu"]),
                                   o(t["wdv"]), o(t["wex"]), Nn(t["eb1"]), Nn(t["w2"]), float(t["b2"][0]), act)
    cap = cap_ranks(N)
    ridx, rval, reid = O.edgelist_topk_p(p_cpu, N, Nn(rowptr), Nn(col), cap, O.NOISE_HASH, None, SEED)
    rex = np.where(reid >= 0, ex_cpu[np.maximum(reid, 0)], 0.0).astype(np.float32) if ex_mode else np.zeros_like(rval)
    ref = cut_to_degrees((ridx, rval, rex), Nn(t["k"]), mode, cap)
    assert_chunks_equal(lay, (idx, val, torch.zeros_like(val), w.detach(), rs), (ref[0], ref[1], np.zeros_like(ref[1]), ref[3], ref[4]), scorer)
    # the same cotangent on the complete pattern: entry (i, j) of the CSR form takes the cotangent of the slot that holds column j
    idx_rows = torch.from_numpy(chunked_to_rows(lay, idx, -1))
    cot_rows = torch.from_numpy(chunked_to_rows(lay, cot, 0.0))
    dense = torch.zeros(N, N)
    ii = torch.arange(N)[:, None].expand_as(idx_rows)
    dense[ii[idx_rows >= 0], idx_rows[idx_rows >= 0].long()] = cot_rows[idx_rows >= 0]
    sel["cot_csr"] = dense.reshape(-1).to(dev)
    out_old, g_old = run(False)
    # (the two forwards agree on the selected entries, to the project's forward bar against its CSR form: 1e-5 of the largest entry)
    w_rows = torch.from_numpy(chunked_to_rows(lay, w.detach(), 0.0))
    w_csr = out_old.detach().cpu().view(N, N)[ii[idx_rows >= 0], idx_rows[idx_rows >= 0].long()]
    assert float((w_csr - w_rows[idx_rows >= 0]).abs().max()) <= 1e-5 * float(w_rows.abs().max())
    Gn = torch.from_numpy(O.noise_matrix(N, SEED[0], SEED[1], symmetric=False))
    ref64 = _float64_grads_chunked(t, deg, cot_rows, idx_rows, Gn, scorer)
    RUNS = 8
    errs = {True: {n: 0.0 for n in names}, False: {n: 0.0 for n in names}}
    for new, g0 in ((True, g_new), (False, g_old)):
        for i in range(RUNS):
            gr = g0 if i == 0 else run(new)[1]
            for n in names:
                errs[new][n] = max(errs[new][n], float((gr[n].double() - ref64[n]).abs().max()))
    bad = []
    for n in names:
        r = ref64[n]
        e_new, e_old = errs[True][n], errs[False][n]
        ulp = float(np.spacing(np.float32(r.abs().max())))
        print(f"{scorer:13s} d{n:5s} max|g|={float(r.abs().max()):.3e}  new {e_new:.3e}  existing {e_old:.3e}  ulp {ulp:.1e}")
        assert float(r.abs().max()) > 0, f"d{n}: the float64 gradient is identically zero (nothing checked)"
        if not e_new <= 4.0 * e_old + ulp:
            bad.append(f"d{n}: new {e_new:.3e} > 4 x {e_old:.3e} + {ulp:.1e}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("scorer", SCORERS)
def test_the_existing_path_of_the_gradient_bar_is_what_the_module_runs(dev, scorer, monkeypatch):
    """the gradient test above composes _DGGScoresFn + ops.CsrSoftkFn by hand (it needs a GIVEN k, which the module learns): the module
    under dgg_wide_rows = "csr" on the complete in_adj must run exactly these two nodes, once each, the second on the first's output,
    with the configuration keys, pattern and mode the test hands them -- if the module's CSR form changes, this fails"""
    import dgg_amd
    from dgg_amd import dgm, ops
    N = 70
    _, m2 = _module_pair(scorer, dev)
    calls = {"scores": [], "softk": []}
    real_scores, real_softk = dgm._DGGScoresFn.apply, ops.CsrSoftkFn.apply

    def spy_scores(*a):
        out = real_scores(*a)
        calls["scores"].append((a, out))
        return out

    def spy_softk(*a):
        out = real_softk(*a)
        calls["softk"].append((a, out))
        return out

    monkeypatch.setattr(dgm._DGGScoresFn, "apply", spy_scores)
    monkeypatch.setattr(ops.CsrSoftkFn, "apply", spy_softk)
    x = torch.rand(N, 24, generator=torch.Generator().manual_seed(1)).to(dev)
    prior = 80.0 + torch.arange(N).float() % 7
    a2 = m2(x, complete_in_adj(prior, dev))
    assert isinstance(a2, dgg_amd.CsrAdjacency)
    assert len(calls["scores"]) == 1 and len(calls["softk"]) == 1
    sa, p = calls["scores"][0]
    cfg = sa[-1]
    ex_mode, act = (2 if scorer == "u-v-deg-dist" else 0), (0 if scorer == "edge_conv" else 1)
    assert set(cfg) == {"cand", "t", "rows", "ex_mode", "t_ex", "act"}
    assert cfg["t"] == ops.T_DIST and cfg["rows"] is None and cfg["ex_mode"] == ex_mode and cfg["act"] == act
    assert sa[2] is None, "these scorers take no per-edge extra array"
    rowptr, col, erow = (T(a, dev) for a in complete_pattern(N))
    for got, want in zip(cfg["cand"], (rowptr, col, erow)):
        assert torch.equal(got.long(), want.long())
    ka, _ = calls["softk"][0]
    assert ka[0] is p and torch.equal(ka[2].long(), rowptr.long()) and torch.equal(ka[3].long(), col.long())
    assert ka[5] is None and ka[7] == ops.MODE_K_TIMES_EDGE_PROB          # (a counter-based generator, no noise tensor)


# ---------------------------------------------------------------------------------------------------------------
# 7. the module
# ---------------------------------------------------------------------------------------------------------------
def _module_pair(scorer, dev, **kw):
    import dgg_amd
    torch.manual_seed(5)
    m1 = dgg_amd.DGG_LearnableK_debug(in_dim=24, latent_dim=32, args=module_args(scorer, dgg_allpairs_mlp_rows="chunked", **kw)).to(dev)
    with torch.no_grad():
        m1.k_net.k_project.weight.mul_(0.1)
    m2 = copy.deepcopy(m1)
    m2.args = module_args(scorer, dgg_wide_rows="csr", **kw)
    for m in (m1, m2):
        m.set_seed(77, 5)
    return m1, m2


@pytest.mark.parametrize("scorer", SCORERS)
def test_module_opt_in_keeps_every_weighted_rank(dev, scorer):
    """(fails before this feature: the argument is ignored, the list drops weight and check_ell_bound raises)"""
    import dgg_amd
    N = 130
    m1, m2 = _module_pair(scorer, dev)
    for nm in range(6):
        assert m1.wide_row_plan(N, True, nm) == "chunked" and m2.wide_row_plan(N, True, nm) == "list"
    x = torch.rand(N, 24, generator=torch.Generator().manual_seed(1)).to(dev)
    prior = 80.0 + torch.arange(N).float() % 7                         # k ~ 84: k + 8.5 > 64
    a1 = m1(x, dgg_amd.AllPairs(prior.to(dev)))
    m1.check_ell_bound()
    assert isinstance(a1, dgg_amd.EllAdjacency) and a1.layout is not None and a1.layout.wide and a1.owner is m1
    assert float(a1.k.max()) + 8.5 > 64
    a2 = m2(x, complete_in_adj(prior, dev))
    assert isinstance(a2, dgg_amd.CsrAdjacency)
    assert torch.equal(a1.k, a2.k)
    d1, d2 = a1.to_dense().detach(), a2.to_dense().detach()
    diff, top = float((d1 - d2).abs().max()), float(d2.abs().max())
    print(f"{scorer}: max |chunked - csr| = {diff:.3e}, largest entry {top:.3e}")
    assert top > 0 and diff <= 1e-5 * top


def test_module_dgg_hard_and_a_backward_run_on_chunked_rows(dev):
    import dgg_amd
    N = 130
    m1, m2 = _module_pair("u-v-deg", dev, dgg_hard=True)
    x = torch.rand(N, 24, generator=torch.Generator().manual_seed(1)).to(dev).requires_grad_(True)
    prior = 80.0 + torch.arange(N).float() % 7
    a1 = m1(x, dgg_amd.AllPairs(prior.to(dev)))
    assert a1.layout is not None and a1.layout.wide
    d1 = a1.to_dense()
    d2 = m2(x, complete_in_adj(prior, dev)).to_dense().detach()
    assert float((d1.detach() - d2).abs().max()) <= 1e-5 * float(d2.abs().max())
    d1.sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    for n, p in m1.named_parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), n


@pytest.mark.parametrize("scorer", SCORERS)
def test_module_without_wide_rows_and_without_the_opt_in_is_the_list_path(dev, scorer):
    """learned degrees that fit the list: the opt-in reads the layout back, finds no wide row and runs the list kernel -- the bits of the
    module without the argument, which is today's path; beyond the list the module without the argument still reports the bound"""
    import dgg_amd
    N = 130
    m1, _ = _module_pair(scorer, dev)
    m0 = copy.deepcopy(m1)
    m0.args = module_args(scorer)
    assert not hasattr(m0.args, "dgg_allpairs_mlp_rows")
    m0.set_seed(77, 5)
    x = torch.rand(N, 24, generator=torch.Generator().manual_seed(1)).to(dev)
    A = dgg_amd.AllPairs(torch.full((N,), 9.0, device=dev))
    a1, a0 = m1(x, A), m0(x, A)
    for m in (m1, m0):
        m.check_ell_bound()
    assert a1.layout is None and a0.layout is None and torch.equal(a1.idx, a0.idx)
    for f1, f0, what in ((a1.values(), a0.values(), "w"), (a1.rs, a0.rs, "rs"), (a1.k, a0.k, "k"), (a1.score, a0.score, "score")):
        assert torch.equal(f1.detach().view(torch.int32), f0.detach().view(torch.int32)), what
    m0(x, dgg_amd.AllPairs(80.0 + torch.arange(N, device=dev).float() % 7))
    with pytest.raises(RuntimeError, match="ell_width"):
        m0.check_ell_bound()


# ---------------------------------------------------------------------------------------------------------------
# 8. training
# ---------------------------------------------------------------------------------------------------------------
def test_gcn_dgg_trains_past_the_list_with_the_opt_in(dev):
    """(fails before this feature: the learned degrees outgrow the list and check_ell_bound raises)"""
    import dgg_amd
    N, d_in, h, C = 300, 40, 32, 7
    args = module_args("u-v-deg", dgg_wide_rows="auto", dgg_allpairs_mlp_rows="chunked")
    torch.manual_seed(3)
    model = dgg_amd.GCN_DGG(nfeat=d_in, nhidden=h, nclass=C, args=args).to(dev)
    with torch.no_grad():
        model.dggs[0].k_net.k_project.weight.mul_(0.1)
    x = torch.rand(N, d_in, generator=torch.Generator().manual_seed(1)).to(dev)
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(2)).to(dev)
    # priors around 48: the learned degree k = relu(kp sd + mu) + 1 starts a few ranks below the list's bound k + 8.5 = 64
    A = dgg_amd.AllPairs(torch.randint(40, 56, (N,), generator=torch.Generator().manual_seed(4)).float().to(dev))
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    wide_steps, kmax = 0, []
    for step in range(80):
        opt.zero_grad()
        logp, adj, _ = model(x, A)
        torch.nn.functional.nll_loss(logp, y).backward()
        for n, p in model.named_parameters():
            assert p.grad is None or bool(torch.isfinite(p.grad).all()), f"step {step}: {n}"
        opt.step()
        kmax.append(float(adj.k.max()))
        wide_steps += int(kmax[-1] + 8.5 > 64)
        if wide_steps >= 4:
            break
    print("k_max per step:", " ".join(f"{v:.1f}" for v in kmax))
    assert wide_steps >= 4 and kmax[-1] + 8.5 > 64, "the learned degrees must outgrow the 64-rank list in this run"
    dgg = model.dggs[0]
    dgg.check_ell_bound()
    assert isinstance(adj, dgg_amd.EllAdjacency) and adj.layout is not None and adj.layout.wide and bool(torch.isfinite(logp).all())
    assert set(dgg.fused_fallback) == {"edge-MLP scorer on all-pairs candidates"}
