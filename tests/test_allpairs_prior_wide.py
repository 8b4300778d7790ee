"""All-pairs candidates scored against a sparse PRIOR graph (u-v-A_uv) on CHUNKED rows: dgg_allpairs_mlp_topk_wide_prior, its
autograd node and the module's opt-in args.dgg_allpairs_mlp_rows = "chunked".

Definition under test: row i keeps the L_i = ceil(k_i + 8.5) + 1 best columns of the composed CPU path oracle.edge_mlp_fwd (ex_mode 1,
ex_in = the prior's dense values) + oracle.edgelist_topk_p on the COMPLETE candidate pattern, in the chunks of
ops.chunk_layout(k, ncols=N), with the ramp of oracle.softk (the ranked-and-cut oracle of tests/test_allpairs_mlp_wide.py with the
prior extra).  Forward checks are bit for bit.

Gradient check (N = 200, h = 32, k up to ~150, hash noise): the error of each gradient against a dense float64 restatement with the
GIVEN selection, for the new node and for _DGGScoresFn + ops.CsrSoftkFn on the complete pattern with the dense ex_in; each runs 8
times, its largest error counts.  Bar: new <= 4 x existing + one float32 ulp of the gradient's largest magnitude.

Measured on an MI355X (largest of 8 runs, max abs error vs float64; new node / existing nodes):

    gradient   max |g|    new node / existing nodes
    dx         1.2e+01    5.2e-06 / 3.3e-06
    dk         2.7e+00    4.5e-07 / 3.9e-07
    dWe        7.2e+01    1.7e-05 / 1.5e-05
    dbe        2.5e+01    1.4e-05 / 1.3e-05
    dWcat      4.8e+01    2.1e-05 / 1.8e-05
    dwex       6.9e+00    6.3e-06 / 4.2e-06
    deb1       1.4e+01    3.9e-06 / 2.3e-06
    dw2        1.1e+02    3.7e-05 / 2.9e-05
    db2        3.4e+01    9.9e-06 / 6.1e-06

(largest ratio new / existing 1.74, deb1; the module's dense adjacency on chunked rows against its CSR form on the complete in_adj
that stores the prior: 0.0 difference, largest entry 10.9)
"""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_allpairs_mlp import NOISE_MODE, NOISES, SEED, Nn, T, complete_pattern, module_args, to_dev
from test_allpairs_mlp_wide import CanariedChunks, assert_chunks_equal, cap_ranks, cut_to_degrees, degrees
from test_allpairs_prior import (GRAD_NAMES, complete_in_adj_with, float64_grads_prior, gradient_bar, make_prior, module_prior, node_inputs_prior,
                                 oracle_scores_prior, oracle_topk_prior, prior_csr, prior_inputs, switch_args)
from test_chunked_rows import chunked_to_rows, rank_limit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def ranked_prior(N, hw, switches, noise):
    """every column of every row in key order (computed once per case, shared, never modified) -> idx, val, ex [N, cap_ranks(N)]"""
    d = prior_inputs(N, hw)
    P, _ = make_prior(N)
    p, ex = oracle_scores_prior(d, P, switches)
    out = oracle_topk_prior(d, p, ex, noise, k=cap_ranks(N))
    for a in out:
        a.setflags(write=False)
    return out


def run_wide_prior(dv, switches, noise, k, lay, mode, csr, dev, rows=None, out=None, ex_mode=1):
    from dgg_amd import ops
    deg, wdu, wdv, act = switch_args(dv, switches)
    return ops.allpairs_mlp_topk_wide(dv["AB"], dv["xp"], deg, ex_mode, 0.0, wdu, wdv, dv["wex"], dv["b1"], dv["w2"], dv["b2"], act, k, lay, mode,
                                      NOISE_MODE[noise], dv["G"] if noise == "explicit" else None, SEED, rows=rows, out=out, prior=csr)


# ---------------------------------------------------------------------------------------------------------------
# 4. the wide kernel against the ranked-and-cut CPU oracle, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,hw", [(N, hw) for N in (1, 63, 65, 130, 257, 600) for hw in (16, 64)])
def test_wide_kernel_matches_the_composed_cpu_oracle_bit_for_bit(dev, N, hw):
    """four noise settings (mode 1 under symmetric noise, mode 0 otherwise); idx / val / ex / w / rs exact, written into NaN / -7
    buffers of chunks + 37 chunks between canaries; the spare chunks come back empty.  N = 600 holds rows of 9 and 10 chunks: their
    continuation pass sweeps the columns again and must walk the prior again from the row's start (ex of the chunks beyond the
    eighth is compared like every other)"""
    from dgg_amd import ops
    dv = to_dev(prior_inputs(N, hw), dev)
    P, stored = make_prior(N)
    csr = tuple(T(a, dev) for a in prior_csr(stored, P))
    k = degrees(N)
    if N == 600:
        k[0] = 520.0                                             # the row that stores ALL columns: 9 chunks, prior values in every one
    kd = T(k, dev)
    lay = ops.chunk_layout(kd, ncols=N)
    Mi = (rank_limit(k, cap_ranks(N)) + 63) // 64
    if N == 600:
        assert Mi.max() > ops.APMLP_WIDE_REG_CHUNKS and Mi[0] == 9 and ((Mi > 1) & (Mi <= ops.APMLP_WIDE_REG_CHUNKS)).any(), "the continuation pass must run"
    if N >= 130:
        assert 1 in Mi and Mi.max() >= 4, "rows of 1 to 4 chunks"
    for switches in ("u-v-A_uv", "prior+deg+identity") if hw == 64 else ("u-v-A_uv",):
        for noise in NOISES:
            mode = 1 if noise == "sym" else 0
            ref = cut_to_degrees(ranked_prior(N, hw, switches, noise), k, mode, cap_ranks(N))
            if N > 64:
                assert (ref[2] != 0).any(), "no kept entry carries a prior value"
            if N == 600:
                assert (ref[2][0, 512:] != 0).any(), "the continuation pass of row 0 must keep prior edges"
            buf = CanariedChunks(lay.chunks + 37, N, dev)
            run_wide_prior(dv, switches, noise, kd, lay, mode, csr, dev, out=buf.views())
            got = buf.views()
            what = f"{switches} / {noise} / mode {mode}"
            assert_chunks_equal(lay, got, ref, what)
            spare = slice(lay.chunks, lay.chunks + 37)
            assert bool((got[0][spare] == -1).all()) and all(bool((g[spare] == 0).all()) for g in got[1:4]), f"{what}: spare chunks not empty"
            assert buf.canaries_intact(), f"{what}: written outside the outputs"


def test_rows_of_one_chunk_equal_the_list_kernel(dev):
    from dgg_amd import ops
    from test_allpairs_prior import run_prior
    N, hw = 257, 64
    dv = to_dev(prior_inputs(N, hw), dev)
    P, stored = make_prior(N)
    csr = tuple(T(a, dev) for a in prior_csr(stored, P))
    rng = np.random.default_rng(3)
    k = (1.0 + 53.5 * rng.random(N)).astype(np.float32)
    k[:3] = (1.0, 54.5, 30.0)
    kd = T(k, dev)
    lay = ops.chunk_layout(kd, ncols=N)
    assert lay.chunks == N and lay.maxm == 1 and not lay.wide
    live = torch.arange(64, device=dev)[None, :] < T(rank_limit(k, 64), dev)[:, None]
    for noise, mode in (("hash", 0), ("none", 1), ("sym", 3)):
        idx, val, ex, w, rs = run_wide_prior(dv, "u-v-A_uv", noise, kd, lay, mode, csr, dev)
        lidx, lval, lex = run_prior(dv, "u-v-A_uv", noise, csr, dev)
        lidx, lval = torch.where(live, lidx, torch.full_like(lidx, -1)), torch.where(live, lval, torch.zeros_like(lval))
        assert torch.equal(idx, lidx) and torch.equal(val.view(torch.int32), lval.view(torch.int32)), noise
        assert torch.equal(ex.view(torch.int32), torch.where(live, lex, torch.zeros_like(lex)).view(torch.int32)), noise
        assert float(ex.abs().max()) > 0
        lw, lrs = ops.softk_fwd(lidx, lval, kd, mode)
        assert torch.equal(w.view(torch.int32), lw.view(torch.int32)) and torch.equal(rs.view(torch.int32), lrs.view(torch.int32)), noise


@pytest.mark.parametrize("noise", ["hash", "sym"])
def test_row_ranges_equal_the_slices_of_the_whole_graph(dev, noise):
    from dgg_amd import ops
    N, hw = 257, 64
    dv = to_dev(prior_inputs(N, hw), dev)
    P, stored = make_prior(N)
    csr = tuple(T(a, dev) for a in prior_csr(stored, P))
    kd = T(degrees(N), dev)
    lay = ops.chunk_layout(kd, ncols=N)
    full = run_wide_prior(dv, "u-v-A_uv", noise, kd, lay, 0, csr, dev)
    fr = [chunked_to_rows(lay, a, f) for a, f in zip(full[:4], (-1, 0.0, 0.0, 0.0))]
    for r0, r1 in ((37, 101), (3, 9), (N - 1, N)):
        ks = kd[r0:r1].contiguous()
        ls = ops.chunk_layout(ks, ncols=N)
        buf = CanariedChunks(ls.chunks, r1 - r0, dev)
        part = run_wide_prior(dv, "u-v-A_uv", noise, ks, ls, 0, csr, dev, rows=(r0, r1), out=buf.views())
        pr = [chunked_to_rows(ls, a, f) for a, f in zip(part[:4], (-1, 0.0, 0.0, 0.0))]
        for a, b, f in zip(pr, fr, (-1, 0.0, 0.0, 0.0)):
            assert np.array_equal(a.view(np.int32), b[r0:r1, :a.shape[1]].view(np.int32)) and (b[r0:r1, a.shape[1]:] == f).all(), f"rows {r0}:{r1}"
        assert torch.equal(part[4].view(torch.int32), full[4][r0:r1].view(torch.int32)), f"rows {r0}:{r1}: rs"
        assert buf.canaries_intact(), f"rows {r0}:{r1}: written outside the range"


@pytest.mark.parametrize("what", ["null_col", "ex_mode=0", "ex_mode=2", "noise=4", "noise=5", "hw=8"])
def test_refusals_return_the_code_and_write_nothing(dev, what):
    from dgg_amd import ops
    from dgg_amd._lib import DggHipError
    from test_allpairs_mlp import make_inputs
    key, _, v = what.partition("=")
    N, hw, ex_mode, noise = 70, 64, 1, 2
    if key == "hw":
        hw = int(v)
    elif key == "ex_mode":
        ex_mode = int(v)
    elif key == "noise":
        noise = int(v)
    dv = to_dev(make_inputs(N, hw, 64), dev)
    P, stored = make_prior(N)
    csr = [T(a, dev) for a in prior_csr(stored, P)]
    kd = T(degrees(N), dev)
    lay = ops.chunk_layout(kd, ncols=N)
    buf = CanariedChunks(lay.chunks, N, dev)
    if key == "null_col":                                       # (the wrapper never passes a NULL array: the C entry itself)
        from dgg_amd import _lib
        o = lambda t_: None if t_ is None else ops._ptr(t_)  # noqa: E731
        idx, val, ex, w, rs = buf.views()
        rc = _lib.lib().dgg_allpairs_mlp_topk_wide_prior(o(dv["AB"]), o(dv["xp"]), N, 64, 64, 0, N, None, 1, 0.0, None, None, o(dv["wex"]),
                                                         o(dv["b1"]), o(dv["w2"]), o(dv["b2"]), 1, 2, None, 0, SEED[0], SEED[1], o(kd), 0, lay.maxm,
                                                         o(lay.cptr), idx.shape[0], o(idx), o(val), o(ex), o(w), o(rs), o(csr[0]), None, o(csr[2]),
                                                         ops._stream())
        assert rc == 1, "a NULL CSR array is DGG_ERR_ARG"
    else:
        with pytest.raises(DggHipError, match=r"code 2"):
            ops.allpairs_mlp_topk_wide(dv["AB"], dv["xp"], None, ex_mode, 0.0, None, None, dv["wex"], dv["b1"], dv["w2"], dv["b2"], 1, kd, lay, 0,
                                       noise, None, SEED, out=buf.views(), prior=tuple(csr))
    torch.cuda.synchronize()
    assert buf.untouched()


# ---------------------------------------------------------------------------------------------------------------
# 5. the autograd node on chunked rows
# ---------------------------------------------------------------------------------------------------------------
def test_autograd_node_forward_bits_and_gradients(dev):
    from dgg_amd import ops
    from dgg_amd.dgm import _DGGAllPairsMlpWideAdjFn, _DGGScoresFn
    N, d_in, h = 200, 24, 32
    t, deg, _, P, stored = node_inputs_prior(N, d_in, h, dev)
    g = torch.Generator().manual_seed(12)
    t["k"] = 5.0 + 145.0 * torch.rand(N, generator=g) ** 2
    t["k"][:5] = torch.tensor([1.0, 54.5, 54.6, 118.49, 118.51])
    rowptr, col, erow = (T(a, dev) for a in complete_pattern(N))
    csr = tuple(T(a, dev) for a in prior_csr(stored, P))
    ex_in = T(np.ascontiguousarray(P.reshape(-1)), dev)
    lay = ops.chunk_layout(t["k"].to(dev), ncols=N)
    assert lay.wide and lay.maxm >= 3
    cot = torch.randn(lay.chunks, 64, generator=g)
    mode = ops.MODE_K_TIMES_EDGE_PROB
    sel = {}

    def run(new):
        leaf = {n: (None if v is None else v.to(dev).requires_grad_(True)) for n, v in t.items()}
        par = (leaf["We"], leaf["be"], leaf["Wcat"], None, None, leaf["wex"], leaf["eb1"], leaf["w2"], leaf["b2"])
        if new:
            cfg = dict(K=64, noise_mode=ops.NOISE_HASH, G=None, seed=SEED, mode=mode, ex_mode=1, t_ex=0.0, act=1, layout=lay, prior=csr)
            out = _DGGAllPairsMlpWideAdjFn.apply(leaf["x"], leaf["k"], deg.to(dev), *par, cfg)
            (out[0] * cot.to(dev)).sum().backward()
        else:                                              # the nodes the module's CSR form composes, complete pattern, dense ex_in
            cfg = dict(cand=(rowptr, col, erow), t=ops.T_DIST, rows=None, ex_mode=1, t_ex=0.0, act=1)
            p = _DGGScoresFn.apply(leaf["x"], deg.to(dev), ex_in, *par, cfg)
            out = ops.CsrSoftkFn.apply(p, leaf["k"], rowptr, col, ops.NOISE_HASH, None, SEED, mode)
            (out * sel["cot_csr"]).sum().backward()
        return out, {n: leaf[n].grad.detach().cpu() for n in GRAD_NAMES}

    out_new, g_new = run(True)
    w, idx, val, rs = out_new
    # forward: the ranked-and-cut reference on the node's own projection and first-layer products
    with torch.no_grad():
        xp = ops.linear_fwd(t["x"].to(dev), t["We"].to(dev), t["be"].to(dev), ops.ACT_LEAKY)
        AB = ops.linear_fwd(xp, t["Wcat"].to(dev), None, ops.ACT_NONE)
    p_cpu, ex_cpu = O.edge_mlp_fwd(Nn(AB), Nn(xp), Nn(erow), Nn(col), None, Nn(ex_in), 1, 0.0, None, None, Nn(t["wex"]), Nn(t["eb1"]), Nn(t["w2"]),
                                   float(t["b2"][0]), 1)
    cap = cap_ranks(N)
    ridx, rval, reid = O.edgelist_topk_p(p_cpu, N, Nn(rowptr), Nn(col), cap, O.NOISE_HASH, None, SEED)
    rex = np.where(reid >= 0, ex_cpu[np.maximum(reid, 0)], 0.0).astype(np.float32)
    ref = cut_to_degrees((ridx, rval, rex), Nn(t["k"]), mode, cap)
    assert_chunks_equal(lay, (idx, val, torch.zeros_like(val), w.detach(), rs), (ref[0], ref[1], np.zeros_like(ref[1]), ref[3], ref[4]), "node")
    idx_rows = torch.from_numpy(chunked_to_rows(lay, idx, -1))
    cot_rows = torch.from_numpy(chunked_to_rows(lay, cot, 0.0))
    dense = torch.zeros(N, N)
    ii = torch.arange(N)[:, None].expand_as(idx_rows)
    dense[ii[idx_rows >= 0], idx_rows[idx_rows >= 0].long()] = cot_rows[idx_rows >= 0]
    sel["cot_csr"] = dense.reshape(-1).to(dev)
    out_old, g_old = run(False)
    w_rows = torch.from_numpy(chunked_to_rows(lay, w.detach(), 0.0))
    w_csr = out_old.detach().cpu().view(N, N)[ii[idx_rows >= 0], idx_rows[idx_rows >= 0].long()]
    assert float((w_csr - w_rows[idx_rows >= 0]).abs().max()) <= 1e-5 * float(w_rows.abs().max())
    Gn = torch.from_numpy(O.noise_matrix(N, SEED[0], SEED[1], symmetric=False))
    ref64 = float64_grads_prior(t, torch.from_numpy(P), cot_rows, idx_rows, Gn)
    gradient_bar(run, g_new, g_old, ref64, "chunked")


# ---------------------------------------------------------------------------------------------------------------
# the module on chunked rows
# ---------------------------------------------------------------------------------------------------------------
def test_module_opt_in_keeps_every_weighted_rank(dev):
    """wide_row_plan, _allpairs_mlp_chunked and check_ell_bound behave as for u-v-deg; the dense adjacency equals the module's CSR form
    on the complete in_adj that stores the prior (1e-5 of the largest entry: the project's forward bar against its CSR form)"""
    import dgg_amd
    N = 130
    torch.manual_seed(5)
    m1 = dgg_amd.DGG_LearnableK_debug(in_dim=24, latent_dim=32, args=module_args("u-v-A_uv", dgg_allpairs_mlp_rows="chunked")).to(dev)
    with torch.no_grad():
        m1.k_net.k_project.weight.mul_(0.1)
        m1.k_net.k_project.bias.fill_(30.0)                    # k = relu(kp sd + mu) + 1 with kp ~ 30: beyond the list
    m2 = copy.deepcopy(m1)
    m2.args = module_args("u-v-A_uv", dgg_wide_rows="csr")
    for m in (m1, m2):
        m.set_seed(77, 5)
    for nm in range(6):
        assert m1.wide_row_plan(N, True, nm) == "chunked" and m2.wide_row_plan(N, True, nm) == "list"
    x = torch.rand(N, 24, generator=torch.Generator().manual_seed(1)).to(dev)
    P = module_prior(N)
    deg = P.double().sum(1).float()
    a1 = m1(x, dgg_amd.AllPairs(deg.to(dev), prior=P.to_sparse().to(dev)))
    m1.check_ell_bound()
    assert isinstance(a1, dgg_amd.EllAdjacency) and a1.layout is not None and a1.layout.wide and a1.owner is m1
    assert float(a1.k.max()) + 8.5 > 64
    a2 = m2(x, complete_in_adj_with(P, dev))
    assert isinstance(a2, dgg_amd.CsrAdjacency)
    assert torch.equal(a1.k, a2.k)
    d1, d2 = a1.to_dense().detach(), a2.to_dense().detach()
    diff, top = float((d1 - d2).abs().max()), float(d2.abs().max())
    print(f"u-v-A_uv: max |chunked - csr| = {diff:.3e}, largest entry {top:.3e}")
    assert top > 0 and diff <= 1e-5 * top
