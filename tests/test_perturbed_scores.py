"""Perturbed edge probabilities returned as the adjacency: debug_step 1 and k-select `edge_p-cdf` of DGG_LearnableK_debug with
perturb_edge_prob=True (reference dgm.py:1211-1239, 1368-1401) on edge lists.

The stored entries carry q_e = exp(log(p_e + 1e-8) + G_e), one rounding per step (dgg_csr_perturb_fwd): the bits the top-k searches
rank under the same noise.  The reference's non-edges (1e-8 exp(G) <= ~3e-7, below the 1e-5 forward bar) are not produced.

Bars: q BIT-EXACT against the oracle's scalar functions composed in binary32; the reference goldens to 1e-5; gradients to 3e-4 of
the gradient's maximum; the backward kernel to 1e-6 relative (one multiply, one add and one divide in fp32 -- 3 x 2^-24 ~ 1.8e-7 --
with ~5x headroom) against float64.
"""
import functools

import numpy as np
import pytest
import torch

from golden_noise import grid_gumbel, grid_normal
from helpers import csr_from_coo, load_fixture
from oracle import oracle as O
from test_oracle_golden import oracle_scores

PERT_FIXTURES = ["debug1_uvdist_asym", "cdf_uvdeg_sym", "debug1_edgeconv_asym", "cdf_uvdegdist_sym"]
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


def T(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def Nn(t):
    return t.detach().cpu().numpy()


def compose(p, rows, cols, G):
    """exp(log(f32(p) + f32(1e-8)) + G[i, j]) entry by entry through the oracle's scalar functions, every sum in binary32"""
    out = np.empty(len(p), F32)
    for e in range(len(p)):
        lp = F32(O.log(F32(p[e]) + F32(1e-8)))
        out[e] = O.exp(lp + F32(G[rows[e], cols[e]]))
    return out


@functools.lru_cache(maxsize=None)
def golden_composition(tag):
    """(fixture, oracle p [E], oracle q [E]) of one golden, computed once and shared (read-only)"""
    fx = load_fixture("scores_pert_" + tag)
    p, col = oracle_scores(fx)
    assert np.array_equal(col, fx["cols"])
    q = compose(p, fx["rows"], fx["cols"], fx["G"])
    p.setflags(write=False)
    q.setflags(write=False)
    return fx, p, q


def rows_to_csr(lens, N, rng):
    """random pattern with the given row lengths: columns of a row distinct and ascending -> rowptr int64, col int32, erow int32"""
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(N, size=int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    erow = np.repeat(np.arange(len(lens)), lens).astype(np.int32)
    return rowptr, col, erow


def probabilities(E, rng):
    """p in (0, 1] with entries forced to exactly 0.0, 1.0 and 1e-30"""
    p = (1.0 - rng.random(E)).astype(F32)
    assert p.min() > 0 and p.max() <= 1
    sl = rng.choice(E, size=min(E, 9), replace=False)
    for n, v in enumerate(sl):
        p[v] = (0.0, 1.0, 1e-30)[n % 3]
    return p


def mk_args(**kw):
    from argparse import Namespace
    base = dict(extra_edge_dim=0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288, dgg_mode_edge_net="u-v-dist",
                dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=True, symmetric_noise=False,
                stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
    base.update(kw)
    return Namespace(**base)


def symmetric_graph(N, avg_deg, rng, self_loops=True):
    A = rng.random((N, N)) < avg_deg / (2.0 * N)
    A = A | A.T
    np.fill_diagonal(A, self_loops)
    r, c = np.nonzero(A)
    return r.astype(np.int64), c.astype(np.int64)


def coo(rows, cols, vals, N, dev):
    ind = torch.from_numpy(np.stack([rows, cols]).astype(np.int64))
    return torch.sparse_coo_tensor(ind, torch.from_numpy(np.asarray(vals, F32)), (N, N)).coalesce().to(dev)


# ---------------------------------------------------------------------------------------------------------------
# CPU: the goldens are the oracle's composition on the pattern and (almost) nothing off it
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", PERT_FIXTURES)
def test_perturbed_scores_fixture_is_the_oracles_composition(tag):
    fx, p, q = golden_composition(tag)
    N = fx["meta"]["N"]
    a = fx["meta"]["args"]
    assert a["perturb_edge_prob"] and (a["debug_step"] == 1 or a["dgg_mode_k_select"] == "edge_p-cdf")
    on = np.zeros((N, N), bool)
    on[fx["rows"], fx["cols"]] = True
    err_on = np.abs(fx["out"][fx["rows"], fx["cols"]] - q).max()
    off = np.abs(fx["out"][~on]).max()
    print(f"{tag}: on-pattern |ref - oracle| max {err_on:.3e}, off-pattern |ref| max {off:.3e}, q max {q.max():.3f}")
    assert err_on <= 1e-5
    assert off <= 1e-5
    assert off == pytest.approx(fx["meta"]["off_pattern_max"]) and off < 1e-6
    assert int(np.diff(csr_from_coo(fx["rows"], fx["cols"], N)[0]).max()) > 64
    if a["symmetric_noise"]:
        assert np.array_equal(fx["G"], fx["G"].T) and not fx["G"].diagonal().any()


# ---------------------------------------------------------------------------------------------------------------
# GPU: the kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["explicit", "hash", "hash_sym"])
def test_csr_perturb_bit_exact(dev, mode):
    from dgg_amd import ops
    rng = np.random.default_rng(31)
    N, seed = 130, (77, 5)
    lens = np.concatenate([[0, 1, 63, 64, 65, 130], rng.integers(0, 21, N - 6)])
    rowptr, col, erow = rows_to_csr(lens, N, rng)
    p = probabilities(len(col), rng)
    if mode == "explicit":
        nm, G = ops.NOISE_EXPLICIT, grid_gumbel(301, (N, N))
    else:
        nm = ops.NOISE_HASH if mode == "hash" else ops.NOISE_HASH_SYM
        G = O.noise_matrix(N, seed[0], seed[1], symmetric=mode == "hash_sym")
    Gd = T(G, dev) if mode == "explicit" else None
    q = Nn(ops.csr_perturb_fwd(T(p, dev), T(erow, dev), T(col, dev), N, nm, Gd, seed))
    ref = compose(p, erow, col, G)
    assert np.array_equal(q.view(np.uint32), ref.view(np.uint32))
    assert np.isfinite(q).all() and (q > 0).all()
    # the scores the top-k search of the same rows ranks (oracle), matched through eid; rows of at most 64 entries are listed whole
    idx, val, eid = O.edgelist_topk_p(p, N, rowptr, col, 64, nm, G if mode == "explicit" else None, seed)
    narrow = lens <= 64
    m = (eid >= 0) & narrow[:, None]
    assert int(m.sum()) == int(lens[narrow].sum())
    assert np.array_equal(q[eid[m]].view(np.uint32), val[m].view(np.uint32))
    if mode != "explicit":                       # the ranked generators do not apply to stored entries: mapped to the per-pair hash
        ranked = ops.NOISE_RANKED if mode == "hash" else ops.NOISE_RANKED_SYM
        assert np.array_equal(Nn(ops.csr_perturb_fwd(T(p, dev), T(erow, dev), T(col, dev), N, ranked, None, seed)), q)
    if mode == "hash_sym":                       # constant p on a symmetric pattern: q symmetric bitwise, diagonal unperturbed
        r, c = symmetric_graph(N, 12, rng)
        pc = np.full(len(r), 0.37, F32)
        qs = Nn(ops.csr_perturb_fwd(T(pc, dev), T(r.astype(np.int32), dev), T(c.astype(np.int32), dev), N, nm, None, seed))
        D = np.zeros((N, N), F32)
        D[r, c] = qs
        assert np.array_equal(D.view(np.uint32), D.T.copy().view(np.uint32))
        assert len(np.unique(qs)) > len(qs) // 4
        d0 = F32(O.exp(O.log(F32(0.37) + F32(1e-8))))
        assert np.array_equal(D.diagonal(), np.full(N, d0, F32))


@pytest.mark.gpu
def test_csr_perturb_sizes(dev):
    """grid tails and out-of-range writes: the C entry points write into buffers between guard words"""
    from dgg_amd import _lib, ops
    rng = np.random.default_rng(32)
    N, GUARD = 97, 64
    G = grid_gumbel(302, (N, N))
    Gd = T(G, dev)
    L = _lib.lib()
    for nnz in (0, 1, 255, 256, 257, 5000):
        flat = np.sort(rng.choice(N * N, size=nnz, replace=False))
        erow, col = (flat // N).astype(np.int32), (flat % N).astype(np.int32)
        p = probabilities(nnz, rng) if nnz else np.zeros(0, F32)
        dq = rng.standard_normal(nnz).astype(F32)
        pd, ed, cd, dqd = T(p, dev), T(erow, dev), T(col, dev), T(dq, dev)
        qbuf = torch.full((nnz + 2 * GUARD,), -7.0, device=dev)
        dbuf = torch.full((nnz + 2 * GUARD,), -7.0, device=dev)
        qv, dv = qbuf[GUARD:GUARD + nnz], dbuf[GUARD:GUARD + nnz]
        _lib.check(L.dgg_csr_perturb_fwd(ops._ptr(pd), ops._ptr(ed), ops._ptr(cd), nnz, N, ops.NOISE_EXPLICIT, ops._ptr(Gd), N, 0, 0,
                                         ops._ptr(qv), ops._stream()), "csr_perturb_fwd")
        _lib.check(L.dgg_csr_perturb_bwd(ops._ptr(pd), ops._ptr(qv), ops._ptr(dqd), nnz, ops._ptr(dv), ops._stream()), "csr_perturb_bwd")
        torch.cuda.synchronize()
        for buf in (qbuf, dbuf):
            assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[GUARD + nnz:] == -7.0).all()), f"nnz={nnz}: guard words overwritten"
        q = Nn(qv)
        assert np.array_equal(q, compose(p, erow, col, G)), f"nnz={nnz}"
        ref = dq.astype(np.float64) * q.astype(np.float64) / (p.astype(np.float64) + 1e-8)
        assert np.all(np.abs(Nn(dv) - ref) <= 1e-6 * np.abs(ref)), f"nnz={nnz}"
        # the tensor-level wrappers on the same sizes (nnz == 0 launches nothing)
        q2 = ops.csr_perturb_fwd(pd, ed, cd, N, ops.NOISE_EXPLICIT, Gd)
        assert q2.shape == (nnz,) and np.array_equal(Nn(q2), q)
        assert np.array_equal(Nn(ops.csr_perturb_bwd(pd, q2, dqd)), Nn(dv))
    with pytest.raises(_lib.DggHipError):       # unperturbed / ranked modes are the caller's business
        _lib.check(L.dgg_csr_perturb_fwd(ops._ptr(pd), ops._ptr(ed), ops._ptr(cd), nnz, N, ops.NOISE_NONE, None, 0, 0, 0, ops._ptr(qv),
                                         ops._stream()), "csr_perturb_fwd")


@pytest.mark.gpu
def test_csr_perturb_backward(dev):
    """dp = dq q / (p + 1e-8) against float64 with the kernel's own q; through autograd the same bits"""
    from dgg_amd import ops
    rng = np.random.default_rng(33)
    N = 130
    lens = np.concatenate([[0, 1, 63, 64, 65, 130], rng.integers(0, 21, N - 6)])
    rowptr, col, erow = rows_to_csr(lens, N, rng)
    p = probabilities(len(col), rng)
    dq = rng.standard_normal(len(col)).astype(F32)
    pd = T(p, dev).requires_grad_(True)
    q = ops.CsrPerturbFn.apply(pd, T(rowptr, dev), T(col, dev), T(erow, dev), N, ops.NOISE_HASH, None, (9, 10))
    q.backward(T(dq, dev))
    dp = Nn(ops.csr_perturb_bwd(pd.detach(), q.detach(), T(dq, dev)))
    assert np.array_equal(Nn(pd.grad), dp)
    ref = dq.astype(np.float64) * Nn(q).astype(np.float64) / (p.astype(np.float64) + 1e-8)
    rel = np.abs(dp - ref) / np.abs(ref)
    print(f"csr_perturb_bwd: relative error max {rel.max():.3e}")
    assert rel.max() <= 1e-6
    # = dq exp(G), the noise read back from the oracle's generator.  q / (p + 1e-8) carries the roundings of the forward: log p + G
    # (|.| <= 18.5, half an ulp there is 9.5e-7) is rounded twice and goes through exp (~2 ulp): under 3e-6 in all, bound 1e-5
    G = O.noise_matrix(N, 9, 10)[erow, col].astype(np.float64)
    assert np.abs(dp / (dq.astype(np.float64) * np.exp(G)) - 1).max() <= 1e-5


@pytest.mark.gpu
def test_perturbed_scores_match_the_ranked_path_on_the_same_seed(dev):
    """the debug view shows exactly what the selector ranks: GPU against GPU, bitwise, matched by column"""
    from dgg_amd import ops
    rng = np.random.default_rng(34)
    N, seed = 300, (2024, 3)
    lens = np.concatenate([[0, 64, 1, 63], rng.integers(0, 65, N - 4)])
    rowptr, col, erow = rows_to_csr(lens, N, rng)
    pd = T(probabilities(len(col), rng), dev)
    q = ops.csr_perturb_fwd(pd, T(erow, dev), T(col, dev), N, ops.NOISE_HASH, None, seed)
    idx, val, _ = ops.edgelist_topk_p(pd, N, T(rowptr, dev), T(col, dev), 64, ops.NOISE_HASH, None, seed)
    Dq = torch.zeros((N, N), device=dev, dtype=torch.int32)
    Dq[T(erow, dev).long(), T(col, dev).long()] = q.view(torch.int32)
    sel = idx >= 0
    assert int(sel.sum()) == len(col)
    Dv = torch.zeros((N, N), device=dev, dtype=torch.int32)
    Dv[torch.arange(N, device=dev)[:, None].expand_as(idx)[sel], idx[sel].long()] = val.view(torch.int32)[sel]
    assert torch.equal(Dq, Dv)


# ---------------------------------------------------------------------------------------------------------------
# GPU: the modules
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tag", PERT_FIXTURES)
def test_perturbed_scores_module_matches_reference_golden(dev, tag):
    """DGG_LearnableK_debug with debug_step 1 / edge_p-cdf and perturb_edge_prob: CsrAdjacency on the pattern of in_adj, values ==
    oracle composition bit-for-bit, reference to 1e-5, gradients of x and of every parameter that receives one to 3e-4"""
    import dgg_amd
    from argparse import Namespace
    fx, _, q = golden_composition(tag)
    meta = fx["meta"]
    N = meta["N"]
    m = dgg_amd.DGG_LearnableK_debug(in_dim=meta["d"], latent_dim=meta["h"], args=Namespace(**meta["args"]))
    m.load_state_dict({k_[2:]: torch.from_numpy(v) for k_, v in fx.items() if k_.startswith("p.")}, strict=True)
    m = m.to(dev).eval()
    m.set_noise(T(fx["G"], dev))
    A = coo(fx["rows"], fx["cols"], fx["adj_vals"], N, dev)
    x = T(fx["x"], dev).requires_grad_(True)
    adj = m(x, A)
    assert isinstance(adj, dgg_amd.CsrAdjacency)
    assert np.array_equal(Nn(adj.erow), fx["rows"]) and np.array_equal(Nn(adj.col), fx["cols"])
    assert np.array_equal(Nn(adj.values()).view(np.uint32), q.view(np.uint32))
    err = np.abs(Nn(adj.to_dense()) - fx["out"]).max()
    print(f"{tag}: |module - reference| max {err:.3e}")
    assert err <= 1e-5
    (adj.to_dense() * T(fx["cot"], dev)).sum().backward()
    grads = {n_: p_.grad for n_, p_ in m.named_parameters()}
    grads["x"] = x.grad
    checked = 0
    for key, got in grads.items():
        ref = fx["g." + key]
        if np.abs(ref).max() == 0:
            assert got is None or float(got.abs().max()) == 0, key
            continue
        e = np.abs(Nn(got).reshape(ref.shape) - ref).max() / np.abs(ref).max()
        print(f"{tag}: grad {key} rel-to-max error {e:.3e}")
        assert e <= 3e-4, f"grad {key}: {e:.3e}"
        checked += 1
    assert checked >= 3
    assert bool(torch.isfinite(adj.normalize().matmul(T(fx["x"], dev))).all())


@pytest.mark.gpu
def test_perturbed_scores_counter_noise_through_the_module(dev):
    """noise from _noise_cfg: set_seed reproduces, another seed differs, no seed draws fresh noise per forward; symmetric noise on
    a symmetric pattern gives a bitwise symmetric matrix"""
    import dgg_amd
    rng = np.random.default_rng(35)
    N, d = 150, 20
    r, c = symmetric_graph(N, 10, rng)
    A = coo(r, c, np.ones(len(r)), N, dev)
    x = T(rng.standard_normal((N, d)).astype(F32), dev)
    for sym in (False, True):
        torch.manual_seed(3)
        m = dgg_amd.DGG_LearnableK_debug(in_dim=d, latent_dim=16, args=mk_args(debug_step=1, symmetric_noise=sym)).to(dev).eval()
        plain = dgg_amd.DGG_LearnableK_debug(in_dim=d, latent_dim=16, args=mk_args(debug_step=1, perturb_edge_prob=False)).to(dev).eval()
        plain.load_state_dict(m.state_dict())
        f1, f2 = m(x, A).values(), m(x, A).values()
        assert not torch.equal(f1, f2), "no seed: fresh noise per forward"
        m.set_seed(5, 6)
        a1, a2 = m(x, A), m(x, A)
        assert torch.equal(a1.values(), a2.values())
        m.set_seed(7, 8)
        b = m(x, A)
        assert not torch.equal(a1.values(), b.values())
        assert not torch.equal(a1.values(), plain(x, A).values())
        D = a1.to_dense()
        if sym:
            assert torch.equal(D.view(torch.int32), D.T.contiguous().view(torch.int32))
            assert torch.equal(D.diagonal(), b.to_dense().diagonal())       # the symmetric diagonal is unperturbed under every seed
        else:
            assert not torch.equal(D, D.T)


@pytest.mark.gpu
def test_gcn_dgg_runs_with_cdf_selector_under_noise(dev):
    """GCN_DGG with --dgg_mode_k_select edge_p-cdf --perturb_edge_prob true trains: logits and gradients against a dense float64
    restatement -- (p + 1e-8) exp(G) on the pattern of in_adj + I, normalize_adj, two GCNConv layers.  Features of scale 0.5 keep
    the activations O(1), where fp32 rounding over the few dozen terms of a row stays well inside the 1e-5 forward bar."""
    import dgg_amd
    rng = np.random.default_rng(36)
    N, d, h, C = 200, 32, 16, 5
    r, c = symmetric_graph(N, 8, rng, self_loops=False)
    A = coo(r, c, np.ones(len(r)), N, dev)
    x0 = (0.5 * rng.standard_normal((N, d))).astype(F32)
    G = grid_gumbel(303, (N, N))
    cot = grid_normal(304, (N, C))
    torch.manual_seed(4)
    model = dgg_amd.GCN_DGG(nfeat=d, nhidden=h, nclass=C, args=mk_args(dgg_mode_k_select="edge_p-cdf")).to(dev).eval()
    model.dggs[0].set_noise(T(G, dev))
    logp, adj, _ = model(T(x0, dev), A)
    (logp * T(cot, dev)).sum().backward()
    assert isinstance(adj, dgg_amd.CsrAdjacency)
    assert any("k-select" in why for why in model.dggs[0].fused_fallback), model.dggs[0].fused_fallback
    # dense float64 restatement
    g = model.dggs[0]
    We = g.node_encode_for_edges[0].weight.detach().double().cpu().requires_grad_(True)
    be = g.node_encode_for_edges[0].bias.detach().double().cpu()
    W1 = model.conv1.W.detach().double().cpu().requires_grad_(True)
    W2 = model.conv2.W.detach().double().cpu()
    xd = torch.from_numpy(x0).double()
    mask = torch.zeros(N, N, dtype=torch.float64)
    mask[torch.from_numpy(r), torch.from_numpy(c)] = 1.0
    mask.fill_diagonal_(1.0)                                          # the wrapper adds the self loops (model.py:1249-1264)
    xp = torch.nn.functional.leaky_relu(xd @ We.T + be)
    eye = torch.eye(N, dtype=torch.float64)
    dist = torch.sqrt(((xp[:, None, :] - xp[None, :, :]) ** 2).sum(-1) + eye) * (1 - eye)       # zero distance: gradient 0, as torch's norm
    p = torch.exp(-0.05 * dist)
    Q = (p + 1e-8) * torch.exp(torch.from_numpy(G).double()) * mask
    rs = Q.sum(1)
    Ah = Q / torch.sqrt(rs)[:, None] / torch.sqrt(rs)[None, :]
    z = torch.relu(Ah @ torch.relu(Ah @ xd @ W1) @ W2)
    ref = torch.log_softmax(z, -1)
    (ref * torch.from_numpy(cot).double()).sum().backward()
    err = float((logp.detach().cpu().double() - ref.detach()).abs().max())
    print(f"GCN_DGG edge_p-cdf under noise: |logits - float64| max {err:.3e}")
    assert err <= 1e-5
    for name_, got, want in (("conv1.W", model.conv1.W.grad, W1.grad), ("node_encode_for_edges.0.weight", g.node_encode_for_edges[0].weight.grad, We.grad)):
        e = float((got.detach().cpu().double() - want).abs().max() / want.abs().max())
        print(f"GCN_DGG edge_p-cdf under noise: grad {name_} rel-to-max error {e:.3e}")
        assert float(want.abs().max()) > 0 and e <= 3e-4, f"grad {name_}: {e:.3e}"
    assert g.signal_project.weight.grad is None and g.k_net.k_project.weight.grad is None      # the learned k never reaches the output
    # what stays outside: dgg_hard (a dense all-ones matrix in the reference) and all-pairs candidates (truly dense)
    xs = T(x0, dev)
    hard = dgg_amd.DGG_LearnableK_debug(in_dim=d, latent_dim=h, args=mk_args(dgg_mode_k_select="edge_p-cdf", dgg_hard=True)).to(dev)
    with pytest.raises(NotImplementedError, match="dgg_hard"):
        hard(xs, A)
    soft = dgg_amd.DGG_LearnableK_debug(in_dim=d, latent_dim=h, args=mk_args(debug_step=1)).to(dev)
    with pytest.raises(NotImplementedError, match="all-pairs"):
        soft(xs, dgg_amd.AllPairs(torch.full((N,), 8.0, device=dev)))
