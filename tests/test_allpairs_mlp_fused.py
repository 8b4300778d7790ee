"""Edge-MLP scorers (u-v-deg / u-v-deg-dist / edge_conv) on all-pairs candidates inside the FUSED layer (DGG_LearnableK_debug.forward_conv
on dgg_amd.parallel.ShardedDGGConv; opt-in args.dgg_allpairs_mlp_fused = True), list and chunked form, and the kernel the chunked form adds: dgg_softk_bwd_rows_chunked, the ramp +
normalisation backward on the chunked rows of a row shard.

Bars.  Kernel against float64 (cases 1, 3): rtol = 2e-4, atol = 2e-4 x the largest reference entry -- the bars of
test_softk_bwd_chunked_matches_the_float64_oracle (tests/test_allpairs_mlp_wide.py), whose kernel this one extends by the normalisation.
The reference is torch CPU float64 autograd of sum(dA * ahat), ahat_ir = w_ir rs_i^-1/2 rs_j^-1/2, w = the ramp (times the score in mode
0), rs = the row sums of w; the kernel's inputs rs / ahat / da_cols are that computation's float64 values cast to float32 (relative error
6e-8 each, three orders below the bar).  Row ranges (case 2): bit for bit -- rs and da_cols are global and a row depends on nothing else.
Fused layer against the separate modules (cases 5, 6): the bars of test_gcn_dgg_fused_first_layer_matches_the_separate_modules
(tests/test_hip_parity.py): identical neighbour lists on weighted entries, values atol 1e-6, log-probabilities 1e-5, every parameter's
gradient within 3e-4 of its largest entry."""
import copy
from argparse import Namespace

import numpy as np
import pytest
import torch

from test_allpairs_mlp import PAD, Nn, T, module_args
from test_chunked_rows import chunked_to_rows, rank_limit

pytestmark = pytest.mark.gpu

SCORERS = ("u-v-deg", "u-v-deg-dist", "edge_conv")
NOISES = {"hash": dict(perturb=True, sym=False), "sym": dict(perturb=True, sym=True), "none": dict(perturb=False, sym=False)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------
# the new kernel
# ---------------------------------------------------------------------------------------------------------------
_DATA = {}


def chunk_data(dev, mode, one_chunk=False):
    """301 rows = 301 columns, learned degrees 1 .. 620 (rows of 1 to 10 chunks; one_chunk: k <= 54, one chunk per row), a few empty slots
    inside rows, three spare chunks; random val / dA; float64 reference of sum(dA * ahat).  Computed once per case, shared, read only."""
    key = (mode, one_chunk)
    if key in _DATA:
        return _DATA[key]
    from dgg_amd import ops
    rows = 301
    rng = np.random.default_rng(5 + mode + 10 * one_chunk)
    if one_chunk:
        k = (1.0 + 53.0 * rng.random(rows)).astype(np.float32)
        k[:3] = (1.0, 54.0, 30.0)
    else:
        k = (1.0 + 620.0 * rng.random(rows) ** 2).astype(np.float32)
        k[:5] = (1.0, 54.5, 54.6, 118.49, 620.0)
    kd = T(k, dev)
    lay = ops.chunk_layout(kd, ncols=4096)                   # (ncols only caps a row's width: 65 chunks, beyond every row here)
    L = rank_limit(k, 64 * ops.chunk_maxm_for(4096))
    if one_chunk:
        assert lay.chunks == rows and lay.maxm == 1 and not lay.wide
    else:
        assert lay.maxm == 10 and int(Nn(lay.cptr)[1]) == 1, "rows of 1 to 10 chunks"
    C = lay.chunks + 3                                       # (spare chunks: dval comes back 0 there)
    rank = np.full((C, 64), 1 << 30, np.int64)
    rank[:lay.chunks] = Nn(lay.ranks())
    Lc = np.zeros(C, np.int64)
    cnode = np.zeros(C, np.int64)
    cnode[:lay.chunks] = Nn(lay.cnode).astype(np.int64)
    Lc[:lay.chunks] = L[cnode[:lay.chunks]]
    live = (rank < Lc[:, None]) & (rng.random((C, 64)) > 0.05)          # empty beyond L_i, and a few empty slots inside
    live[:lay.chunks][rank[:lay.chunks] == 0] = True                     # (rank 0 stays: every row sum is positive)
    idx = np.where(live, rng.integers(0, rows, (C, 64)), -1).astype(np.int32)
    val = np.where(live, 0.05 + 0.95 * rng.random((C, 64)), 0).astype(np.float32)
    dA = rng.standard_normal((C, 64)).astype(np.float32)
    # float64 autograd of sum(dA * ahat) over the live entries
    v = torch.from_numpy(val).double().requires_grad_(True)
    kk = torch.from_numpy(k).double().requires_grad_(True)
    lv = torch.from_numpy(live)
    node = torch.from_numpy(cnode)
    f = 1 - 0.5 * (1 + torch.tanh(torch.from_numpy(np.minimum(rank, 1 << 20)).double() - kk[node][:, None]))
    w = torch.where(lv, v * f if mode == 0 else f, torch.zeros_like(f))
    rs = torch.zeros(rows, dtype=torch.float64).index_add(0, node, w.sum(1))
    a = rs.rsqrt()
    j = torch.from_numpy(np.maximum(idx, 0)).long()
    ahat = w * a[node][:, None] * a[j]
    (torch.from_numpy(dA).double() * ahat).sum().backward()
    # the neighbour-side sums of d loss / d (rs^-1/2): da_cols[j] = sum over the entries (i, r) with idx = j of dA_ir w_ir a_i
    contrib = (torch.from_numpy(dA).double() * w * a[node][:, None]).detach()
    da_cols = torch.zeros(rows, dtype=torch.float64).index_add(0, j[lv], contrib[lv])
    ref_dval = np.where(live, v.grad.numpy(), 0.0) if mode == 0 else np.zeros((C, 64))
    d = dict(rows=rows, k=k, kd=kd, lay=lay, C=C, live=live, idx=T(idx, dev), val=T(val, dev), dA=T(dA, dev),
             rs=rs.detach().float().to(dev), ahat=ahat.detach().float().to(dev).contiguous(), da_cols=da_cols.float().to(dev),
             ref_dval=ref_dval, ref_dk=kk.grad.numpy())
    _DATA[key] = d
    return d


class Canaried:
    """dval [C,64] and dk [rows] handed to the kernel as views between canary words (NaN)"""

    def __init__(self, C, rows, dev):
        self.n, self.rows = C * 64, rows
        self.bv = torch.full((self.n + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)
        self.bk = torch.full((rows + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)

    def views(self):
        return self.bv[PAD:PAD + self.n].view(-1, 64), self.bk[PAD:PAD + self.rows]

    def canaries_intact(self):
        return all(bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[PAD + n:]).all()) for b, n in ((self.bv, self.n), (self.bk, self.rows)))

    def untouched(self):
        return bool(torch.isnan(self.bv).all()) and bool(torch.isnan(self.bk).all())


def run_kernel(d, mode, out=None):
    from dgg_amd import ops
    return ops.softk_bwd_rows_chunked(d["idx"], d["val"], d["kd"], d["rs"], d["dA"], d["da_cols"], d["ahat"], d["lay"], 0, mode, out=out)


@pytest.mark.parametrize("mode", [0, 1])
def test_softk_bwd_rows_chunked_matches_the_float64_autograd(dev, mode):
    d = chunk_data(dev, mode)
    buf = Canaried(d["C"], d["rows"], dev)
    dval, dk = run_kernel(d, mode, out=buf.views())
    dval2, dk2 = run_kernel(d, mode)
    assert torch.equal(bits(dk), bits(dk2)) and torch.equal(bits(dval), bits(dval2)), "not deterministic"
    assert buf.canaries_intact(), "written outside dval / dk"
    dead = torch.from_numpy(~d["live"]).to(dev)
    assert bool((dval[dead] == 0).all()) and bool((dval[d["lay"].chunks:] == 0).all()), "empty slots and spare chunks must get dval = 0"
    rdval, rdk = d["ref_dval"], d["ref_dk"]
    print(f"mode {mode}: max|dval - ref| = {np.abs(Nn(dval) - rdval).max():.3e} of {np.abs(rdval).max():.3e}, "
          f"max|dk - ref| = {np.abs(Nn(dk) - rdk).max():.3e} of {np.abs(rdk).max():.3e}")
    np.testing.assert_allclose(Nn(dval), rdval, rtol=2e-4, atol=2e-4 * np.abs(rdval).max())
    np.testing.assert_allclose(Nn(dk), rdk, rtol=2e-4, atol=2e-4 * np.abs(rdk).max())


@pytest.mark.parametrize("mode", [0, 1])
def test_row_ranges_equal_the_slices_of_the_whole_call(dev, mode):
    from dgg_amd import ops
    d = chunk_data(dev, mode)
    lay = d["lay"]
    dval, dk = run_kernel(d, mode)
    cptr = Nn(lay.cptr).astype(np.int64)
    for r0, r1 in ((0, 97), (97, 301)):
        c0, c1 = int(cptr[r0]), int(cptr[r1])
        ls = ops.ChunkLayout((lay.cptr[r0:r1 + 1] - c0).contiguous(), (lay.cnode[c0:c1] - r0).contiguous(), lay.meta, c1 - c0, lay.maxm, r1 - r0)
        sl = lambda t_: t_[c0:c1].contiguous()  # noqa: E731
        buf = Canaried(c1 - c0, r1 - r0, dev)
        pv, pk = ops.softk_bwd_rows_chunked(sl(d["idx"]), sl(d["val"]), d["kd"][r0:r1].contiguous(), d["rs"], sl(d["dA"]), d["da_cols"],
                                            sl(d["ahat"]), ls, r0, mode, out=buf.views())
        assert torch.equal(bits(pv), bits(dval[c0:c1])) and torch.equal(bits(pk), bits(dk[r0:r1])), f"rows {r0}:{r1}"
        assert buf.canaries_intact(), f"rows {r0}:{r1}: written outside the range"


@pytest.mark.parametrize("mode", [0, 1])
def test_one_chunk_per_row_matches_the_list_kernel(dev, mode):
    """k <= 54: every row is one chunk, and the kernel computes what dgg_softk_bwd_rows computes on the [rows,64] list"""
    from dgg_amd import ops
    d = chunk_data(dev, mode, one_chunk=True)
    n = d["rows"]
    dval, dk = run_kernel(d, mode)
    lval, lk = ops.softk_bwd(d["idx"][:n].contiguous(), d["val"][:n].contiguous(), d["kd"], d["dA"][:n].contiguous(), d["rs"], d["da_cols"], 0, mode,
                             True, ahat_rows=d["ahat"][:n].contiguous())
    same = torch.equal(bits(dval[:n]), bits(lval)) and torch.equal(bits(dk), bits(lk))
    print(f"mode {mode}: one chunk per row against dgg_softk_bwd_rows: bits equal = {same}, max|dval diff| = "
          f"{float((dval[:n] - lval).abs().max()):.3e}, max|dk diff| = {float((dk - lk).abs().max()):.3e}")
    for got, lst, ref in ((Nn(dval), Nn(lval), d["ref_dval"]), (Nn(dk), Nn(lk), d["ref_dk"])):
        np.testing.assert_allclose(got[:len(lst)], lst, rtol=2e-4, atol=2e-4 * np.abs(ref).max())
        np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-4 * np.abs(ref).max())


@pytest.mark.parametrize("what", ["idx", "val", "k", "rs", "dA", "da_cols", "ahat", "cptr", "dval", "dk", "mode=2", "row0=-1"])
def test_refusals_return_the_code_and_write_nothing(dev, what):
    from dgg_amd import _lib
    d = chunk_data(dev, 0)
    buf = Canaried(d["C"], d["rows"], dev)
    dval, dk = buf.views()
    ptr = lambda t_: t_.data_ptr()  # noqa: E731
    a = dict(idx=ptr(d["idx"]), val=ptr(d["val"]), k=ptr(d["kd"]), rs=ptr(d["rs"]), dA=ptr(d["dA"]), da_cols=ptr(d["da_cols"]), ahat=ptr(d["ahat"]),
             rows=d["rows"], cptr=ptr(d["lay"].cptr), ccap=d["C"], row0=0, mode=0, dval=ptr(dval), dk=ptr(dk))
    if "=" in what:
        key, _, v = what.partition("=")
        a[key] = int(v)
    else:
        a[what] = None
    order = ("idx", "val", "k", "rs", "dA", "da_cols", "ahat", "rows", "cptr", "ccap", "row0", "mode", "dval", "dk")
    code = _lib.lib().dgg_softk_bwd_rows_chunked(*[a[n] for n in order], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == 1, "DGG_ERR_ARG"
    assert buf.untouched()
    a.update(idx=ptr(d["idx"]), rows=0, mode=0, row0=0, dval=ptr(dval), dk=ptr(dk))
    if what == "idx":                                        # an empty shard: 0, no launch, nothing written
        assert _lib.lib().dgg_softk_bwd_rows_chunked(*[a[n] for n in order], torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert buf.untouched()


# ---------------------------------------------------------------------------------------------------------------
# the fused layer against the separate modules
# ---------------------------------------------------------------------------------------------------------------
def degree_following_knet(dgg):
    """k-net weights under which the learned degree follows the prior degree, k_i ~ prior_i + 1 (+ a small learned part): two hidden
    units carry +nd and -nd (nd = the normalised prior degree, the k-net's last input), the mean layer takes their difference
    (leaky(a) - leaky(-a) = 1.01 a) and the projection passes it on, so kp ~ nd and k = relu(kp sd + mu) + 1 ~ prior + 1.  The rest of
    the k-net keeps its random weights, the projection's scaled by 0.1 as in tests/test_allpairs_mlp_wide.py."""
    with torch.no_grad():
        kn = dgg.k_net
        kn.k_project.weight.mul_(0.1)
        W1, b1 = dgg.k_embed[0].weight, dgg.k_embed[0].bias
        W1[:2] = 0.0
        W1[0, -1], W1[1, -1] = 1.0, -1.0
        b1[:2] = 0.0
        kn.k_mu.weight[:, :2] = 0.0
        kn.k_mu.weight[0, 0], kn.k_mu.weight[0, 1] = 1.0 / 1.01, -1.0 / 1.01
        kn.k_project.weight[0, 0] = 1.0


def model_pair(dev, scorer, noise, N, d, h, C, chunked):
    import dgg_amd
    kw = dict(dgg_allpairs_mlp_rows="chunked") if chunked else {}
    args = module_args(scorer, dgg_wide_rows="auto", dgg_allpairs_mlp_fused=True, **NOISES[noise], **kw)
    torch.manual_seed(3)
    m1 = dgg_amd.GCN_DGG(nfeat=d, nhidden=h, nclass=C, args=args).to(dev).eval()        # eval: no dropout between the layers
    with torch.no_grad():
        # The 1e-5 bar on the log-probabilities is absolute, set in the referenced test for logits |z| of a few units (conv2.W x 0.2,
        # constant priors: 1e-5 is ~40 ulp of z there); what the two paths differ by is the summation order of the aggregations, an
        # error proportional to |z|.  normalize_adj amplifies a row of ~200 ranks among neighbours of ~20 by sqrt(200 / 20) ~ 3.2 per
        # layer, ~10 over the two layers, so the chunked case scales conv2.W by 0.02 to keep the logits at the magnitude the bar was
        # set for (measured with x 0.2: |z| up to 16, and u-v-deg-dist / hash missed the bar by 2.7e-5 on 2 of 8400 entries)
        m1.conv2.W.mul_(0.02 if chunked else 0.2)
        if chunked:
            degree_following_knet(m1.dggs[0])
        else:
            m1.dggs[0].k_net.k_project.weight.mul_(0.1)
    m2 = copy.deepcopy(m1)
    m2.dggs[0].args = Namespace(**dict(vars(args), dgg_fused_layer=False))
    for m in (m1, m2):
        m.dggs[0].set_seed(77, 5)
    return m1, m2


def compare_fused_with_separate(dev, scorer, noise, prior, chunked):
    N, d, h, C = 1200, 40, 32, 7
    import dgg_amd
    m1, m2 = model_pair(dev, scorer, noise, N, d, h, C, chunked)
    x = torch.rand(N, d, generator=torch.Generator().manual_seed(1)).to(dev)
    A = dgg_amd.AllPairs(prior.to(dev))
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(2)).to(dev)
    outs = []
    for m in (m1, m2):
        logp, adj, _ = m(x, A)
        torch.nn.functional.nll_loss(logp, y).backward()
        outs.append((logp, adj))
    g1, g2 = m1.dggs[0], m2.dggs[0]
    assert g1.__dict__.get("_fused_layer") is not None and g2.__dict__.get("_fused_layer") is None
    assert not g1.__dict__.get("fused_fallback") and g2.fused_fallback == {"args.dgg_fused_layer = False": 1}
    for m in (m1, m2):
        m.dggs[0].check_ell_bound()
    a1, a2 = outs[0][1], outs[1][1]
    assert (a1.layout is not None) == chunked and (a2.layout is not None) == chunked
    kept = a2.idx >= 0
    assert a1.idx.shape == a2.idx.shape
    assert torch.equal(a1.idx[kept & (a1.values() != 0)], a2.idx[kept & (a1.values() != 0)])
    np.testing.assert_allclose(Nn(a1.values()), Nn(a2.values()), rtol=0, atol=1e-6)
    np.testing.assert_allclose(Nn(outs[0][0]), Nn(outs[1][0]), rtol=1e-5, atol=1e-5)
    worst = ("", 0.0)
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        if p2.grad is None:
            assert p1.grad is None or float(p1.grad.abs().max()) == 0.0, n1
            continue
        ref = Nn(p2.grad)
        assert p1.grad is not None, n1
        err = np.abs(Nn(p1.grad) - ref).max() / max(np.abs(ref).max(), 1e-30)
        worst = max(worst, (n1, err), key=lambda t_: t_[1])
        assert err <= 3e-4, f"{n1}: {err:.2e}"
    print(f"{scorer} / {noise} / {'chunked' if chunked else 'list'}: largest gradient error {worst[1]:.2e} of max ({worst[0]})")
    own = ("edge_conv_phi.weight", "edge_conv_theta.weight", "edge_conv_encode.weight") if scorer == "edge_conv" else \
        ("edge_encode.0.weight", "edge_encode.0.bias", "edge_encode.2.weight", "edge_encode.2.bias")
    for n_ in own:                                           # the scorer's own parameters have gradients
        p_ = dict(g1.named_parameters())[n_]
        assert p_.grad is not None and float(p_.grad.abs().max()) > 0, n_
    return a1, a2


@pytest.mark.parametrize("noise", list(NOISES))
@pytest.mark.parametrize("scorer", SCORERS)
def test_fused_layer_matches_the_separate_modules(dev, scorer, noise):
    """(fails before this feature at the fused_fallback assertion: clause "edge-MLP scorer on all-pairs candidates", which now stands
    only without the opt-in)"""
    prior = torch.randint(6, 31, (1200,), generator=torch.Generator().manual_seed(4)).float()      # spread over 6 .. 30, not a constant
    compare_fused_with_separate(dev, scorer, noise, prior, chunked=False)


@pytest.mark.parametrize("noise", list(NOISES))
@pytest.mark.parametrize("scorer", SCORERS)
def test_fused_layer_matches_the_separate_modules_on_chunked_rows(dev, scorer, noise):
    """args.dgg_allpairs_mlp_rows = "chunked", learned degrees ~ 200 on every eighth row and under 40 on the others: the fused node's
    idx / val / w equal _DGGAllPairsMlpWideAdjFn's (the separate modules' node) bit for bit"""
    g = torch.Generator().manual_seed(4)
    prior = torch.randint(6, 31, (1200,), generator=g).float()
    prior[::8] = torch.randint(150, 200, (150,), generator=g).float()
    a1, a2 = compare_fused_with_separate(dev, scorer, noise, prior, chunked=True)
    k = a1.k
    print(f"{scorer} / {noise}: k in {float(k.min()):.1f} .. {float(k.max()):.1f}, {a1.layout.chunks} chunks for {a1.layout.rows} rows")
    assert float(k.max()) > 150 and float(k.min()) < 40 and a1.layout.wide
    assert torch.equal(bits(a1.k), bits(a2.k)) and torch.equal(a1.layout.cptr, a2.layout.cptr)
    assert torch.equal(a1.idx, a2.idx), "idx"
    assert torch.equal(bits(a1.score), bits(a2.score.detach())), "val"
    assert torch.equal(bits(a1.values()), bits(a2.values().detach())), "w"


def test_gcn_dgg_trains_past_the_list_inside_the_fused_layer(dev):
    """GCN_DGG with the reference script's default scorer, opt-in chunked rows: Adam steps push k_max past the 64-rank list, and every
    step runs the fused layer (after test_gcn_dgg_trains_past_the_list_with_the_opt_in, tests/test_allpairs_mlp_wide.py)"""
    import dgg_amd
    N, d_in, h, C = 600, 40, 32, 7
    args = module_args("u-v-deg", dgg_wide_rows="auto", dgg_allpairs_mlp_rows="chunked", dgg_allpairs_mlp_fused=True)
    torch.manual_seed(3)
    model = dgg_amd.GCN_DGG(nfeat=d_in, nhidden=h, nclass=C, args=args).to(dev)
    with torch.no_grad():
        model.dggs[0].k_net.k_project.weight.mul_(0.1)
    x = torch.rand(N, d_in, generator=torch.Generator().manual_seed(1)).to(dev)
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(2)).to(dev)
    # priors around 52: the learned degree k = relu(kp sd + mu) + 1 starts just below the list's bound k + 8.5 = 64
    A = dgg_amd.AllPairs(torch.randint(44, 60, (N,), generator=torch.Generator().manual_seed(4)).float().to(dev))
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    kmax, wide, losses = [], [], []
    for step in range(12):
        opt.zero_grad()
        logp, adj, _ = model(x, A)
        loss = torch.nn.functional.nll_loss(logp, y)
        loss.backward()
        opt.step()
        kmax.append(float(adj.k.max()))
        wide.append(adj.layout is not None)
        losses.append(float(loss.detach()))
    print("k_max per step:", " ".join(f"{v:.1f}" for v in kmax), "| chunked:", "".join("x" if w_ else "." for w_ in wide))
    dgg = model.dggs[0]
    assert dgg.__dict__.get("_fused_layer") is not None and not dgg.__dict__.get("fused_fallback"), "the fused layer ran every step"
    assert all(np.isfinite(losses)) and bool(torch.isfinite(logp).all())
    assert max(kmax) + 8.5 > 64 and any(wide), "the learned degrees must outgrow the 64-rank list in this run"
    dgg.check_ell_bound()
