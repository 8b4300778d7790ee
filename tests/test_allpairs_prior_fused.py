"""u-v-A_uv on all-pairs candidates that carry a prior graph inside the FUSED layer (DGG_LearnableK_debug.forward_conv on
dgg_amd.parallel.ShardedDGGConv; opt-in args.dgg_allpairs_prior_fused = True, alone), list and chunked form, against the separate modules
(args.dgg_fused_layer = False: _DGGAllPairsMlpAdjFn / _DGGAllPairsMlpWideAdjFn with cfg["prior"]).

Bars: those of tests/test_allpairs_mlp_fused.py (compare_fused_with_separate, whose models -- model_pair, degree_following_knet -- are
imported from there; the comparison is restated here because that one builds its candidates without a prior and at N = 1200): identical
neighbour lists on weighted entries, values atol 1e-6, log-probabilities 1e-5, every parameter's gradient within 3e-4 of its largest
entry; on chunked rows idx / val / w / k / cptr bit for bit.

N = 600: not a multiple of 64 and several 64-column tiles -- the smallest size at which a prior cursor crosses tiles and a row block
straddles the end.

What keeps the comparison honest: among the weighted kept entries both prior edges and non-edges make up at least 1 %, and the prior's
column of edge_encode.0.weight (column 2h) has a non-zero gradient inside the bar.  With the random initialisation (seed 3) that column
moves the score of a prior edge from 0.515 to 0.509 -- far below the noise, and downwards -- so that the entries with rank below k + 9,
~28 of 600 columns, hold the 0.7 % of prior edges a random choice would (0.1 % without noise).  The set-up therefore scales the column by
PRIOR_COLUMN_SCALE = -128 (negative: the initialisation's net effect of a positive prior value is negative).  The factor was found on the
CPU with the oracle's scorer + top-K on the complete pattern under these parameters and this prior: the mean score of a prior edge is
then 0.88 against 0.515, and prior edges are 14.4 % (list) / 8.5 % (chunked) of those entries without noise, 3.6 % / 2.8 % under the hash
and the symmetric hash noise, whose Gumbel scale of 1 in log p a score bounded by 1 can only outweigh by log(1 / 0.515) = 0.66
(x -32: 1.6 % / 1.4 %; x -512: 4.9 % / 3.5 %)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from test_allpairs_mlp import Nn, module_args
from test_allpairs_mlp_fused import NOISES, bits, model_pair

pytestmark = pytest.mark.gpu

N_NODES = 600
PRIOR_COLUMN_SCALE = -128.0                                    # of column 2h of edge_encode.0.weight (module docstring)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


def make_prior(N, cross=()):
    """-> the prior graph as a sparse COO [N, N] tensor (CPU): about 4 random entries per row with values in [0.5, 1.5] (multiples of
    2^-7), and the awkward rows: row 2 empty; row 5 storing 80 columns (more than the 64-rank list), every fourth of them negative; row 7
    storing exactly the columns 63, 64, N - 1 and a 0.0 at column 9 (a stored zero means the same as an absent entry); for every b in
    `cross` (a shard boundary) rows b - 1 and b storing the columns b - 2 .. b + 1: entries that cross the boundary in both directions"""
    rng = np.random.default_rng(17 + N)
    stored = rng.random((N, N)) < 4.0 / N
    P = rng.integers(64, 193, (N, N)).astype(np.float64) * 2.0 ** -7
    stored[2] = False
    stored[5] = False
    c5 = np.sort(rng.choice(N, 80, replace=False))
    stored[5, c5] = True
    P[5, c5[::4]] *= -1.0
    stored[7] = False
    stored[7, [9, 63, 64, N - 1]] = True
    P[7, 9] = 0.0
    for b in cross:
        stored[b - 1:b + 1, b - 2:b + 2] = True
    r, c = np.nonzero(stored)
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([r, c])), torch.from_numpy(P[r, c].astype(np.float32)), (N, N)).coalesce()


def prior_degrees(N, chunked, seed=4):
    """prior degrees spread over 6 .. 30 (they are given, not the prior's row sums: AllPairs(deg, prior=P)); chunked: every eighth in
    150 .. 199, which the degree-following k-net turns into learned degrees of that size"""
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(6, 31, (N,), generator=g).float()
    if chunked:
        deg[::8] = torch.randint(150, 200, (len(deg[::8]),), generator=g).float()
    return deg


def opt_in(model, **more):
    """the model's generator under args.dgg_allpairs_prior_fused = True ALONE (model_pair builds its arguments with the other scorers'
    opt-in, dgg_allpairs_mlp_fused, which this scorer does not need)"""
    dgg = model.dggs[0]
    dgg.args = Namespace(**dict(vars(dgg.args), dgg_allpairs_mlp_fused=False, dgg_allpairs_prior_fused=True, **more))


def prior_pair(dev, noise, chunked, d=40, h=32, C=7):
    m1, m2 = model_pair(dev, "u-v-A_uv", noise, N_NODES, d, h, C, chunked)
    for m in (m1, m2):
        with torch.no_grad():
            m.dggs[0].edge_encode[0].weight[:, 2 * h].mul_(PRIOR_COLUMN_SCALE)
    opt_in(m1)
    opt_in(m2, dgg_fused_layer=False)
    return m1, m2


def test_the_prior_holds_what_the_cases_need():
    import dgg_amd
    N = N_NODES
    rowptr, col, val, _ = dgg_amd.AllPairs(torch.ones(N), prior=make_prior(N, cross=(300,))).prior_csr()
    row = lambda i: col[rowptr[i]:rowptr[i + 1]].tolist()  # noqa: E731
    assert row(2) == [] and len(row(5)) == 80 and row(7) == [9, 63, 64, N - 1] and float(val[rowptr[7]]) == 0.0
    assert {298, 299, 300, 301} <= set(row(299)) and {298, 299, 300, 301} <= set(row(300))
    per_row = rowptr.diff().float()
    assert 3.0 < float(per_row.mean()) < 5.5


def compare(dev, noise, chunked):
    import dgg_amd
    N, d, h, C = N_NODES, 40, 32, 7
    m1, m2 = prior_pair(dev, noise, chunked, d, h, C)
    x = torch.rand(N, d, generator=torch.Generator().manual_seed(1)).to(dev)
    P = make_prior(N).to(dev)
    A = dgg_amd.AllPairs(prior_degrees(N, chunked).to(dev), prior=P)
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(2)).to(dev)
    outs = []
    for m in (m1, m2):
        logp, adj, _ = m(x, A)
        torch.nn.functional.nll_loss(logp, y).backward()
        outs.append((logp, adj))
    g1, g2 = m1.dggs[0], m2.dggs[0]
    # (fails before this feature: fused_fallback == {"edge-MLP scorer on all-pairs candidates": 1} and no _fused_layer)
    assert not g1.__dict__.get("fused_fallback") and g1.__dict__.get("_fused_layer") is not None
    assert g2.__dict__.get("_fused_layer") is None and g2.fused_fallback == {"args.dgg_fused_layer = False": 1}
    for m in (m1, m2):
        m.dggs[0].check_ell_bound()
    a1, a2 = outs[0][1], outs[1][1]
    assert (a1.layout is not None) == chunked and (a2.layout is not None) == chunked
    kept = a2.idx >= 0
    assert a1.idx.shape == a2.idx.shape
    weighted = kept & (a1.values() != 0)
    assert torch.equal(a1.idx[weighted], a2.idx[weighted])
    np.testing.assert_allclose(Nn(a1.values()), Nn(a2.values()), rtol=0, atol=1e-6)
    np.testing.assert_allclose(Nn(outs[0][0]), Nn(outs[1][0]), rtol=1e-5, atol=1e-5)
    # prior edges and non-edges among the weighted kept entries
    rows = (a1.layout.cnode.long() if chunked else torch.arange(N, device=dev))[:, None].expand_as(a1.idx)
    on_prior = P.to_dense()[rows[weighted], a1.idx[weighted].long()] != 0
    frac = float(on_prior.float().mean())
    print(f"u-v-A_uv / {noise} / {'chunked' if chunked else 'list'}: {int(weighted.sum())} weighted entries, {100 * frac:.1f} % of them prior edges")
    assert frac >= 0.01 and 1.0 - frac >= 0.01, "the weighted kept entries must hold prior edges and non-edges"
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
    for n_ in ("edge_encode.0.weight", "edge_encode.0.bias", "edge_encode.2.weight", "edge_encode.2.bias"):
        p_ = dict(g1.named_parameters())[n_]
        assert p_.grad is not None and float(p_.grad.abs().max()) > 0, n_
    # the prior's column: a gradient of its own, inside the bar on its own scale
    c1, c2 = Nn(g1.edge_encode[0].weight.grad[:, 2 * h]), Nn(g2.edge_encode[0].weight.grad[:, 2 * h])
    assert np.abs(c2).max() > 0 and np.abs(c1).max() > 0, "edge_encode.0.weight.grad[:, 2h]"
    err_c = np.abs(c1 - c2).max() / np.abs(c2).max()
    print(f"largest gradient error {worst[1]:.2e} of max ({worst[0]}); prior column: {err_c:.2e} of its max {np.abs(c2).max():.2e}")
    assert err_c <= 3e-4, f"edge_encode.0.weight.grad[:, 2h]: {err_c:.2e}"
    return a1, a2


@pytest.mark.parametrize("noise", list(NOISES))
def test_fused_layer_matches_the_separate_modules(dev, noise):
    compare(dev, noise, chunked=False)


@pytest.mark.parametrize("noise", list(NOISES))
def test_fused_layer_matches_the_separate_modules_on_chunked_rows(dev, noise):
    a1, a2 = compare(dev, noise, chunked=True)
    k = a1.k
    print(f"u-v-A_uv / {noise}: k in {float(k.min()):.1f} .. {float(k.max()):.1f}, {a1.layout.chunks} chunks for {a1.layout.rows} rows")
    assert float(k.max()) > 150 and float(k.min()) < 40 and a1.layout.wide
    assert torch.equal(bits(a1.k), bits(a2.k)) and torch.equal(a1.layout.cptr, a2.layout.cptr)
    assert torch.equal(a1.idx, a2.idx), "idx"
    assert torch.equal(bits(a1.score), bits(a2.score.detach())), "val"
    assert torch.equal(bits(a1.values()), bits(a2.values().detach())), "w"


def test_without_the_opt_in_the_forward_keeps_the_separate_modules(dev):
    """args.dgg_allpairs_prior_fused absent: the clause every earlier forward of this configuration was counted under, with or without
    the other scorers' opt-in"""
    import dgg_amd
    N, d, h, C = N_NODES, 40, 32, 7
    x = torch.rand(N, d, generator=torch.Generator().manual_seed(1)).to(dev)
    A = dgg_amd.AllPairs(prior_degrees(N, False).to(dev), prior=make_prior(N).to(dev))
    for kw, clause in (({}, "edge-MLP scorer on all-pairs candidates"),
                       ({"dgg_allpairs_mlp_fused": True}, "edge-MLP scorer on all-pairs candidates that reads the stored values of in_adj (u-v-A_uv / A_uv)")):
        torch.manual_seed(3)
        m = dgg_amd.GCN_DGG(nfeat=d, nhidden=h, nclass=C, args=module_args("u-v-A_uv", dgg_wide_rows="auto", **kw)).to(dev).eval()
        m(x, A)
        assert m.dggs[0].fused_fallback == {clause: 1} and m.dggs[0].__dict__.get("_fused_layer") is None


def test_gcn_dgg_trains_past_the_list_inside_the_fused_layer(dev):
    """GCN_DGG on chunked rows under the opt-in, priors 44 .. 59 (after test_gcn_dgg_trains_past_the_list_inside_the_fused_layer of
    tests/test_allpairs_mlp_fused.py): six Adam steps, every one inside the fused layer, k_max + 8.5 past the 64-rank list.
    The k-net: that test's (k_project.weight x 0.1) gives every row nearly the same degree, the priors' mean, and needs its twelve steps
    to move it -- measured here on an MI355X: k_max 51.5 51.6 51.8 52.0 52.2 52.6 over six steps, the bound is k_max > 55.5 -- so this
    one uses the degree-following k-net of the chunked comparisons, k_i ~ prior_i + 1 in 45 .. 60: the rows with priors above 54 are
    wider than the list from the first step, the others fit it, and Adam moves every row's degree under a layout that is read back
    in every step."""
    import dgg_amd
    from test_allpairs_mlp_fused import degree_following_knet
    N, d_in, h, C = N_NODES, 40, 32, 7
    args = module_args("u-v-A_uv", dgg_wide_rows="auto", dgg_allpairs_mlp_rows="chunked", dgg_allpairs_prior_fused=True)
    torch.manual_seed(3)
    model = dgg_amd.GCN_DGG(nfeat=d_in, nhidden=h, nclass=C, args=args).to(dev)
    with torch.no_grad():
        degree_following_knet(model.dggs[0])
        model.dggs[0].edge_encode[0].weight[:, 2 * h].mul_(PRIOR_COLUMN_SCALE)
    x = torch.rand(N, d_in, generator=torch.Generator().manual_seed(1)).to(dev)
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(2)).to(dev)
    A = dgg_amd.AllPairs(torch.randint(44, 60, (N,), generator=torch.Generator().manual_seed(4)).float().to(dev), prior=make_prior(N).to(dev))
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    kmax, wide, losses = [], [], []
    for step in range(6):
        opt.zero_grad()
        logp, adj, _ = model(x, A)
        loss = torch.nn.functional.nll_loss(logp, y)
        loss.backward()
        g = model.dggs[0].edge_encode[0].weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g[:, 2 * h].abs().max()) > 0, f"step {step}: the prior column's gradient"
        opt.step()
        kmax.append(float(adj.k.max()))
        wide.append(adj.layout is not None)
        losses.append(float(loss.detach()))
    print("k_max per step:", " ".join(f"{v:.1f}" for v in kmax), "| chunked:", "".join("x" if w_ else "." for w_ in wide))
    dgg = model.dggs[0]
    assert dgg.__dict__.get("_fused_layer") is not None and not dgg.__dict__.get("fused_fallback"), "the fused layer ran every step"
    assert all(np.isfinite(losses)) and bool(torch.isfinite(logp).all())
    assert max(kmax) + 8.5 > 64 and all(wide), "the learned degrees must outgrow the 64-rank list in this run"
    assert float(adj.k.min()) + 9.5 < 64 and adj.layout.wide, "rows that fit the list beside rows that do not"
    dgg.check_ell_bound()
