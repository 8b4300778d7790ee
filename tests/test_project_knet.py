"""The learned-degree k-net inside the projection kernel (dgg_project_knet_fwd, include/dgg_hip_next.h) against the pair it replaces, in the
SAME build and bit for bit -- linear_fwd_multi (weights stacked by dgg_linear_pack_weights) + knet_x_fwd_slim: the fused kernel runs the
same k-ordered chains on the same operand values, so there is no tolerance anywhere on the forward.  Also: the CPU oracle, the shapes
the entry refuses, the whole layer with and without the fused route, and the fused forward captured into a hipGraph."""
import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
D, H = 128, 64
# the smallest N at which each path of the work split can go wrong (256 workgroups x 4 wavefronts = 1024 wavefronts at most):
#   5       one partial row block: everything is a remainder unit
#   135     several remainder blocks (4 whole + 1 partial) on two workgroups
#   256     whole blocks only, one per wavefront
#   32937   one whole round (1024 blocks) + 5 whole remainder blocks + a partial one
#   65633   two rounds (the row prefetch crosses an iteration) + 3 remainder blocks, the last partial
SIZES = (5, 135, 256, 32937, 65633)
MU, SD = 32.0, 5.0


def within_own_spread(d_new_old, d_old_old):
    """tests/test_spmm_norm.py's rule for gradients: new / old within 4x old / old, or one ulp of the largest element"""
    return d_new_old <= max(4 * d_old_old, ULP)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


def bench_layers(P):
    """the bench's layer list: We / be leaky, Wk / bk leaky, Wc in layout 1 without bias or activation"""
    return [(P["We"], P["be"], 1, 0), (P["Wk"], P["bk"], 1, 0), (P["Wc"], None, 0, 1)]


def knet_args(P):
    return P["W1"], P["b1"], P["Wmu"], P["bmu"], P["Wp"].reshape(-1), P["bp"]


@pytest.fixture(scope="module")
def inputs(dev):
    """make_params weights; features scaled by 1e3 (both signs of every LeakyReLU in every block, u of both signs); deg[0] == mu.
    One set of max(SIZES) rows: every size takes its first N."""
    import bench
    P = bench.make_params(D, H, dev)
    n = max(SIZES)
    x = (torch.randn(n, D, generator=torch.Generator().manual_seed(11)) * 1e3).to(dev)
    deg = 24 + 16 * torch.rand(n, generator=torch.Generator().manual_seed(12))
    deg[0] = MU
    return P, x, deg.to(dev), torch.tensor([MU, SD], device=dev)


def the_pair(ops, x, P, deg, mu_sd):
    xp, xk, Hc = ops.linear_fwd_multi(x, bench_layers(P))
    k, u = ops.knet_x_fwd_slim(xk, deg, mu_sd, *knet_args(P))
    return dict(xp=xp, xk=xk, H=Hc, k=k, u=u)


def fused(ops, x, P, deg, mu_sd, force=1):
    got = ops.project_knet(x, bench_layers(P), 1, deg, mu_sd, *knet_args(P), force=force)
    if got is None:
        return None
    (xp, xk, Hc), k, u = got
    return dict(xp=xp, xk=xk, H=Hc, k=k, u=u)


@pytest.mark.parametrize("N", SIZES)
def test_fused_equals_the_pair_bit_for_bit(dev, inputs, N):
    from dgg_amd import ops
    P, x, deg, mu_sd = inputs
    x, deg = x[:N].contiguous(), deg[:N].contiguous()
    old, new = the_pair(ops, x, P, deg, mu_sd), fused(ops, x, P, deg, mu_sd)
    torch.cuda.synchronize()
    assert new is not None, "force = 1 takes the fused kernel at any N"
    for name in ("xp", "xk", "H", "k", "u"):
        assert old[name].shape == new[name].shape and torch.equal(old[name], new[name]), name
    # the inputs do what they are there for: both signs in every 32 x 32 block of the two activated layers, a row with deg == mu,
    # a negative u and k = 1 exactly there
    for name in ("xp", "xk"):
        y = old[name]
        nb = (N + 31) // 32
        pad = torch.zeros(nb * 32 - N, 64, device=dev)
        pos = torch.cat([y > 0, pad > 1]).view(nb, 32, 2, 32).any(3).any(1)
        neg = torch.cat([y < 0, pad > 1]).view(nb, 32, 2, 32).any(3).any(1)
        assert bool(pos.all()) and bool(neg.all()), name
    assert float(deg[0]) == float(mu_sd[0])
    u = old["u"]
    assert bool((u < 0).any()) and bool((u > 0).any())
    assert torch.equal(old["k"], torch.clamp(u, min=0) + 1) and bool((old["k"][u < 0] == 1).all())


def test_fused_equals_the_cpu_oracle(dev, inputs):
    """xp, k and u at N = 135: the exact k-ordered fmaf chains the stand-alone kernels are held to"""
    from dgg_amd import ops
    P, x, deg, mu_sd = inputs
    N = 135
    x, deg = x[:N].contiguous(), deg[:N].contiguous()
    new = fused(ops, x, P, deg, mu_sd)
    torch.cuda.synchronize()
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    xp_o = O.linear(c(x), c(P["We"]), c(P["be"]), O.ACT_LEAKY)
    xk_o = O.linear(c(x), c(P["Wk"]), c(P["bk"]), O.ACT_LEAKY)
    k_o, _, _, u_o = O.knet_x(xk_o, c(deg), np.float32(MU), np.float32(SD), *[c(t) for t in knet_args(P)], save=True)
    assert np.array_equal(c(new["xp"]), xp_o)
    assert np.array_equal(c(new["k"]), k_o)
    assert np.array_equal(c(new["u"]), u_o)


def test_refusals_return_none(dev, inputs):
    from dgg_amd import ops
    P, x, deg, mu_sd = inputs
    N = 135
    x, deg = x[:N].contiguous(), deg[:N].contiguous()
    assert fused(ops, x, P, deg, mu_sd, force=0) is None, "force = 0"
    assert fused(ops, x, P, deg, mu_sd, force=-1) is None, "the automatic choice below the projection's threshold"
    # d = 64
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.1).to(dev)  # noqa: E731
    P64 = dict(P, We=rnd(64, 64), Wk=rnd(64, 64), Wc=rnd(64, 64))
    assert fused(ops, x[:, :64].contiguous(), P64, deg, mu_sd) is None, "d = 64"
    # a k-net segment of width 96 (and a k-net built for it)
    P96 = dict(P, Wk=rnd(96, D), bk=rnd(96), W1=rnd(48, 97), b1=rnd(48), Wmu=rnd(24, 48), bmu=rnd(24), Wp=rnd(1, 24))
    assert fused(ops, x, P96, deg, mu_sd) is None, "a 96-wide k-net segment"
    # a misaligned view of x
    flat = torch.empty(N * D + 1, device=dev)
    xm = flat[1:].view(N, D)
    xm.copy_(x)
    assert xm.is_contiguous() and xm.data_ptr() % 16 == 4
    assert fused(ops, xm, P, deg, mu_sd) is None, "x not 16-byte aligned"
    torch.cuda.synchronize()


# ---- the whole layer -------------------------------------------------------------------------------------------------------------
def _layer(dev, N, d, fuse):
    import bench
    from dgg_amd import ops
    from dgg_amd.parallel import ShardedDGGConv
    P = bench.make_params(d, H, dev)
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(1000)).to(dev)
    deg = (24 + 16 * torch.rand(N, generator=torch.Generator().manual_seed(7))).to(dev)
    layer = ShardedDGGConv(ops, N, K=64, noise_mode=ops.NOISE_RANKED, seed=(1234, 0))
    layer.fuse_knet = fuse
    return layer, x, deg, P


@pytest.fixture()
def forced(monkeypatch):
    """ops.PROJECT_KNET_FORCE = 1 (the fused kernel below the automatic threshold) and a record of what ops.project_knet answered"""
    from dgg_amd import ops
    answers = []
    real = ops.project_knet

    def recording(*a, **kw):
        got = real(*a, **kw)
        answers.append(got is not None)
        return got

    monkeypatch.setattr(ops, "PROJECT_KNET_FORCE", 1)
    monkeypatch.setattr(ops, "project_knet", recording)
    return answers


def test_whole_layer_with_and_without_the_fused_route(dev, forced):
    """N = 4096, d = 128: the two-call route twice, the fused route once.  Forward bit-identical; the backward is untouched and keeps
    its own run-to-run spread (within_own_spread)."""
    N = 4096
    runs = []
    for fuse in (False, False, True):
        layer, x, deg, P = _layer(dev, N, D, fuse)
        Z = layer.forward(x, deg, P)
        grads = layer.backward(torch.randn(Z.shape, generator=torch.Generator().manual_seed(3)).to(dev), x, P)
        torch.cuda.synchronize()
        s = layer.saved
        assert s["z"] is None and s["feat"] is None and s["mu_sd"].shape == (2,) and s["deg_local"].shape == (N,)
        runs.append((dict(Z=Z, idx=s["idx"], w=s["w"], k=s["k"], u=s["u"], xk=s["xk"]),
                     {n_: g_.detach().clone() for n_, g_ in grads.items() if torch.is_tensor(g_)}))
    assert forced == [True], "the fused route ran exactly once, on the layer that allows it"
    old, old2, new = runs
    for name in old[0]:
        assert torch.equal(old[0][name], new[0][name]), name
    assert set(old[1]) == set(new[1]) and len(old[1]) >= 11
    bad = {}
    for name, g_ in old[1].items():
        scale = float(g_.abs().max())
        assert scale > 0 and torch.isfinite(new[1][name]).all(), name
        d_oo = float((g_ - old2[1][name]).abs().max()) / scale
        d_no = float((new[1][name] - g_).abs().max()) / scale
        print(f"{name}: old/old {d_oo:.3e}  new/old {d_no:.3e}")
        if not within_own_spread(d_no, d_oo):
            bad[name] = (d_no, d_oo)
    assert not bad, f"new / old difference beyond 4x the old / old difference: {bad}"


def test_layer_takes_the_two_calls_where_the_entry_refuses(dev, forced):
    """d = 64: ops.project_knet answers None and the layer's Z is the two-call route's"""
    N, d = 4096, 64
    Zs = []
    for fuse in (False, True):
        layer, x, deg, P = _layer(dev, N, d, fuse)
        Zs.append(layer.forward(x, deg, P))
        torch.cuda.synchronize()
    assert forced == [False]
    assert torch.equal(Zs[0], Zs[1])


def test_fused_forward_captures_into_a_hipgraph(dev, forced):
    """one capture + three replays = the eager result: no readback, no host decision in the fused route"""
    N = 4096
    layer, x, deg, P = _layer(dev, N, D, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Z_eager = layer.forward(x, deg, P).clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        Zg = layer.forward(x, deg, P)
    assert forced == [True, True]
    for _ in range(3):
        Zg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(Zg, Z_eager)
