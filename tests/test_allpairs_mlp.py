"""Edge-MLP scorers (u-v-deg / u-v-deg-dist / edge_conv) on ALL-PAIRS candidates: dgg_allpairs_mlp_topk, its autograd node and the
module path that uses them.

Definition under test: the result is what the edge-list path returns on the COMPLETE candidate pattern (row i lists columns 0..N-1,
self included) with the prior degrees in the place of the row sums of in_adj, kept to the 64-rank list; ties: lower column first.

Forward checks are bit for bit (the kernel shares its score chain with the edge-list kernels).  Gradient check (test 5, N = 130,
h = hw = 32, hash noise, k_times_edge_prob): error of each gradient against a dense float64 torch restatement, for the new node and
for the existing edge-list node (_DGGEdgeMlpAdjFn on the complete pattern, same inputs); both backwards use float atomics, so each
node is run 8 times and its largest error counts.  Bar: new <= 4 x existing + one float32 ulp
of the gradient's largest magnitude (4 = the project's tier-2 margin for float-atomic ordering, the only thing that differs between
the two paths; the reference figure is measured from the EXISTING node, never from the code under test).

Measured on an MI355X (largest of 8 runs, max abs error vs float64; new node / existing node):

    gradient   u-v-deg              u-v-deg-dist         edge_conv
    dx         4.9e-06 / 4.9e-06    4.8e-06 / 4.9e-06    1.7e-06 / 2.1e-06
    dk         5.8e-07 / 5.8e-07    5.9e-07 / 5.9e-07    3.7e-07 / 3.7e-07
    dWe        1.5e-05 / 1.5e-05    1.5e-05 / 1.5e-05    1.0e-05 / 1.2e-05
    dbe        9.5e-06 / 7.6e-06    1.1e-05 / 1.1e-05    7.7e-06 / 8.7e-06
    dWcat      1.5e-05 / 1.5e-05    1.4e-05 / 1.5e-05    1.4e-05 / 1.1e-05
    dwdu       7.8e-05 / 7.0e-05    7.3e-05 / 7.3e-05    -
    dwdv       6.8e-05 / 6.5e-05    5.4e-05 / 5.0e-05    -
    dwex       -                    4.4e-07 / 4.7e-07    -
    deb1       4.9e-06 / 4.5e-06    5.8e-06 / 5.8e-06    7.4e-06 / 7.7e-06
    dw2        3.3e-05 / 3.7e-05    2.2e-05 / 2.2e-05    2.4e-05 / 2.3e-05
    db2        2.8e-06 / 1.8e-06    1.8e-06 / 1.8e-06    6.8e-06 / 7.3e-06

(gradient maxima 0.4 .. 170; largest ratio new / existing 1.53: the two nodes run the same backward on the same bits, what differs
is the order of its float atomics)
"""
import copy
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

K = 64
T_EX = -1.0
SCORERS = ("u-v-deg", "u-v-deg-dist", "edge_conv")
NOISES = ("none", "explicit", "hash", "sym")
NOISE_MODE = {"none": 0, "explicit": 1, "hash": 2, "sym": 3}
SEED = (9, 4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def Nn(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------
# inputs, reference, canaried outputs
# ---------------------------------------------------------------------------------------------------------------
def make_inputs(N, hw, h, seed=0, saturate=False, with_G=True):
    """per-node arrays with exact ties: nodes 1, 5, N//2, N-1 (where they exist) share feature rows AND prior degree; node 3 has the
    same rows with ANOTHER degree (no tie under u-v-deg).  saturate: w2 scaled so that many scores are exactly 1.0f."""
    rng = np.random.default_rng(1000 * N + hw + seed)
    f = np.float32
    AB = (rng.standard_normal((N, 2 * hw)) * 0.5).astype(f)
    xp = (rng.standard_normal((N, h)) * 0.3).astype(f)
    deg = rng.integers(3, 20, N).astype(f)
    for j in sorted({5, N // 2, N - 1, 3}):
        if 1 < j < N:
            AB[j], xp[j] = AB[1], xp[1]
            deg[j] = deg[1] + 2.0 if j == 3 else deg[1]
    v = lambda s_: (rng.standard_normal(hw) * s_).astype(f)  # noqa: E731
    d = dict(AB=AB, xp=xp, deg=deg, wdu=v(0.05), wdv=v(0.05), wex=v(0.5), b1=v(0.1), w2=v(0.4 * (40.0 if saturate else 1.0)),
             b2=np.array([0.1], f), G=(rng.gumbel(size=(N, N)) * 0.3).astype(f) if with_G else None)
    return d


def scorer_args(d, scorer):
    """-> (deg, ex_mode, wdu, wdv, wex, act)"""
    if scorer == "u-v-deg":
        return d["deg"], 0, d["wdu"], d["wdv"], None, 1
    if scorer == "u-v-deg-dist":
        return d["deg"], 2, d["wdu"], d["wdv"], d["wex"], 1
    if scorer == "edge_conv":
        return None, 0, None, None, None, 0
    # combinations of the switches that none of the three scorers uses (the kernel's run-time variant)
    return {"deg+identity": (d["deg"], 0, d["wdu"], d["wdv"], None, 0), "leaky-only": (None, 0, None, None, None, 1),
            "dist-only": (None, 2, None, None, d["wex"], 1), "deg+dist+identity": (d["deg"], 2, d["wdu"], d["wdv"], d["wex"], 0)}[scorer]


OTHER_SWITCHES = ("deg+identity", "leaky-only", "dist-only", "deg+dist+identity")


def complete_pattern(N):
    ar = np.arange(N, dtype=np.int32)
    return np.arange(N + 1, dtype=np.int64) * N, np.tile(ar, N), np.repeat(ar, N)      # rowptr, col, erow


def oracle_scores(d, scorer):
    N = d["AB"].shape[0]
    _, col, erow = complete_pattern(N)
    deg, ex_mode, wdu, wdv, wex, act = scorer_args(d, scorer)
    return O.edge_mlp_fwd(d["AB"], d["xp"], erow, col, deg, None, ex_mode, T_EX, wdu, wdv, wex, d["b1"], d["w2"], d["b2"][0], act)


def oracle_topk(d, p, ex, scorer, noise):
    """the composed CPU path on the complete pattern -> idx, val, ex_out [N,K]"""
    N = d["AB"].shape[0]
    rowptr, col, _ = complete_pattern(N)
    idx, val, eid = O.edgelist_topk_p(p, N, rowptr, col, K, NOISE_MODE[noise], d["G"] if noise == "explicit" else None, SEED)
    exo = np.where(eid >= 0, ex[np.maximum(eid, 0)], 0.0).astype(np.float32) if scorer_args(d, scorer)[1] == 2 else np.zeros((N, K), np.float32)
    return idx, val, exo


PAD = 96


class Canaried:
    """idx / val / ex [n, k] handed to the kernel as views between canary words, filled with -7 / NaN"""

    def __init__(self, n, dev, k=K):
        self.n, self.k = n, k
        self.bi = torch.full((n * k + 2 * PAD,), -7, dtype=torch.int32, device=dev)
        self.bv = torch.full((n * k + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)
        self.be = torch.full((n * k + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)

    def views(self):
        return tuple(b[PAD:PAD + self.n * self.k].view(self.n, self.k) for b in (self.bi, self.bv, self.be))

    def canaries_intact(self):
        ok = bool((self.bi[:PAD] == -7).all()) and bool((self.bi[PAD + self.n * self.k:] == -7).all())
        for b in (self.bv, self.be):
            ok = ok and bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[PAD + self.n * self.k:]).all())
        return ok

    def untouched(self):
        return self.canaries_intact() and bool((self.bi == -7).all()) and bool(torch.isnan(self.bv).all()) and bool(torch.isnan(self.be).all())


def run_kernel(dv, scorer, noise, dev, rows=None, out=None, k=K):
    from dgg_amd import ops
    deg, ex_mode, wdu, wdv, wex, act = scorer_args(dv, scorer)
    return ops.allpairs_mlp_topk(dv["AB"], dv["xp"], deg, ex_mode, T_EX, wdu, wdv, wex, dv["b1"], dv["w2"], dv["b2"], act, k, NOISE_MODE[noise],
                                 dv["G"] if noise == "explicit" else None, SEED, rows=rows, out=out)


def to_dev(d, dev):
    return {k_: T(v_, dev) for k_, v_ in d.items()}


# ---------------------------------------------------------------------------------------------------------------
# 1. the kernel against the CPU oracle, bit for bit
# ---------------------------------------------------------------------------------------------------------------
CASES = [(N, hw, False) for N in (1, 2, 63, 64, 65, 129, 257) for hw in (16, 64, 128)] + [(600, 64, False), (257, 64, True)]


@pytest.mark.parametrize("N,hw,saturate", CASES)
def test_kernel_matches_the_composed_cpu_oracle_bit_for_bit(dev, N, hw, saturate):
    """oracle.edge_mlp_fwd + oracle.edgelist_topk_p on the complete pattern; three scorers x four noise settings; idx / val / ex_out exact,
    written into NaN / -7 buffers between canaries"""
    d = make_inputs(N, hw, hw, saturate=saturate)
    dv = to_dev(d, dev)
    for scorer in SCORERS:
        p, ex = oracle_scores(d, scorer)
        if saturate:
            assert (p == np.float32(1.0)).sum() > N, "the saturated case must hold many scores of exactly 1.0f"
        for noise in NOISES:
            ridx, rval, rex = oracle_topk(d, p, ex, scorer, noise)
            if N < K:
                assert (ridx[:, N:] == -1).all() and (rval[:, N:] == 0).all()
            buf = Canaried(N, dev)
            run_kernel(dv, scorer, noise, dev, out=buf.views())
            idx, val, exo = (Nn(t) for t in buf.views())
            what = f"{scorer} / {noise}"
            assert np.array_equal(idx, ridx), f"{what}: indices differ from the oracle"
            assert np.array_equal(val.view(np.int32), rval.view(np.int32)), f"{what}: scores differ from the oracle"
            assert np.array_equal(exo.view(np.int32), rex.view(np.int32)), f"{what}: extras differ from the oracle"
            assert buf.canaries_intact(), f"{what}: written outside the outputs"


@pytest.mark.parametrize("N,hw", [(257, 16), (129, 32), (257, 64), (600, 64), (257, 128)])
def test_both_row_blockings_and_every_switch_combination_match_the_oracle(dev, monkeypatch, N, hw):
    """The launch picks the rows-per-wavefront variant from the row count: 8 rows (4 at hw = 128) from 1024 workgroups on -- the kernels
    of the large graphs -- else 2.  DGG_APMLP_RW forces either, so BOTH are held to the CPU oracle here at small N, on the last, partial
    row block as well (N is no multiple of 16 or 32), for the three scorers and for the switch combinations none of them uses."""
    d = make_inputs(N, hw, hw)
    dv = to_dev(d, dev)
    for scorer in SCORERS + OTHER_SWITCHES:
        p, ex = oracle_scores(d, scorer)
        for noise in NOISES:
            ridx, rval, rex = oracle_topk(d, p, ex, scorer, noise)
            for force in ("big", "small"):
                monkeypatch.setenv("DGG_APMLP_RW", force)
                buf = Canaried(N, dev)
                run_kernel(dv, scorer, noise, dev, out=buf.views())
                idx, val, exo = (Nn(t) for t in buf.views())
                what = f"{scorer} / {noise} / {force}"
                assert np.array_equal(idx, ridx), f"{what}: indices differ from the oracle"
                assert np.array_equal(val.view(np.int32), rval.view(np.int32)), f"{what}: scores differ from the oracle"
                assert np.array_equal(exo.view(np.int32), rex.view(np.int32)), f"{what}: extras differ from the oracle"
                assert buf.canaries_intact(), f"{what}: written outside the outputs"
                if force == "big":                                     # a row range that starts and ends inside row blocks
                    r0, r1 = 37, min(N, 37 + 70)
                    part = Canaried(r1 - r0, dev)
                    run_kernel(dv, scorer, noise, dev, rows=(r0, r1), out=part.views())
                    assert np.array_equal(Nn(part.views()[0]), ridx[r0:r1]) and part.canaries_intact(), f"{what}: rows {r0}:{r1}"
                    assert np.array_equal(Nn(part.views()[1]).view(np.int32), rval[r0:r1].view(np.int32)), f"{what}: rows {r0}:{r1}"


@pytest.mark.parametrize("N,hw", [(32771, 64), (16389, 128)])
def test_large_graph_launch_equals_row_ranges_and_the_existing_kernels(dev, monkeypatch, N, hw):
    """At these sizes the launch itself takes the 8-row (hw = 128: 4-row) kernels -- 1024 workgroups or more, the last one partial.
    The whole result is compared bit for bit (a) with launches of short row ranges, which take the 2-row kernels, and (b) with
    ops.edge_mlp_fwd + ops.edgelist_topk_p on the complete pattern restricted to those rows."""
    from dgg_amd import ops
    monkeypatch.delenv("DGG_APMLP_RW", raising=False)
    rb = 4 * (4 if hw == 128 else 8)
    assert (N + rb - 1) // rb >= 1024 and N % rb != 0
    dv = to_dev({k_: v_ for k_, v_ in make_inputs(N, hw, hw, with_G=False).items() if v_ is not None}, dev)
    dv["G"] = None
    ar = torch.arange(N, device=dev, dtype=torch.int32)
    ranges = ((0, 40), (N // 2 + 3, N // 2 + 3 + 50), (N - 37, N))
    for scorer in ("u-v-deg", "u-v-deg-dist"):
        deg, ex_mode, wdu, wdv, wex, act = scorer_args(dv, scorer)
        for noise in ("hash", "sym", "none"):
            full = run_kernel(dv, scorer, noise, dev)
            for r0, r1 in ranges:
                n = r1 - r0
                part = run_kernel(dv, scorer, noise, dev, rows=(r0, r1))
                what = f"{scorer} / {noise} rows {r0}:{r1}"
                for got, ref in zip(part, full):
                    if ref is not None:
                        assert torch.equal(got.view(torch.int32), ref[r0:r1].view(torch.int32)), f"{what}: differs from the row-range launch"
                erow, col = torch.arange(r0, r1, device=dev, dtype=torch.int32).repeat_interleave(N), ar.repeat(n)
                rowptr = torch.arange(n + 1, device=dev, dtype=torch.int64) * N
                p, ex = ops.edge_mlp_fwd(dv["AB"], dv["xp"], erow, col, deg, None, ex_mode, T_EX, wdu, wdv, wex, dv["b1"], dv["w2"], dv["b2"], act)
                ridx, rval, reid = ops.edgelist_topk_p(p, N, rowptr, col, K, NOISE_MODE[noise], None, SEED, rows=(r0, r1))
                assert torch.equal(full[0][r0:r1], ridx) and torch.equal(full[1][r0:r1].view(torch.int32), rval.view(torch.int32)), \
                    f"{what}: differs from edge_mlp_fwd + edgelist_topk_p"
                if ex_mode:
                    assert torch.equal(full[2][r0:r1].view(torch.int32), ex[reid.long()].view(torch.int32)), f"{what}: extras"


def test_inputs_hold_the_two_kinds_of_ties():
    """(host-side property of the inputs above, kept next to them) identical nodes tie exactly under every scorer without noise, and the
    tie is broken by the lower column; the node with the same rows and another degree does not tie under u-v-deg"""
    d = make_inputs(257, 64, 64)
    for scorer in SCORERS:
        p, _ = oracle_scores(d, scorer)
        P = p.reshape(257, 257)
        assert np.array_equal(P[:, 1], P[:, 5]) and np.array_equal(P[:, 1], P[:, 128]) and np.array_equal(P[:, 1], P[:, 256])
    P = oracle_scores(d, "u-v-deg")[0].reshape(257, 257)
    assert not np.array_equal(P[:, 1], P[:, 3])
    assert np.array_equal(oracle_scores(d, "edge_conv")[0].reshape(257, 257)[:, 1], oracle_scores(d, "edge_conv")[0].reshape(257, 257)[:, 3])


# ---------------------------------------------------------------------------------------------------------------
# 2. row ranges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["hash", "sym"])
def test_row_ranges_equal_the_slices_of_the_full_result(dev, noise):
    N = 257
    dv = to_dev(make_inputs(N, 64, 64), dev)
    for scorer in ("u-v-deg", "u-v-deg-dist"):
        full = run_kernel(dv, scorer, noise, dev)
        for r0, r1 in ((0, N), (37, 101), (N - 1, N), (5, 5)):
            buf = Canaried(r1 - r0, dev)
            run_kernel(dv, scorer, noise, dev, rows=(r0, r1), out=buf.views())
            assert buf.canaries_intact(), f"rows {r0}:{r1}: written outside the range"
            if r0 == r1:
                assert buf.untouched()
                continue
            for got, ref in zip(buf.views(), full):
                if ref is not None:
                    assert torch.equal(got.view(torch.int32), ref[r0:r1].view(torch.int32)), f"{scorer} rows {r0}:{r1}"


# ---------------------------------------------------------------------------------------------------------------
# 3. against the existing GPU kernels
# ---------------------------------------------------------------------------------------------------------------
def test_equals_the_existing_gpu_kernels_on_the_complete_pattern(dev):
    from dgg_amd import ops
    N, hw = 1000, 64
    d = make_inputs(N, hw, hw)
    dv = to_dev(d, dev)
    rowptr, col, erow = (T(a, dev) for a in complete_pattern(N))
    for scorer, noise in (("u-v-deg", "hash"), ("u-v-deg-dist", "sym"), ("edge_conv", "none"), ("u-v-deg", "explicit")):
        deg, ex_mode, wdu, wdv, wex, act = scorer_args(dv, scorer)
        p, ex = ops.edge_mlp_fwd(dv["AB"], dv["xp"], erow, col, deg, None, ex_mode, T_EX, wdu, wdv, wex, dv["b1"], dv["w2"], dv["b2"], act)
        ridx, rval, reid = ops.edgelist_topk_p(p, N, rowptr, col, K, NOISE_MODE[noise], dv["G"] if noise == "explicit" else None, SEED)
        idx, val, exo = run_kernel(dv, scorer, noise, dev)
        assert torch.equal(idx, ridx) and torch.equal(val.view(torch.int32), rval.view(torch.int32)), f"{scorer} / {noise}"
        if ex_mode:
            assert torch.equal(exo.view(torch.int32), ex[reid.long()].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["hw=8", "hw=256", "h=8", "h=256", "K=65", "ex_mode=1", "noise=4", "noise=5"])
def test_refusals_return_the_code_and_write_nothing(dev, what):
    from dgg_amd import ops
    from dgg_amd._lib import DggHipError
    key, _, v = what.partition("=")
    v = int(v)
    N, hw, h, k, ex_mode, noise = 70, 64, 64, K, 2, 2
    if key == "hw":
        hw = v
    elif key == "h":
        h = v
    elif key == "K":
        k = v
    elif key == "ex_mode":
        ex_mode = v
    else:
        noise = v
    dv = to_dev(make_inputs(N, hw, h), dev)
    buf = Canaried(N, dev, k)
    with pytest.raises(DggHipError, match=r"code 2"):
        ops.allpairs_mlp_topk(dv["AB"], dv["xp"], dv["deg"], ex_mode, T_EX, dv["wdu"], dv["wdv"], dv["wex"], dv["b1"], dv["w2"], dv["b2"], 1, k, noise,
                              None, SEED, out=buf.views())
    torch.cuda.synchronize()
    assert buf.untouched()


# ---------------------------------------------------------------------------------------------------------------
# 5. the autograd node
# ---------------------------------------------------------------------------------------------------------------
def _node_inputs(N, d_in, h, scorer, dev):
    g = torch.Generator().manual_seed(11)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)  # noqa: E731
    hw = h // 2 if scorer == "edge_conv" else h
    t = dict(x=r(N, d_in), k=5.0 + 10.0 * torch.rand(N, generator=g), We=r(h, d_in, sc=0.3), be=r(h, sc=0.1), Wcat=r(2 * hw, h, sc=0.3),
             wdu=r(hw, sc=0.05), wdv=r(hw, sc=0.05), wex=r(hw, sc=0.5), eb1=r(hw, sc=0.1), w2=r(hw, sc=0.4), b2=r(1, sc=0.1))
    if scorer != "u-v-deg-dist":
        t["wex"] = None
    if scorer == "edge_conv":
        t["wdu"] = t["wdv"] = None
    deg = torch.randint(3, 20, (N,), generator=g).float()
    cot = torch.randn(N, K, generator=g)
    return t, deg, cot


def _float64_grads(t, deg, cot, idx, Gn, scorer, mode_k_only=False):
    """dense float64 restatement of the definition: projection, scorer on every pair, perturbation, the GIVEN selection, the ramp"""
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
    val = torch.gather(v, 1, idx.long().clamp(min=0))
    ramp = 1.0 - 0.5 * (1.0 + torch.tanh(torch.arange(K, dtype=torch.float64)[None, :] - leaf["k"][:, None]))
    w = torch.where(idx >= 0, val * ramp, torch.zeros_like(val))
    (w * cot.double()).sum().backward()
    return {n: v.grad for n, v in leaf.items()}


@pytest.mark.parametrize("scorer", SCORERS)
def test_autograd_node_forward_bits_and_gradients(dev, scorer):
    from dgg_amd import ops
    from dgg_amd.dgm import _DGGAllPairsMlpAdjFn, _DGGEdgeMlpAdjFn
    N, d_in, h = 130, 24, 32
    t, deg, cot = _node_inputs(N, d_in, h, scorer, dev)
    ex_mode, act = (2 if scorer == "u-v-deg-dist" else 0), (0 if scorer == "edge_conv" else 1)
    names = [n for n in ("x", "k", "We", "be", "Wcat", "wdu", "wdv", "wex", "eb1", "w2", "b2") if t[n] is not None]
    rowptr, col, erow = (T(a, dev) for a in complete_pattern(N))

    def run(new):
        leaf = {n: (None if v is None else v.to(dev).requires_grad_(True)) for n, v in t.items()}
        cfg = dict(K=K, noise_mode=ops.NOISE_HASH, G=None, seed=SEED, mode=ops.MODE_K_TIMES_EDGE_PROB, ex_mode=ex_mode, t_ex=T_EX, act=act)
        par = (leaf["We"], leaf["be"], leaf["Wcat"], leaf["wdu"], leaf["wdv"], leaf["wex"], leaf["eb1"], leaf["w2"], leaf["b2"])
        if new:
            out = _DGGAllPairsMlpAdjFn.apply(leaf["x"], leaf["k"], deg.to(dev), *par, cfg)
        else:
            cfg["cand"] = (rowptr, col, erow)
            out = _DGGEdgeMlpAdjFn.apply(leaf["x"], leaf["k"], deg.to(dev), None, *par, cfg)
        (out[0] * cot.to(dev)).sum().backward()
        return out, {n: leaf[n].grad.detach().cpu() for n in names}

    out_new, g_new = run(True)
    out_old, g_old = run(False)
    for a, b, what in zip(out_new, out_old, ("w", "idx", "val", "rs")):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), f"{what} differs from the edge-list node on the complete pattern"
    Gn = torch.from_numpy(O.noise_matrix(N, SEED[0], SEED[1], symmetric=False))
    ref = _float64_grads(t, deg, cot, out_new[1].cpu(), Gn, scorer)
    # The shared backward sums the neighbour side and the parameter gradients with float atomics, so the error of ONE node differs from
    # run to run (db2 of the same node: 3.9e-7 in one run, 2.9e-6 in the next): each node runs RUNS times and its LARGEST error enters the bar
    RUNS = 8
    errs = {True: {n: 0.0 for n in names}, False: {n: 0.0 for n in names}}
    for new, g0 in ((True, g_new), (False, g_old)):
        for i in range(RUNS):
            g = g0 if i == 0 else run(new)[1]
            for n in names:
                errs[new][n] = max(errs[new][n], float((g[n].double() - ref[n]).abs().max()))
    bad = []
    for n in names:
        r = ref[n]
        e_new, e_old = errs[True][n], errs[False][n]
        ulp = float(np.spacing(np.float32(r.abs().max())))
        print(f"{scorer:13s} d{n:5s} max|g|={float(r.abs().max()):.3e}  new {e_new:.3e}  existing {e_old:.3e}  ulp {ulp:.1e}")
        assert float(r.abs().max()) > 0, f"d{n}: the float64 gradient is identically zero (nothing checked)"
        if not e_new <= 4.0 * e_old + ulp:
            bad.append(f"d{n}: new {e_new:.3e} > 4 x {e_old:.3e} + {ulp:.1e}")
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# 6. - 8. the module
# ---------------------------------------------------------------------------------------------------------------
def module_args(scorer, perturb=True, sym=False, **kw):
    base = dict(extra_edge_dim={"u-v-deg": 2, "u-v-deg-dist": 3, "u-v-A_uv": 1}.get(scorer, 0), extra_k_dim=1, dgg_hard=False, deg_mean=3.899,
                deg_std=5.288, dgg_mode_edge_net=scorer, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3,
                perturb_edge_prob=perturb, symmetric_noise=sym, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1,
                dgg_wide_rows="ell")
    base.update(kw)
    return Namespace(**base)


def complete_in_adj(prior, dev):
    """complete sparse in_adj whose float64 row sums are exactly the (integer) priors: 2^-7 everywhere, the first entry of row i
    m_i - (N - 1) 2^-7.  The three scorers do not read the values."""
    N = prior.shape[0]
    vals = torch.full((N, N), 2.0 ** -7, dtype=torch.float64)
    vals[:, 0] = prior.double() - (N - 1) * 2.0 ** -7
    assert torch.equal(vals.sum(1), prior.double()) and torch.equal(vals.float().double(), vals)
    ar = torch.arange(N)
    ind = torch.stack([ar.repeat_interleave(N), ar.repeat(N)])
    return torch.sparse_coo_tensor(ind, vals.float().reshape(-1), (N, N)).coalesce().to(dev)


@pytest.mark.parametrize("noise", ["off", "asymmetric", "symmetric"])
@pytest.mark.parametrize("scorer", SCORERS)
def test_module_on_all_pairs_equals_the_module_on_the_complete_in_adj(dev, scorer, noise):
    """(fails before this feature: forward raised NotImplementedError for every scorer but u-v-dist on AllPairs)"""
    import dgg_amd
    N, d_in, h = 130, 24, 32
    torch.manual_seed(5)
    args = module_args(scorer, perturb=noise != "off", sym=noise == "symmetric")
    m1 = dgg_amd.DGG_LearnableK_debug(in_dim=d_in, latent_dim=h, args=args).to(dev)
    with torch.no_grad():
        m1.k_net.k_project.weight.mul_(0.1)
    m2 = copy.deepcopy(m1)
    m2.load_state_dict(m1.state_dict())
    for m in (m1, m2):
        m.set_seed(77, 5)
    x = torch.rand(N, d_in, generator=torch.Generator().manual_seed(1)).to(dev)
    prior = torch.randint(4, 20, (N,), generator=torch.Generator().manual_seed(2)).float()
    a1 = m1(x, dgg_amd.AllPairs(prior.to(dev)))
    a2 = m2(x, complete_in_adj(prior, dev))
    assert isinstance(a1, dgg_amd.EllAdjacency) and isinstance(a2, dgg_amd.EllAdjacency)
    for m in (m1, m2):
        m.check_ell_bound()
    assert torch.equal(a1.idx, a2.idx)
    for f1, f2, what in ((a1.values(), a2.values(), "w"), (a1.rs, a2.rs, "rs"), (a1.k, a2.k, "k"), (a1.score, a2.score, "score")):
        assert torch.equal(f1.detach().view(torch.int32), f2.detach().view(torch.int32)), what
    assert int((a1.idx >= 0).sum()) == N * K and a1.owner is m1


@pytest.mark.parametrize("what", ["u-v-A_uv", "A_uv", "gcn-x-deg", "dgg_hard_literal"])
def test_unsupported_configurations_on_all_pairs_still_raise(dev, what):
    import dgg_amd
    kw = {}
    scorer = what if what in ("u-v-A_uv", "A_uv") else "u-v-deg"
    if what == "gcn-x-deg":
        kw["dgg_mode_k_net"] = "gcn-x-deg"
    if what == "dgg_hard_literal":
        kw.update(dgg_hard=True, dgg_hard_literal=True)
    m = dgg_amd.DGG_LearnableK_debug(in_dim=24, latent_dim=32, args=module_args(scorer, **kw)).to(dev)
    with pytest.raises(NotImplementedError) as e:
        m(torch.rand(130, 24, device=dev), dgg_amd.AllPairs(torch.full((130,), 9.0, device=dev)))
    if what in ("u-v-A_uv", "A_uv", "dgg_hard_literal"):
        assert all(s in str(e.value) for s in SCORERS), "the message names the supported scorers"


@pytest.mark.parametrize("scorer", SCORERS)
def test_learned_degrees_beyond_the_list_are_reported(dev, scorer):
    import dgg_amd
    N = 130
    for policy in ("ell", "auto", "csr"):
        m = dgg_amd.DGG_LearnableK_debug(in_dim=24, latent_dim=32, args=module_args(scorer, dgg_wide_rows=policy)).to(dev)
        for nm in range(6):
            assert m.wide_row_plan(N, True, nm) == "list"
    m.set_seed(3)
    with torch.no_grad():
        m.k_net.k_project.weight.mul_(0.1)
    x = torch.rand(N, 24, device=dev)
    adj = m(x, dgg_amd.AllPairs(torch.full((N,), 9.0, device=dev)))
    m.check_ell_bound()                                         # k ~ 10: fits
    assert isinstance(adj, dgg_amd.EllAdjacency)
    m(x, dgg_amd.AllPairs(80.0 + torch.arange(N, device=dev).float() % 7))       # k ~ 84: k + 8.5 > 64
    with pytest.raises(RuntimeError, match="ell_width"):
        m.check_ell_bound()


def test_dgg_hard_straight_through_on_all_pairs(dev):
    """dgg_hard works through fwd_mode as in the edge-list node: the same bits as the module on the complete in_adj"""
    import dgg_amd
    N = 130
    torch.manual_seed(6)
    m1 = dgg_amd.DGG_LearnableK_debug(in_dim=24, latent_dim=32, args=module_args("u-v-deg", dgg_hard=True)).to(dev)
    m2 = copy.deepcopy(m1)
    for m in (m1, m2):
        m.set_seed(4, 1)
    x = torch.rand(N, 24, generator=torch.Generator().manual_seed(1)).to(dev)
    prior = torch.randint(4, 20, (N,), generator=torch.Generator().manual_seed(2)).float()
    a1, a2 = m1(x, dgg_amd.AllPairs(prior.to(dev))), m2(x, complete_in_adj(prior, dev))
    assert torch.equal(a1.idx, a2.idx) and torch.equal(a1.values().detach().view(torch.int32), a2.values().detach().view(torch.int32))


def test_gcn_dgg_trains_on_all_pairs_with_the_default_scorer(dev):
    import dgg_amd
    N, d_in, h, C = 300, 40, 32, 7
    args = module_args("u-v-deg", dgg_wide_rows="auto")
    torch.manual_seed(3)
    model = dgg_amd.GCN_DGG(nfeat=d_in, nhidden=h, nclass=C, args=args).to(dev)
    with torch.no_grad():
        model.dggs[0].k_net.k_project.weight.mul_(0.1)
    x = torch.rand(N, d_in, generator=torch.Generator().manual_seed(1)).to(dev)
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(2)).to(dev)
    # (priors that differ: the learned degree is k = relu(kp sd + mu) + 1 with sd the priors' std -- constant priors give the k-net no gradient)
    A = dgg_amd.AllPairs(torch.randint(6, 20, (N,), generator=torch.Generator().manual_seed(4)).float().to(dev))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(3):
        opt.zero_grad()
        logp, adj, _ = model(x, A)
        torch.nn.functional.nll_loss(logp, y).backward()
        for n, p in model.named_parameters():
            assert p.grad is None or bool(torch.isfinite(p.grad).all()), n
        opt.step()
    dgg = model.dggs[0]
    for p in (dgg.edge_encode[0].weight, dgg.edge_encode[2].weight, dgg.node_encode_for_edges[0].weight, dgg.k_net.k_project.weight,
              dgg.k_embed[0].weight, dgg.node_encode_for_k[0].weight):
        assert p.grad is not None and float(p.grad.abs().max()) > 0
    assert dgg.fused_fallback == {"edge-MLP scorer on all-pairs candidates": 3}
    dgg.check_ell_bound()
    assert isinstance(adj, dgg_amd.EllAdjacency) and bool(torch.isfinite(logp).all())
