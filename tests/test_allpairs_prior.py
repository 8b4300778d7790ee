"""All-pairs candidates scored against a sparse PRIOR graph (u-v-A_uv): dgg_allpairs_mlp_topk_prior, its autograd node, the module
and GCN_DGG on AllPairs(prior_degree, prior=P), and the k-net gcn-x-deg on the prior.

Definition under test: the result is what the edge-list path returns on the COMPLETE candidate pattern with ex_in = the prior's dense
values (0.0f where nothing is stored), kept to the 64-rank list; ties: lower column first.  Forward checks are bit for bit.

Gradient check (test 5, N = 130, h = hw = 32, hash noise, k_times_edge_prob): error of each gradient against a dense float64 torch
restatement, for the new node and for the existing edge-list node (_DGGEdgeMlpAdjFn on the complete pattern with the dense ex_in);
each node runs 8 times and its largest error counts.  Bar: new <= 4 x existing + one float32 ulp of the gradient's largest magnitude
(the convention of tests/test_allpairs_mlp.py; the reference figure is measured from the EXISTING node).

Measured on an MI355X (largest of 8 runs, max abs error vs float64; new node / existing node):

    gradient   max |g|    new node / existing node
    dx         5.8e+00    4.3e-06 / 4.3e-06
    dk         2.6e+00    5.3e-07 / 5.3e-07
    dWe        2.5e+01    1.5e-05 / 1.5e-05
    dbe        1.7e+01    7.8e-06 / 8.2e-06
    dWcat      3.1e+01    1.4e-05 / 1.4e-05
    dwex       2.9e+00    9.4e-07 / 1.1e-06
    deb1       1.5e+01    5.2e-06 / 5.4e-06
    dw2        5.0e+01    2.9e-05 / 3.1e-05
    db2        1.4e+01    7.8e-06 / 8.7e-06

(two runs of the test; the largest ratio new / existing in either was 1.12, db2: the two nodes run the same backward on the same bits,
what differs is the order of its float atomics)
"""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_allpairs_mlp import (K, NOISE_MODE, NOISES, SEED, Canaried, Nn, T, complete_pattern, make_inputs, module_args, to_dev,
                               _node_inputs)

pytestmark = pytest.mark.gpu

# the switch sets with the prior extra: the specialised one (u-v-A_uv: LeakyReLU, no degree term) and the run-time variant's
PRIOR_SWITCHES = {"u-v-A_uv": (False, 1), "prior+deg": (True, 1), "prior+identity": (False, 0), "prior+deg+identity": (True, 0)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------
# inputs and reference
# ---------------------------------------------------------------------------------------------------------------
def make_prior(N, seed=0):
    """-> (P dense float32 [N,N], stored bool [N,N]): a sparse prior with, where N has room for them (N >= 8),
    row 0 storing ALL N columns, row 2 storing nothing, row 4 storing entries of the last (partial) 64-column tile only, row 6 storing
    exactly the columns 0, 63, 64, N - 1 and an explicit 0 at column 7; the other rows store about a quarter of the columns with values
    of order 1 of both signs, a few of them explicit zeros; of the tie nodes of make_inputs (columns 1, 5, N // 2, N - 1: identical
    rows of AB) those rows store column 5 only (every second row), never its twins."""
    rng = np.random.default_rng(500 + 7 * N + seed)
    f = np.float32
    stored = rng.random((N, N)) < 0.25
    v = rng.standard_normal((N, N))
    P = (np.sign(v) * (0.25 + np.abs(v))).astype(f)
    if N < 8:
        stored[:] = False
        stored[0, :] = True                                     # (N = 1: the one pair; N = 2: a full row and an empty one)
        return np.where(stored, P, 0).astype(f), stored
    zero = stored & (rng.random((N, N)) < 0.05)
    P[zero] = 0.0                                               # explicitly stored zeros
    twins = sorted({1, N // 2, N - 1} - {5})
    stored[:, twins] = False
    stored[:, 5] = False
    stored[::2, 5] = True
    P[::2, 5] = 0.75
    stored[0, :] = True
    P[0, P[0] == 0] = -0.5
    stored[2, :] = False
    last = 64 * ((N - 1) // 64)
    stored[4, :] = False
    stored[4, last:] = rng.random(N - last) < 0.5
    stored[4, N - 1] = True
    P[4, N - 1] = 1.25
    stored[6, :] = False
    for c in (0, 63, 64, N - 1):
        if c < N:
            stored[6, c] = True
            P[6, c] = -1.5 if c == 63 else 1.5
    stored[6, 7] = True
    P[6, 7] = 0.0
    return np.where(stored, P, 0).astype(f), stored


def prior_csr(stored, P):
    """-> rowptr int64 [N+1], col int32, val float32 (columns ascending within a row, the explicit zeros stored)"""
    N = stored.shape[0]
    rows, cols = np.nonzero(stored)
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=N))
    return rowptr, cols.astype(np.int32), P[rows, cols].astype(np.float32)


def prior_inputs(N, hw, seed=0):
    """make_inputs with wex = 0.5 sign(w2): a positive prior value raises the score of its pair, a negative one lowers it"""
    d = make_inputs(N, hw, hw, seed=seed)
    d["wex"] = (0.5 * np.where(d["w2"] >= 0, 1.0, -1.0)).astype(np.float32)
    return d


def switch_args(d, switches):
    has_deg, act = PRIOR_SWITCHES[switches]
    return (d["deg"], d["wdu"], d["wdv"], act) if has_deg else (None, None, None, act)


def oracle_scores_prior(d, P, switches):
    N = d["AB"].shape[0]
    _, col, erow = complete_pattern(N)
    deg, wdu, wdv, act = switch_args(d, switches)
    return O.edge_mlp_fwd(d["AB"], d["xp"], erow, col, deg, np.ascontiguousarray(P.reshape(-1)), 1, 0.0, wdu, wdv, d["wex"], d["b1"], d["w2"],
                          d["b2"][0], act)


def oracle_topk_prior(d, p, ex, noise, k=K):
    N = d["AB"].shape[0]
    rowptr, col, _ = complete_pattern(N)
    idx, val, eid = O.edgelist_topk_p(p, N, rowptr, col, k, NOISE_MODE[noise], d["G"] if noise == "explicit" else None, SEED)
    return idx, val, np.where(eid >= 0, ex[np.maximum(eid, 0)], 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(N, hw, switches, noise, empty=False):
    """the composed CPU oracle of one case (computed once, shared, never modified) -> idx, val, ex_out [N, K]"""
    d = prior_inputs(N, hw)
    P, _ = make_prior(N)
    if empty:
        P = np.zeros_like(P)
    p, ex = oracle_scores_prior(d, P, switches)
    out = oracle_topk_prior(d, p, ex, noise)
    for a in out:
        a.setflags(write=False)
    return out


def check_not_vacuous(N, ref, ref_empty, stored, what):
    """conditions on the INPUTS, read off the oracle's output: the prior must matter"""
    idx, _, exo = ref
    if N <= K:
        return
    assert (exo != 0).any(), f"{what}: no kept entry carries a prior value"
    kept = np.zeros((N, N), bool)
    kept[np.repeat(np.arange(N), K)[idx.reshape(-1) >= 0], idx.reshape(-1)[idx.reshape(-1) >= 0]] = True
    assert (stored & ~kept).any(), f"{what}: every stored entry is kept"
    differ = sum(set(a) != set(b) for a, b in zip(idx, ref_empty[0]))
    assert differ > N // 2, f"{what}: the kept set differs from the empty prior's in {differ} of {N} rows only"


def run_prior(dv, switches, noise, csr, dev, rows=None, out=None, k=K, ex_mode=1):
    from dgg_amd import ops
    deg, wdu, wdv, act = switch_args(dv, switches)
    return ops.allpairs_mlp_topk(dv["AB"], dv["xp"], deg, ex_mode, 0.0, wdu, wdv, dv["wex"], dv["b1"], dv["w2"], dv["b2"], act, k, NOISE_MODE[noise],
                                 dv["G"] if noise == "explicit" else None, SEED, rows=rows, out=out, prior=csr)


def assert_bits(buf, ref, what):
    idx, val, exo = (Nn(t) for t in buf.views())
    assert np.array_equal(idx, ref[0]), f"{what}: indices differ from the oracle"
    assert np.array_equal(val.view(np.int32), ref[1].view(np.int32)), f"{what}: scores differ from the oracle"
    assert np.array_equal(exo.view(np.int32), ref[2].view(np.int32)), f"{what}: extras differ from the oracle"
    assert buf.canaries_intact(), f"{what}: written outside the outputs"


def empty_csr(N, dev):
    return (torch.zeros(N + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
            torch.zeros(0, dtype=torch.float32, device=dev))


# ---------------------------------------------------------------------------------------------------------------
# 1. the list kernel against the composed CPU oracle, bit for bit
# ---------------------------------------------------------------------------------------------------------------
CASES = [(N, hw) for N in (1, 2, 63, 64, 65, 129, 257) for hw in (16, 64, 128)] + [(600, 64)]


def test_prior_inputs_hold_what_the_cases_need():
    """(host-side property of the inputs, kept next to them)"""
    for N in (63, 65, 129, 257, 600):
        P, stored = make_prior(N)
        last = 64 * ((N - 1) // 64)
        assert stored[0].all() and (P[0] != 0).all() and not stored[2].any()
        assert stored[4].any() and not stored[4, :last].any()
        assert set(np.nonzero(stored[6])[0]) == {c for c in (0, 63, 64, N - 1) if c < N} | {7} and P[6, 7] == 0
        assert (stored & (P == 0)).sum() > 1 and (P < 0).any() and (P > 0).any()
        twins = sorted({1, N // 2, N - 1} - {5})
        assert stored[8, 5] and not stored[8, twins].any()
        rowptr, col, val = prior_csr(stored, P)
        for i in range(N):
            assert (np.diff(col[rowptr[i]:rowptr[i + 1]]) > 0).all()
        d = prior_inputs(N, 64)
        assert np.array_equal(d["AB"][1], d["AB"][5]) and np.array_equal(d["AB"][1], d["AB"][N - 1])


@pytest.mark.parametrize("N,hw", CASES)
def test_kernel_matches_the_composed_cpu_oracle_bit_for_bit(dev, N, hw):
    """oracle.edge_mlp_fwd (ex_mode 1, ex_in = the dense prior) + oracle.edgelist_topk_p on the complete pattern; four noise settings;
    the prior of make_prior and the EMPTY prior (the oracle with an all-zero ex_in: the same switches with wex unused)"""
    d = prior_inputs(N, hw)
    dv = to_dev(d, dev)
    P, stored = make_prior(N)
    csr = tuple(T(a, dev) for a in prior_csr(stored, P))
    for noise in NOISES:
        ref, ref0 = reference(N, hw, "u-v-A_uv", noise), reference(N, hw, "u-v-A_uv", noise, empty=True)
        check_not_vacuous(N, ref, ref0, stored, f"N {N} / {noise}")
        if N < K:
            assert (ref[0][:, N:] == -1).all() and (ref[1][:, N:] == 0).all() and (ref[2][:, N:] == 0).all()
        buf = Canaried(N, dev)
        run_prior(dv, "u-v-A_uv", noise, csr, dev, out=buf.views())
        assert_bits(buf, ref, f"prior / {noise}")
        buf = Canaried(N, dev)
        run_prior(dv, "u-v-A_uv", noise, empty_csr(N, dev), dev, out=buf.views())
        assert_bits(buf, ref0, f"empty prior / {noise}")


@pytest.mark.parametrize("N,hw", [(257, 16), (129, 32), (257, 64), (257, 128)])
def test_both_row_blockings_and_the_run_time_switches_match_the_oracle(dev, monkeypatch, N, hw):
    """DGG_APMLP_RW = big / small: the 8-row (hw = 128: 4-row) and the 2-row kernels, on a partial last row block (N is no multiple of
    16 or 32), for u-v-A_uv and for the run-time variant (prior + degrees, prior + identity activation, both)"""
    dv = to_dev(prior_inputs(N, hw), dev)
    P, stored = make_prior(N)
    csr = tuple(T(a, dev) for a in prior_csr(stored, P))
    for switches in PRIOR_SWITCHES:
        for noise in NOISES:
            ref = reference(N, hw, switches, noise)
            for force in ("big", "small"):
                monkeypatch.setenv("DGG_APMLP_RW", force)
                buf = Canaried(N, dev)
                run_prior(dv, switches, noise, csr, dev, out=buf.views())
                assert_bits(buf, ref, f"{switches} / {noise} / {force}")


# ---------------------------------------------------------------------------------------------------------------
# 2. row ranges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["hash", "sym"])
def test_row_ranges_equal_the_slices_of_the_full_result(dev, monkeypatch, noise):
    """the CSR arrays stay the whole graph's; r0 = 37 and 3 are no multiples of a row block (8, 16, 32)"""
    N, hw = 257, 64
    dv = to_dev(prior_inputs(N, hw), dev)
    P, stored = make_prior(N)
    csr = tuple(T(a, dev) for a in prior_csr(stored, P))
    for force in ("big", "small"):
        monkeypatch.setenv("DGG_APMLP_RW", force)
        full = run_prior(dv, "u-v-A_uv", noise, csr, dev)
        assert np.array_equal(Nn(full[0]), reference(N, hw, "u-v-A_uv", noise)[0])
        for r0, r1 in ((0, N), (37, 101), (3, 9), (N - 1, N), (5, 5)):
            buf = Canaried(r1 - r0, dev)
            run_prior(dv, "u-v-A_uv", noise, csr, dev, rows=(r0, r1), out=buf.views())
            assert buf.canaries_intact(), f"rows {r0}:{r1}: written outside the range"
            if r0 == r1:
                assert buf.untouched()
                continue
            for got, ref in zip(buf.views(), full):
                assert torch.equal(got.view(torch.int32), ref[r0:r1].view(torch.int32)), f"{force} rows {r0}:{r1}"


# ---------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["null_rowptr", "null_col", "null_val", "ex_mode=0", "ex_mode=2", "noise=4", "noise=5", "hw=8", "K=65"])
def test_refusals_return_the_code_and_write_nothing(dev, what):
    from dgg_amd import ops
    from dgg_amd._lib import DggHipError
    key, _, v = what.partition("=")
    N, hw, k, ex_mode, noise = 70, 64, K, 1, 2
    if key == "hw":
        hw = int(v)
    elif key == "K":
        k = int(v)
    elif key == "ex_mode":
        ex_mode = int(v)
    elif key == "noise":
        noise = int(v)
    d = make_inputs(N, hw, 64)
    dv = to_dev(d, dev)
    P, stored = make_prior(N)
    csr = [T(a, dev) for a in prior_csr(stored, P)]
    buf = Canaried(N, dev, k)
    o = lambda t_: None if t_ is None else ops._ptr(t_)  # noqa: E731
    if key.startswith("null"):
        csr[("null_rowptr", "null_col", "null_val").index(key)] = None
    idx, val, ex = buf.views()
    from dgg_amd import _lib
    with pytest.raises(DggHipError, match=r"code [12]") as e:
        _lib.check(_lib.lib().dgg_allpairs_mlp_topk_prior(o(dv["AB"]), o(dv["xp"]), N, 64, hw, 0, N, None, ex_mode, 0.0, None, None, o(dv["wex"]),
                                                          o(dv["b1"]), o(dv["w2"]), o(dv["b2"]), 1, noise, None, 0, SEED[0], SEED[1], k, o(idx), o(val),
                                                          o(ex), o(csr[0]), o(csr[1]), o(csr[2]), ops._stream()), "allpairs_mlp_topk_prior")
    assert ("code 1" in str(e.value)) == key.startswith("null"), "NULL arrays are an argument error, the rest is unsupported"
    torch.cuda.synchronize()
    assert buf.untouched()


# ---------------------------------------------------------------------------------------------------------------
# 5. the autograd node
# ---------------------------------------------------------------------------------------------------------------
def float64_grads_prior(t, P, cot_rows, idx_rows, Gn):
    """dense float64 restatement of the definition with the prior extra: projection, u-v-A_uv on every pair, perturbation, the GIVEN
    selection idx_rows [N, R] (-1 = empty; rank = position), the ramp"""
    leaf = {n: v.double().clone().requires_grad_(True) for n, v in t.items() if v is not None}
    lrelu = torch.nn.functional.leaky_relu
    xp = lrelu(leaf["x"] @ leaf["We"].T + leaf["be"], 0.01)
    AB = xp @ leaf["Wcat"].T
    hw = AB.shape[1] // 2
    z = AB[:, None, :hw] + AB[None, :, hw:] + leaf["eb1"] + P.double()[:, :, None] * leaf["wex"]
    p = torch.sigmoid(lrelu(z, 0.01) @ leaf["w2"] + leaf["b2"])
    v = (p + 1e-8) * torch.exp(Gn.double())
    val = torch.gather(v, 1, idx_rows.long().clamp(min=0))
    ramp = 1.0 - 0.5 * (1.0 + torch.tanh(torch.arange(idx_rows.shape[1], dtype=torch.float64)[None, :] - leaf["k"][:, None]))
    w = torch.where(idx_rows >= 0, val * ramp, torch.zeros_like(val))
    (w * cot_rows.double()).sum().backward()
    return {n: v.grad for n, v in leaf.items()}


def node_inputs_prior(N, d_in, h, dev):
    t, deg, cot = _node_inputs(N, d_in, h, "u-v-deg-dist", dev)         # (the scorer with a wex)
    t["wdu"] = t["wdv"] = None
    t["wex"] = 0.5 * torch.where(t["w2"] >= 0, 1.0, -1.0)
    P, stored = make_prior(N)
    return t, deg, cot, P, stored


GRAD_NAMES = ("x", "k", "We", "be", "Wcat", "wex", "eb1", "w2", "b2")


def gradient_bar(run, g_new, g_old, ref, tag):
    """each node RUNS times, its largest error; new <= 4 x existing + one ulp of the gradient's largest magnitude"""
    RUNS = 8
    errs = {True: {n: 0.0 for n in GRAD_NAMES}, False: {n: 0.0 for n in GRAD_NAMES}}
    for new, g0 in ((True, g_new), (False, g_old)):
        for i in range(RUNS):
            g = g0 if i == 0 else run(new)[1]
            for n in GRAD_NAMES:
                errs[new][n] = max(errs[new][n], float((g[n].double() - ref[n]).abs().max()))
    bad = []
    for n in GRAD_NAMES:
        r = ref[n]
        e_new, e_old = errs[True][n], errs[False][n]
        ulp = float(np.spacing(np.float32(r.abs().max())))
        print(f"{tag:9s} d{n:5s} max|g|={float(r.abs().max()):.3e}  new {e_new:.3e}  existing {e_old:.3e}  ulp {ulp:.1e}")
        assert float(r.abs().max()) > 0, f"d{n}: the float64 gradient is identically zero (nothing checked)"
        if not e_new <= 4.0 * e_old + ulp:
            bad.append(f"d{n}: new {e_new:.3e} > 4 x {e_old:.3e} + {ulp:.1e}")
    assert not bad, "; ".join(bad)


def test_autograd_node_forward_bits_and_gradients(dev):
    from dgg_amd import ops
    from dgg_amd.dgm import _DGGAllPairsMlpAdjFn, _DGGEdgeMlpAdjFn
    N, d_in, h = 130, 24, 32
    t, deg, cot, P, stored = node_inputs_prior(N, d_in, h, dev)
    rowptr, col, erow = (T(a, dev) for a in complete_pattern(N))
    csr = tuple(T(a, dev) for a in prior_csr(stored, P))
    ex_in = T(np.ascontiguousarray(P.reshape(-1)), dev)

    def run(new):
        leaf = {n: (None if v is None else v.to(dev).requires_grad_(True)) for n, v in t.items()}
        cfg = dict(K=K, noise_mode=ops.NOISE_HASH, G=None, seed=SEED, mode=ops.MODE_K_TIMES_EDGE_PROB, ex_mode=1, t_ex=0.0, act=1)
        par = (leaf["We"], leaf["be"], leaf["Wcat"], None, None, leaf["wex"], leaf["eb1"], leaf["w2"], leaf["b2"])
        if new:
            cfg["prior"] = csr
            out = _DGGAllPairsMlpAdjFn.apply(leaf["x"], leaf["k"], deg.to(dev), *par, cfg)
        else:
            cfg["cand"] = (rowptr, col, erow)
            out = _DGGEdgeMlpAdjFn.apply(leaf["x"], leaf["k"], deg.to(dev), ex_in, *par, cfg)
        (out[0] * cot.to(dev)).sum().backward()
        return out, {n: leaf[n].grad.detach().cpu() for n in GRAD_NAMES}

    out_new, g_new = run(True)
    out_old, g_old = run(False)
    for a, b, what in zip(out_new, out_old, ("w", "idx", "val", "rs")):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), f"{what} differs from the edge-list node on the complete pattern"
    idx = out_new[1].cpu()
    assert float(torch.from_numpy(P)[torch.arange(N)[:, None].expand_as(idx), idx.long()].abs().max()) > 0, "no kept entry carries a prior value"
    Gn = torch.from_numpy(O.noise_matrix(N, SEED[0], SEED[1], symmetric=False))
    ref = float64_grads_prior(t, torch.from_numpy(P), cot, idx, Gn)
    gradient_bar(run, g_new, g_old, ref, "list")


# ---------------------------------------------------------------------------------------------------------------
# 6. the module
# ---------------------------------------------------------------------------------------------------------------
def module_prior(N, seed=3, nonneg=False):
    """a sparse prior whose values are multiples of 2^-7 (float row sums exact) -> dense float32 [N, N], about 6 entries per row, row 2
    empty"""
    rng = np.random.default_rng(seed)
    stored = rng.random((N, N)) < 6.0 / N
    stored[2] = False
    v = rng.integers(-256, 257, (N, N)).astype(np.float64) * 2.0 ** -7
    if nonneg:
        v = np.abs(v) + 2.0 ** -7
    return torch.from_numpy(np.where(stored, v, 0.0).astype(np.float32))


def complete_in_adj_with(P, dev):
    """the complete sparse in_adj that stores P's dense values, zeros stored explicitly"""
    N = P.shape[0]
    ar = torch.arange(N)
    ind = torch.stack([ar.repeat_interleave(N), ar.repeat(N)])
    a = torch.sparse_coo_tensor(ind, P.reshape(-1), (N, N)).coalesce()
    assert a.values().numel() == N * N
    return a.to(dev)


@pytest.mark.parametrize("noise", ["off", "asymmetric", "symmetric"])
def test_module_on_all_pairs_equals_the_module_on_the_complete_in_adj(dev, noise):
    """(fails before this feature: AllPairs takes no prior)"""
    import dgg_amd
    N, d_in, h = 130, 24, 32
    torch.manual_seed(5)
    args = module_args("u-v-A_uv", perturb=noise != "off", sym=noise == "symmetric")
    m1 = dgg_amd.DGG_LearnableK_debug(in_dim=d_in, latent_dim=h, args=args).to(dev)
    with torch.no_grad():
        m1.k_net.k_project.weight.mul_(0.1)
    m2 = copy.deepcopy(m1)
    m2.load_state_dict(m1.state_dict())
    for m in (m1, m2):
        m.set_seed(77, 5)
    x = torch.rand(N, d_in, generator=torch.Generator().manual_seed(1)).to(dev)
    P = module_prior(N)
    prior_degree = P.double().sum(1)
    assert torch.equal(prior_degree.float().double(), prior_degree), "the float row sums must be exact"
    A1 = dgg_amd.AllPairs(prior_degree.float().to(dev), prior=P.to_sparse().to(dev))
    A2 = complete_in_adj_with(P, dev)
    assert torch.equal(dgg_amd.csr_candidates(A2)[2].cpu(), prior_degree.float())
    a1 = m1(x, A1)
    a2 = m2(x, A2)
    assert isinstance(a1, dgg_amd.EllAdjacency) and isinstance(a2, dgg_amd.EllAdjacency)
    for m in (m1, m2):
        m.check_ell_bound()
    assert torch.equal(a1.idx, a2.idx)
    for f1, f2, what in ((a1.values(), a2.values(), "w"), (a1.rs, a2.rs, "rs"), (a1.k, a2.k, "k"), (a1.score, a2.score, "score")):
        assert torch.equal(f1.detach().view(torch.int32), f2.detach().view(torch.int32)), what
    assert int((a1.idx >= 0).sum()) == N * K and a1.owner is m1
    kept_prior = P.to(dev)[torch.arange(N, device=dev)[:, None].expand_as(a1.idx), a1.idx.long()]
    assert int((kept_prior != 0).sum()) > 0, "no kept entry is a prior edge"


def test_module_dgg_hard_is_straight_through_and_a_backward_runs(dev):
    import dgg_amd
    N, d_in, h = 130, 24, 32
    torch.manual_seed(5)
    m = dgg_amd.DGG_LearnableK_debug(in_dim=d_in, latent_dim=h, args=module_args("u-v-A_uv", dgg_hard=True)).to(dev)
    with torch.no_grad():
        m.k_net.k_project.weight.mul_(0.1)
    m.set_seed(77, 5)
    x = torch.rand(N, d_in, generator=torch.Generator().manual_seed(1)).to(dev)
    P = module_prior(N)
    a = m(x, dgg_amd.AllPairs(P.double().sum(1).float().to(dev), prior=P.to(dev)))       # (a dense prior is converted)
    w = a.values()
    # straight-through: the forward value is hard = the ramp mask at the selected columns, (hard - soft) + soft in float32 -- the score
    # does not enter it.  Against the ramp in float64: float32 rounding of the ramp and of the two additions, a few ulp of 1
    ramp = 1.0 - 0.5 * (1.0 + torch.tanh(torch.arange(K, device=dev, dtype=torch.float64)[None, :] - a.k.double()[:, None]))
    assert float((w.detach().double() - ramp).abs().max()) <= 1e-6 and float((a.score - w.detach()).abs().max()) > 0.1
    w.sum().backward()
    g = m.edge_encode[0].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g[:, 2 * h].abs().max()) > 0, "the weights of the prior column get a gradient"


# ---------------------------------------------------------------------------------------------------------------
# 7. the k-net gcn-x-deg on the prior
# ---------------------------------------------------------------------------------------------------------------
def test_gcn_x_deg_on_all_pairs_with_a_prior_equals_the_edge_list_k(dev):
    """same pattern (P + I), same kernels: k is equal as bits"""
    import dgg_amd
    N, d_in, h = 130, 24, 32
    torch.manual_seed(5)
    m1 = dgg_amd.DGG_LearnableK_debug(in_dim=d_in, latent_dim=h, args=module_args("u-v-A_uv", dgg_mode_k_net="gcn-x-deg")).to(dev)
    with torch.no_grad():
        m1.k_net.k_project.weight.mul_(0.1)
    m2 = copy.deepcopy(m1)
    for m in (m1, m2):
        m.set_seed(77, 5)
    x = torch.rand(N, d_in, generator=torch.Generator().manual_seed(1)).to(dev)
    P = module_prior(N, nonneg=True).to_sparse().to(dev)
    A = dgg_amd.AllPairs.from_graph(P, self_loops=True)
    eye = torch.arange(N, device=dev)
    PI = (P + torch.sparse_coo_tensor(torch.stack([eye, eye]), torch.ones(N, device=dev), (N, N))).coalesce()
    assert torch.equal(A.prior_degree, dgg_amd.csr_candidates(PI)[2])
    a1 = m1(x, A)
    a2 = m2(x, PI)
    assert torch.equal(a1.k.view(torch.int32), a2.k.view(torch.int32))
    a1.values().sum().backward()
    for p, name in ((m1.k_W, "k_W"), (m1.node_encode_for_k[0].weight, "node_encode_for_k"), (m1.k_net.k_project.weight, "k_project")):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name


# ---------------------------------------------------------------------------------------------------------------
# 8. training
# ---------------------------------------------------------------------------------------------------------------
def training_graph(N, dev):
    """row i has (i % 13) + 1 edges of weight 1 at fixed pseudo-random columns"""
    rng = np.random.default_rng(8)
    rows = np.concatenate([np.full((i % 13) + 1, i) for i in range(N)])
    cols = np.concatenate([rng.choice(N, (i % 13) + 1, replace=False) for i in range(N)])
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols])), torch.ones(len(rows)), (N, N)).coalesce().to(dev)


def _train(dev, chunked):
    import dgg_amd
    N, d_in, h, C = 257, 40, 32, 7
    kw = dict(dgg_allpairs_mlp_rows="chunked") if chunked else {}
    args = module_args("u-v-A_uv", dgg_wide_rows="auto", **kw)
    torch.manual_seed(3)
    model = dgg_amd.GCN_DGG(nfeat=d_in, nhidden=h, nclass=C, args=args).to(dev)
    with torch.no_grad():
        model.dggs[0].k_net.k_project.weight.mul_(0.1)
        if chunked:                                                # learned degrees beyond the list: k = relu(kp sd + mu) + 1 with kp ~ 20
            model.dggs[0].k_net.k_project.bias.fill_(20.0)
    x = torch.rand(N, d_in, generator=torch.Generator().manual_seed(1)).to(dev)
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(2)).to(dev)
    A = dgg_amd.AllPairs.from_graph(training_graph(N, dev), self_loops=True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    for step in range(5):
        opt.zero_grad()
        logp, adj, _ = model(x, A)
        loss = torch.nn.functional.nll_loss(logp, y)
        loss.backward()
        for n, p in model.named_parameters():
            assert p.grad is None or bool(torch.isfinite(p.grad).all()), f"step {step}: {n}"
        opt.step()
        losses.append(float(loss.detach()))
    print("loss per step:", " ".join(f"{v:.4f}" for v in losses))
    return model, adj, losses


def test_gcn_dgg_trains_on_all_pairs_with_a_prior(dev):
    """(fails before this feature: AllPairs has no from_graph and takes no prior)"""
    import dgg_amd
    model, adj, losses = _train(dev, chunked=False)
    assert all(np.isfinite(losses)) and losses[4] < losses[0]
    dgg = model.dggs[0]
    dgg.check_ell_bound()
    assert isinstance(adj, dgg_amd.EllAdjacency) and adj.layout is None
    assert set(dgg.fused_fallback) == {"edge-MLP scorer on all-pairs candidates"}


def test_gcn_dgg_trains_past_the_list_on_chunked_rows(dev):
    import dgg_amd
    model, adj, losses = _train(dev, chunked=True)
    assert all(np.isfinite(losses)) and losses[4] < losses[0]
    assert float(adj.k.max()) + 8.5 > 64, "the learned degrees must outgrow the 64-rank list in this run"
    model.dggs[0].check_ell_bound()
    assert isinstance(adj, dgg_amd.EllAdjacency) and adj.layout is not None and adj.layout.wide
