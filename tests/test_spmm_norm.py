"""normalize_adj inside the forward aggregation (dgg_ell_spmm_norm_act_fwd[_chunked], include/dgg_hip_next.h) against the pair it replaces,
in the SAME build and bit for bit: partp_build(rs_all) -> ahat, spmm_fwd(idx, ahat, H, relu) on one side, partp_build(rs_all,
want_ahat=False) -> spmm_norm_fwd on the other.  Also: the partition's records and nodeptr with and without the fused ahat, the row
kernel of the score backward with a_j from the partition's table and from the expression, the count-only partition of a forward without
a backward, and the whole layer under DGG_NORM_IN_SPMM = 0 / 1."""
import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

T_DIST = -0.05
ULP = 2.0 ** -23          # one float32 ulp of a gradient's largest element, relative to it


def within_own_spread(d_new_old, d_old_old):
    """The rule for gradients: new / old within 4x old / old, both relative to the gradient's largest element.  Two
    runs of the old order can agree exactly -- `bp` is ONE number that moves by one ulp or not at all -- and 4 x 0 would then demand
    bit equality of a backward that is not reproducible bit for bit; the smallest difference float32 can show at the largest element,
    one ulp, is therefore always allowed."""
    return d_new_old <= max(4 * d_old_old, ULP)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


def Nn(t):
    return t.detach().cpu().numpy()


def make_block(rows, ncols, row0, seed, hub_everywhere=False):
    """idx / w / val [rows,64], rs_all [ncols] on the host.  Rows 0..5 are the named cases (64 live entries; 41; the self loop alone;
    idx = -1 holes in the middle; idx >= 0 with w == 0; repeated columns); every other row has 12..64 ranks with random holes and zero
    weights.  Column `hub` is an entry of every row but the single-entry one (hub_everywhere: no single-entry row, so of EVERY row)."""
    g = np.random.default_rng(seed)
    idx = np.full((rows, 64), -1, np.int32)
    w = np.zeros((rows, 64), np.float32)
    hub = 7
    for i in range(rows):
        L = int(g.integers(12, 65))
        if i == 0:
            L = 64
        elif i == 1:
            L = 41
        idx[i, :L] = g.permutation(ncols)[:L]
        w[i, :L] = g.uniform(0.01, 1.0, L).astype(np.float32)
        if i == 2 and not hub_everywhere:                          # the self loop alone
            idx[i], w[i] = -1, 0.0
            idx[i, 0], w[i, 0] = row0 + i, 1.0
            continue
        if i == 3:
            idx[i, 5:9] = -1                                       # holes in the middle (their weights stay: the index decides)
            idx[i, 17] = -1
        elif i == 4:
            w[i, [0, 3, 20, L - 1]] = 0.0                          # idx >= 0 and w == 0
        elif i == 5:
            idx[i, 10:14] = idx[i, 2]                              # repeated columns
            idx[i, 30] = idx[i, 31]
        elif i > 5:
            idx[i, g.integers(0, L, 2)] = -1
            w[i, g.integers(0, L, 2)] = 0.0
        idx[i, int(g.integers(0, min(L, 12)))] = hub
        if w[i][idx[i] == hub].max() == 0.0:
            w[i, np.nonzero(idx[i] == hub)[0][0]] = 0.5
    val = g.uniform(0.05, 1.0, (rows, 64)).astype(np.float32)
    rs_all = g.uniform(0.3, 40.0, ncols).astype(np.float32)
    return idx, w, val, rs_all


def to_dev(dev, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def sorted_records(ops, part):
    """(nodeptr, records with every node's records ordered by slot) of a sorted payload partition, on the host"""
    nodeptr, recs = ops.partp_records(part)
    nodeptr, recs = Nn(nodeptr).astype(np.int64), Nn(recs)
    node = np.repeat(np.arange(nodeptr.shape[0] - 1), np.diff(nodeptr))
    order = np.lexsort((recs[:, 0], node))
    return nodeptr, recs[order]


def oracle_ahat(idx, w, rs_all, row0):
    """oracle.normalize on the host for the rows [row0, row0 + rows) of an ncols-node graph"""
    ncols, rows = rs_all.shape[0], idx.shape[0]
    fi = np.full((ncols, 64), -1, np.int32)
    fw = np.zeros((ncols, 64), np.float32)
    fi[row0:row0 + rows], fw[row0:row0 + rows] = idx, w
    live = (idx >= 0) & (w != 0)
    return np.where(live, O.normalize(fi, fw, rs_all)[row0:row0 + rows], np.float32(0))


def pair_and_new(ops, dev, idx, w, val, rs_all, row0, F, act, layout=None, seed=3):
    rows = idx.shape[0] if layout is None else layout.rows
    ncols = rs_all.shape[0]
    H = torch.randn(ncols, F, generator=torch.Generator().manual_seed(seed)).to(dev)
    rs_rows = rs_all[row0:row0 + rows].contiguous()
    kw = {} if layout is None else {"layout": layout}
    part_o, ahat_o = ops.partp_build(idx, w, val, rs_rows, ncols, rs_all, **kw)
    Y_o = ops.spmm_fwd(idx, ahat_o, H, act, **kw)
    part_n, none = ops.partp_build(idx, w, val, rs_rows, ncols, rs_all, want_ahat=False, **kw)
    assert none is None and part_n.has_ainv
    Y_n, ahat_n = ops.spmm_norm_fwd(idx, w, rs_rows, part_n, H, act, **kw)
    torch.cuda.synchronize()
    return (part_o, ahat_o, Y_o), (part_n, ahat_n, Y_n)


@pytest.mark.parametrize("F", [16, 32, 64])
@pytest.mark.parametrize("shape", ["whole", "shard", "hub"])
def test_new_path_equals_the_old_pair_bit_for_bit(dev, F, shape):
    """rows = 259 (no multiple of 4 or 16) of ncols = 300, and the row shard 100..199 of 300 nodes (row0 > 0, ncols > rows): Y, ahat,
    nodeptr and the slot-ordered records; ahat also against oracle.normalize on the host"""
    from dgg_amd import ops
    rows, ncols, row0 = {"whole": (259, 300, 0), "shard": (100, 300, 100), "hub": (259, 300, 0)}[shape]
    hi, hw, hv, hrs = make_block(rows, ncols, row0, 11, hub_everywhere=shape == "hub")
    if shape == "hub":
        assert ((hi == 7) & (hw != 0)).any(1).all()
    else:
        assert ((hi[2] >= 0).sum(), hi[2, 0]) == (1, row0 + 2) and (hi[0] >= 0).all() and (hi[1] >= 0).sum() == 41
    idx, w, val, rs_all = to_dev(dev, hi, hw, hv, hrs)
    for act in (ops.ACT_RELU, ops.ACT_NONE):
        (part_o, ahat_o, Y_o), (part_n, ahat_n, Y_n) = pair_and_new(ops, dev, idx, w, val, rs_all, row0, F, act)
        assert torch.equal(ahat_n, ahat_o), "ahat differs from the fill pass's"
        assert torch.equal(Y_n, Y_o), "Y differs from spmm_fwd on the fill pass's ahat"
    assert np.array_equal(Nn(ahat_n), oracle_ahat(hi, hw, hrs, row0)), "ahat differs from oracle.normalize"
    assert bool((ahat_n[(idx < 0) | (w == 0)] == 0).all())
    np_o, rec_o = sorted_records(ops, part_o)
    np_n, rec_n = sorted_records(ops, part_n)
    assert np.array_equal(np_o, np_n), "nodeptr differs"
    assert np.array_equal(rec_o, rec_n), "records differ"
    assert rec_o.shape[0] == int(((hi >= 0) & (hw != 0)).sum())


def chunked_block(dev, ops, nodes, ncols, seed):
    """chunked rows with 1, 2 and 3 chunks per node (dgg_chunk_layout of learned degrees 10 / 80 / 150)"""
    k = torch.tensor([(10.0, 80.0, 150.0)[i % 3] for i in range(nodes)], device=dev)
    lay = ops.chunk_layout(k, ncols=ncols)
    per = Nn(lay.cptr[1:] - lay.cptr[:-1])
    assert lay.wide and sorted(set(per.tolist())) == [1, 2, 3]
    hi, hw, hv, hrs = make_block(lay.chunks, ncols, 0, seed, hub_everywhere=True)
    return (k, lay, hi, hw, hv, hrs) + tuple(to_dev(dev, hi, hw, hv, hrs))


@pytest.mark.parametrize("F", [16, 32, 64])
def test_chunked_rows_equal_the_old_pair_bit_for_bit(dev, F):
    from dgg_amd import ops
    nodes, ncols = 91, 300
    k, lay, hi, hw, hv, hrs, idx, w, val, rs_all = chunked_block(dev, ops, nodes, ncols, 5)
    (part_o, ahat_o, Y_o), (part_n, ahat_n, Y_n) = pair_and_new(ops, dev, idx, w, val, rs_all, 0, F, ops.ACT_RELU, layout=lay)
    assert tuple(Y_n.shape) == (nodes, F)
    assert torch.equal(ahat_n, ahat_o) and torch.equal(Y_n, Y_o)
    # a_i of a chunk is its NODE's: the host restatement normalises every chunk as a row of its node
    cn = Nn(lay.cnode)
    want = np.zeros_like(hw)
    ainv = (np.float32(1) / np.sqrt(hrs)).astype(np.float32)
    live = (hi >= 0) & (hw != 0)
    want[live] = ((ainv[cn][:, None] * hw).astype(np.float32) * ainv[np.where(hi >= 0, hi, 0)]).astype(np.float32)[live]
    assert np.array_equal(Nn(ahat_n), want), "ahat differs from the host restatement of oracle.normalize on chunked rows"
    np_o, rec_o = sorted_records(ops, part_o)
    np_n, rec_n = sorted_records(ops, part_n)
    assert np.array_equal(np_o, np_n) and np.array_equal(rec_o, rec_n)


def test_spare_chunks_of_a_fixed_capacity_get_zero_ahat(dev):
    """chunks in [cptr[rows], chunks) -- the spare capacity of a fixed-size layout -- are written 0, as the fill pass writes them"""
    from dgg_amd import ops
    nodes, ncols, F = 91, 300, 32
    k, lay, hi, hw, hv, hrs, idx, w, val, rs_all = chunked_block(dev, ops, nodes, ncols, 6)
    spare = 9
    cap = ops.ChunkLayout(lay.cptr, torch.cat([lay.cnode, lay.cnode.new_zeros(spare)]), lay.meta, lay.chunks + spare, lay.maxm, nodes)
    pad_i = torch.cat([idx, idx.new_full((spare, 64), -1)])
    pad_w, pad_v = torch.cat([w, w.new_zeros(spare, 64)]), torch.cat([val, val.new_zeros(spare, 64)])
    (_, ahat_o, Y_o), (_, ahat_n, Y_n) = pair_and_new(ops, dev, pad_i, pad_w, pad_v, rs_all, 0, F, ops.ACT_RELU, layout=cap)
    assert torch.equal(ahat_n, ahat_o) and torch.equal(Y_n, Y_o) and bool((ahat_n[lay.chunks:] == 0).all())


@pytest.mark.parametrize("form", ["list", "chunked"])
def test_every_way_to_build_the_partition_gives_the_same_partition(dev, form):
    """partp_build in every supported (phase, want_ahat), phase 1 finished by partp_sort: one nodeptr, one set of slot-ordered records,
    one ahat; and the count-only partition (phase 3) normalises inside the aggregation to the bits of the records-only one"""
    from dgg_amd import ops
    if form == "chunked":
        nodes, ncols = 91, 300
        k, lay, hi, hw, hv, hrs, idx, w, val, rs_all = chunked_block(dev, ops, nodes, ncols, 5)
        kw = {"layout": lay}
    else:
        nodes, ncols = 259, 300
        idx, w, val, rs_all = to_dev(dev, *make_block(nodes, ncols, 0, 11))
        kw = {}
    rs_rows = rs_all[:nodes].contiguous()
    parts, ahats = {}, {}
    for phase, want_ahat in ((0, True), (1, True), (0, False), (1, False), (3, False)):
        part, ahat = ops.partp_build(idx, w, val, rs_rows, ncols, rs_all, phase=phase, want_ahat=want_ahat, **kw)
        assert part.has_ainv and (ahat is not None) == want_ahat
        if phase == 1:
            ops.partp_sort(part)
        parts[phase, want_ahat] = part
        if want_ahat:
            ahats[phase, want_ahat] = ahat
    if form == "list":
        parts["plain"] = ops.partp_build(idx, w, val, rs_rows, ncols)
        assert isinstance(parts["plain"], ops.PartP) and not parts["plain"].has_ainv
    torch.cuda.synchronize()
    count_only = parts.pop((3, False))           # (never filled: it has no records to compare)
    nodeptr0, rec0 = sorted_records(ops, parts[0, True])
    assert rec0.shape[0] == int(((idx >= 0) & (w != 0)).sum())
    for how, part in parts.items():
        nodeptr, rec = sorted_records(ops, part)
        assert np.array_equal(nodeptr, nodeptr0), f"{how}: nodeptr differs"
        assert np.array_equal(rec, rec0), f"{how}: records differ"
    assert torch.equal(ahats[1, True], ahats[0, True]), "ahat of phase 1 differs from phase 0's"
    H = torch.randn(ncols, 32, generator=torch.Generator().manual_seed(3)).to(dev)
    Y_c, ahat_c = ops.spmm_norm_fwd(idx, w, rs_rows, count_only, H, ops.ACT_RELU, **kw)
    Y_r, ahat_r = ops.spmm_norm_fwd(idx, w, rs_rows, parts[0, False], H, ops.ACT_RELU, **kw)
    torch.cuda.synchronize()
    assert torch.equal(Y_c, Y_r) and torch.equal(ahat_c, ahat_r), "the count-only partition normalises differently"
    assert torch.equal(ahat_r, ahats[0, True]), "ahat of the aggregation differs from the fill pass's"


@pytest.mark.parametrize("h", [16, 64, 128])
@pytest.mark.parametrize("form", ["list", "shard", "chunked"])
def test_row_kernel_with_the_table_equals_the_expression(dev, h, form):
    """ONE sorted partition, one dA: the row kernel of the score backward with a_j from the partition's rs^-1/2 table and with the
    division and square root per lane -- dxp (the rows' own side), dk and rowinfo bit for bit"""
    from dgg_amd import ops
    g = torch.Generator().manual_seed(h)
    if form == "chunked":
        nodes, ncols, row0 = 91, 300, 0
        k, lay, hi, hw, hv, hrs, idx, w, val, rs_all = chunked_block(dev, ops, nodes, ncols, 8)
        kw = {"layout": lay}
    else:
        nodes, ncols, row0 = (259, 300, 0) if form == "list" else (100, 300, 100)
        idx, w, val, rs_all = to_dev(dev, *make_block(nodes, ncols, row0, 9))
        k = (5 + 45 * torch.rand(nodes, generator=g)).to(dev)
        kw = {}
    n = idx.shape[0]
    part, ahat = ops.partp_build(idx, w, val, rs_all[row0:row0 + nodes].contiguous(), ncols, rs_all, **kw)
    xp = torch.randn(ncols, h, generator=g).to(dev)
    dA, da = torch.randn(n, 64, generator=g).to(dev), torch.randn(ncols, generator=g).to(dev)
    dA_rec = torch.randn(n * 64, generator=g).to(dev)
    out = []
    for tab in (False, True):
        dxp, dk, st = ops.softk_edge_bwd_p(xp, idx, val, k, dA, dA_rec, rs_all, da, row0, T_DIST, True, ops.MODE_K_TIMES_EDGE_PROB, True, part,
                                           ahat_rows=ahat, phase=1, ainv_table=tab)
        torch.cuda.synchronize()
        out.append((dxp[row0:row0 + nodes].clone(), dk.clone(), st[2].clone()))
    for name, a, b in zip(("dxp", "dk", "rowinfo"), out[0], out[1]):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"{name}: the table and the expression differ"
    assert float(out[0][0].abs().max()) > 0 and float(out[0][1].abs().max()) > 0


def _layer(dev, N, d, h, norm, want_backward=True):
    import bench
    from dgg_amd import ops
    from dgg_amd.parallel import ShardedDGGConv
    P = bench.make_params(d, h, dev)
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(1000)).to(dev)
    deg = (24 + 16 * torch.rand(N, generator=torch.Generator().manual_seed(7))).to(dev)
    layer = ShardedDGGConv(ops, N, K=64, noise_mode=ops.NOISE_RANKED, seed=(1234, 0))
    layer.norm_in_spmm = norm
    layer.want_backward = want_backward
    return layer, x, deg, P


def test_forward_without_backward_runs_the_count_pass_only(dev):
    """want_backward = False: Z and ahat as from the old pair, and under ops.PROBE neither the fill pass nor the sort is recorded"""
    from dgg_amd import ops
    N, d, h = 4096, 32, 64
    res = {}
    for norm in (False, True):
        layer, x, deg, P = _layer(dev, N, d, h, norm, want_backward=False)
        ops.PROBE = {}
        try:
            Z = layer.forward(x, deg, P)
            torch.cuda.synchronize()
        finally:
            probe, ops.PROBE = ops.PROBE, None
        res[norm] = (Z, layer.saved["ahat"], set(probe))
        assert not layer.saved["partp_sorted"]
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert "pp_count" in res[True][2] and not {"pp_fill", "pp_sort"} & res[True][2], res[True][2]
    assert "spmm_fwd" in res[True][2]


@pytest.fixture(scope="module")
def layer_runs(dev):
    """the whole layer at N = 4096, d = 32, h = F = 64 under ranked noise, fixed seed: the old order twice, the new order once"""
    N, d, h = 4096, 32, 64
    runs = []
    for norm in (False, False, True):
        layer, x, deg, P = _layer(dev, N, d, h, norm)
        Z = layer.forward(x, deg, P)
        dZ = torch.randn(Z.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        grads = layer.backward(dZ, x, P)
        torch.cuda.synchronize()
        s = layer.saved
        runs.append((dict(Z=Z, idx=s["idx"], w=s["w"], ahat=s["ahat"]), {n_: g_.detach().clone() for n_, g_ in grads.items() if torch.is_tensor(g_)}))
    return runs


def test_whole_layer_forward_is_bit_identical(layer_runs):
    old, _, new = layer_runs
    for name in ("Z", "idx", "w", "ahat"):
        assert torch.equal(old[0][name], new[0][name]), name


def test_sort_beside_the_normalising_aggregation(dev, layer_runs):
    """DGG_OVERLAP=1's placement (the partition's sort on the second stream, beside the aggregation) with the records-only fill pass:
    the forward is the old order's bit for bit, the gradients stay inside the same 4x rule"""
    old, old2, _ = layer_runs
    layer, x, deg, P = _layer(dev, 4096, 32, 64, True)
    layer.overlap, layer.overlap_sort = True, True
    Z = layer.forward(x, deg, P)
    assert layer.saved["side_join"]
    grads = layer.backward(torch.randn(Z.shape, generator=torch.Generator().manual_seed(3)).to(dev), x, P)
    torch.cuda.synchronize()
    assert torch.equal(Z, old[0]["Z"]) and torch.equal(layer.saved["ahat"], old[0]["ahat"])
    for name, g_ in old[1].items():
        scale = float(g_.abs().max())
        assert within_own_spread(float((grads[name] - g_).abs().max()) / scale, float((g_ - old2[1][name]).abs().max()) / scale), name


def test_whole_layer_gradients_within_four_times_the_old_paths_own_spread(layer_runs):
    """The record order inside a node is an LDS arrival order, so the backward is not reproducible bit for bit: the new / old difference
    of every gradient must stay within 4x the old / old difference, relative to the gradient's largest element (within_own_spread)."""
    old, old2, new = layer_runs
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
