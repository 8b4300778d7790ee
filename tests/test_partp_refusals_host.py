"""Host-side characterisation (no GPU) of the payload-partition entry points' argument checks: the build, conv-backward and
score-backward entries for 64-rank lists and for chunked rows.  Their checks run entirely on the host, so a refused call -- or a valid
call on an EMPTY block -- never touches a device: every call below is one of the two, made with dummy addresses that are never
dereferenced.  The expected codes are written out from the entries' documented rules (order: phase range, unsupported size / NULL
workspace, operands, alignment, empty block)."""
import pytest

OK, ARG, UNSUPPORTED = 0, 1, 2                   # DGG_ERR_ARG, DGG_ERR_UNSUPPORTED (include/dgg_hip.h)
NCOLS, ROWS = 300, 259
P = 0x100000                                     # a 16-byte aligned dummy address; P + 4 is a misaligned one
T_DIST = -0.05


@pytest.fixture(scope="module")
def L():
    import dgg_amd
    return dgg_amd._lib.lib()


def expect(L, what, rc, want):
    assert rc == want, "%s: status %d, expected %d (%s)" % (what, rc, want, L.dgg_last_error().decode())
    if want != OK:
        text = L.dgg_last_error().decode()
        assert text != "" and "partp" in text, "%s: dgg_last_error() does not describe the refusal: %r" % (what, text)


# ---- build ------------------------------------------------------------------------------------------------------------------------
def build(L, entry, **over):
    """one call of a build entry on an empty block (rows = 0 / chunks = 0) unless `rows` says otherwise"""
    a = dict(idx=P, w=P, val=P, rs_rows=P, rows=0, K=64, ncols=NCOLS, rs_all=None, ahat=None, ws=P, phase=0, cnode=P)
    a.update(over)
    if entry == "dgg_partp_build":
        return L.dgg_partp_build(a["idx"], a["w"], a["val"], a["rs_rows"], a["rows"], a["K"], a["ncols"], a["ws"], None)
    if entry == "dgg_partp_build_norm":
        return L.dgg_partp_build_norm(a["idx"], a["w"], a["val"], a["rs_rows"], a["rows"], a["K"], a["ncols"], a["rs_all"], a["ahat"], a["ws"], None)
    if entry == "dgg_partp_build_phase":
        return L.dgg_partp_build_phase(a["idx"], a["w"], a["val"], a["rs_rows"], a["rows"], a["K"], a["ncols"], a["rs_all"], a["ahat"], a["ws"],
                                       a["phase"], None)
    assert entry == "dgg_partp_build_chunked" and a["K"] == 64
    return L.dgg_partp_build_chunked(a["idx"], a["w"], a["val"], a["rs_rows"], a["rows"], a["cnode"], a["ncols"], a["rs_all"], a["ahat"], a["ws"],
                                     a["phase"], None)


PHASED = ("dgg_partp_build_phase", "dgg_partp_build_chunked")
# phase -> status for (rs_all, ahat) = (NULL, NULL), (given, NULL), (NULL, given), (given, given)
PHASE_GRID = {
    -1: (ARG, ARG, ARG, ARG),
    0: (OK, ARG, ARG, OK),                       # phases 0..2: rs_all and ahat go together ("rs_all-without-ahat")
    1: (OK, ARG, ARG, OK),
    2: (OK, ARG, ARG, OK),
    3: (ARG, OK, ARG, OK),                       # the count pass: rs_all, whatever ahat is
    4: (ARG, OK, ARG, ARG),                      # records only: rs_all and no ahat
    5: (ARG, OK, ARG, ARG),
    6: (ARG, ARG, ARG, ARG),
}


@pytest.mark.parametrize("entry", PHASED)
def test_build_phase_against_rs_all_and_ahat(L, entry):
    for phase, row in PHASE_GRID.items():
        for (rs_all, ahat), want in zip(((None, None), (P, None), (None, P), (P, P)), row):
            expect(L, "%s phase %d rs_all=%s ahat=%s" % (entry, phase, rs_all, ahat), build(L, entry, phase=phase, rs_all=rs_all, ahat=ahat), want)


@pytest.mark.parametrize("entry", PHASED)
def test_build_order_of_checks_and_operands(L, entry):
    for what, over, want in (
            ("NULL ws", dict(ws=None), UNSUPPORTED),
            ("NULL ws, rows > 0", dict(ws=None, rows=ROWS), UNSUPPORTED),
            ("phase before ws", dict(ws=None, phase=6), ARG),
            ("ws before operands", dict(ws=None, val=None), UNSUPPORTED),
            ("no destination nodes", dict(ncols=0), UNSUPPORTED),
            ("missing val", dict(val=None), ARG),
            ("missing rs_rows", dict(rs_rows=None, rows=ROWS), ARG),
            ("phase 2 still demands val", dict(val=None, phase=2), ARG),
            ("phase 2 still demands rs_rows", dict(rs_rows=None, phase=2), ARG),
            ("phase 3 without rs_all", dict(phase=3, rows=ROWS), ARG),
            ("phase 3 without idx", dict(phase=3, rs_all=P, idx=None), ARG),
            ("phase 3 without w", dict(phase=3, rs_all=P, w=None), ARG),
            ("phase 3 reads neither val nor rs_rows", dict(phase=3, rs_all=P, val=None, rs_rows=None), OK),
            ("phase 3 aligns idx", dict(phase=3, rs_all=P, idx=P + 4), ARG),
            ("phase 3 does not align val", dict(phase=3, rs_all=P, val=P + 4), OK),
            ("misaligned idx", dict(idx=P + 4), ARG),
            ("misaligned idx, rows > 0", dict(idx=P + 4, rows=ROWS), ARG),
            ("misaligned w", dict(w=P + 8), ARG),
            ("misaligned val", dict(val=P + 4), ARG),
            ("misaligned ahat", dict(rs_all=P, ahat=P + 4), ARG),
            ("empty block", dict(), OK)):
        expect(L, "%s: %s" % (entry, what), build(L, entry, **over), want)


def test_build_list_only(L):
    e = "dgg_partp_build_phase"
    expect(L, "K = 65", build(L, e, K=65), UNSUPPORTED)
    expect(L, "K = 0", build(L, e, K=0), UNSUPPORTED)
    expect(L, "K = 32 aligns nothing", build(L, e, K=32, idx=P + 4), OK)
    expect(L, "K = 32 aligns nothing at phase 3", build(L, e, K=32, phase=3, rs_all=P, idx=P + 4), OK)
    expect(L, "K = 32, empty block", build(L, e, K=32), OK)
    expect(L, "cnode is no operand of the list entry", build(L, e, cnode=None), OK)
    # the two older spellings of phase 0
    expect(L, "build", build(L, "dgg_partp_build"), OK)
    expect(L, "build, NULL ws", build(L, "dgg_partp_build", ws=None), UNSUPPORTED)
    expect(L, "build, missing val", build(L, "dgg_partp_build", val=None, rows=ROWS), ARG)
    expect(L, "build, misaligned idx", build(L, "dgg_partp_build", idx=P + 4), ARG)
    expect(L, "build_norm", build(L, "dgg_partp_build_norm", rs_all=P, ahat=P), OK)
    expect(L, "build_norm without either", build(L, "dgg_partp_build_norm"), OK)
    expect(L, "build_norm, rs_all without ahat", build(L, "dgg_partp_build_norm", rs_all=P, rows=ROWS), ARG)
    expect(L, "build_norm, ahat without rs_all", build(L, "dgg_partp_build_norm", ahat=P), ARG)
    expect(L, "build_norm, NULL ws", build(L, "dgg_partp_build_norm", rs_all=P, ahat=P, ws=None), UNSUPPORTED)


def test_build_chunked_only(L):
    e = "dgg_partp_build_chunked"
    expect(L, "missing cnode", build(L, e, cnode=None), ARG)
    expect(L, "missing cnode, rows > 0, records only", build(L, e, cnode=None, phase=5, rs_all=P, rows=ROWS), ARG)
    expect(L, "missing cnode at phase 2", build(L, e, cnode=None, phase=2), ARG)
    expect(L, "phase 3 does not look at cnode", build(L, e, cnode=None, phase=3, rs_all=P), OK)


# ---- conv backward -----------------------------------------------------------------------------------------------------------------
CONV = ("dgg_ell_conv_bwd_partp", "dgg_ell_conv_bwd_partp_ext", "dgg_ell_conv_bwd_partp_chunked")


def conv(L, entry, **over):
    a = dict(G=P, H=P, rows=0, K=64, F=32, ws=P, ncols=NCOLS, rs=P, dA_ext=None, dA=P, dA_rec=P, dH=P, da=P)
    a.update(over)
    if entry == "dgg_ell_conv_bwd_partp":
        return L.dgg_ell_conv_bwd_partp(a["G"], a["H"], a["rows"], a["K"], a["F"], a["ws"], a["ncols"], a["rs"], a["dA"], a["dA_rec"], a["dH"], a["da"], None)
    if entry == "dgg_ell_conv_bwd_partp_ext":
        return L.dgg_ell_conv_bwd_partp_ext(a["G"], a["H"], a["rows"], a["K"], a["F"], a["ws"], a["ncols"], a["rs"], a["dA_ext"], a["dA"], a["dA_rec"],
                                            a["dH"], a["da"], None)
    assert entry == "dgg_ell_conv_bwd_partp_chunked" and a["K"] == 64
    return L.dgg_ell_conv_bwd_partp_chunked(a["G"], a["H"], a["rows"], a["F"], a["ws"], a["ncols"], a["rs"], a["dA_ext"], a["dA"], a["dA_rec"], a["dH"],
                                            a["da"], None)


@pytest.mark.parametrize("entry", CONV)
def test_conv_backward(L, entry):
    for what, over, want in (
            ("F-48", dict(F=48, rows=ROWS), UNSUPPORTED),
            ("misaligned G", dict(G=P + 4), UNSUPPORTED),
            ("misaligned H", dict(H=P + 8, rows=ROWS), UNSUPPORTED),
            ("misaligned dH", dict(dH=P + 4), UNSUPPORTED),
            ("width before operands", dict(F=48, rs=None), UNSUPPORTED),
            ("missing-rs", dict(rs=None, rows=ROWS), ARG),
            ("missing dA_rec", dict(dA_rec=None), ARG),
            ("no partition", dict(ws=None, rows=ROWS), ARG),
            ("no destination nodes", dict(ncols=0), ARG),
            ("da is optional", dict(da=None), OK),
            ("zero-rows-conv", dict(), OK),
            ("zero-rows-conv, F = 128", dict(F=128), OK)):
        expect(L, "%s: %s" % (entry, what), conv(L, entry, **over), want)


def test_conv_backward_list_and_chunked_differ_in_dA(L):
    expect(L, "list without dA", conv(L, "dgg_ell_conv_bwd_partp"), OK)
    expect(L, "list without dA", conv(L, "dgg_ell_conv_bwd_partp_ext", dA=None), OK)
    expect(L, "chunked without dA", conv(L, "dgg_ell_conv_bwd_partp_chunked", dA=None), ARG)
    expect(L, "chunked without dA, rows > 0", conv(L, "dgg_ell_conv_bwd_partp_chunked", dA=None, rows=ROWS), ARG)
    expect(L, "list, K = 65", conv(L, "dgg_ell_conv_bwd_partp_ext", K=65), ARG)


# ---- score backward ----------------------------------------------------------------------------------------------------------------
EDGE_LIST = ("dgg_softk_edge_bwd_partp", "dgg_softk_edge_bwd_partp_phase", "dgg_softk_edge_bwd_partp_tab")
EDGE_CHUNKED = ("dgg_softk_edge_bwd_partp_chunked", "dgg_softk_edge_bwd_partp_chunked_tab")
ROWS_NOMAP = 40000                               # a block too large for the slot -> record map (dgg_partp_has_map)


def edge(L, entry, **over):
    a = dict(xp=P, rows=0, chunks=0, cptr=P, h=16, idx=P, val=P, k=P, rs=P, dA=P, dA_rec=P, da=P, ahat=P, K=64, row0=0, mode=0, normalized=1, ws=P,
             ncols=NCOLS, rowinfo=P, dk=P, dxp=P, out_act=0, phase=0, tab=0)
    a.update(over)
    if entry in EDGE_LIST:
        args = [a["xp"], a["rows"], a["h"], a["idx"], a["val"], a["k"], a["rs"], a["dA"], a["dA_rec"], a["da"], a["ahat"], a["K"], a["row0"], T_DIST, 1,
                a["mode"], a["normalized"], a["ws"], a["ncols"], a["rowinfo"], a["dk"], a["dxp"], a["out_act"]]
    else:
        assert entry in EDGE_CHUNKED and a["K"] == 64
        args = [a["xp"], a["rows"], a["cptr"], a["chunks"], a["h"], a["idx"], a["val"], a["k"], a["rs"], a["dA"], a["dA_rec"], a["da"], a["ahat"],
                a["row0"], T_DIST, 1, a["mode"], a["normalized"], a["ws"], a["ncols"], a["rowinfo"], a["dk"], a["dxp"], a["out_act"]]
    if entry != "dgg_softk_edge_bwd_partp":
        args.append(a["phase"])
    if entry.endswith("_tab"):
        args.append(a["tab"])
    return getattr(L, entry)(*args, None)


@pytest.mark.parametrize("entry", EDGE_LIST + EDGE_CHUNKED)
def test_score_backward(L, entry):
    big = dict(rows=ROWS, chunks=ROWS + 40)      # (a refusal must not depend on the block being empty)
    rows = [
        ("mode-2", dict(mode=2), ARG),
        ("mode -1", dict(mode=-1, **big), ARG),
        ("out_act-with-mode-1", dict(mode=1, out_act=1), ARG),
        ("out_act 2", dict(out_act=2, **big), ARG),
        ("missing k", dict(k=None), ARG),
        ("missing dA_rec", dict(dA_rec=None, **big), ARG),
        ("missing dk", dict(dk=None), ARG),
        ("missing rowinfo_ws", dict(rowinfo=None), ARG),
        ("normalised without rs", dict(rs=None, **big), ARG),
        ("normalised without da", dict(da=None), ARG),
        ("null-dA-unnormalised", dict(normalized=0, dA=None, ahat=None, **big), ARG),
        ("ahat_rows-unnormalised", dict(normalized=0, **big), ARG),
        ("no partition", dict(ws=None, **big), ARG),
        ("no destination nodes", dict(ncols=0), ARG),
        ("h-24", dict(h=24, **big), UNSUPPORTED),
        ("operands before the width", dict(h=24, k=None, **big), ARG),
        ("unnormalised: rs, da and ahat_rows are optional", dict(normalized=0, rs=None, da=None, ahat=None), OK),
        ("mode 1", dict(mode=1), OK),
        ("LeakyReLU mask", dict(out_act=1), OK),
        ("zero-rows-edge", dict(), OK),
        ("zero-rows-edge, h = 128", dict(h=128), OK)]
    if entry != "dgg_softk_edge_bwd_partp":
        rows += [("phase-3", dict(phase=3, **big), ARG), ("phase -1", dict(phase=-1), ARG), ("phase before mode", dict(phase=3, mode=2), ARG),
                 ("phase 1", dict(phase=1), OK), ("phase 2", dict(phase=2), OK)]
    if entry.endswith("_tab"):
        rows += [("table", dict(tab=1), OK)]
    for what, over, want in rows:
        expect(L, "%s: %s" % (entry, what), edge(L, entry, **over), want)


@pytest.mark.parametrize("entry", EDGE_LIST)
def test_score_backward_list_dA_may_be_null_with_a_map(L, entry):
    if L.dgg_partp_has_map(0):                   # (DGG_DA_MAP=0 / 1 forces the map off / on for every block)
        expect(L, "%s: NULL dA, normalised with ahat_rows" % entry, edge(L, entry, dA=None), OK)
    expect(L, "%s: NULL dA without ahat_rows" % entry, edge(L, entry, dA=None, ahat=None, rows=ROWS), ARG)
    if not L.dgg_partp_has_map(ROWS_NOMAP):
        expect(L, "%s: null-dA-without-map" % entry, edge(L, entry, dA=None, rows=ROWS_NOMAP), ARG)
    expect(L, "%s: cptr is no operand of the list entry" % entry, edge(L, entry, cptr=None), OK)
    expect(L, "%s: K = 65" % entry, edge(L, entry, K=65), ARG)


@pytest.mark.parametrize("entry", EDGE_CHUNKED)
def test_score_backward_chunked_requires_cptr_and_dA(L, entry):
    expect(L, "%s: chunked without dA" % entry, edge(L, entry, dA=None), ARG)
    expect(L, "%s: chunked without dA, rows > 0" % entry, edge(L, entry, dA=None, rows=ROWS, chunks=ROWS + 40), ARG)
    expect(L, "%s: chunked without cptr" % entry, edge(L, entry, cptr=None), ARG)
    expect(L, "%s: chunked without cptr, rows > 0" % entry, edge(L, entry, cptr=None, rows=ROWS, chunks=ROWS + 40), ARG)
    expect(L, "%s: no nodes, some chunks" % entry, edge(L, entry, chunks=ROWS), OK)
