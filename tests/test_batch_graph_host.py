"""Host-side checks (no GPU) of the batch edit: the numpy restatement the GPU tests compare against (tests/batch_graph_ref.py) equals a
dense construction from masks; the noise law hits at its rate (a derived binomial bar, not a measured one) and is not symmetric;
include/dgg_hip_batch_graph.h is C99, parses into a table of its own and collides with no other header; every refusal of the entry is
decided on the host, before any launch (dummy addresses that are never dereferenced, as tests/test_partp_refusals_host.py does); the
harness's parser and the samplers' noise seeds."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import batch_graph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dgg_hip_batch_graph.h")
EDIT = "dgg_batch_graph_edit"
ARG = 1                                          # DGG_ERR_ARG (include/dgg_hip.h)
P = 0x100000                                     # a dummy address
SEED = (42, 65537)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.0014, 0.3, 1.0])
@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_restatement_equals_the_dense_construction(n, p):
    thr = R.threshold(p)
    for name in R.GRAPHS:
        rowptr, col, values = R.graph(name, n)
        for kind in ("three", "equal", None):
            lab = R.labels(kind, n)
            got = R.edit(rowptr, col, values, thr, SEED, lab)
            noisy, pattern, target = R.dense(rowptr, col, values, thr, SEED, lab)
            assert got["e"] == int(pattern.sum()) and got["nrowptr"][-1] == got["e"] == got["ncol"].size
            assert np.array_equal(np.diff(got["nrowptr"]), pattern.sum(1))
            assert np.array_equal(R.to_dense(n, got["nrowptr"], got["ncol"], got["nval"]), noisy)
            assert np.array_equal(got["nrow"], np.repeat(np.arange(n), np.diff(got["nrowptr"])))
            assert all((np.diff(got["ncol"][got["nrowptr"][i]:got["nrowptr"][i + 1]]) > 0).all() for i in range(n))
            st = got["nsrc"] >= 0                                        # a stored entry points at itself, a noisy one at nothing
            assert np.array_equal(got["nsrc"][st], np.arange(col.size)) and np.array_equal(got["ncol"][st], col)
            assert np.array_equal(got["nval"][st], values) and (got["nval"][~st] == 1).all() and (got["nsrc"][~st] == -1).all()
            if lab is None:
                assert "tcol" not in got and got["e_t"] == 0
            else:
                assert np.array_equal(R.to_dense(n, got["trowptr"], got["tcol"], np.ones(got["e_t"], np.float32)), target)
                assert np.array_equal(got["trow"], np.repeat(np.arange(n), np.diff(got["trowptr"])))
                assert all((np.diff(got["tcol"][got["trowptr"][i]:got["trowptr"][i + 1]]) > 0).all() for i in range(n))


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_p_one_is_the_complete_graph_without_new_diagonal_entries(n):
    for name in ("empty", "selfloops", "random"):
        rowptr, col, values = R.graph(name, n)
        got = R.edit(rowptr, col, values, R.threshold(1.0), SEED)
        A = R.to_dense(n, got["nrowptr"], got["ncol"], np.ones(got["e"], np.float32)).astype(bool)
        stored_diag = R.dense_graph(rowptr, col, np.ones(col.size, np.float32)).astype(bool) & np.eye(n, dtype=bool)
        assert np.array_equal(A, ~np.eye(n, dtype=bool) | stored_diag)
    assert R.threshold(1.0) == 1 << 32 and R.threshold(0.0) == 0 and R.threshold(0.5) == 1 << 31 and R.threshold(0.0014) == int(0.0014 * 2 ** 32)


@pytest.mark.parametrize("n", [2, 65, 300])
def test_p_zero_gives_the_graph_back_and_the_target_of_remove_interclass_edges(n):
    import dgg_amd.data as D
    for name in ("random", "selfloops", "sparse_full"):
        rowptr, col, values = R.graph(name, n)
        lab = R.labels("three", n)
        got = R.edit(rowptr, col, values, 0, SEED, lab)
        assert np.array_equal(got["nrowptr"], rowptr) and np.array_equal(got["ncol"], col) and np.array_equal(got["nval"], values)
        assert np.array_equal(got["nsrc"], np.arange(col.size))
        rows = np.repeat(np.arange(n), np.diff(rowptr))
        adj = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, col.astype(np.int64)])), torch.from_numpy(values), (n, n))
        want = D.remove_interclass_edges(adj, torch.from_numpy(lab)).to_dense().numpy()
        assert np.array_equal(R.to_dense(n, got["trowptr"], got["tcol"], np.ones(got["e_t"], np.float32)), want)


# ---- the law's rate ------------------------------------------------------------------------------------------------------------------
RATE_SEEDS = [(0, 0), (42, 1), (42, 65537), (7, 12345), (0xdeadbeef, 99)]


@pytest.mark.parametrize("seed", RATE_SEEDS, ids=["%x-%d" % s for s in RATE_SEEDS])
@pytest.mark.parametrize("p", [0.0014, 0.05, 0.5])
@pytest.mark.parametrize("n", [512, 2048])
def test_the_law_hits_at_its_rate(n, p, seed):
    """the bars are binomial, derived: hits ~ B(n(n-1), q) and symmetric coincidences ~ B(n(n-1)/2, q^2) for independent pairs,
    q = thr / 2^32; 6 sigma either side (3.0 and 2.6 sigma are the worst seen over these 30 cases)"""
    q = R.threshold(p) / 2.0 ** 32
    hits, both, _ = R.noise_counts(n, R.threshold(p), seed)
    pairs = n * (n - 1)
    sd = math.sqrt(pairs * q * (1 - q))
    sd2 = math.sqrt(pairs / 2 * q * q * (1 - q * q))
    print(f"n {n} p {p} seed {seed}: hits {hits} mean {pairs * q:.1f} ({(hits - pairs * q) / sd:+.2f} sigma); both directions {both} "
          f"mean {pairs / 2 * q * q:.2f} ({(both - pairs / 2 * q * q) / sd2:+.2f} sigma)")
    assert abs(hits - pairs * q) <= 6 * sd
    assert abs(both - pairs / 2 * q * q) <= 6 * sd2


def test_two_steps_get_different_noise():
    import dgg_amd
    s = dgg_amd.RandomWalkSampler(small_graph(), batch_size=4, walk_length=1, num_steps=3, seed=42)
    thr = R.threshold(0.0014)
    a, b = (R.noise_counts(512, thr, s.noise_seed(step))[2] for step in (0, 1))
    assert a.sum() > 200 and b.sum() > 200 and int((a & b).sum()) <= 3          # (about 355 each; a shared hit has probability 2e-6 a pair)
    _, _, c = R.noise_counts(512, thr, (42, 1))
    _, _, d = R.noise_counts(512, thr, (42, 2))
    assert int((c & d).sum()) <= 3 and not np.array_equal(c, d)


# ---- the header and its table ----------------------------------------------------------------------------------------------------------
def test_the_header_compiles_as_c99():
    assert shutil.which("gcc") is not None, "the header check needs gcc"
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(HEADER).read()
    assert '#include "dgg_hip.h"' in text and "train_large_graphs.py:230-236" in text and "0x9E3779B9" in text
    assert "np.random.seed(0)" in text and "reference_stream=False" in text and "1.6e8" in text      # the two deviations and the cost


def test_the_header_has_a_table_of_its_own():
    import dgg_amd
    L_ = dgg_amd._lib
    Pv, I, I64, U32, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
    assert set(L_.BATCH_GRAPH_PROTOTYPES) == set(L_.BATCH_GRAPH_RESTYPES) == {EDIT}
    #                                          phase rowptr col values n E     labels s0  s1   thr  ndeg tdeg nrowptr E_n ncol nrow nval nsrc trowptr E_t tcol trow status stream
    assert L_.BATCH_GRAPH_PROTOTYPES[EDIT] == [I, Pv, Pv, Pv, I64, I64, Pv, U32, U32, U64, Pv, Pv, Pv, I64, Pv, Pv, Pv, Pv, Pv, I64, Pv, Pv, Pv, Pv]
    assert L_.BATCH_GRAPH_RESTYPES[EDIT] is ctypes.c_int
    raw = ctypes.CDLL(L_.SO_PATH)
    assert hasattr(raw, EDIT), f"libdgg_hip.so does not export {EDIT}"
    assert list(getattr(L_.lib(), EDIT).argtypes) == L_.BATCH_GRAPH_PROTOTYPES[EDIT]                  # lib() binds it with the rest
    assert (dgg_amd.ops.BATCH_EDIT_COUNT, dgg_amd.ops.BATCH_EDIT_FILL) == (0, 1)
    text = open(HEADER).read()
    for k_, v in (("DGG_BATCH_EDIT_COUNT", 0), ("DGG_BATCH_EDIT_FILL", 1), ("DGG_BATCH_EDIT_BAD_GRAPH", 1)):
        assert f"#define {k_} {v}\n" in text
    assert set(dgg_amd.ops.BATCH_EDIT_STATUS) == {1}


def test_no_name_collides_with_the_other_headers():
    import dgg_amd
    L_ = dgg_amd._lib
    others = (set(L_.PROTOTYPES) | set(L_._INFO) | set(L_.NEXT_PROTOTYPES) | {n for b in L_.NEXT_BLOCKS.values() for n in b} | set(L_.ADJ_LOSS_PROTOTYPES) |
              set(L_.SAMPLING_PROTOTYPES))
    assert not others & set(L_.BATCH_GRAPH_PROTOTYPES)
    assert set(L_.SAMPLING_PROTOTYPES) == {"dgg_random_walk_nodes", "dgg_induced_subgraph"} and set(L_.ADJ_LOSS_PROTOTYPES) == {"dgg_adj_mse_loss"}
    assert L_.lib().dgg_abi_version() == 6
    src = open(os.path.join(os.path.dirname(L_.__file__), "_lib.py")).read()
    assert "set(_BATCH_GRAPH_DECLS) & (set(_DECLS) | set(_NEXT_DECLS) | set(_LATER_DECLS) | set(_ADJ_LOSS_DECLS) | set(_SAMPLING_DECLS))" in src


# ---- refusals of the entry, decided before any launch ----------------------------------------------------------------------------------
def call_edit(L, **over):
    a = dict(phase=0, rowptr=P, col=P, values=P, n=300, E=2000, labels=P, s0=1, s1=2, thr=1 << 20, ndeg_i=P, tdeg_i=P, nrowptr=P, E_n=2100, ncol=P,
             nrow=P, nval=P, nsrc=P, trowptr=P, E_t=900, tcol=P, trow=P, status=P)
    a.update(over)
    assert over, "a call without a reason to be refused would launch"
    return L.dgg_batch_graph_edit(a["phase"], a["rowptr"], a["col"], a["values"], a["n"], a["E"], a["labels"], a["s0"], a["s1"], a["thr"], a["ndeg_i"],
                                  a["tdeg_i"], a["nrowptr"], a["E_n"], a["ncol"], a["nrow"], a["nval"], a["nsrc"], a["trowptr"], a["E_t"], a["tcol"],
                                  a["trow"], a["status"], None)


NO_TARGET = dict(trowptr=None, tcol=None, trow=None)
REFUSALS = [
    ("phase -1", dict(phase=-1)), ("phase 2", dict(phase=2)), ("n < 0", dict(n=-1)), ("n = 2^31", dict(n=1 << 31)), ("E < 0", dict(E=-1)),
    ("E_n < 0", dict(E_n=-1)), ("E_t < 0", dict(E_t=-1)), ("thr = 2^32 + 1", dict(thr=(1 << 32) + 1)), ("NULL status", dict(status=None)),
    ("FILL: NULL status", dict(phase=1, status=None)),
    ("COUNT: NULL rowptr", dict(rowptr=None)), ("COUNT: NULL col", dict(col=None)), ("COUNT: NULL ndeg_i", dict(ndeg_i=None)),
    ("COUNT: labels without tdeg_i", dict(tdeg_i=None)), ("COUNT: tdeg_i without labels", dict(labels=None)),
    ("FILL: NULL rowptr", dict(phase=1, rowptr=None)), ("FILL: NULL col", dict(phase=1, col=None)), ("FILL: NULL values", dict(phase=1, values=None)),
    ("FILL: NULL nrowptr", dict(phase=1, nrowptr=None)), ("FILL: NULL ncol", dict(phase=1, ncol=None)), ("FILL: NULL nrow", dict(phase=1, nrow=None)),
    ("FILL: NULL nval", dict(phase=1, nval=None)), ("FILL: NULL nsrc", dict(phase=1, nsrc=None)),
    ("FILL: labels without trowptr", dict(phase=1, trowptr=None)), ("FILL: NULL tcol", dict(phase=1, tcol=None)), ("FILL: NULL trow", dict(phase=1, trow=None)),
    ("FILL: trowptr without labels", dict(phase=1, labels=None, tcol=None, trow=None)), ("FILL: tcol without labels", dict(phase=1, labels=None, trowptr=None, trow=None)),
    ("FILL: trow without labels", dict(phase=1, labels=None, trowptr=None, tcol=None)),
    ("FILL without labels: NULL ncol", dict(phase=1, labels=None, ncol=None, **NO_TARGET)),
]


@pytest.mark.parametrize("what,over", REFUSALS, ids=[w for w, _ in REFUSALS])
def test_refusals_are_decided_on_the_host(what, over):
    import dgg_amd
    L = dgg_amd._lib.lib()
    rc = call_edit(L, **over)
    text = L.dgg_last_error().decode()
    assert rc == ARG and text.startswith(EDIT + ":"), f"{what}: status {rc} ({text!r})"


def test_the_empty_problem_launches_nothing():
    """the return that comes before any launch: with NULL everywhere else it would fault if anything were read"""
    import dgg_amd
    L = dgg_amd._lib.lib()
    none = dict(rowptr=None, col=None, values=None, labels=None, ndeg_i=None, tdeg_i=None, nrowptr=None, ncol=None, nrow=None, nval=None, nsrc=None,
                trowptr=None, tcol=None, trow=None)
    for ph in (0, 1):
        assert call_edit(L, phase=ph, n=0, E=0, E_n=0, E_t=0, **none) == 0
        assert call_edit(L, phase=ph, n=0, E=0, E_n=0, E_t=0, thr=1 << 32, **none) == 0      # (thr = 2^32 is a legal threshold)
        assert call_edit(L, phase=ph, n=0, E=0, E_n=0, E_t=0, status=None, **none) == ARG    # ... but status is never optional


# ---- ops, the samplers, the harness ----------------------------------------------------------------------------------------------------
def small_graph(n=12):
    i = torch.arange(n)
    return torch.sparse_coo_tensor(torch.stack([i, (i + 1) % n]), torch.ones(n), (n, n)).coalesce()


def test_the_threshold_of_ops_is_the_restatements():
    from dgg_amd import ops
    for p in (0.0, 0.0014, 1e-9, 0.3, 0.5, 1.0 - 2.0 ** -40, 1.0):
        assert ops.noise_threshold(p) == R.threshold(p) <= 1 << 32
    for p in (-1e-9, 1.0000001, float("nan")):
        with pytest.raises(ValueError, match="p must be"):
            ops.noise_threshold(p)


def test_noise_seed_is_a_fixed_function_of_seed_epoch_and_step():
    import dgg_amd
    g = small_graph()
    for make in (lambda seed: dgg_amd.RandomWalkSampler(g, 5, 2, 3, seed=seed),
                 lambda seed: dgg_amd.ClusterSampler(g, dgg_amd.contiguous_parts(12, 4), batch_size=1, seed=seed)):
        s, again, other = make(4), make(4), make(5)
        seeds = [s.noise_seed(i) for i in range(4)]
        assert seeds == [again.noise_seed(i) for i in range(4)] and len(set(seeds)) == 4
        assert all(0 <= v < 1 << 32 for sd in seeds for v in sd)
        assert other.noise_seed(0) != seeds[0]
        s.set_epoch(1)
        assert not set(s.noise_seed(i) for i in range(4)) & set(seeds)
        again.set_epoch(1)
        assert s.noise_seed(2) == again.noise_seed(2)
    r = dgg_amd.RandomWalkSampler(g, 5, 2, 3, seed=4)
    for epoch in (0, 1, 7):
        r.set_epoch(epoch)
        assert all(r.noise_seed(i) != r.walk_seed(i) for i in range(5))                    # another stream than the walks'
        assert not set(r.noise_seed(i) for i in range(50)) & set(r.walk_seed(i) for i in range(50))


def test_the_harness_parser_knows_batch_noise():
    from dgg_amd import train_large_graphs as H
    a = H.build_parser().parse_args(["--data_dir", "x"])
    assert a.batch_noise == "host" and a.edge_noise_level == 0.00014
    assert H.build_parser().parse_args(["--data_dir", "x", "--batch_noise", "device"]).batch_noise == "device"
    with pytest.raises(SystemExit):
        H.build_parser().parse_args(["--data_dir", "x", "--batch_noise", "numpy"])
    assert "--batch_noise device" in H.__doc__ and "re-seeds numpy to 0" in H.__doc__ and "reference_stream=False" in H.__doc__
