"""Host-side checks (no GPU) of the train_stats/* surface: include/dgg_hip_next.h declares dgg_adj_diff_stats in a block of its own that
parses and binds while the earlier blocks stay what they were; the float64 restatement the GPU tests measure against reproduces the
scalars the REFERENCE wrote (fixtures adj_stats_{a,b,c}.npz, tests/golden/make_golden_adj_stats.py) within the reference's own recorded
float32 error; ScalarLog round-trips; the harness parses its two new flags."""
import ctypes
import math
import os

import numpy as np
import pytest

import adj_stats_ref as R
from helpers import load_fixture

ENTRY = "dgg_adj_diff_stats"
CASES = ("a", "b", "c")


def test_the_block_parses_and_binds():
    import dgg_amd
    L_ = dgg_amd._lib
    assert set(L_.NEXT_BLOCKS["adj_stats"]) == {ENTRY}
    restype, argtypes = L_.NEXT_BLOCKS["adj_stats"][ENTRY]
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    #                   idx w rows K cptr chunks rowptr col aval k ws out stream
    assert argtypes == [P, P, I64, I, P, I64, P, P, P, P, P, P, P]
    assert restype is ctypes.c_int
    raw = ctypes.CDLL(L_.SO_PATH)
    assert hasattr(raw, ENTRY), f"libdgg_hip.so does not export {ENTRY}"
    fn = getattr(L_.bind(raw, [ENTRY]), ENTRY)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes
    assert list(getattr(L_.lib(), ENTRY).argtypes) == argtypes          # lib() binds every block


def test_the_earlier_blocks_and_the_recorded_abi_do_not_see_it():
    import dgg_amd
    L_ = dgg_amd._lib
    assert set(L_.NEXT_PROTOTYPES) == set(L_.NEXT_RESTYPES) == {"dgg_edgelist_topk_chunked", "dgg_edgelist_topk_p_chunked"}
    assert list(L_.NEXT_BLOCKS) == ["norm_spmm", "project_knet", "adj_stats"]
    assert set(L_.NEXT_BLOCKS["project_knet"]) == {"dgg_project_knet_fwd"}
    assert set(L_.NEXT_BLOCKS["norm_spmm"]) == {"dgg_ell_spmm_norm_act_fwd", "dgg_ell_spmm_norm_act_fwd_chunked", "dgg_softk_edge_bwd_partp_tab",
                                                "dgg_softk_edge_bwd_partp_chunked_tab"}
    assert ENTRY not in L_.PROTOTYPES and ENTRY not in L_.NEXT_PROTOTYPES


def test_the_result_layout_of_the_header_is_the_wrappers():
    import re
    import dgg_amd
    with open(dgg_amd._lib.NEXT_HEADER) as f:
        defs = dict(re.findall(r"^#define DGG_ADJ_STATS_(\w+) (\d+)$", f.read(), flags=re.M))
    assert int(defs.pop("COUNT")) == len(dgg_amd.ops.ADJ_STATS_FIELDS) == 10
    assert tuple(sorted(defs, key=lambda n: int(defs[n]))) == tuple(f.upper() for f in dgg_amd.ops.ADJ_STATS_FIELDS)
    assert dgg_amd.ops.ADJ_STATS_FIELDS == R.FIELDS


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference_scalars(case):
    fx = load_fixture("adj_stats_" + case)
    n = fx["meta"]["N"]
    assert tuple(fx["meta"]["tags"]) == R.TAGS
    A = R.dense_from_triplets(n, fx["rows"], fx["cols"], fx["adj_vals"])
    W = R.dense_from_triplets(n, fx["out_rows"], fx["out_cols"], fx["out_vals"])
    assert int((W != 0).sum(1).max()) <= 64
    mine = R.stats_dense(A, W, fx["k"])
    for i, tag in enumerate(R.TAGS):
        f = R.TAG_FIELD[tag]
        # this file's restatement is the generator's, evaluated again: the same float64 up to summation order
        assert R.close(mine[f], fx["f64"][i], 0.0, 1e-12), (tag, mine[f], fx["f64"][i])
        # ... and the reference's float32 scalar lies within its own recorded error of it
        assert R.close(mine[f], fx["ref"][i], float(fx["dist"][i])), (tag, mine[f], fx["ref"][i], fx["dist"][i])
    if case == "a":
        assert math.isnan(fx["ref"][2]) and math.isnan(fx["ref"][3]) and mine["off_n"] == 0
    else:
        assert mine["on_n"] >= 2 and mine["off_n"] >= 2 and fx["meta"]["complete"]
    if case == "c":
        assert (fx["adj_vals"] == 0).sum() == 3 and (fx["adj_vals"] < 0).sum() == 1 and fx["adj_vals"].max() <= 2.0


def test_restatement_edge_cases():
    A = np.zeros((3, 3), np.float32)
    W = np.zeros((3, 3), np.float32)
    A[0, 1], W[0, 1] = 0.5, 0.5              # a == w exactly: d == 0, kept by neither population
    A[1, 2] = -1.0                           # a stored negative: neither
    W[2, 0] = 0.25                           # one off-edge pair: a mean and no std
    s = R.stats_dense(A, W, [1.0, 2.0, 3.0])
    assert s["on_n"] == 0 and math.isnan(s["on_mean"]) and math.isnan(s["on_std"])
    assert s["off_n"] == 1 and s["off_mean"] == -0.25 and math.isnan(s["off_std"])
    assert s["in_deg_mean"] == pytest.approx(-0.5 / 3) and s["k_mean"] == 2.0
    assert R.close(float("nan"), float("nan")) and not R.close(1.0, float("nan")) and not R.close(float("nan"), 1.0)
    assert R.close(1.0 + 2.0 ** -23, 1.0) and not R.close(1.0 + 2.0 ** -21, 1.0)


def test_scalar_log_round_trips(tmp_path):
    import torch
    import dgg_amd
    log = dgg_amd.ScalarLog(tmp_path / "run")                     # a directory, as SummaryWriter's log_dir
    log.add_scalar("train_stats/on_edge_mean", 0.125, 3)
    log.add_scalar("train_stats/off_edge_std", float("nan"), 3)
    log.add_scalar("values/first_k_mean", torch.tensor(2.5), 4)
    log.add_histogram("gcn_conv1_dist", torch.tensor([[1.0, -2.0], [4.0, 5.0]]), 4)
    log.add_histogram("empty", [], 5)
    log.close()
    log.close()
    path = os.path.join(tmp_path, "run", "scalars.jsonl")
    assert log.path == path
    recs = dgg_amd.ScalarLog.read(path)
    assert recs[0] == {"tag": "train_stats/on_edge_mean", "step": 3, "value": 0.125}
    assert recs[1]["tag"] == "train_stats/off_edge_std" and math.isnan(recs[1]["value"])
    assert recs[2] == {"tag": "values/first_k_mean", "step": 4, "value": 2.5}
    assert recs[3] == {"tag": "gcn_conv1_dist", "step": 4, "min": -2.0, "mean": 2.0, "max": 5.0, "count": 4}
    assert recs[4]["count"] == 0 and math.isnan(recs[4]["mean"])
    with dgg_amd.ScalarLog(tmp_path / "other.jsonl") as lg:       # a file name is taken as it is; appended to
        lg.add_scalar("a", 1, 0)
    with dgg_amd.ScalarLog(tmp_path / "other.jsonl") as lg:
        lg.add_scalar("a", 2, 1)
    assert [r["value"] for r in dgg_amd.ScalarLog.read(tmp_path / "other.jsonl")] == [1.0, 2.0]


def test_the_harness_parses_its_new_flags(tmp_path):
    from dgg_amd import train_small_graphs as T
    a = T.build_parser().parse_args(["--data_dir", "x"])
    assert a.log_dir is None and a.dgg_writer_fused is False
    a = T.build_parser().parse_args(["--data_dir", "x", "--log_dir", str(tmp_path), "--dgg_writer_fused", "true"])
    assert a.log_dir == str(tmp_path) and a.dgg_writer_fused is True
    w = T.make_writer(str(tmp_path / "logs"))
    assert all(callable(getattr(w, n)) for n in ("add_scalar", "add_histogram", "close"))
    w.close()


def test_model_opt_in_and_module_signatures():
    import inspect
    import dgg_amd
    sig = inspect.signature(dgg_amd.DGG_LearnableK_debug.forward_conv)
    assert list(sig.parameters)[1:] == ["x", "in_adj", "conv_weight", "want_norm", "writer", "epoch"]
    assert sig.parameters["writer"].default is None and sig.parameters["epoch"].default is None
    assert list(inspect.signature(dgg_amd.DGG_LearnableK_debug._log_adj_stats).parameters)[1:8] == ["writer", "epoch", "graph_csr", "idx", "w", "layout", "k"]
    from argparse import Namespace
    base = dict(extra_edge_dim=0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288, dgg_mode_edge_net="u-v-dist",
                dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=False, symmetric_noise=False,
                stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
    assert dgg_amd.GCN_DGG(nfeat=8, nhidden=16, nclass=3, args=Namespace(**base)).writer_fused is False
    assert dgg_amd.GCN_DGG(nfeat=8, nhidden=16, nclass=3, args=Namespace(dgg_writer_fused=True, **base)).writer_fused is True
    # the writer adds no clause to the fused layer's coverage
    assert "writer" not in inspect.getsource(dgg_amd.DGG_LearnableK_debug._fused_outside)
