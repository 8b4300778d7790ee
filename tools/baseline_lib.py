"""A second build of libdgg_hip.so (for instance the parent commit's) beside the tree's, for the timing tools' --baseline-lib: its four
dgg_allpairs_mlp_topk* entry points are reached through the SAME ops wrappers as the tree's (one marshalling, one set of buffers), so two
builds are compared in one process, window by window, under the same clocks.

    base = Baseline(path);  fn_base = base.calls(fn)      # fn calls ops.allpairs_mlp_topk / ops.allpairs_mlp_topk_wide

compare(...) is the verdict the tools print: the two medians differ by no more than the larger of the two builds' window spreads
(largest minus smallest window) of that run -- the spread is what a difference has to exceed."""
import ctypes
import statistics

import torch

from dgg_amd import _lib

ENTRIES = ("dgg_allpairs_mlp_topk", "dgg_allpairs_mlp_topk_prior", "dgg_allpairs_mlp_topk_wide", "dgg_allpairs_mlp_topk_wide_prior")


class Baseline:
    def __init__(self, path):
        self.tree = _lib.lib()
        self.base = _lib.bind(ctypes.CDLL(path), ENTRIES)

    def __getattr__(self, name):                                # (every other symbol stays the tree's)
        return getattr(self.base if name in ENTRIES else self.tree, name)

    def calls(self, fn):
        def run():
            _lib._lib = self
            try:
                return fn()
            finally:
                _lib._lib = self.tree
        return run


def same_bits(x, y):
    """two results of one entry point (tuples of tensors / None), bit for bit"""
    return all((p is None and q is None) or torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x, y))


def compare(ts_tree, ts_base):
    """window times [ms] of the tree's build and of the baseline build -> dict(ratio, diff_ms, spread_ms, within_spread)"""
    diff = statistics.median(ts_tree) - statistics.median(ts_base)
    spread = max(max(ts_tree) - min(ts_tree), max(ts_base) - min(ts_base))
    return dict(ratio_to_baseline=round(statistics.median(ts_tree) / statistics.median(ts_base), 4), diff_ms=round(diff, 4), spread_ms=round(spread, 4),
                within_spread=abs(diff) <= spread)
