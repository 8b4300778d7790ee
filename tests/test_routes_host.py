"""The route DGG_LearnableK_debug takes for every configuration of tools/record_routes.py's grid equals the table recorded from the commit
before the host-side restructuring of dgm.py (tests/golden/routes_parent.json): the same refusal -- exception type and text -- or the same
terminal with the same decisions and the same tensors handed to it, and the same answer of _fused_outside.  No GPU: the walk stubs every
kernel-touching piece (see the recorder's docstring)."""
import functools
import json
import os
import sys
import zlib

from helpers import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_routes as R  # noqa: E402


@functools.lru_cache(maxsize=None)
def tables():
    with open(os.path.join(GOLDEN, "routes_parent.json")) as f:
        return json.load(f), R.walk()


def rows(table):
    """-> per cell (outcome, args, outside), strings"""
    s, a, c = table["strings"], table["args"], table["cells"]
    return [(s[c[j]], a[c[j + 1]], s[c[j + 2]]) for j in range(0, len(c), 3)]


def test_grid_covers_every_scorer_and_candidate_form_under_every_value_of_every_axis():
    cells = R.grid()
    assert R.coverage_gaps(cells) == []
    assert len(set(cells)) == len(cells)
    need = dict(scorer=6, form=4, knet=5, ksel=3, debug=2, perturb=3, hard=3, latent=3, ell=2, k=2, wide_rows=3, mlp_rows=2, mlp_fused=2,
                prior_fused=2)
    assert all(len(R.AXES[n]) >= v for n, v in need.items())
    assert set(R.AXES["latent"]) == {16, 48, 64} and set(R.AXES["ell"]) == {32, 64} and set(R.AXES["debug"]) == {None, 1}


def test_the_fixture_is_the_table_of_this_grid():
    want, _ = tables()
    cells = R.grid()
    assert want["axes"] == {n: list(v) for n, v in R.AXES.items()}
    assert want["grid"] == zlib.crc32(repr(cells).encode()) and len(want["cells"]) == 3 * len(cells)


def test_every_cell_ends_in_a_refusal_or_a_recorded_terminal():
    _, got = tables()
    got = rows(got)
    assert len(got) == len(R.grid()), "no cell may be skipped"
    for outcome, args, outside in got:
        assert outcome.startswith(("TERMINAL ", "RAISED ")) and (args != "") == outcome.startswith("TERMINAL "), outcome
        for s in (outcome, outside):
            assert "dgg ops run on the GPU only" not in s and "libdgg_hip" not in s, f"a cell reached a kernel call: {s}"
    seen = {o.split(" ")[1] for o, _, _ in got if o.startswith("TERMINAL ")}
    assert seen == set(R.TERMINALS) | {"_csr_soft_adjacency"}, "every terminal is reached by some cell"


def test_routes_equal_the_parent_s_cell_by_cell():
    want, got = tables()
    want, got = rows(want), rows(got)
    assert len(want) == len(got)
    bad = [(dict((n, R.AXES[n][i]) for n, i in zip(R.NAMES, cell)), w, g) for cell, w, g in zip(R.grid(), want, got) if w != g]
    assert not bad, f"{len(bad)} cells differ; the first: {bad[0]}"
