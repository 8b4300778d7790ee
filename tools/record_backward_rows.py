#!/usr/bin/env python3
"""Records tests/golden/backward_rows_parent.npz: the outputs of the row kernel of the score backward (edge_bwd_rows: row part of dxp,
dk, rowinfo) on the seeded graph of tests/test_backward_walk_blocks.py::rows_phase_outputs, from the library that DGG_HIP_SO names
(the build BEFORE a change to that kernel; without it, the in-tree library):

    DGG_HIP_SO=/path/to/libdgg_hip.so python tools/record_backward_rows.py [out.npz]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dgg_amd  # noqa: E402,F401
import test_backward_walk_blocks as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
got = T.rows_phase_outputs(torch.device("cuda:0"))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
np.savez(out, **got)
print("recorded %s from %s: %s" % (out, os.environ.get("DGG_HIP_SO", "the in-tree library"),
                                   ", ".join("%s %s" % (k, v.shape) for k, v in got.items())))
