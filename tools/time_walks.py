#!/usr/bin/env python3
"""Times the three backward walks of the payload partition (csrc/dgg_scatter.hip) on the adjacency of one real step of the synthetic
workload (diagnostic): python tools/time_walks.py [N].

Prints the histogram of records per destination node (what conv_bwd_node / edge_bwd_node walk) and of live entries per row (what
edge_bwd_rows walks), then event-times, 20 launches each after 3 warm-ups,
  conv   the conv backward call (conv_bwd_node: dA, dA_rec, dH, da)
  rows   phase 1 of the score backward (edge_bwd_rows: row side of dxp, dk, rowinfo)
  nodes  phase 2 of the score backward (edge_bwd_node: destination side of dxp)
DGG_HIP_SO=<path> times another build of the library with the same script."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from dgg_amd import ops  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
WARM, R = 3, 20
dev = torch.device("cuda", 0)
a = argparse.Namespace(algo=0)
run = bench.SyntheticRun(a, dev, 1, 0, False, N, 128, 64, ops.NOISE_RANKED)
run.step(0)
torch.cuda.synchronize()
layer = run.layer
kern, s = layer.kern, layer.saved
assert s["partp"] is not None and s["layout"] is None, "the step did not run on the payload partition of a plain [N,64] list"


def hist(name, v):
    v = v.to(torch.float32)
    q = torch.quantile(v, torch.tensor([0.25, 0.5, 0.75], device=v.device)).tolist()
    above = "  ".join(f">{b}: {float((v > b).float().mean()) * 100:.2f}%" for b in (32, 48, 64))
    print(f"{name}: min {int(v.min())}  q1 {q[0]:.0f}  median {q[1]:.0f}  q3 {q[2]:.0f}  max {int(v.max())}  mean {float(v.mean()):.2f}   {above}")


nodeptr, recs = ops.partp_records(s["partp"])
hist("records per destination node", nodeptr[1:] - nodeptr[:-1])
hist("live entries per row        ", ((s["idx"] >= 0) & (s["w"] != 0)).sum(1))
live = (s["idx"] >= 0) & (s["w"] != 0)
top = torch.where(live.any(1), 63 - live.flip(1).to(torch.int8).argmax(1), torch.full((live.shape[0],), -1, device=live.device))
hist("highest live rank per row   ", top)

G = torch.randn_like(s["Z"])
pre = layer._premask()


def conv():
    return layer._conv_backward(G, None)


dA, dA_rec, dH, da, ahat_rows = conv()
args = (s["xp"], s["idx"], s["val"], s["k"], dA, dA_rec, s["rs"], da, layer.r0, layer.t, layer.noise_mode != 0, layer.mode, True, s["partp"])
kw = dict(ahat_rows=ahat_rows, out_act=1 if pre else 0)
state = {}


def rows():
    state["st"] = kern.softk_edge_bwd_p(*args, **kw, phase=1)[2]


def nodes():
    kern.softk_edge_bwd_p(*args, **kw, phase=2, state=state["st"])


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(R)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return us[0], us[len(us) // 2], us[-1]


print(f"N={N} records={int(nodeptr[-1])} lib={os.environ.get('DGG_HIP_SO', 'in-tree')}  (us per call: min / median / max of {R})")
for name, fn in (("conv ", conv), ("rows ", rows), ("nodes", nodes)):
    lo, med, hi = timed(fn)
    print(f"WALK {name} {lo:8.1f} {med:8.1f} {hi:8.1f}")
