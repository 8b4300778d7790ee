#!/usr/bin/env python3
"""bench.py -- DGG adjacency build + normalise + graph-conv aggregation, forward AND backward, on synthetic
N-node x d-feature graphs (BASELINE.json metric).

    python bench.py [--gpus N --steps K --warmup W] [--nodes N --feat 128 --latent 64]

One step = one pass of the hot path over the whole graph: node projections (one fp32 MFMA GEMM: [xp | xk | x Wc]) ->
learned degree k -> all-pairs Gumbel-perturbed scores + per-row top-64 -> smooth first-k ramp -> D^-1/2 A D^-1/2 ->
relu(A (x Wc)), then the full backward with a ones cotangent (all DGG parameters + conv weight; the input features are
data, as in the reference's training loop, unless --x-grad).  Inputs are resident in HBM before the timed region; every
step draws fresh noise (seed cycled over NGRAPH values).
W warm-up steps, then ONE window of exactly K timed steps (or `--repeats` windows of K steps), bracketed by barrier + synchronize
(max over ranks); `value` / `ms_per_step` come from the (median) window.
One GPU: N = 100 000 (the BASELINE.json metric config).  Several GPUs (torchrun, one rank per GPU, RCCL): BASELINE.json
configs[3], ONE graph of 500 000 nodes node-range sharded (strong scaling); --weak: 100 000 rows per GPU.

Prints ONE JSON line (rank 0), at most LINE_LIMIT bytes: the driver's fields, `config` and `repeats`.  --dump-outputs DIR writes what the
last timed step returned (the layer output Z and every parameter gradient) as DIR/<name>.npy.
--full adds everything beyond the headline figure: an eager window, as many windows as fill MIN_TIMED_S (unless --repeats), `roofline`
(dominant kernel), `cpu_baseline`, a compact `configs` map ({ms_per_step, value, frac} per secondary BASELINE config); the full result --
`kernels`, `variants` (symmetric / unperturbed / hash noise, latent 128, x-grad), `data_regimes`, per-config detail -- goes to the detail
file (DETAIL_PATH) and to stderr.
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

FLOP_PER_PAIR = 232.0        # 3h (sub, mul, add) + ~40 (sqrt, exp, 3 log, exp, RNG, compare), h = 64
FP32_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: peak fp32 vector = fp32 matrix
HBM_PEAK_GBPS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec); ~6.3 TB/s achievable
GATHER_CEILING_GBPS = 8600.0 # MI355X_MICROARCH.md "Indexed rows": uniformly random rows of a 38 MB (Infinity-Cache resident) table
BF16_PEAK_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 MFMA peak (32 cycles per v_mfma_f32_32x32x16_bf16 per SIMD at 2.4 GHz)
HASH_CYCLES_PER_WAVE_COLUMN = 21.0   # measured floor of the 6-VALU pair hash, cycles per wavefront and 64 pairs
SIMD_CYCLES_PER_S = 1024 * 2.4e9     # 256 CUs x 4 SIMDs at the 2.4 GHz peak clock
# BASELINE.json's metric string (value = the edges/sec part; the HBM GB/s part is the `roofline` object)
METRIC = "DGG adj-build+SpMM fwd/bwd edges/sec & achieved HBM GB/s, N=100k d=128 k=32"


def load_traffic(N, d, h):
    """Fabric bytes per launch (L2 -> fabric requests: Infinity-Cache hits included, MI355X_MICROARCH.md 'HBM') from the
    rocprofv3 PMC passes (FETCH_SIZE doubled as the gfx950 guide prescribes + WRITE_SIZE), committed under profiles/ by
    tools/pmc_traffic.py together with the shape they were measured on; {} when there is no file FOR THIS SHAPE."""
    try:
        names = sorted(n for n in os.listdir(os.path.join(ROOT, "profiles")) if n.endswith("_traffic.json"))     # newest round last
        with open(os.path.join(ROOT, "profiles", names[-1])) as f:
            t = json.load(f)
        if t.get("shape") != {"nodes": N, "feat": d, "latent": h}:
            return {}
        out = {k: v["fabric_bytes_per_launch"] for k, v in t["kernels"].items()}
        out["_source"] = "replayed:profiles/" + names[-1]        # (PMC passes cannot run inside a timed bench: the numbers are REPLAYED)
        return out
    except Exception:  # noqa: BLE001
        return {}


def make_params(d, h, dev, seed=0):
    """Default-initialised reference modules under a fixed seed (on the CPU generator), k_project.weight *= 0.1 so
    that k stays in ~[24,41]."""
    import dgg_amd
    from argparse import Namespace
    args = Namespace(extra_edge_dim=0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288,
                     dgg_mode_edge_net="u-v-dist", dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob",
                     debug_step=3, perturb_edge_prob=True, symmetric_noise=False, stochastic_k=False,
                     dgg_adj_input="input_adj", n_dgg_layers=1)
    torch.manual_seed(seed)
    m = dgg_amd.DGG_LearnableK_debug(in_dim=d, latent_dim=h, args=args)
    conv = dgg_amd.GCNConv(d, 64)
    with torch.no_grad():
        m.k_net.k_project.weight.mul_(0.1)
    P = dict(We=m.node_encode_for_edges[0].weight, be=m.node_encode_for_edges[0].bias, Wk=m.node_encode_for_k[0].weight,
             bk=m.node_encode_for_k[0].bias, W1=m.k_embed[0].weight, b1=m.k_embed[0].bias, Wmu=m.k_net.k_mu.weight,
             bmu=m.k_net.k_mu.bias, Wp=m.k_net.k_project.weight, bp=m.k_net.k_project.bias, Wc=conv.W)
    return {k: v.detach().to(dev).contiguous() for k, v in P.items()}


def cpu_baseline(N, d, h, P, rows, threads, noise_mode=4):
    """The CPU oracle (oracle/dgg_oracle.c, a port of the reference's arithmetic) timed on a bounded row sample of
    the same N-node problem: `rows` output rows against all N candidate columns, forward + backward."""
    from oracle import oracle as O
    os.environ.setdefault("OMP_NUM_THREADS", str(threads))
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, d)).astype(np.float32)
    deg = (24 + 16 * rng.random(N)).astype(np.float32)
    Pn = {k: v.cpu().numpy() for k, v in P.items()}
    R = rows
    t0 = time.perf_counter()
    xp = O.linear(x, Pn["We"], Pn["be"], O.ACT_LEAKY)            # all N nodes are candidates
    t_proj = time.perf_counter() - t0
    t0 = time.perf_counter()
    xs = x[:R]
    xk = O.linear(xs, Pn["Wk"], Pn["bk"], O.ACT_LEAKY)
    mu, sd = O.degree_stats(deg)
    k, z, m, u = O.knet_x(xk, deg[:R], mu, sd, Pn["W1"], Pn["b1"], Pn["Wmu"], Pn["bmu"], Pn["Wp"].reshape(-1), Pn["bp"], save=True)
    idx, val = O.allpairs_topk(xp, K=64, noise_mode=noise_mode, seed=(1234, 0), rows=(0, R))
    w, rs_s = O.softk(idx, val, k)
    rs = np.full((N,), rs_s.mean(), np.float32)               # row sums of unsampled columns: timing-neutral filler
    rs[:R] = rs_s
    ahat = O.normalize(idx, w, rs)
    Y = O.spmm(idx, ahat, x)
    Z = O.linear(Y, Pn["Wc"], None, O.ACT_RELU, w_layout=1)
    dZ = np.ones_like(Z)
    dY, dWc, _ = O.linear_bwd(Y, Pn["Wc"], Z, dZ, act=O.ACT_RELU, w_layout=1)
    dA, _ = O.spmm_bwd(idx, ahat, x, dY, need_dx=False)
    # the oracle's normalisation backward works on square problems; run it on the sample's own index space
    dval, dk = O.softk_bwd(idx, val, k, dA)
    dxp = O.edge_bwd(xp, idx, val, dval, perturb=True) if R == N else _edge_bwd_rows(O, xp, idx, val, dval, R)
    O.linear_bwd(xs, Pn["We"], xp[:R], dxp[:R], act=O.ACT_LEAKY, need_dx=False)
    O.knet_x_bwd(xk, deg[:R], mu, sd, Pn["W1"], Pn["Wmu"], Pn["Wp"].reshape(-1), z, m, u, dk)
    O.linear_bwd(xs, Pn["Wk"], xk, np.zeros_like(xk), act=O.ACT_LEAKY, need_dx=False)
    t_rows = time.perf_counter() - t0
    t_total = t_proj * (R / N) + t_rows
    return dict(value=float(R * k.mean() / t_total), unit="edges/s", cores=threads, kind="port",
                sample=f"oracle fwd+bwd on {R} of {N} output rows vs all {N} candidate columns "
                       f"({t_rows:.1f}s; + projection of all nodes {t_proj:.2f}s scaled by {R}/{N})")


def _edge_bwd_rows(O, xp, idx, val, dval, R):
    """score backward for the first R rows only (oracle edge_bwd walks the rows of idx; xp is global)."""
    import ctypes as C
    N, h = xp.shape
    dxp = np.empty_like(xp)
    # ora_edge_bwd(xp, N, h, idx, val, dval, K, t, perturb, dxp): its row loop runs over N rows of idx, so call it
    # with a zero-padded ELL of N rows would cost memory; instead run it on an [R]-row view by passing N=R for the
    # loop while columns still index the global xp (rows 0..R-1 of xp are the sampled nodes themselves).
    buf = np.zeros((N, h), np.float32)
    O.lib().ora_edge_bwd_rows(O._p(xp), C.c_int64(N), C.c_int64(R), C.c_int(h), O._p(idx), O._p(val), O._p(dval),
                              C.c_int(idx.shape[1]), C.c_float(-0.05), C.c_int(1), O._p(buf))
    return buf


def pubmed_graph(N, n_und, seed=0):
    """Synthetic symmetric graph with a power-law-ish degree profile + self loops (Pubmed shape)."""
    rng = np.random.default_rng(seed)
    wgt = (1.0 / np.arange(1, N + 1) ** 0.5)
    wgt /= wgt.sum()
    u = rng.choice(N, size=2 * n_und, p=wgt)
    v = rng.integers(0, N, size=2 * n_und)
    keep = u != v
    e = np.unique(np.stack([np.minimum(u, v)[keep], np.maximum(u, v)[keep]], 1), axis=0)[:n_und]
    rows = np.concatenate([e[:, 0], e[:, 1], np.arange(N)])
    cols = np.concatenate([e[:, 1], e[:, 0], np.arange(N)])
    return rows, cols


def probe_steps(step_fn, nsteps=5):
    """per-kernel time INSIDE running steps (ops.PROBE events around the C-ABI calls): {name: (ms per step, calls per step)}"""
    from dgg_amd import ops
    step_fn()
    ops.PROBE = {}
    for _ in range(nsteps):
        step_fn()
    torch.cuda.synchronize()
    probe, ops.PROBE = ops.PROBE, None
    return {n: (sum(e0.elapsed_time(e1) for e0, e1 in ev) / nsteps, len(ev) / nsteps) for n, ev in probe.items()}


def bench_edgelist(a, dev):
    emit_json(run_edgelist(a, dev))


def run_edgelist(a, dev):
    """BASELINE.json configs[1] (Pubmed shape: N=19 717, d=500, edge-list candidates, k~16): the drop-in MODULES
    (DGG_LearnableK_debug -> normalize -> GCNConv) under autograd, forward + backward, one GPU; the oracle pipeline on
    all host cores beside it.  Not the headline metric (that is the default workload): run with --workload pubmed."""
    import dgg_amd
    from argparse import Namespace
    shape = getattr(a, "graph", "pubmed")
    N, d, nund, ncls = {"pubmed": (19_717, 500, 44_324, 3), "cora": (2_708, 1_433, 5_278, 7)}[shape]   # nodes, features, undirected edges, classes
    h = a.latent
    rows, cols = pubmed_graph(N, nund)
    E = rows.shape[0]
    extra = {"u-v-dist": 0, "u-v-deg": 2, "u-v-A_uv": 1, "u-v-deg-dist": 3, "edge_conv": 0, "A_uv": 0}[a.edge_mode]
    args = Namespace(extra_edge_dim=extra, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288,
                     dgg_mode_edge_net=a.edge_mode, dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob",
                     debug_step=3, perturb_edge_prob=True, symmetric_noise=False, stochastic_k=False,
                     dgg_adj_input="input_adj", n_dgg_layers=1)
    torch.manual_seed(0)
    dgg = dgg_amd.DGG_LearnableK_debug(in_dim=d, latent_dim=h, args=args)
    conv = dgg_amd.GCNConv(d, 64)
    with torch.no_grad():
        dgg.k_net.k_project.weight.mul_(0.1)
    dgg, conv = dgg.to(dev), conv.to(dev)
    dgg.set_seed(1234, 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(N, d, generator=g).to(dev)
    vals = torch.full((E,), 16.0 * N / E)                         # row sums (the prior degree fed to the k-net) average 16
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols])), vals, (N, N)).coalesce().to(dev)
    params = [p_ for p_ in list(dgg.parameters()) + list(conv.parameters())]

    from dgg_amd import ops as _ops

    fused = getattr(a, "edgelist_api", "fused") == "fused" and a.edge_mode in ("u-v-dist", "u-v-deg", "u-v-A_uv", "u-v-deg-dist", "edge_conv", "A_uv")

    cot = torch.ones((N, 64), device=dev)                         # the cotangent is an INPUT of the backward: resident, as in the headline step

    def step():
        for p_ in params:
            p_.grad = None
        if fused:                                                 # generator + normalisation + GCNConv as one autograd node
            got = dgg.forward_conv(x, A, conv.W)
            assert got is not None, "this configuration is outside the fused layer: use --edgelist-api modules"
            out, adj = got
            out.backward(cot)
            return adj
        with _ops.step_zero_pool(dev, N, 64, 64, params):        # the step's zeroed accumulators from one filled buffer
            adj = dgg(x, A)
            out = conv(x, adj.normalize())
            out.backward(cot)
        return adj

    # a few dozen launches of a few microseconds each: launch latency dominates at this size, so the whole autograd step (forward,
    # backward, fresh gradient tensors) is captured once into a hipGraph and replayed -- same kernels, same work.  The
    # warm-up runs on a side stream, as torch's whole-network capture recipe requires (AccumulateGrad nodes remember the
    # stream they were created on).
    def timed(step_fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(a.warmup, 3)):
                res = step_fn()
        torch.cuda.current_stream().wait_stream(side)
        gr = None
        if a.hipgraph:
            try:
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=side):               # (capture ON the warm-up's stream: the AccumulateGrad nodes' stream)
                    res = step_fn()
                gr.replay()
                torch.cuda.synchronize()
            except Exception as e:  # noqa: BLE001
                print(f"hipGraph capture failed ({e!r}); timing eager launches", file=sys.stderr)
                gr = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            if gr is not None:
                gr.replay()
            else:
                res = step_fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps, gr, res

    T, graph, adj = timed(step)
    # the same step with a scalar loss in front of the backward (out.sum().backward(): + a reduction, a fill and an expanding copy), as
    # the rounds before round 5's second half timed it -- reported beside the figure above, not instead of it
    def step_sum_loss():
        for p_ in params:
            p_.grad = None
        if fused:
            out, adj_ = dgg.forward_conv(x, A, conv.W)
            out.sum().backward()
            return adj_
        with _ops.step_zero_pool(dev, N, 64, 64, params):
            adj_ = dgg(x, A)
            conv(x, adj_.normalize()).sum().backward()
        return adj_

    T_sum = timed(step_sum_loss)[0]
    kmean = float(adj.k.mean().item())
    nsel = float((adj.values() != 0).sum().item())
    # the whole two-layer model of this config (GCN_DGG, reference model.py:1183-1311: generator + conv1 fused as above, dropout,
    # conv2 on the same adjacency, log-softmax, NLL loss on 60 training nodes), forward + backward, beside the layer step
    model_ms = None
    if fused:
        try:
            torch.manual_seed(0)
            net = dgg_amd.GCN_DGG(nfeat=d, nhidden=h, nclass=ncls, args=args).to(dev).train()
            with torch.no_grad():
                net.dggs[0].k_net.k_project.weight.mul_(0.1)
            net.dggs[0].set_seed(1234, 0)
            keep = rows != cols                                    # (the wrapper adds the self loops itself)
            A2 = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows[keep], cols[keep]])), torch.full((int(keep.sum()),), 16.0 * N / E),
                                         (N, N)).coalesce().to(dev)
            ytr = torch.randint(0, ncls, (60,), generator=g).to(dev)
            itr = torch.randperm(N, generator=g)[:60].to(dev)
            nparams = list(net.parameters())

            def model_step():
                for p_ in nparams:
                    p_.grad = None
                logp, _, _ = net(x, A2)
                torch.nn.functional.nll_loss(logp[itr], ytr).backward()

            model_ms = timed(model_step)[0] * 1e3
        except Exception as e:  # noqa: BLE001
            print(f"GCN_DGG model timing failed: {e!r}", file=sys.stderr)
    out = {"metric": f"DGG adj-build+SpMM fwd/bwd edges/sec (edge-list candidates, {shape.capitalize()} shape)", "value": nsel / T, "unit": "edges/s", "n_gpus": 1,
           "steps": a.steps, "warmup": a.warmup, "ms_per_step": T * 1e3, "ms_per_step_with_sum_loss": T_sum * 1e3, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"{shape.capitalize()}-shape edge-list DGG N={N} d={d} h={h} E={E} (incl. self loops) k~{kmean:.1f}, "
                                  f"{a.edge_mode}/x/k_times_edge_prob, Gumbel(0,0.3) hash noise, module API under autograd "
                                  + ("(DGG_LearnableK_debug.forward_conv: generator + normalize + GCNConv as one autograd node)" if fused
                                     else "(DGG_LearnableK_debug + normalize + GCNConv)") + ", fwd+bwd (out.backward(cotangent), the cotangent resident as in the headline step)",
                      "api": "fused layer" if fused else "separate modules", "gcn_dgg_model_ms_per_step": model_ms,
                      "nodes": N, "feat": d, "latent": h, "candidate_edges": E, "selected_edges": nsel,
                      "candidate_edges_per_s": E / T, "edge_mode": a.edge_mode, "hipgraph": graph is not None},
           "roofline": None}
    # dominant kernel of the step from event probes in eager steps; its compulsory bytes (every operand once)
    pk = probe_steps(step)
    dom = max(pk, key=lambda n: pk[n][0])
    nsel_i = int(nsel)
    comp = {"linear_fwd": 4.0 * (N * d + N * h + d * h) * pk.get("linear_fwd", (0, 0))[1],
            "linear_bwd": 4.0 * (N * d + N * h + d * h) * pk.get("linear_bwd", (0, 0))[1],
            "spmm_fwd": nsel_i * 8 + 2 * N * 4.0 * 64, "conv_bwd": nsel_i * 16 + 3 * N * 4.0 * 64, "edge_bwd": nsel_i * 36 + 4 * N * 4.0 * h}
    ms = pk[dom][0]
    cb = comp.get(dom)
    if fused:
        # the STEP against the HBM roofline: every operand of every stage touched once (projection and weight gradients read x once
        # each; 64-wide ELL arrays idx / score / w / ahat / dA; one h- or F-wide gathered row per selected edge in the search, the
        # aggregation and the three backward kernels; 16-byte partition records written once and read twice)
        F = 64
        step_bytes = (4.0 * (N * d + 3 * 64 * d + N * (2 * h + F)) * 2            # projection + weight gradients
                      + 4.0 * N * h * 3 + 16.0 * N                                 # k-net forward + backward (xk twice, dxk)
                      + 8.0 * N + 4.0 * E + 4.0 * E * h + 4.0 * N * h + 12.0 * N * 64 + 4.0 * N     # search + ramp
                      + 12.0 * N * 64 + 4.0 * N * 64 + 16.0 * nsel_i                            # partition + normalisation
                      + 8.0 * N * 64 + 4.0 * nsel_i * F + 4.0 * N * F                           # aggregation
                      + 12.0 * N * F                                                          # ReLU backward
                      + 16.0 * nsel_i + 4.0 * nsel_i * F + 8.0 * N * F + 8.0 * nsel_i           # aggregation backward (per destination)
                      + 16.0 * N * 64 + 4.0 * N * h + 8.0 * N                                  # score backward, row side
                      + 16.0 * nsel_i + 4.0 * nsel_i * h + 4.0 * N * h)                         # score backward, per destination
        out["roofline"] = {"bound": "hbm", "kernel": "whole step (about 25 launches)", "calls_per_step": 1.0, "kernel_ms": T * 1e3,
                           "achieved": step_bytes / T / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": step_bytes / T / 1e9 / HBM_PEAK_GBPS,
                           "traffic": None, "algorithmic_bytes": step_bytes,
                           "note": "bytes = every operand of every stage of the step touched once; at this size the step is bound by launch "
                                   "and dependency latency (25 kernels of 5-70 us, the two MFMA products over the 500-wide input are 40 %), "
                                   f"not by bandwidth; slowest probed call: {dom} {ms * 1e3:.0f} us"}
    else:
        out["roofline"] = {"bound": "hbm", "kernel": dom, "calls_per_step": pk[dom][1], "kernel_ms": ms,
                           "achieved": (cb / (ms * 1e-3) / 1e9) if cb else None, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                           "frac": (cb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS) if cb else None, "traffic": None, "algorithmic_bytes": cb,
                           "note": "event-timed inside eager steps; bytes = every operand of the named kernel's calls touched once; the step is "
                                   "~80 launches of a few microseconds at this size (latency-, not bandwidth-bound)"}
    out["kernels_ms_per_step"] = {n: v[0] for n, v in pk.items()}
    if a.cpu_rows >= 0 and a.edge_mode == "u-v-dist":
        out["cpu_baseline"] = cpu_baseline_edgelist(N, d, h, rows, cols, x.cpu().numpy(), vals.numpy(), dgg, conv,
                                                    os.cpu_count() or 1)
        if a.cpu_dense:
            # the dense reference-shaped formulation at the Pubmed size (about 26 GB of host memory)
            out["cpu_baseline"]["dense_formulation"] = cpu_dense_formulation([("edgelist", N, d, h)], min(os.cpu_count() or 1, 32))
    return out


def allpairs_module_api(a, dev, N, steps, warmup, windows=5):
    """BASELINE configs[2] through the nn.Module API north_star names: GCN_DGG's first layer = DGG_LearnableK_debug.forward_conv
    (generator + normalize_adj + GCNConv as ONE autograd node, _FusedDGGConvFn) on AllPairs candidates, under torch autograd, eager
    launches: loss.backward() through the node, gradients into the nn.Parameters.  -> ms per step (median window), k mean."""
    import dgg_amd
    from argparse import Namespace
    d, h = a.feat, a.latent
    args = Namespace(extra_edge_dim=0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288, dgg_mode_edge_net="u-v-dist",
                     dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=True,
                     symmetric_noise=False, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
    torch.manual_seed(0)
    dgg = dgg_amd.DGG_LearnableK_debug(in_dim=d, latent_dim=h, args=args)
    conv = dgg_amd.GCNConv(d, 64)
    with torch.no_grad():
        dgg.k_net.k_project.weight.mul_(0.1)
    dgg, conv = dgg.to(dev), conv.to(dev)
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(1000)).to(dev)
    cand = dgg_amd.AllPairs((24 + 16 * torch.rand(N, generator=torch.Generator().manual_seed(7))).to(dev))
    params = list(dgg.parameters()) + list(conv.parameters())
    # (a second set of modules for the captured measurement below: torch's whole-network capture recipe wants the parameters'
    #  AccumulateGrad nodes created on a side stream, and the eager steps here create them on the default one)
    dgg_c, conv_c = copy.deepcopy(dgg), copy.deepcopy(conv)

    cot = torch.ones((N, 64), device=dev)                         # the cotangent is an INPUT of the backward: resident, as in the headline step

    def step(dgg=dgg, conv=conv, params=params):
        for p_ in params:
            p_.grad = None
        Z, adj = dgg.forward_conv(x, cand, conv.W)
        Z.backward(cot)
        return adj

    for _ in range(warmup):
        adj = step()
    tws = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            adj = step()
        torch.cuda.synchronize()
        tws.append((time.perf_counter() - t0) / steps)
    dgg.check_ell_bound()
    T = float(np.median(tws))
    km = float(adj.k.mean().item())
    # the same autograd step captured ONCE into a hipGraph and replayed: warm-up on a side stream, then capture; the node takes the
    # last eager forward's chunk layout as a fixed capacity (device-side flags say if a replay outgrew it: check_ell_bound)
    params_c = list(dgg_c.parameters()) + list(conv_c.parameters())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(dgg_c, conv_c, params_c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):                      # capture ON the stream the parameters' AccumulateGrad nodes were made on
        step(dgg_c, conv_c, params_c)
    for _ in range(warmup):
        gr.replay()
    cws = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            gr.replay()
        torch.cuda.synchronize()
        cws.append((time.perf_counter() - t0) / steps)
    dgg_c.check_ell_bound()
    captured = {"ms_per_step": float(np.median(cws)) * 1e3, "windows_ms": [w_ * 1e3 for w_ in cws],
                "note": "the whole autograd step (forward_conv, loss, backward, fresh gradients) as one replayed hipGraph"}
    return {"captured_hipgraph": captured,
            "workload": f"synthetic all-pairs DGG N={N} d={d} h={h} k~{km:.1f} through DGG_LearnableK_debug.forward_conv (_FusedDGGConvFn: "
                        "generator + normalize_adj + GCNConv as one autograd node) under torch autograd, eager launches, one readback of "
                        "the chunk layout per forward (rows wider than the list would be chunked); Z.backward(cotangent), the cotangent resident",
            "ms_per_step": T * 1e3, "windows_ms": [w_ * 1e3 for w_ in tws], "steps": steps, "value": N * km / T, "unit": "edges/s", "dtype": "f32"}


def bench_module_api(a, dev):
    """The headline configuration through the DROP-IN MODULES under torch autograd (DGG_LearnableK_debug with all-pairs
    candidates -> normalize -> GCNConv, forward + backward): what a training script that swaps the imports gets, next to
    the hand-scheduled step of the default workload.  Run with --workload synthetic-module."""
    import dgg_amd
    from argparse import Namespace
    N, d, h = (a.nodes or 100_000), a.feat, a.latent
    args = Namespace(extra_edge_dim=0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288, dgg_mode_edge_net="u-v-dist",
                     dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=True,
                     symmetric_noise=False, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
    torch.manual_seed(0)
    dgg = dgg_amd.DGG_LearnableK_debug(in_dim=d, latent_dim=h, args=args)
    conv = dgg_amd.GCNConv(d, 64)
    with torch.no_grad():
        dgg.k_net.k_project.weight.mul_(0.1)
    dgg, conv = dgg.to(dev), conv.to(dev)
    dgg.set_seed(1234, 0)
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(1000)).to(dev)
    cand = dgg_amd.AllPairs((24 + 16 * torch.rand(N, generator=torch.Generator().manual_seed(7))).to(dev))
    params = list(dgg.parameters()) + list(conv.parameters())

    def step():
        for p_ in params:
            p_.grad = None
        adj = dgg(x, cand)
        conv(x, adj.normalize()).sum().backward()
        return adj

    for _ in range(a.warmup):
        adj = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        adj = step()
    torch.cuda.synchronize()
    T = (time.perf_counter() - t0) / a.steps
    kmean = float(adj.k.mean().item())
    emit_json(({
        "metric": METRIC, "value": N * kmean / T, "unit": "edges/s", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": T * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"synthetic all-pairs DGG N={N} d={d} h={h} k~{kmean:.1f} through the drop-in modules under torch "
                               "autograd (DGG_LearnableK_debug + normalize + GCNConv), fwd+bwd, eager launches",
                   "nodes": N, "feat": d, "latent": h}, "roofline": None}))


def bench_ppi(a, dev):
    emit_json(run_ppi(a, dev))


def run_ppi(a, dev):
    """BASELINE.json configs[4] (PPI shape: graphs of 591..3480 nodes, d=50, hidden 2048, 9 GCNII layers, 121 labels,
    train_ppi.py:43-44): dgg_amd.GCNIIppi_DGG under autograd, one forward + backward per graph; fp32, or with --bf16 the GCNII
    layer products on the hand-written bf16 MFMA kernel (dgg_bf16.hip).  The DGG runs at latent_dim = hidden = 2048
    (model.py:907-910).  cpu_baseline: the reference-shaped DENSE formulation of the same model in torch CPU ops on (up to) four
    graphs of the batch (cpu_baseline_ppi)."""
    import dgg_amd
    from argparse import Namespace
    d, hid, C, L = 50, 2048, 121, 9
    rng = np.random.default_rng(5)
    sizes = rng.integers(591, 3481, size=a.graphs)
    args = Namespace(extra_edge_dim=0, extra_k_dim=1, dgg_hard=False, deg_mean=3.899, deg_std=5.288, dgg_mode_edge_net="u-v-dist",
                     dgg_mode_k_net="x", dgg_mode_k_select="k_times_edge_prob", debug_step=3, perturb_edge_prob=True,
                     symmetric_noise=False, stochastic_k=False, dgg_adj_input="input_adj", n_dgg_layers=1)
    torch.manual_seed(0)
    m = dgg_amd.GCNIIppi_DGG(nfeat=d, nlayers=L, nhidden=hid, nclass=C, dropout=0.2, lamda=0.5, alpha=0.5, variant=True,
                             args=args).to(dev)
    with torch.no_grad():
        for dg in m.dggs:
            dg.k_net.k_project.weight.mul_(0.1)
    if a.bf16:
        for conv in m.convs:
            conv.gemm_dtype = torch.bfloat16
        for dg in m.dggs:                                        # the latent-2048 k-net's two wide products on the bf16 matrix cores as well
            dg.gemm_dtype = torch.bfloat16
    m.train()
    graphs = []
    for n in sizes:
        rows, cols = pubmed_graph(int(n), int(n) * 14, seed=int(n))
        keep = rows != cols                                      # the wrapper adds the self loops (model.py:935-938)
        A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows[keep], cols[keep]])), torch.ones(int(keep.sum())),
                                    (int(n), int(n))).coalesce().to(dev)
        graphs.append((torch.randn(int(n), d).to(dev), A, (torch.rand(int(n), C) < 0.3).float().to(dev)))
    params = list(m.parameters())

    def step():
        nsel = 0.0
        for x, A, y in graphs:
            for p_ in params:
                p_.grad = None
            out = m(x, A)
            torch.nn.functional.binary_cross_entropy(out, y).backward()
            nsel += float(A._nnz() + x.shape[0])
        return nsel

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        cand = step()
    torch.cuda.synchronize()
    T = (time.perf_counter() - t0) / a.steps
    gemm_flop = sum(3 * 2.0 * int(n) * (2 * hid) * hid * L for n in sizes)       # fwd + dX + dW of the variant GCNII layers
    # in-kernel rate of the layer GEMMs (event probes around the C-ABI calls inside running steps): flops of the probed calls /
    # their summed duration -- the figure to hold against the dense bf16 / fp32 MFMA peak
    pk = probe_steps(step, 2)
    stack = a.bf16 and "gcnii_stack_fwd" in pk          # the fused stack (ops.GcniiStackBf16Fn): probes around the whole forward / backward of the stack
    if stack:
        # the stack's launches are not probed one by one (the GEMM share: profiles/r04_ppi_bf16_kernel_stats.csv): the line holds the
        # layer-product flops against the stack's own forward + backward time
        t_g = (pk["gcnii_stack_fwd"][0] + pk["gcnii_stack_bwd"][0]) * 1e-3
        per_kernel = {"gcnii_stack_fwd": {"ms_per_step": pk["gcnii_stack_fwd"][0]}, "gcnii_stack_bwd": {"ms_per_step": pk["gcnii_stack_bwd"][0]}}
    elif a.bf16:
        t_g = (pk["gemm_bf16_fwd"][0] + pk["gemm_bf16_bwd"][0]) * 1e-3
        per_kernel = {"gemm_bf16_fwd": {"ms_per_step": pk["gemm_bf16_fwd"][0], "tflops": gemm_flop / 3 / (pk["gemm_bf16_fwd"][0] * 1e-3) / 1e12},
                      "gemm_bf16_bwd": {"ms_per_step": pk["gemm_bf16_bwd"][0], "tflops": 2 * gemm_flop / 3 / (pk["gemm_bf16_bwd"][0] * 1e-3) / 1e12}}
    else:
        t_g = (pk["linear_fwd"][0] + pk["linear_bwd"][0]) * 1e-3      # includes the (small) DGG projections
        per_kernel = {"linear_fwd": {"ms_per_step": pk["linear_fwd"][0]}, "linear_bwd": {"ms_per_step": pk["linear_bwd"][0]}}
    return ({
        "metric": "DGG adj-build+SpMM fwd/bwd edges/sec (multi-graph, PPI shape)", "value": cand / T, "unit": "edges/s", "n_gpus": 1,
        "steps": a.steps, "warmup": a.warmup, "ms_per_step": T * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16 GEMMs / f32 DGG" if a.bf16 else "f32", "data": "synthetic",
        "config": {"workload": f"PPI-shape multi-graph GCNIIppi_DGG: {len(sizes)} graphs of {int(sizes.min())}..{int(sizes.max())} nodes, "
                               f"d={d}, hidden={hid}, {L} variant GCNII layers, {C} labels, DGG latent {hid} on edge-list candidates "
                               "(value counts candidate edges), module API under autograd, fwd+bwd, " +
                               (("fused bf16 GCNII stack (ops.GcniiStackBf16Fn)" if stack else "bf16 GCNII GEMMs") if a.bf16 else "fp32"),
                   "graphs": len(sizes), "nodes_total": int(sizes.sum()), "graphs_per_s": len(sizes) / T,
                   "gcnii_gemm_tflops": gemm_flop / T / 1e12},
        "roofline": {"bound": "mfma", "kernel": ("fused GCNII stack (ops.GcniiStackBf16Fn: aggregation, gemm_nt_bf16 products with fused epilogues, SDDMM, transposed "
                                                 "SpMM of all layers): the layer-product flops over the stack's whole time" if stack else
                                                 "GCNII layer GEMMs (gemm_nt_bf16: fwd with fused epilogue, d support, d weight)") if a.bf16 else
                               "linear_fwd_mfma / gemm_tn (fp32 MFMA)",
                     "achieved": gemm_flop / t_g / 1e12, "peak": 2500.0 if a.bf16 else FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": gemm_flop / t_g / 1e12 / (2500.0 if a.bf16 else FP32_PEAK_TFLOPS), "traffic": None,
                     "kernel_ms_per_step": t_g * 1e3, "per_kernel": per_kernel, "whole_step_gemm_tflops": gemm_flop / T / 1e12,
                     "note": "GEMM flops of the GCNII layers / summed event-timed duration of the GEMM calls inside running steps"},
        "kernels_ms_per_step": {n_: v[0] for n_, v in pk.items()},
        # (the WHOLE batch, every graph once: ~20 s of CPU work for the 20 graphs of SURVEY 8(d) on 32 threads; DGG_BENCH_PPI_CPU_GRAPHS=n
        #  bounds it to the n smallest)
        "cpu_baseline": (cpu_baseline_ppi(m, sorted(graphs, key=lambda g_: g_[0].shape[0])[:int(os.environ.get("DGG_BENCH_PPI_CPU_GRAPHS", "1000"))],
                                          min(os.cpu_count() or 1, 32))
                         if a.cpu_rows >= 0 else None)})


def cpu_baseline_ppi(m, graphs, threads, lamda=0.5, alpha=0.5):
    """BASELINE.md section 3 for configs[4]: the reference-shaped dense formulation (oracle/dense_ref.py: [N,N] adjacency, torch.mm
    per layer, autograd) of GCNIIppi_DGG on the given graphs of the batch one after the other (train_ppi.py:204-219 steps per graph),
    forward + backward, torch CPU ops on `threads` threads, eval-mode dropout and no perturbation (the same arithmetic volume)."""
    tot_e, tot_t, sizes = 0.0, 0.0, []
    for g_ in graphs:
        r_ = _cpu_baseline_ppi_one(m, g_, threads, lamda, alpha)
        tot_e += r_[0]
        tot_t += r_[1]
        sizes.append(r_[2])
    return dict(value=tot_e / tot_t, unit="edges/s", cores=threads, kind="port",
                sample=f"dense torch-CPU formulation of GCNIIppi_DGG on {len(graphs)} graphs of the batch ({sizes} nodes, {int(tot_e)} candidate "
                       f"entries in all), forward + backward per graph, {tot_t:.2f} s")


def _cpu_baseline_ppi_one(m, graph, threads, lamda, alpha):
    import math
    from oracle import dense_ref as D
    torch.set_num_threads(threads)
    x, A, y = (t_.cpu() for t_ in graph)
    n = x.shape[0]
    A = A.coalesce()
    eye = torch.arange(n)
    rows, cols = torch.cat([A.indices()[0], eye]), torch.cat([A.indices()[1], eye])
    dg = m.dggs[0]
    P = {"We": dg.node_encode_for_edges[0].weight, "be": dg.node_encode_for_edges[0].bias, "Wk": dg.node_encode_for_k[0].weight,
         "bk": dg.node_encode_for_k[0].bias, "W1": dg.k_embed[0].weight, "b1": dg.k_embed[0].bias, "Wmu": dg.k_net.k_mu.weight,
         "bmu": dg.k_net.k_mu.bias, "Wp": dg.k_net.k_project.weight, "bp": dg.k_net.k_project.bias}
    P = {k_: v.detach().cpu().clone().requires_grad_(True) for k_, v in P.items()}
    Ws = [c.weight.detach().cpu().clone().requires_grad_(True) for c in m.convs]
    f0w, f0b, f1w, f1b = (t_.detach().cpu().clone().requires_grad_(True) for t_ in (m.fcs[0].weight, m.fcs[0].bias, m.fcs[1].weight, m.fcs[1].bias))
    deg = torch.zeros(n).index_add_(0, rows, torch.ones(rows.shape[0]))
    t0 = time.perf_counter()
    h0 = torch.relu(x @ f0w.t() + f0b)
    Adense, _ = D.dgg_dense(x, rows, cols, deg, P, None)
    Ahat = D.normalize_dense(Adense)
    hcur = h0
    for l, W in enumerate(Ws):
        theta = math.log(lamda / (l + 1) + 1)
        hi = Ahat @ hcur
        hcur = torch.relu(theta * (torch.cat([hi, h0], 1) @ W) + (1 - theta) * ((1 - alpha) * hi + alpha * h0) + hcur)
    out = torch.sigmoid(hcur @ f1w.t() + f1b)
    torch.nn.functional.binary_cross_entropy(out, y).backward()
    dt = time.perf_counter() - t0
    return float(rows.shape[0]), dt, int(n)


def cpu_baseline_edgelist(N, d, h, rows, cols, x, vals, dgg, conv, threads):
    """The oracle's edge-list pipeline (forward + backward) on the whole Pubmed-shape problem, all host cores."""
    from oracle import oracle as O
    os.environ.setdefault("OMP_NUM_THREADS", str(threads))
    sd = {k_: v.detach().cpu().numpy() for k_, v in dgg.state_dict().items()}
    Wc = conv.W.detach().cpu().numpy()
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.zeros(N + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    rowptr = np.cumsum(rowptr)
    deg = np.zeros(N, np.float32)
    np.add.at(deg, rows, vals)
    t0 = time.perf_counter()
    xp = O.linear(x, sd["node_encode_for_edges.0.weight"], sd["node_encode_for_edges.0.bias"], O.ACT_LEAKY)
    xk = O.linear(x, sd["node_encode_for_k.0.weight"], sd["node_encode_for_k.0.bias"], O.ACT_LEAKY)
    mu, sdv = O.degree_stats(deg)
    Wp = sd["k_net.k_project.weight"].reshape(-1)
    k, z, m, u = O.knet_x(xk, deg, mu, sdv, sd["k_embed.0.weight"], sd["k_embed.0.bias"], sd["k_net.k_mu.weight"],
                          sd["k_net.k_mu.bias"], Wp, sd["k_net.k_project.bias"], save=True)
    idx, val = O.edgelist_topk(xp, rowptr, cols.astype(np.int32), K=64, noise_mode=O.NOISE_HASH, seed=(1234, 0))
    w, rs = O.softk(idx, val, k)
    ahat = O.normalize(idx, w, rs)
    Y = O.spmm(idx, ahat, x)
    Z = O.linear(Y, Wc, None, O.ACT_RELU, w_layout=1)
    dY, _, _ = O.linear_bwd(Y, Wc, Z, np.ones_like(Z), act=O.ACT_RELU, w_layout=1)
    dA, _ = O.spmm_bwd(idx, ahat, x, dY, need_dx=False)
    dval, dk = O.softk_norm_bwd(idx, val, k, w, rs, dA)
    dxp = O.edge_bwd(xp, idx, val, dval, perturb=True)
    O.linear_bwd(x, sd["node_encode_for_edges.0.weight"], xp, dxp, act=O.ACT_LEAKY, need_dx=False)
    O.knet_x_bwd(xk, deg, mu, sdv, sd["k_embed.0.weight"], sd["k_net.k_mu.weight"], Wp, z, m, u, dk)
    O.linear_bwd(x, sd["node_encode_for_k.0.weight"], xk, np.zeros_like(xk), act=O.ACT_LEAKY, need_dx=False)
    dt = time.perf_counter() - t0
    nsel = float((w != 0).sum())
    return dict(value=nsel / dt, unit="edges/s", cores=threads, kind="port",
                sample=f"oracle edge-list pipeline fwd+bwd on the whole problem ({dt:.2f}s)")


_JSON_FD = None


def isolate_stdout():
    """Native libraries write banners to fd 1 (RCCL prints its version block there when the process group is torn down, AFTER
    the result line): send everything that is not the result line to stderr and keep the real stdout for emit_json()."""
    global _JSON_FD
    sys.stdout.flush()
    _JSON_FD = os.dup(1)
    os.dup2(2, 1)


LINE_LIMIT = 6000         # bytes: the driver keeps only a tail of stdout; the result line must fit in it with room to spare
DETAIL_PATH = os.environ.get("DGG_BENCH_DETAIL", os.path.join("gpurun_out", "bench_detail.json"))     # (relative to the repository root)
_TOP = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
_SUB = {"config": ("workload", "nodes", "feat", "latent", "parallelism", "rows_per_rank", "hipgraph", "noise", "api", "graphs", "selected_edges",
                   "candidate_edges"),
        "roofline": ("bound", "kernel", "rocprof_kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "kernel_ms",
                     "algorithmic_bytes", "algorithmic_flop"),
        "cpu_baseline": ("value", "unit", "cores", "kind", "sample"),
        "repeats": ("windows", "steps_per_window", "value_from", "window_ms_per_step_min_median_max", "eager_ms_per_step")}


def _sig(v, digits=6):
    """floats to `digits` significant figures, strings cut at 200 characters (recursively): the line is a summary"""
    if isinstance(v, float):
        return float(f"{v:.{digits}g}") if np.isfinite(v) else None
    if isinstance(v, str):
        return v if len(v) <= 200 else v[:197] + "..."
    if isinstance(v, dict):
        return {k_: _sig(x, digits) for k_, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_sig(x, digits) for x in v]
    if isinstance(v, (np.floating, np.integer)):
        return _sig(v.item(), digits)
    return v


def compact_result(obj):
    """The driver's line: the contract's fields, `roofline`, `cpu_baseline`, `repeats` and ONE map of {ms_per_step, value, frac} per
    secondary config.  Everything else (variants, data regimes, per-kernel tables, notes) lives in the detail file only."""
    out = {k_: obj[k_] for k_ in _TOP if k_ in obj}
    for name, keys in _SUB.items():
        if isinstance(obj.get(name), dict):
            out[name] = {k_: obj[name][k_] for k_ in keys if k_ in obj[name]}
    if isinstance(obj.get("configs"), dict):
        cfg = {}
        for name, c_ in obj["configs"].items():
            if not isinstance(c_, dict):
                continue
            if "error" in c_:
                cfg[name] = {"error": str(c_["error"])[:120]}
                continue
            rf = c_.get("roofline") if isinstance(c_.get("roofline"), dict) else {}
            cfg[name] = {"ms_per_step": c_.get("ms_per_step"), "value": c_.get("value"), "frac": rf.get("frac", c_.get("step_frac_hbm"))}
        out["configs"] = cfg
    out["detail"] = DETAIL_PATH
    out = _sig(out)
    line = json.dumps(out, separators=(",", ":"))
    for drop in ("configs", "repeats"):                         # (never expected: a guard, so that the line ALWAYS parses)
        if len(line) > LINE_LIMIT and drop in out:
            out.pop(drop)
            line = json.dumps(out, separators=(",", ":"))
    assert len(line) <= LINE_LIMIT, f"result line of {len(line)} bytes"
    return line


def emit_json(obj):
    """Full result -> gpurun_out/bench_detail.json and stderr; compact summary (<= LINE_LIMIT bytes) -> the ONE stdout line, last."""
    full = json.dumps(obj, default=lambda v: v.item() if hasattr(v, "item") else repr(v))
    try:
        os.makedirs(os.path.join(ROOT, os.path.dirname(DETAIL_PATH)), exist_ok=True)
        with open(os.path.join(ROOT, DETAIL_PATH), "w") as f:
            f.write(full + "\n")
    except OSError as e:
        print(f"bench detail file not written: {e!r}", file=sys.stderr)
    sys.stderr.write("BENCH_DETAIL " + full + "\n")
    sys.stderr.flush()
    line = (compact_result(json.loads(full)) + "\n").encode()
    if _JSON_FD is None:
        sys.stdout.write(line.decode())
        sys.stdout.flush()
    else:
        os.write(_JSON_FD, line)


DUMP_LIMIT = 60_000_000    # bytes: all arrays of --dump-outputs together (below 64 MB, headers included)


def dump_outputs(path, last):
    """--dump-outputs: the last timed step's output Z and gradients as <path>/Z.npy, <path>/grad_<name>.npy (float32).  If they do not
    fit in DUMP_LIMIT, the per-node arrays (Z, and the feature gradient with --x-grad) are cut to one fixed sample of rows (seed 0,
    ascending), whose row numbers go to <path>/sample_rows.npy (float64)."""
    Z, grads = last
    arrs = {"Z": Z.detach().float().cpu().numpy()}
    arrs.update({"grad_" + k_: v.detach().float().cpu().numpy() for k_, v in sorted(grads.items())})
    total = sum(v.nbytes for v in arrs.values())
    if total > DUMP_LIMIT:
        nrow = arrs["Z"].shape[0]
        per_node = [k_ for k_, v in arrs.items() if v.ndim == 2 and v.shape[0] == nrow]
        fixed = total - sum(arrs[k_].nbytes for k_ in per_node)
        n = (DUMP_LIMIT - fixed) // (sum(arrs[k_].shape[1] * 4 for k_ in per_node) + 8)
        rows = np.sort(np.random.default_rng(0).choice(nrow, size=n, replace=False))
        for k_ in per_node:
            arrs[k_] = arrs[k_][rows]
        arrs["sample_rows"] = rows.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k_, v in arrs.items():
        np.save(os.path.join(path, k_ + ".npy"), np.ascontiguousarray(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["synthetic", "synthetic-module", "pubmed", "ppi"], default="synthetic",
                    help="synthetic = the BASELINE.json metric config (default); pubmed = configs[1], edge-list candidates; "
                         "ppi = configs[4], multi-graph GCNIIppi_DGG (fp32)")
    ap.add_argument("--graphs", type=int, default=4, help="--workload ppi: number of graphs per step")
    ap.add_argument("--bf16", action="store_true", help="--workload ppi: GCNII layer GEMMs on bf16 operands (library GEMM, fp32 "
                                                        "accumulate); the DGG path stays fp32")
    ap.add_argument("--graph", default="pubmed", choices=["pubmed", "cora"],
                    help="--workload pubmed: the synthetic edge list's shape -- Pubmed (19 717 nodes, 500 features; BASELINE configs[1]) or Cora "
                         "(2 708 nodes, 1 433 features; configs[0]'s graph)")
    ap.add_argument("--edgelist-api", default="fused", choices=["fused", "modules"],
                    help="--workload pubmed: the fused layer (DGG_LearnableK_debug.forward_conv) or the separate modules")
    ap.add_argument("--edge-mode", default="u-v-dist", choices=["u-v-dist", "u-v-deg", "u-v-A_uv", "u-v-deg-dist", "edge_conv", "A_uv"],
                    help="--workload pubmed: edge scorer (dgm.py:1607-1725)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=0, help="node count: total (one GPU, or several with strong scaling) or per GPU (--weak); "
                                                          "0 = 100 000 on one GPU, 500 000 in total on several (BASELINE.json configs[3])")
    ap.add_argument("--weak", action="store_true", help="multi-GPU: --nodes (default 100 000) rows PER GPU of a (nodes x GPUs)-node graph")
    ap.add_argument("--repeats", type=int, default=0, help="timed windows of --steps steps each; value = median window; 0 = one window, "
                                                            "with --full as many as make the timed region last >= 3 s (at least 11)")
    ap.add_argument("--full", action="store_true",
                    help="default workload: besides the headline figure, measure everything else -- eager window, per-kernel roofline, "
                         "data regimes, variants, the other BASELINE.json configs, CPU baselines (the options below select among them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="default workload: write what the last timed step returned (Z and every parameter gradient) as DIR/<name>.npy")
    ap.add_argument("--no-variants", dest="variants", action="store_false",
                    help="--full: skip the symmetric / unperturbed / hash / latent-128 / x-grad variants of the step (one GPU only)")
    ap.add_argument("--no-configs", dest="configs", action="store_false",
                    help="--full: skip the compact lines of the other BASELINE.json configs (Pubmed shape, PPI bf16, N = 500 000 on one GPU) "
                         "that the run appends under `configs`")
    ap.add_argument("--no-cpu-dense", dest="cpu_dense", action="store_false",
                    help="--full: skip the dense reference-shaped CPU formulation at N = 2 708 / 4 000 (BASELINE.md section 3)")
    ap.add_argument("--prior", default="24,40", help="synthetic workload: prior degrees lo,hi (uniform); 24,40 = SURVEY 8(d) (k ~ 32); 100,164: k ~ 128")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--algo", type=int, default=0, help="all-pairs kernel for --noise hash: 0 auto, 1 exhaustive, 2 MFMA-bounded, "
                                                         "3 adaptive noise prefilter, 4 guess-and-verify")
    ap.add_argument("--noise", choices=["ranked", "hash", "sym", "rsym", "none"], default="ranked",
                    help="counter-based Gumbel generator: ranked (per-row order statistics, O(N*150) search), hash (per-pair hash, "
                         "N^2 sweep), sym (symmetric per-pair hash: the reference's symmetric_noise=True), rsym (the ranked symmetric generator: "
                         "same symmetric law, owners list their largest noises first, O(N*300)), all iid Gumbel(0,0.3); "
                         "none = unperturbed scores (the reference's perturb_edge_prob=False: bf16-MFMA-bounded N^2 sweep)")
    ap.add_argument("--feat-scale", type=float, default=1.0,
                    help="multiply the synthetic node features by this factor (the ranked search's walk depth grows like "
                         "exp(spread of 0.05 ||xp_i - xp_j|| / 0.3): see `data_regimes` in the output line)")
    ap.add_argument("--data", choices=["randn", "clustered"], default="randn",
                    help="clustered: a tight blob of 3 000 nodes + 40 far outliers inside randn features (tests/test_hip_parity.py)")
    ap.add_argument("--x-grad", action="store_true", help="also compute d loss / d x (reduce-scatter across ranks)")
    ap.add_argument("--strong", action="store_true", help="(default for several GPUs; kept for compatibility)")
    ap.add_argument("--exchange", choices=["hybrid", "replicate", "gather"], default="hybrid",
                    help="multi-GPU, features as data (no --x-grad): 'hybrid' (default) = the node features are placed on every GPU "
                         "once at load, each rank projects xp of all rows itself but H = X Wc of its own rows only: H is all-gathered "
                         "behind the k-net / search / partition and the partial dH reduce-scattered behind the score backward; "
                         "'replicate' = each rank projects [xp | H] of all rows and forms every weight gradient from full-N partials "
                         "(per-step collectives: row sums, da, weight gradients only); 'gather' = all-gather [xp | H] every step (the "
                         "path for inputs that are activations)")
    ap.add_argument("--emulate-world", type=int, default=0,
                    help="DIAGNOSTIC, single GPU: time the per-step COMPUTE of one rank of a W-GPU weak-scaling run (own --nodes rows "
                         "against W * --nodes columns, replicated features, no collectives); not a throughput measurement")
    ap.add_argument("--no-hipgraph", dest="hipgraph", action="store_false", help="time eager launches instead of a captured hipGraph")
    ap.add_argument("--cpu-rows", type=int, default=0,
                    help="row sample of the cpu_baseline leg: 0 = auto (64 rows per host core, ~10-20 s), <0 = skip")
    a = ap.parse_args()
    if a.dump_outputs and a.workload != "synthetic":
        ap.error("--dump-outputs is implemented for the default (synthetic) workload")
    isolate_stdout()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus}"
    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU fallback for the product path)"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    force = os.environ.get("DGG_FORCE_COLLECTIVES") == "1"     # 1-rank RCCL group: every collective of the N>1 path on one GPU
    if force and world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", device_id=dev, rank=0, world_size=1)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    import dgg_amd
    from dgg_amd import ops
    from dgg_amd.parallel import ShardedDGGConv, shard_bounds
    if a.workload == "pubmed":
        assert world == 1, "--workload pubmed is a single-GPU measurement"
        return bench_edgelist(a, dev)
    if a.workload == "synthetic-module":
        assert world == 1, "--workload synthetic-module is a single-GPU measurement"
        return bench_module_api(a, dev)
    if a.workload == "ppi":
        assert world == 1, "--workload ppi is a single-GPU measurement (graphs are independent: replicas across GPUs)"
        return bench_ppi(a, dev)

    return bench_synthetic(a, dev, world, rank, force)


class SyntheticRun:
    """One configuration of the synthetic all-pairs workload: inputs resident in HBM, the layer, and the step function."""

    def __init__(self, a, dev, world, rank, force, N, d, h, noise_mode, x_grad=False, emu=0, exchange="replicate", feat_scale=None,
                 data=None, prior=None):
        from dgg_amd import ops
        from dgg_amd.parallel import ShardedDGGConv, shard_bounds, _all_gather_rows
        self.N, self.d, self.h, self.world, self.rank, self.emu = N, d, h, world, rank, emu
        self.P = make_params(d, h, dev)
        self.erank = emu // 2
        self.r0, self.r1, _ = shard_bounds(N, emu, self.erank) if emu else shard_bounds(N, world, rank)
        g = torch.Generator(device="cpu").manual_seed(1000 + rank)
        x_cpu = torch.randn(self.r1 - self.r0, d, generator=g)
        if (data or getattr(a, "data", "randn")) == "clustered" and N >= 30_000 and world == 1 and not emu:
            x_cpu[20_000:23_000] *= 0.05                          # tight cluster: tiny neighbour radius
            x_cpu[23_000:23_040] = x_cpu[23_000:23_040] * 0.01 + 3.0   # 40 outliers far from everything
        fs = float(feat_scale if feat_scale is not None else getattr(a, "feat_scale", 1.0))
        self.x_local = (x_cpu * fs).to(dev)
        # prior degrees c_i = lo + (hi - lo) U(0,1): SURVEY 8(d)'s 24..40 (mean 32) unless --prior says otherwise (100,164: learned
        # degrees ~128, rows of three 64-rank chunks)
        lo, hi = prior if prior is not None else tuple(float(v) for v in getattr(a, "prior", "24,40").split(","))
        self.deg = (lo + (hi - lo) * torch.rand(N, generator=torch.Generator(device="cpu").manual_seed(7))).to(dev)
        # features are DATA unless x_grad: with more than one rank they are replicated once, here, outside the timed region (data
        # placement: 4*N*d bytes per GPU), and no feature tensor crosses the fabric per step (dgg_amd/parallel.py)
        x_full = None
        if (world > 1 or force) and not x_grad and exchange in ("replicate", "hybrid"):
            x_full = _all_gather_rows(self.x_local, N, shard_bounds(N, world, rank)[2], None).contiguous()
        if emu:
            x_full = torch.randn(N, d, generator=g).to(dev)
            x_full[self.r0:self.r1] = self.x_local
        self.x_full = x_full
        self.layer = ShardedDGGConv(ops, N, group=None, K=64, noise_mode=noise_mode, seed=(1234, 0), algo=a.algo, x_grad=x_grad, x_full=x_full,
                                    hybrid=(exchange == "hybrid" and x_full is not None))
        if emu:
            self.layer.emulate_rank(emu, self.erank)
        # rows wider than the 64-rank list (learned degrees k_i + 9.5 > 64) are kept in CHUNKED rows -- the configuration a model can be
        # TRAINED in (the learned degree is unbounded, dgm.py:1580-1584).  One rank: the eager warm-up steps read the chunk count back,
        # the captured graph replays that layout as a fixed capacity (no wide row at this prior: the plain [N,64] list, same graph as
        # without the option).  Several ranks run eagerly: the list with its enforced bound (no readback per step).
        self.wide = world == 1 and not force and not emu and hasattr(ops, "chunk_layout") and h in (16, 32, 64, 128)
        if self.wide:
            self.layer.wide_rows = "auto"
        if noise_mode == ops.NOISE_RANKED and world == 1 and not force and not emu:
            # the search's stop tests take the rows' nearest-neighbour bound when a pilot walk says the data makes it walk deep (one probe
            # every 16 EAGER forwards; a captured step replays the decision of the warm-up)
            self.layer.tight_bound = os.environ.get("DGG_BENCH_TIGHT", "auto")
        self.grads = None
        # ranked noise: the seed lives in DEVICE memory and is advanced by a (captured) increment at the top of every step, so ONE
        # hipGraph draws fresh noise on every replay -- what training does per forward (reference dgm.py:1226); the other
        # generators take the seed by value and cycle NGRAPH captured graphs
        self.seed_dev = self.seed_inc = None
        if noise_mode == ops.NOISE_RANKED and hasattr(ops, "allpairs_topk_softk"):
            self.seed_dev = torch.tensor([1234, 0], dtype=torch.int32, device=dev)
            self.seed_inc = torch.tensor([0, 1], dtype=torch.int32, device=dev)
        self.cot = None

    def step(self, seed_lo=0):
        """one pass of the hot path over the whole graph, forward + backward; a different noise realisation per step"""
        if self.seed_dev is not None:
            self.seed_dev.add_(self.seed_inc)
            self.layer.seed = self.seed_dev
        else:
            self.layer.seed = (1234, seed_lo)
        if self.wide and self.layer.wide_cap is None and torch.cuda.is_current_stream_capturing():
            c_, m_ = self.layer.last_layout                      # (layout of the last eager step; + 6 % spare chunks)
            if c_ == self.r1 - self.r0:
                self.layer.wide_rows = "off"
            else:
                self.layer.wide_cap = (c_ + c_ // 16 + 64, m_)
        Z = self.layer.forward(self.x_local, self.deg, self.P)
        if self.cot is None or self.cot.shape != Z.shape:
            self.cot = torch.ones_like(Z)                            # the cotangent is an INPUT of the backward: resident, not refilled
        self.grads = self.layer.backward(self.cot, self.x_local, self.P)
        self.Z = Z
        return self.grads


MIN_TIMED_S = 3.3   # the timed region (all windows) lasts at least this long
NGRAPH = 4      # captured hipGraphs, one per noise seed: consecutive steps see different graphs (idx / partition / gather pattern)


def time_windows(run, a, world, force, dev, use_graph, repeats):
    """W untimed warm-up steps, then windows of EXACTLY a.steps steps, each bracketed by barrier + synchronize; returns
    (per-window seconds, max over ranks), whether hipGraphs were used, the per-step time of one EAGER window (--full only, else
    None) and the (Z, gradients) of the last timed step.
    Noise: a fresh realisation every step -- device-resident seed advanced inside the step (ONE captured graph), or, for the
    generators that take the seed by value, NGRAPH captured graphs cycled.  `repeats` <= 0: one window; with --full as many windows
    as make the timed region last >= MIN_TIMED_S seconds (so that the driver's GPU-busy sampler sees it), at least 11."""
    coll = world > 1 or force
    ngraph = 1 if getattr(run, "seed_dev", None) is not None else NGRAPH
    for s_ in range(max(a.warmup, 1)):
        run.step(s_ % NGRAPH)

    def window(launch):
        if coll:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s_ in range(a.steps):
            launch(s_)
        torch.cuda.synchronize()
        if coll:
            dist.barrier()
        return time.perf_counter() - t0

    full = a.full
    eager_s = window(lambda s_: run.step(s_ % NGRAPH)) if full else None     # one eager window (also the estimate for the window count)
    graphs, outs = None, None
    if use_graph:
        try:
            torch.cuda.synchronize()
            graphs, outs = [], []
            for s_ in range(ngraph):
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph):
                    run.step(s_)
                graphs.append(gph)
                outs.append((run.Z, run.grads))                       # (the captured step's output tensors, rewritten by each replay)
            for s_ in range(len(graphs) if full else max(a.warmup, len(graphs))):    # (plain run: the W warm-up steps on the timed path too)
                graphs[s_ % len(graphs)].replay()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            print(f"hipGraph capture failed ({e!r}); timing eager launches", file=sys.stderr)
            graphs = None
    launch = (lambda s_: graphs[s_ % ngraph].replay()) if graphs is not None else (lambda s_: run.step(s_ % NGRAPH))
    if repeats <= 0 and full:
        first = window(launch)
        est = torch.tensor([first], device=dev, dtype=torch.float64)
        if coll:
            dist.all_reduce(est, op=dist.ReduceOp.MAX)
        repeats = int(min(max(11, np.ceil(MIN_TIMED_S / max(float(est.item()), 1e-6))), 400))
    times = [window(launch) for _ in range(max(repeats, 1))]
    last = outs[(a.steps - 1) % ngraph] if graphs is not None else (run.Z, run.grads)
    tm = torch.tensor(times + ([eager_s] if full else []), device=dev, dtype=torch.float64)
    if coll:
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
    tm = [float(v) for v in tm.tolist()]
    return tm[:len(times)], graphs is not None, (tm[-1] / a.steps if full else None), last


def cpu_dense_formulation(sizes, threads):
    """the dense, reference-shaped formulation (oracle/dense_ref.py: one [N,N] torch tensor per stage, as
    the reference computes) timed on the host for the sizes where it can be allocated.  One forward + backward each."""
    from oracle import dense_ref as D
    torch.set_num_threads(threads)
    out = []
    for kind, N, d, h in sizes:
        g = torch.Generator().manual_seed(0)
        x = torch.randn(N, d, generator=g)
        P = {k_: v.cpu() for k_, v in make_params(d, h, torch.device("cpu")).items()}
        if kind == "allpairs":
            rows = cols = None
            deg = 24 + 16 * torch.rand(N, generator=g)
            npairs = float(N) * N
        else:                                                    # edge-list candidates, Cora / Pubmed shaped
            und = {2708: 5278, 19717: 44324}.get(N, 2 * N)
            r_, c_ = pubmed_graph(N, und)
            rows, cols = torch.from_numpy(r_.astype(np.int64)), torch.from_numpy(c_.astype(np.int64))
            deg = torch.zeros(N).index_add_(0, rows, torch.ones(rows.shape[0]))
            npairs = float(N) * N                               # the dense formulation still sweeps N^2 entries per stage
        try:
            dt, kmean = D.timed_step(x, rows, cols, deg, P)
            out.append({"candidates": kind, "nodes": N, "feat": d, "latent": h, "threads": threads, "seconds_fwd_bwd": dt, "dense_entries_per_s": npairs / dt,
                        "edges_per_s": N * kmean / dt})
        except Exception as e:  # noqa: BLE001
            out.append({"candidates": kind, "nodes": N, "error": repr(e)})
    return out


def wide_rows_config(a, dev, prior, N=100_000, noise_mode=None):
    """The headline step with learned degrees BEYOND the 64-rank list (prior degrees `prior`: k ~ 128, every row three chunks of 64
    ranks -- where a model sits after some tens of Adam steps, tests/test_chunked_rows.py): chunked rows through the same engine,
    captured into one hipGraph with the chunk count of the warm-up steps as its capacity.  noise_mode: the ranked generator (default),
    or the reference's own defaults -- symmetric noise (NOISE_RANKED_SYM: wide rows are evaluated under the symmetric per-pair hash),
    unperturbed scores (NOISE_NONE) -- through the threshold-buffer evaluator (dgg_allpairs_topk_anywide)."""
    import copy
    from dgg_amd import ops
    b = copy.copy(a)
    b.steps, b.warmup, b.repeats = 10, 3, 5
    if noise_mode is not None:
        b.steps, b.repeats = 5, 3
    run = SyntheticRun(b, dev, 1, 0, False, N, a.feat, a.latent, ops.NOISE_RANKED if noise_mode is None else noise_mode, prior=prior)
    times, graphed, eager_T, _ = time_windows(run, b, 1, False, dev, a.hipgraph, b.repeats)
    T = float(np.median(times)) / b.steps
    run.layer.check_wide()
    sv = run.layer.saved
    lay = sv["layout"]
    k = sv["k"]
    ops.PROBE = {}
    run.step(0)
    torch.cuda.synchronize()
    pv, ops.PROBE = ops.PROBE, None
    kern = {n_: sum(e0.elapsed_time(e1) for e0, e1 in ev) for n_, ev in pv.items()}
    kept = float((sv["idx"] >= 0).sum().item())
    active = float((sv["w"] != 0).sum().item())
    h, F = a.latent, int(sv["H"].shape[1])
    # compulsory bytes of the step as SURVEY 8(d) counts them (every array once), with K' = kept ranks per row instead of 41
    comp = N * 4.0 * (a.feat + 3 * 64 + 2) + kept * 12 + active * (8 + 24 + 36) + N * 4.0 * (3 * F + 4 * h)
    return {"workload": f"synthetic all-pairs DGG N={N} d={a.feat} h={h}, prior degrees {prior[0]:.0f}..{prior[1]:.0f}: learned k ~ {float(k.mean()):.1f} "
                        f"(max {float(k.max()):.1f}), chunked rows ({'no wide row' if lay is None else f'{int(lay.meta[0])} chunks, widest row {int(lay.meta[1])}'})",
            "ms_per_step": T * 1e3, "eager_ms_per_step": eager_T * 1e3, "hipgraph": graphed, "value": N * float(k.mean()) / T, "unit": "edges/s",
            "steps": b.steps, "windows": len(times), "dtype": "f32", "kept_ranks_per_row": kept / N, "active_edges_per_row": active / N,
            "kernels_ms_per_step": kern, "step_compulsory_bytes": comp, "step_frac_hbm": comp / T / 1e9 / HBM_PEAK_GBPS}


def other_configs(a, dev):
    """Compact results of BASELINE.json configs[1], [4] and [3] (single GPU) for the default run's JSON line: ms per step, value,
    roofline of the dominant kernel / GEMMs, CPU baseline.  Short windows (these are secondary lines; the full ones: --workload
    pubmed / --workload ppi --bf16 / --nodes 500000)."""
    import copy
    from dgg_amd import ops
    res = {}
    only = [c_ for c_ in os.environ.get("DGG_BENCH_CONFIGS", "pubmed,ppi,module,k128,n500k").split(",") if c_]     # (diagnostic: a subset)

    def pick(o, extra=()):
        keep = ("metric", "value", "unit", "ms_per_step", "ms_per_step_with_sum_loss", "steps", "dtype", "roofline", "cpu_baseline", "kernels_ms_per_step") + tuple(extra)
        d_ = {k_: o.get(k_) for k_ in keep if k_ in o}
        d_["workload"] = o["config"]["workload"]
        for k_ in ("api", "gcn_dgg_model_ms_per_step", "selected_edges", "candidate_edges"):
            if k_ in o["config"]:
                d_[k_] = o["config"][k_]
        return d_
    try:
        if "pubmed" in only:
            b = copy.copy(a)
            b.steps, b.warmup, b.edge_mode, b.cpu_dense = 20, 3, "u-v-dist", False
            res["pubmed_uvdist"] = pick(run_edgelist(b, dev))
    except Exception as e:  # noqa: BLE001
        res["pubmed_uvdist"] = {"error": repr(e)}
    try:
        if "pubmed" in only:                                 # the same shape with the reference script's DEFAULT scorer (train_small_graphs.py:184-191)
            b = copy.copy(a)
            b.steps, b.warmup, b.edge_mode, b.cpu_dense, b.cpu_rows = 20, 3, "u-v-deg", False, -1
            res["pubmed_uvdeg"] = pick(run_edgelist(b, dev))
    except Exception as e:  # noqa: BLE001
        res["pubmed_uvdeg"] = {"error": repr(e)}
    try:
        if "pubmed" in only:                                 # configs[0]'s graph (Cora: 2 708 nodes, 1 433 features) through the same layer
            b = copy.copy(a)
            b.steps, b.warmup, b.edge_mode, b.cpu_dense, b.graph = 20, 3, "u-v-dist", False, "cora"           # (+ the oracle's pipeline on the host: 0.1 s)
            res["cora_uvdist"] = pick(run_edgelist(b, dev))
    except Exception as e:  # noqa: BLE001
        res["cora_uvdist"] = {"error": repr(e)}
    torch.cuda.empty_cache()
    try:
        if "module" in only:
            res["allpairs_module_api"] = allpairs_module_api(a, dev, 100_000, 20, 5)
    except Exception as e:  # noqa: BLE001
        res["allpairs_module_api"] = {"error": repr(e)}
    torch.cuda.empty_cache()
    nthreads = torch.get_num_threads()
    try:
        if "ppi" in only:
            b = copy.copy(a)
            b.steps, b.warmup, b.graphs, b.bf16 = 10, 2, 20, True       # 20 graphs of 591..3480 nodes
            res["ppi_bf16"] = pick(run_ppi(b, dev))
    except Exception as e:  # noqa: BLE001
        res["ppi_bf16"] = {"error": repr(e)}
    import gc
    gc.collect()                                             # (the PPI models' cycles: collected here, not inside the next config's windows)
    torch.cuda.empty_cache()
    torch.set_num_threads(nthreads)                          # (the PPI CPU baseline sets its own count)
    for name, nm_ in (("k128_chunked_rows", None), ("k128_chunked_rows_symmetric", ops.NOISE_RANKED_SYM), ("k128_chunked_rows_unperturbed", ops.NOISE_NONE)):
        try:
            if "k128" in only:
                res[name] = wide_rows_config(a, dev, (100.0, 164.0), noise_mode=nm_)
                if nm_ is not None:
                    res[name]["workload"] += {ops.NOISE_RANKED_SYM: "; symmetric noise (symmetric_noise=True): wide rows under the symmetric per-pair hash generator",
                                              ops.NOISE_NONE: "; unperturbed scores (perturb_edge_prob=False)"}[nm_]
        except Exception as e:  # noqa: BLE001
            res[name] = {"error": repr(e)}
        torch.cuda.empty_cache()
    try:
        if "n500k" not in only:
            return res
        N5 = 500_000
        r5 = SyntheticRun(a, dev, 1, 0, False, N5, a.feat, a.latent, ops.NOISE_RANKED, feat_scale=1.0, data="randn")
        for s_ in range(3):
            r5.step(s_)
        w5 = []
        for _ in range(3):                                   # median of three 5-step windows (eager launches: a busy host shows up as an outlier)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s_ in range(5):
                r5.step(s_ % NGRAPH)
            torch.cuda.synchronize()
            w5.append((time.perf_counter() - t0) / 5)
        T5 = sorted(w5)[1]
        ops.PROBE = {}
        r5.step(0)
        torch.cuda.synchronize()
        pv, ops.PROBE = ops.PROBE, None
        km = float(r5.layer.saved["k"].mean().item())
        kern5 = {n_: sum(e0.elapsed_time(e1) for e0, e1 in ev) for n_, ev in pv.items()}
        kept5 = float((r5.layer.saved["idx"] >= 0).sum().item())
        dom5 = max(kern5, key=kern5.get)
        comp5 = N5 * 4.0 * a.latent + kept5 * 8 + N5 * 4
        try:                                                 # the oracle on a bounded row sample of the same 500 000-node problem
            cores5 = os.cpu_count() or 1
            cpu5 = cpu_baseline(N5, a.feat, a.latent, r5.P, min(16 * cores5, N5), cores5, ops.NOISE_RANKED) if a.cpu_rows >= 0 else None
        except Exception as e:  # noqa: BLE001
            cpu5 = {"value": None, "unit": "edges/s", "cores": os.cpu_count(), "kind": "port", "sample": f"failed: {e!r}"}
        res["n500k_one_gpu"] = {"workload": f"synthetic all-pairs DGG N={N5} d={a.feat} h={a.latent} k~{km:.1f} on ONE GPU (BASELINE configs[3]'s graph), "
                                            "eager launches", "ms_per_step": T5 * 1e3, "windows_ms": [w_ * 1e3 for w_ in w5], "value": N5 * km / T5, "unit": "edges/s", "steps": 5,
                                "dtype": "f32", "kernels_ms_per_step": kern5,
                                "roofline": {"bound": "hbm", "kernel": "allpairs_topk", "kernel_ms": kern5.get("allpairs_topk"),
                                             "algorithmic_bytes": comp5, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "traffic": None,
                                             "achieved": comp5 / (kern5["allpairs_topk"] * 1e-3) / 1e9,
                                             "frac": comp5 / (kern5["allpairs_topk"] * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                                             "dominant_by_time": dom5},
                                "cpu_baseline": cpu5}
        del r5
    except Exception as e:  # noqa: BLE001
        res["n500k_one_gpu"] = {"error": repr(e)}
    torch.cuda.empty_cache()
    return res


def bench_synthetic(a, dev, world, rank, force):
    from dgg_amd import ops
    d, h = a.feat, a.latent
    emu = a.emulate_world if (a.emulate_world > 1 and world == 1 and not force) else 0
    # Graph size.  One GPU: the BASELINE.json metric configuration, N = 100 000.  Several GPUs: BASELINE.json configs[3] -- ONE
    # graph of 500 000 nodes, node-range sharded (strong scaling: 62 500 rows per rank at 8 GPUs); --weak gives every rank
    # 100 000 rows of a (100 000 x GPUs)-node graph instead.  --nodes overrides the count (total if strong, per GPU if weak).
    if world > 1 or emu:
        weak = a.weak or bool(emu)
        per = a.nodes if a.nodes else 100_000
        N = per * max(world, emu) if weak else (a.nodes if a.nodes else 500_000)
    else:
        weak, N = True, (a.nodes if a.nodes else 100_000)
    noise_mode = {"ranked": ops.NOISE_RANKED, "hash": ops.NOISE_HASH, "sym": ops.NOISE_HASH_SYM, "rsym": ops.NOISE_RANKED_SYM,
                  "none": ops.NOISE_NONE}[a.noise]
    run = SyntheticRun(a, dev, world, rank, force, N, d, h, noise_mode, a.x_grad, emu, a.exchange)
    # one rank: the step is captured -- also with DGG_FORCE_COLLECTIVES=1, so that the multi-collective step of the N > 1 path has run under
    # capture on the one GPU there is (DGG_BENCH_GRAPH_DIST=0 times it eagerly).  Several ranks: eager unless DGG_BENCH_GRAPH_DIST=1.
    gd = os.environ.get("DGG_BENCH_GRAPH_DIST")
    use_graph = a.hipgraph and ((world == 1 and gd != "0") if (world == 1 and force) else (world == 1 or gd == "1"))
    times, graphed, eager_T, last = time_windows(run, a, world, force, dev, use_graph, a.repeats)
    T = float(np.median(times)) / a.steps
    layer, P, r0, r1 = run.layer, run.P, run.r0, run.r1
    ksum = layer.saved["k"].sum().reshape(1).double()
    kmaxv = layer.saved["k"].max().reshape(1)
    if world > 1 or force:
        dist.all_reduce(ksum)
        dist.all_reduce(kmaxv, op=dist.ReduceOp.MAX)
    Nval = (r1 - r0) if emu else N                            # emulation: one rank's rows only
    kmean = float(ksum.item()) / Nval
    lay = layer.saved.get("layout")
    assert lay is not None or float(kmaxv.item()) + 8.5 <= 64, "learned degree exceeds the ELL width: results would be truncated"
    if lay is not None:
        layer.check_wide()                                        # (a captured step's fixed chunk capacity held every row)
    assert all(torch.isfinite(v).all() for v in run.grads.values())
    coll = world > 1 or force
    rows_loc = r1 - r0
    out = {
        "metric": METRIC, "value": Nval * kmean / T, "unit": "edges/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": T * 1e3, "higher_is_better": True,
        "scaling": "weak" if weak else "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "repeats": {"windows": len(times), "steps_per_window": a.steps, "value_from": "median window",
                    "window_ms_per_step_min_median_max": [float(np.min(times)) / a.steps * 1e3, float(np.median(times)) / a.steps * 1e3,
                                                           float(np.max(times)) / a.steps * 1e3],
                    "timed_seconds_total": float(sum(times)),
                    "noise": "fresh seed every step: device-resident seed advanced inside the captured step (one hipGraph)"
                             if getattr(run, "seed_dev", None) is not None else f"{NGRAPH} captured graphs with different seeds, cycled"},
        "config": {"workload": f"synthetic all-pairs DGG N={N} d={d} h={h} k~{kmean:.1f} K=64, u-v-dist/x/"
                               f"k_times_edge_prob, Gumbel(0,0.3) perturbation, + normalize + GCNConv({d},64), fwd+bwd",
                   "nodes": N, "feat": d, "latent": h, "ell_width": 64, "pairs_per_s": N * float(N) / T,
                   "x_grad": a.x_grad, "topk_algo": a.algo, "noise": a.noise, "hipgraph": graphed,
                   "hipgraph_note": None if graphed or not coll else "steps with collectives are launched eagerly (set "
                                    "DGG_BENCH_GRAPH_DIST=1 to try capturing the RCCL calls)",
                   "parallelism": f"row-shard x{world}" if not emu else f"DIAGNOSTIC: compute of rank {run.erank} of {emu}, no collectives",
                   "rows_per_rank": rows_loc,
                   "feature_exchange": ("single GPU" if not coll else
                                        "hybrid: features replicated at load, every rank projects xp of all rows and H of its own rows; per step: "
                                        "async all-gather of H (N*F*4 B, behind k-net + search + partition), all-gather row sums, async "
                                        "reduce-scatter of the partial dH (behind the score backward), all-reduce da + weight gradients"
                                        if (run.x_full is not None and run.layer.hybrid) else
                                        "features replicated at load, every rank projects all rows; per-step collectives: all-gather row sums, "
                                        "all-reduce da + weight gradients" if run.x_full is not None else
                                        "per step: all-gather [xp | H] (projections of the own rows), all-gather row sums, all-reduce da, "
                                        "reduce-scatter [dxp | dH], all-reduce weight gradients")},
    }
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, last)
    if not a.full:
        if rank == 0:
            emit_json(out)
        if dist.is_initialized():
            dist.destroy_process_group()
        return
    out["repeats"]["eager_ms_per_step"] = eager_T * 1e3

    # Per-kernel roofline figures: durations taken INSIDE running steps.  dgg_amd.ops records a pair of events on the launch
    # stream around the C-ABI call of each gather kernel (ops.PROBE); PROBE_STEPS eager steps are run for that after the timed
    # region (same kernels, same inputs, same cache state as in the timed steps; the events themselves are not in `value`).
    PROBE_STEPS = 10
    run.step(0)
    ops.PROBE = {}
    for s_ in range(PROBE_STEPS):
        run.step(s_ % NGRAPH)
    torch.cuda.synchronize()
    probe, ops.PROBE = ops.PROBE, None
    tk = {n: sum(e0.elapsed_time(e1) for e0, e1 in ev) / len(ev) * 1e-3 for n, ev in probe.items()}
    if "edge_bwd" not in tk:                                      # two-stream step: the score backward is probed as its two launches
        tk["edge_bwd"] = tk["edge_bwd_rows"] + tk["edge_bwd_node"]
    sv = layer.saved
    F = int(sv["H"].shape[1])                                     # width of the aggregated (projected) rows
    active = float((sv["w"] != 0).sum().item())                   # edges with a non-saturated ramp (~ k + 8.5 per row)
    kept = float((sv["idx"] >= 0).sum().item())                   # ranks kept by k_limit (~ k + 9.5 per row)
    # Two byte counts per kernel.  `compulsory` = SURVEY 8(d)'s algorithmic bytes: every array the kernel has to touch, ONCE
    # (perfect reuse of gathered rows) -- this is what `frac` is computed on.  `gathered` = the same with every gathered row
    # counted once per use: what an L2-missing gather kernel actually has to pull through the fabric (the tables are 25.6 MB,
    # Infinity-Cache resident, the XCD L2 is 4 MB), compared with the guide's measured random-row ceiling.
    kern = {
        # pair scoring + top-k: xp read once, idx / score written for the kept ranks; gathered: one xp row per KEPT entry
        "allpairs_topk": dict(ms=tk["allpairs_topk"] * 1e3, compulsory=N * 4.0 * h + kept * 8 + rows_loc * 4,
                              gathered=kept * 4 * h + rows_loc * (4 * h + 2 * 256)),
        # aggregation Z = relu(A H): idx, ahat per active entry, H read once, Z written
        "spmm_fwd": dict(ms=tk["spmm_fwd"] * 1e3, compulsory=active * 8 + N * 4.0 * F + rows_loc * 4.0 * F,
                         gathered=active * 4 * F + rows_loc * (4 * F + 2 * 256)),
        # conv backward, one wavefront per destination node: record (16) + dA row-major and in record order (8) per active entry,
        # G and H read once, dH and da written; gathered: one G row per entry
        "conv_bwd": dict(ms=tk["conv_bwd"] * 1e3, compulsory=active * 24 + rows_loc * 4.0 * F + 2 * N * 4.0 * F + N * 4,
                         gathered=active * (4 * F + 24) + N * 8.0 * F),
        # score backward (row kernel + per-destination kernel): idx, score, dA, ahat per entry in row order, record + dA in record
        # order, xp read once per pass, dxp written; gathered: xp_j (row pass) and xp_i (column pass) per active entry
        "edge_bwd": dict(ms=tk["edge_bwd"] * 1e3, compulsory=active * 36 + 4 * N * 4.0 * h,
                         gathered=active * (8 * h + 36) + rows_loc * (4 * 256 + 8 * h) + N * 8.0 * h),
    }
    kern["edge_bwd"]["composite"] = "edge_bwd_rows (ramp / normalisation backward inside) + edge_bwd_node (one C-ABI call, two launches)"
    traffic = load_traffic(N, d, h) if not emu and world == 1 else {}
    # the roofline object describes ONE launch (so that its duration can be checked against the rocprofv3 kernel
    # stats under profiles/): the longest single kernel of the step
    dom = max((n for n in kern if "composite" not in kern[n]), key=lambda n: kern[n]["ms"])
    ROCPROF_NAME = {"allpairs_topk": "allpairs_topk_ranked<64>", "conv_bwd": "conv_bwd_node<64>", "spmm_fwd": "spmm_fwd_narrow<64>"}
    for v in kern.values():
        v["GBps"] = v["compulsory"] / (v["ms"] * 1e-3) / 1e9
        v["gather_GBps"] = v["gathered"] / (v["ms"] * 1e-3) / 1e9
    pairs = float(rows_loc) * N
    t_pair = tk["allpairs_topk"]

    # ---- the ranked search's walk, MEASURED on this run's data (not a literal): one probe launch over every row
    walk = None
    if noise_mode == ops.NOISE_RANKED and lay is None:            # (the probe walks the 64-rank list)
        walk = ops.ranked_probe(sv["xp"], sv["k"], layer.t, (1234, 0), rows=(r0, r1))
    # ---- data regimes: the same step on features scaled x4 / x16 and on clustered data.  Per regime: the measured walk (every 16th
    # row, no budget), the PILOT's estimate (~1000 sampled rows, 64-block budget: what DGG_LearnableK_debug runs under
    # args.dgg_asym_generator = "auto"), the step time under the ranked generator and, for comparison, the pair stage of the per-pair
    # hash evaluator (guess-and-verify) on the same data: it depends on the regime as much and is slower wherever the ranked search is.
    regimes = None
    if world == 1 and not force and not emu and a.variants and noise_mode == ops.NOISE_RANKED:
        regimes = {}
        for name, (fs_, dat_) in {"randn_x1": (1.0, "randn"), "randn_x4": (4.0, "randn"), "randn_x16": (16.0, "randn"),
                                   "clustered": (1.0, "clustered")}.items():
            try:
                rr = SyntheticRun(a, dev, 1, 0, False, N, d, h, ops.NOISE_RANKED, feat_scale=fs_, data=dat_)
                xp_r = ops.linear_fwd(rr.x_local, rr.P["We"], rr.P["be"], ops.ACT_LEAKY)
                pilot = ops.ranked_probe(xp_r, None, rr.layer.t, (1234, 0), stride=max(1, N // 1024), max_blocks=64)
                est = ops.ranked_cost_estimate(pilot, N)
                meas = ops.ranked_probe(xp_r, None, rr.layer.t, (1234, 0), stride=16)
                nst = 3 if meas["blocks_per_row"] > 50 else 10
                rr.step(0)
                torch.cuda.synchronize()
                t0_ = time.perf_counter()
                for s_ in range(nst):
                    rr.step(s_ % NGRAPH)
                torch.cuda.synchronize()
                ms_ranked = (time.perf_counter() - t0_) / nst * 1e3
                kk = rr.layer.saved["k"]
                ops.allpairs_topk(xp_r, 64, noise_mode=ops.NOISE_HASH, seed=(1234, 0), algo=4, k_limit=kk)
                torch.cuda.synchronize()
                t0_ = time.perf_counter()
                ops.allpairs_topk(xp_r, 64, noise_mode=ops.NOISE_HASH, seed=(1234, 1), algo=4, k_limit=kk)
                torch.cuda.synchronize()
                ms_hash_pair = (time.perf_counter() - t0_) * 1e3
                ops.PROBE = {}
                rr.step(0)
                torch.cuda.synchronize()
                pv, ops.PROBE = ops.PROBE, None
                e0, e1 = pv["allpairs_topk"][0]
                regimes[name] = {"feat_scale": fs_, "data": dat_, "pilot": pilot, "pilot_estimate_ms": est * 1e-3,
                                 "measured_walk_every_16th_row": meas, "ms_per_step_ranked": ms_ranked,
                                 "pair_stage_ms_ranked": e0.elapsed_time(e1), "pair_stage_ms_hash_guess_and_verify": ms_hash_pair,
                                 # nearest-neighbour bound in the walk's stop tests (dgg_allpairs_rowmin_bound; its sweep is inside
                                 # pair_stage_ms_ranked when on): decided by the layer's own pilot walk
                                 "row_bound_on": bool(rr.layer._tight_on), "row_bound_pilot": rr.layer.tight_probe}
                del rr, xp_r
                torch.cuda.empty_cache()
            except Exception as e:  # noqa: BLE001
                regimes[name] = {"error": repr(e)}

    # ---- variants of the same step ("and a symmetric run", "also report h=128"; the reference script's own defaults
    # are perturb_edge_prob=False / symmetric_noise=True, train_small_graphs.py:153-163): one window each, eager launches
    variants = None
    if world == 1 and not force and not emu and a.variants:
        variants = {}
        vsteps = max(5, a.steps // 2)
        for name, (nm, lat, xg) in {"symmetric": (ops.NOISE_RANKED_SYM, h, False), "hash_symmetric": (ops.NOISE_HASH_SYM, h, False),
                                    "unperturbed": (ops.NOISE_NONE, h, False),
                                    "hash_asymmetric": (ops.NOISE_HASH, h, False), "latent128": (noise_mode, 128, False),
                                    "x_grad": (noise_mode, h, True)}.items():
            try:
                rv = SyntheticRun(a, dev, 1, 0, False, N, d, lat, nm, xg)
                for s_ in range(2):
                    rv.step(s_)
                torch.cuda.synchronize()
                # like the headline: captured once per seed and replayed (two seeds alternate); eager launches if the capture fails
                vgraphs = None
                if a.hipgraph:
                    try:
                        vgraphs = []
                        for s_ in range(2):
                            gph = torch.cuda.CUDAGraph()
                            with torch.cuda.graph(gph):
                                rv.step(s_)
                            vgraphs.append(gph)
                        for gph in vgraphs:
                            gph.replay()
                        torch.cuda.synchronize()
                    except Exception as e:  # noqa: BLE001
                        print(f"variant {name}: hipGraph capture failed ({e!r}); timing eager launches", file=sys.stderr)
                        vgraphs = None
                tws = []
                for _w in range(7):                                 # median of seven windows
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for s_ in range(vsteps):
                        if vgraphs is not None:
                            vgraphs[s_ % 2].replay()
                        else:
                            rv.step(s_ % NGRAPH)
                    torch.cuda.synchronize()
                    tws.append((time.perf_counter() - t0) / vsteps)
                tv = float(np.median(tws))
                vgraphs = None
                ops.PROBE = {}
                rv.step(0)
                torch.cuda.synchronize()
                pv, ops.PROBE = ops.PROBE, None
                e0, e1 = pv["allpairs_topk"][0]
                rv.layer.check_generator()
                kv = float(rv.layer.saved["k"].mean().item())
                pk = e0.elapsed_time(e1)
                variants[name] = {"ms_per_step": tv * 1e3, "edges_per_s": N * kv / tv, "pair_kernel_ms": pk, "steps": vsteps,
                                  "window_ms_min_median_max": [min(tws) * 1e3, tv * 1e3, max(tws) * 1e3],
                                  "note": "ms_per_step: median of seven windows of hipGraph replay (two seeds alternating); pair_kernel_ms: events around the C-ABI call in one eager step"}
                # roofline of the pair stage of the variants that sweep all N^2 pairs (one C-ABI call = several launches, event-timed as a
                # whole; per-launch durations: profiles/r03_*_kernel_stats.csv)
                if name == "unperturbed":
                    flop = 2.0 * N * float(N) * lat                # ALGORITHMIC: one h-long dot product per ordered pair
                    variants[name]["roofline"] = {
                        "bound": "mfma", "kernel": "pair stage: sw_prep + sw_pilot + sw_sweep<A> + sw_select + sw_sweep<B> + sw_finalize (+ fallback)",
                        "achieved": flop / (pk * 1e-3) / 1e12, "peak": BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": flop / (pk * 1e-3) / 1e12 / BF16_PEAK_TFLOPS,
                        "algorithmic_flop": flop, "executed_mfma_flop": 2.0 * N * float(N) * (lat + 16), "traffic": None,
                        "note": "algorithmic flop = 2 N^2 h (the bf16 Gram bound of every ordered pair); executed = 2 N^2 (h + 16): the K-step "
                                "that folds the norms and the row's radius into the accumulator; the two sweeps alone: see "
                                "profiles/r03_unperturbed_kernel_stats.csv"}
                elif name == "symmetric":
                    # ranked symmetric generator (the product default for symmetric_noise=True): owners walk their largest noises,
                    # score each emitted pair once (one gathered row of xp), rows merge.  Counters from one call with statistics on.
                    os.environ["DGG_RSYM_STATS"] = "1"
                    sv = rv.layer.saved
                    _, _, ws_ = ops.allpairs_topk(sv["xp"], 64, noise_mode=nm, seed=(1234, 0), return_ws=True, k_limit=sv["k"])
                    st_ = ops.rsym_status(ws_, N)
                    os.environ.pop("DGG_RSYM_STATS", None)
                    del ws_
                    comp = N * 4.0 * lat + N * 64 * 8.0
                    gath = (st_["emitted"] + st_["tier2_delivered"]) * 4.0 * lat
                    variants[name]["roofline"] = {
                        "bound": "hbm", "kernel": "pair stage: rs_pilot + rs_emit<1> + rs_finalize + rs_emit<2> + rs_finalize2 (+ tier 3)",
                        "achieved": comp / (pk * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": comp / (pk * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                        "algorithmic_bytes": comp, "gathered_bytes": gath, "gather_GBps": gath / (pk * 1e-3) / 1e9,
                        "frac_gather_ceiling": gath / (pk * 1e-3) / 1e9 / GATHER_CEILING_GBPS, "traffic": None,
                        "scored_pairs_per_row": st_["emitted"] / N, "inbox_deliveries_per_row": st_["delivered"] / N,
                        "tier2_rows": st_["tier2_rows"], "tier3_rows": st_["tier3_rows"],
                        "note": "frac = compulsory bytes (xp once + idx/val) / event-timed pair stage / 8 TB/s; the stage is a random-row "
                                "gather (one 4h-byte row per scored pair, every unordered pair scored ONCE for both endpoints) plus one "
                                "memory-side atomic per inbox delivery and a second, deeper walk for the rows that fail verification"}
                elif name in ("hash_symmetric", "hash_asymmetric"):
                    npair = N * float(N) * (0.5 if name == "hash_symmetric" else 1.0)
                    floor_s = npair / 64.0 * HASH_CYCLES_PER_WAVE_COLUMN / SIMD_CYCLES_PER_S
                    variants[name]["roofline"] = {
                        "bound": "valu", "kernel": "pair stage: gv_pilot + gv_sweep" + ("_tri" if name == "hash_symmetric" else "") + " + gv_finalize",
                        "achieved": npair / (pk * 1e-3) / 1e12, "peak": npair / floor_s / 1e12, "unit": "Tpair/s (hash + compare)",
                        "frac": floor_s / (pk * 1e-3), "algorithmic_pairs": npair, "traffic": None,
                        "note": "integer-VALU bound: every (unordered, for symmetric noise) pair costs one 6-instruction hash + compare per "
                                "64 pairs and wavefront; peak = the measured hashing floor of 21 cycles per wavefront-column on 1024 SIMDs "
                                "at 2.4 GHz; frac = floor time / event-timed pair stage"}
                del rv
                torch.cuda.empty_cache()
            except Exception as e:  # noqa: BLE001
                variants[name] = {"error": repr(e)}

    if rank == 0:
        out.update({
            # dominant kernel BY TIME of the step (an O(N*K) gather kernel since the pair stage became O(N*150))
            "roofline": {"bound": "hbm", "kernel": dom, "rocprof_kernel": ROCPROF_NAME.get(dom), "achieved": kern[dom]["GBps"], "peak": HBM_PEAK_GBPS,
                         "unit": "GB/s", "frac": kern[dom]["GBps"] / HBM_PEAK_GBPS, "traffic": traffic.get(dom) if lay is None else None,
                         "traffic_source": (traffic.get("_source") if (lay is None and traffic.get(dom) is not None) else None),
                         "kernel_ms": kern[dom]["ms"], "algorithmic_bytes": kern[dom]["compulsory"],
                         "gathered_bytes": kern[dom]["gathered"], "gather_GBps": kern[dom]["gather_GBps"],
                         "gather_ceiling_GBps": GATHER_CEILING_GBPS, "frac_gather_ceiling": kern[dom]["gather_GBps"] / GATHER_CEILING_GBPS,
                         "note": "frac = SURVEY 8(d) compulsory bytes (every array touched once) / event-timed duration / 8 TB/s; the kernel "
                                 "is a random-row gather from an Infinity-Cache-resident 25.6 MB table, whose ceiling is the guide's "
                                 "measured 8.6 TB/s (MI355X_MICROARCH.md, 'Indexed rows'): frac_gather_ceiling counts every gathered row "
                                 "once per use against that; traffic = fabric bytes per launch from the rocprofv3 PMC passes, NOT measured "
                                 "in this run: replayed from the committed file named in traffic_source (null when there is none for "
                                 "this shape)"},
            "kernels": {n_: {"ms": v["ms"], "GBps": v["GBps"], "frac_hbm": v["GBps"] / HBM_PEAK_GBPS, "gather_GBps": v["gather_GBps"],
                             "frac_gather_ceiling": v["gather_GBps"] / GATHER_CEILING_GBPS, "fabric_bytes_per_launch": traffic.get(n_),
                             **({"composite": v["composite"]} if "composite" in v else {})} for n_, v in kern.items()},
            # the whole-step fractions it asks to be published, labelled.  F = 232 flop/pair over all N^2 pairs (the
            # dense formulation's arithmetic), B = compulsory bytes (12 kB per node: every array touched once), B_virt = the N^2 fp32
            # score matrix scanned once.  T_roof = F/P_fp32 + B/BW_HBM is the roofline time of the DENSE formulation; this build's
            # search never executes the unreachable pairs, so T < T_roof (a fraction above 1 is NOT a kernel-efficiency claim).
            "survey_8d": {"F_flop": FLOP_PER_PAIR * N * float(N), "B_bytes": 12e3 * N * (d / 128.0), "B_virt_bytes": 4.0 * N * float(N),
                          "T_s": T, "T_roof_dense_s": FLOP_PER_PAIR * N * float(N) / (FP32_PEAK_TFLOPS * 1e12) + 12e3 * N / (HBM_PEAK_GBPS * 1e9),
                          "frac_dense_roofline": (FLOP_PER_PAIR * N * float(N) / (FP32_PEAK_TFLOPS * 1e12) + 12e3 * N / (HBM_PEAK_GBPS * 1e9)) / T,
                          "frac_hbm_compulsory": 12e3 * N / T / (HBM_PEAK_GBPS * 1e9),
                          "frac_hbm_virtual_stream": 4.0 * N * float(N) / T / (HBM_PEAK_GBPS * 1e9),
                          "frac_hbm_gathered": sum(v["gathered"] for v in kern.values()) / T / (HBM_PEAK_GBPS * 1e9),
                          "note": "whole-step figures against the DENSE formulation's bounds; frac_hbm_compulsory is the honest HBM fraction "
                                  "of the step (every array once); frac_hbm_gathered counts the gathered rows of the gather kernels once "
                                  "per use over the whole step time"},
            "pair_stage": {"kernel": "allpairs_topk(" + a.noise + ")", "kernel_ms": t_pair * 1e3, "pairs_per_s": pairs / t_pair,
                           "measured_walk": walk,
                           "note": "measured_walk: dgg_allpairs_ranked_probe over EVERY row of this run's projected features (blocks of 64 "
                                   "ranks visited, candidate rows gathered, candidates scored in full, per row): the ranked-noise search "
                                   "scores that many candidates per row, not N, so N^2 flop counts do not apply to it -- and the depth "
                                   "is a property of the DATA (see data_regimes); the kernels that sweep all N^2 pairs are the "
                                   "`symmetric` / `unperturbed` / `hash_asymmetric` variants"},
            "data_regimes": regimes,
            "variants": variants,
        })
        # ---- the other BASELINE.json configs, compact, in the SAME line (the driver runs only this default command): configs[1] Pubmed
        # shape through the drop-in modules, configs[4] PPI shape with bf16 layer products, configs[3]'s 500 000-node graph on one GPU
        if world == 1 and not force and not emu and a.configs and a.variants and N == 100_000:
            out["configs"] = other_configs(a, dev)
        if a.cpu_rows >= 0 and world == 1:
            cores = os.cpu_count() or 1
            crow = a.cpu_rows if a.cpu_rows > 0 else 64 * cores
            try:
                out["cpu_baseline"] = cpu_baseline(N, d, h, P, min(crow, N), cores, noise_mode)
            except Exception as e:  # the baseline leg must never take the measurement down
                out["cpu_baseline"] = {"value": None, "unit": "edges/s", "cores": os.cpu_count(), "kind": "port",
                                       "sample": f"failed: {e!r}"}
            if a.cpu_dense:
                # BASELINE.md section 3 sizes of the dense reference-shaped formulation (Cora-size edge list, 4 000-node all-pairs);
                # N = 19 717 runs with --workload pubmed.  Extrapolation to N = 100 000 from the all-pairs rate, labelled as such.
                # (32 threads: the [N,N] elementwise stages of these sizes do not scale beyond that; more threads only add overhead)
                dense = cpu_dense_formulation([("edgelist", 2708, d, h), ("allpairs", 4000, d, h)], min(cores, 32))
                out["cpu_baseline"]["dense_formulation"] = dense
                ap_ = [q for q in dense if q.get("candidates") == "allpairs" and "dense_entries_per_s" in q]
                if ap_:
                    out["cpu_baseline"]["dense_formulation_extrapolated_s_at_this_N"] = float(N) * N / ap_[0]["dense_entries_per_s"]
        emit_json((out))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
