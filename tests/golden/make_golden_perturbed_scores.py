#!/usr/bin/env python3
"""Golden fixtures of the PERTURBED edge probabilities returned as the adjacency: debug_step 1 (dgm.py:1233-1239) and the k-select
mode `edge_p-cdf` (dgm.py:1368-1401) of DGG_LearnableK_debug with perturb_edge_prob=True (dgm.py:1211-1229).

Companion of make_golden.py (runs only where the reference is available): the reference is imported through make_golden's own
shims, unmodified, and only data is stored -- inputs, state_dict, the injected noise G, the reference output and its gradients for
a fixed cotangent.  Graph of make_golden.scores_cases(): N=96, d=24, h=16, seed 19, row 0 wider than the 64-wide list.

The reference's output is dense here: every non-edge becomes 1e-8 exp(G) > 0.  The script asserts that these values stay below
1e-6 (Gumbel(0, 0.3) over 96^2 samples tops out near G = 2.7: ~1.5e-7) and stores the largest one in meta["off_pattern_max"].

    python tests/golden/make_golden_perturbed_scores.py      # writes tests/golden/scores_pert_*.npz
"""
import json
import os

import numpy as np

# importing make_golden imports the reference behind its shims (torch_geometric stubs, .cuda() no-op, np.float)
from make_golden import HERE, base_args, dgm, grid_gumbel, grid_normal, random_graph, torch

CASES = [
    ("debug1_uvdist_asym", dict(debug_step=1, dgg_mode_edge_net="u-v-dist"), False),
    ("cdf_uvdeg_sym", dict(dgg_mode_k_select="edge_p-cdf", dgg_mode_edge_net="u-v-deg", extra_edge_dim=2), True),
    ("debug1_edgeconv_asym", dict(debug_step=1, dgg_mode_edge_net="edge_conv"), False),
    ("cdf_uvdegdist_sym", dict(dgg_mode_k_select="edge_p-cdf", dgg_mode_edge_net="u-v-deg-dist", extra_edge_dim=3), True),
]


def scores_graph():
    """inputs of make_golden.scores_cases(), drawn in the same order from the same generator"""
    N, d, h = 96, 24, 16
    gen = torch.Generator().manual_seed(19)
    A = random_graph(N, 20, gen).to_dense()
    A[0, :] = (torch.rand(N, generator=gen) < 0.8).float()          # one row wider than the ELL width
    A[0, 0] = 1.0
    Wt = 0.5 + torch.rand(N, N, generator=gen)
    in_adj = (A * Wt).to_sparse().coalesce()
    x = torch.randn(N, d, generator=gen)
    cot = torch.from_numpy(grid_normal(161, (N, N)))
    return N, d, h, in_adj, x, cot


def main():
    N, d, h, in_adj, x, cot = scores_graph()
    Gasym = grid_gumbel(162, (N, N))
    Gsym = grid_gumbel(163, (N, N))
    Gsym = np.triu(Gsym, 1) + np.triu(Gsym, 1).T
    on = in_adj.to_dense() != 0
    old = np.load(os.path.join(HERE, "scores_debug0_uvdist.npz"))       # the unperturbed goldens' graph, bit for bit
    assert np.array_equal(old["x"], x.numpy()) and np.array_equal(old["adj_vals"], in_adj.values().numpy())
    assert np.array_equal(old["rows"], in_adj.indices()[0].numpy()) and np.array_equal(old["cols"], in_adj.indices()[1].numpy())
    for tag, kw, sym in CASES:
        a = base_args(perturb_edge_prob=True, symmetric_noise=sym, **kw)
        torch.manual_seed(1234)
        m = dgm.DGG_LearnableK_debug(in_dim=d, latent_dim=h, args=a)
        m.eval()
        Gt = torch.from_numpy(Gsym if sym else Gasym)
        if sym:                                                 # as run_dgg injects captured noise
            iu, ju = torch.triu_indices(N, N, 1)
            m.gumbel.sample = lambda shape, Gt=Gt, iu=iu, ju=ju: Gt[iu, ju]          # dgm.py:1220 draws len(i) values
        else:
            m.gumbel.sample = lambda shape, Gt=Gt: Gt.reshape(shape)                 # dgm.py:1226 draws [1,N,N]
        xr = x.clone().requires_grad_(True)
        out = m(xr, in_adj).to_dense()
        (out * cot).sum().backward()
        off = float(out.detach()[~on].abs().max())
        assert off < 1e-6, f"{tag}: a non-edge of the reference output carries {off:.3e}"
        assert (np.diag(Gsym) == 0).all()
        ii = in_adj.indices().numpy().astype(np.int32)
        fx = {"x": x.numpy(), "rows": ii[0], "cols": ii[1], "adj_vals": in_adj.values().numpy(), "out": out.detach().numpy(),
              "cot": cot.numpy(), "g.x": xr.grad.numpy(), "G": Gsym if sym else Gasym}
        for k_, v in m.state_dict().items():
            fx["p." + k_] = v.detach().numpy()
        for k_, p_ in m.named_parameters():
            fx["g." + k_] = p_.grad.numpy() if p_.grad is not None else np.zeros_like(p_.detach().numpy())
        meta = dict(name="scores_pert_" + tag, N=N, d=d, h=h, torch=torch.__version__, args=vars(a), off_pattern_max=off,
                    G_max=float(fx["G"].max()), reference="dgm.py:1211-1239, 1368-1401 DGG_LearnableK_debug.forward")
        fx["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        path = os.path.join(HERE, f"scores_pert_{tag}.npz")
        np.savez_compressed(path, **fx)
        print("scores_pert", tag, f"ok: off-pattern max {off:.3e}, G max {meta['G_max']:.3f}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
