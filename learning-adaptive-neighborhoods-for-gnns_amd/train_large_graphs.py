"""Harness counterpart of the reference's mini-batch script (train_large_graphs.py: `train_gcn_dgg` 221-260, `validate` / `test`
308-376, the loaders 402-421): GCN_DGG trained on sub-graphs of one large graph, every step supervised on the learned adjacency,
    loss = nll(output[mask], y_b[mask]) + W * mse(out_adj, remove_interclass_edges(batch_adj, y_b)),   W = 10000
with the batches drawn on the device (dgg_amd.sampling) instead of by PyG's GraphSAINTRandomWalkSampler / ClusterLoader, and the
adjacency term taken on sparse rows (adjacency_mse_loss) instead of on two dense [n_b, n_b] matrices.

    python -m dgg_amd.train_large_graphs --data pubmed --data_dir /path/to/planetoid --dataloader SAINT --epochs 5

DATA: the graph comes through dgg_amd.data.load_planetoid (the ind.<name>.* Planetoid files: cora, citeseer, pubmed; the reference
script reads Pubmed the same way, train_large_graphs.py:393-397).  Reddit, Flickr and the other PyG data sets of the reference script
are downloaded by torch_geometric there; neither PyG nor a download is available to this package, so they CANNOT be loaded here -- a
graph of that size has to be brought as Planetoid-format files.

Flags follow the reference script where it has them (--dataloader, --graphsaint_bs, --graphsaint_wl, --edge_noise_level, --model,
--epochs, --seed, --data) and train_small_graphs.py for everything the model constructors read (its parser is the base of this one).
New here, because the reference hard-codes them: --num_steps (GraphSAINT's num_steps=5), --cluster_parts / --cluster_bs (ClusterData's
num_parts=500, ClusterLoader's batch_size=5), --adj_loss_weight (the reference's constant 10000 is the default; 0 drops the term and
with it dgg_differentiable_adj, so the model stays on its fused layer), --batch_noise {host,device} (where a training batch gets its
noisy edges and its target; below).

What differs from the reference loop, deliberately:
  * the clusters are dgg_amd.sampling.contiguous_parts, NOT a METIS partition (not available);
  * a batch WITHOUT a training node contributes its adjacency term only (the reference's nll_loss of nothing is NaN); with
    --adj_loss_weight 0 such a batch is skipped;
  * check_ell_bound() runs before every optimiser step, as in train_small_graphs.py;
  * evaluation runs on the WHOLE graph (the public validation / test split), once per epoch, as the reference's `test` covers it;
  * noisy edges (--edge_noise_level > 0) are added per batch on the host, as the reference does (add_noisy_edges on the batch's
    scipy matrix): one extra device -> host copy of the batch's edge list per step.  0 keeps the step on the device.

--batch_noise device (the default, host, is the path above, unchanged): one batch.with_noise(edge_noise_level, loader.noise_seed(step),
labels) replaces both add_noisy_edges and remove_interclass_edges for the TRAINING batches (ops.batch_graph_edit,
include/dgg_hip_batch_graph.h).  No .cpu() call and no numpy work stays on the step: a batch costs two read-backs, one for the cut
and one for the edit.  The whole-graph evaluation adjacency stays on the host path.  Two deliberate deviations from the reference:
  * every batch gets its OWN noise, a fixed function of (seed, epoch, step); the reference's add_noisy_edges re-seeds numpy to 0 on
    every call, so every batch there gets the top-left corner of one and the same noise matrix;
  * the realisation is the header's counter-based law (each absent off-diagonal pair independently, with probability
    10 * edge_noise_level), not numpy's stream -- the trade data.add_noisy_edges(reference_stream=False) already makes."""
import random
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import data as D
from . import model as models
from . import ops
from . import train_small_graphs as S
from .adjacency import CsrAdjacency, EllAdjacency, adjacency_mse_loss
from .sampling import ClusterSampler, RandomWalkSampler, contiguous_parts


def build_parser():
    p = S.build_parser()                               # every flag the models and the DGG read, with the small-graph script's defaults
    p.set_defaults(adj_loss_weight=10000.0, epochs=5000, patience=2000)            # reference train_large_graphs.py:43, 57, 251
    p.add_argument("--dataloader", default="SAINT", choices=["SAINT", "Cluster"])
    p.add_argument("--graphsaint_bs", type=int, default=2000, help="roots per batch (GraphSAINTRandomWalkSampler batch_size)")
    p.add_argument("--graphsaint_wl", type=int, default=2, help="walk length")
    p.add_argument("--num_steps", type=int, default=5, help="batches per epoch of the SAINT loader (hard-coded 5 in the reference)")
    p.add_argument("--cluster_parts", type=int, default=500, help="number of clusters (ClusterData num_parts; contiguous runs of ids, not METIS)")
    p.add_argument("--cluster_bs", type=int, default=5, help="clusters per batch (ClusterLoader batch_size)")
    p.add_argument("--batch_noise", default="host", choices=["host", "device"],
                   help="where a training batch gets its noisy edges and its same-class target: host (numpy + torch, as the reference) or "
                        "device (one kernel pair, SubgraphBatch.with_noise)")
    p.add_argument("--print_batches", type=S.str2bool, default=False, help="one line per training batch (nodes, edges, nll, adjacency term)")
    return p


def make_loader(args, adj):
    if args.dataloader == "SAINT":
        return RandomWalkSampler(adj, batch_size=args.graphsaint_bs, walk_length=args.graphsaint_wl, num_steps=args.num_steps, seed=args.seed)
    return ClusterSampler(adj, contiguous_parts(adj.shape[0], min(args.cluster_parts, adj.shape[0])), batch_size=args.cluster_bs, shuffle=True,
                          seed=args.seed)


def noisy_batch_adj(batch, noise_level):
    """the batch graph with the reference's noisy edges (train_large_graphs.py:230-232), through the host as there"""
    if noise_level <= 0.0:
        return batch.adj
    ei = batch.edge_index.cpu().numpy()
    rows, cols, vals = D.add_noisy_edges(ei[0].astype(np.int32), ei[1].astype(np.int32), batch.num_nodes, noise_level)
    ind = torch.from_numpy(np.stack([rows, cols]).astype(np.int64))
    return torch.sparse_coo_tensor(ind, torch.from_numpy(vals), (batch.num_nodes, batch.num_nodes)).coalesce().to(batch.adj.device)


def train_gcn_dgg(args, model, opt, loader, x, y, train_mask, epoch, writer=None):
    """one epoch over the loader (reference train_large_graphs.py:221-260) -> (loss weighted by the batches' training nodes, the
    adjacency term of every batch that took a step)"""
    model.train()
    loader.set_epoch(epoch)
    W = args.adj_loss_weight
    total_loss = total_examples = 0
    terms = []
    for step, batch in enumerate(loader):
        x_b, y_b, mask = batch.take(x), batch.take(y), batch.take(train_mask)
        edited = None
        if args.batch_noise == "device":
            edited = batch.with_noise(args.edge_noise_level, loader.noise_seed(step), labels=y_b if W > 0.0 else None)
            batch_adj, edge_index = edited.adj, edited.edge_index
        else:
            batch_adj, edge_index = noisy_batch_adj(batch, args.edge_noise_level), batch.edge_index
        num_nodes = int(mask.sum())
        if num_nodes == 0 and W <= 0.0:
            continue                                   # nothing to learn from: no training node and no adjacency term
        opt.zero_grad()
        with ops.step_zero_pool(x.device, batch.num_nodes, 64, max(args.hidden, 64), list(model.parameters())):
            if W > 0.0:
                gt = D.remove_interclass_edges(batch_adj, y_b) if edited is None else edited.target
                out, out_adj = S.forward(model, x_b, batch_adj, with_adj=True, edge_index=edge_index, epoch=epoch, writer=writer)
                if not isinstance(out_adj, (EllAdjacency, CsrAdjacency)):
                    raise NotImplementedError(f"--adj_loss_weight: {args.model} returns no learned adjacency (got {type(out_adj).__name__})")
                adj_term = adjacency_mse_loss(out_adj, gt)
                loss = W * adj_term if num_nodes == 0 else F.nll_loss(out[mask], y_b[mask]) + W * adj_term
            else:
                adj_term = None
                out = S.forward(model, x_b, batch_adj, edge_index=edge_index, epoch=epoch, writer=writer)
                loss = F.nll_loss(out[mask], y_b[mask])
            loss.backward()
        for dg in getattr(model, "dggs", []):          # BEFORE the optimiser step, as train_small_graphs.py does
            if hasattr(dg, "check_ell_bound"):
                dg.check_ell_bound()
        opt.step()
        weight = max(num_nodes, 1)
        total_loss += float(loss.detach()) * weight
        total_examples += weight
        if adj_term is not None:
            terms.append(float(adj_term.detach()))
        if args.print_batches:
            print("  batch:{:03d} nodes:{} edges:{} train nodes:{} loss:{:.6f}".format(step, batch.num_nodes, batch.num_edges, num_nodes, float(loss.detach())),
                  *(() if adj_term is None else ("adj loss:{:.9e}".format(float(adj_term.detach())),)))
    return (total_loss / total_examples if total_examples else float("nan")), terms


@torch.no_grad()
def evaluate(model, x, y, adj, idx):
    """accuracy and nll on the nodes `idx` of the whole graph (reference `test`, train_large_graphs.py:339-374)"""
    model.eval()
    out = S.forward(model, x, adj)
    return float(F.nll_loss(out[idx], y[idx])), S.accuracy(out[idx], y[idx])


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.adj_loss_weight > 0.0:
        args.dgg_differentiable_adj = True     # the loss reaches the generator through the returned adjacency (GCN_DGG: separate modules)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    device = torch.device("cuda")
    d = D.load_planetoid(args.data, args.data_dir, cache_dir=args.cache_dir)
    x = torch.from_numpy(d["x"]).to(device)
    y = torch.from_numpy(d["y"]).to(device)
    idx = {k: torch.from_numpy(d[k]).to(device) for k in ("train_idx", "val_idx", "test_idx")}
    train_mask = torch.zeros(x.shape[0], dtype=torch.bool, device=device)
    train_mask[idx["train_idx"]] = True
    graph = S.make_adjacency(d, 0.0, device)                                   # the loaders sample the graph itself; noise is added per batch
    adj_eval = S.make_adjacency(d, args.edge_noise_level, device)              # ... and once for the whole-graph evaluation
    loader = make_loader(args, graph)
    model = models.__dict__[args.model](nfeat=x.shape[1], nlayers=args.layer, nhidden=args.hidden, nclass=d["num_classes"],
                                        dropout=args.dropout, lamda=args.lamda, alpha=args.alpha, variant=args.variant,
                                        args=args).to(device)
    # optimiser groups by model-name substring, as train_small_graphs.py (reference train_large_graphs.py:471-490)
    if "GCN" in args.model and "II" in args.model:
        opt = torch.optim.Adam([{"params": model.params1, "weight_decay": args.wd1},
                                {"params": model.params2, "weight_decay": args.wd2}], lr=args.lr)
    elif "GCN" in args.model:
        opt = torch.optim.Adam([dict(params=model.params1, weight_decay=5e-4), dict(params=model.params2, weight_decay=0)], lr=args.lr)
    elif "GAT" in args.model:
        opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    writer = S.make_writer(args.log_dir) if args.log_dir else None
    t0 = time.time()
    history = []
    for epoch in range(args.epochs):
        loss_train, terms = train_gcn_dgg(args, model, opt, loader, x, y, train_mask, epoch, writer)
        lv, av = evaluate(model, x, y, adj_eval, idx["val_idx"])
        _, at = evaluate(model, x, y, adj_eval, idx["test_idx"])
        history.append(loss_train)
        print("Epoch:{:04d}".format(epoch + 1), "train", "loss:{:.3f}".format(loss_train),
              *(("adj loss:{:.6e}".format(sum(terms) / len(terms)),) if terms else ()),
              "| val loss:{:.3f} acc:{:.2f}".format(lv, 100 * av), "| test acc:{:.2f}".format(100 * at))
        if writer is not None:
            writer.add_scalar("train/loss", loss_train, epoch)
            writer.add_scalar("test/acc", at, epoch)
    if writer is not None:
        writer.close()
    print("Train cost: {:.4f}s".format(time.time() - t0))
    return history


if __name__ == "__main__":
    main()
