"""Mini-batch samplers over one large graph: the reference's large-graph loops (train_large_graphs.py:402-421) draw their batches with
PyG's GraphSAINTRandomWalkSampler and ClusterLoader; PyG is not a dependency here, so the two are restated on the package's own kernels
(ops.random_walk_nodes, ops.induced_subgraph; include/dgg_hip_sampling.h).

    loader = RandomWalkSampler(adj, batch_size=2000, walk_length=4, num_steps=5)         # GraphSAINTRandomWalkSampler(data, ...)
    loader = ClusterSampler(adj, contiguous_parts(N, 500), batch_size=5)                 # ClusterLoader(ClusterData(data, 500), 5)
    for epoch in ...:
        loader.set_epoch(epoch)
        for batch in loader:
            x_b, y_b, mask_b = batch.take(x), batch.take(y), batch.take(train_mask)
            output, out_adj, _ = model(x_b, batch.adj)

`graph` is the WHOLE graph as a sparse COO tensor [N, N] (on the GPU for sampling); it is converted to CSR once, through csr_pattern and
its per-object cache.  A batch costs one kernel for the walks, a clear and four kernels for the cut with two torch.cumsum between
them, the gathers that dress the result as a sparse tensor, and ONE device read-back (the batch's node and edge counts: its tensors'
shapes).

    edited = batch.with_noise(noise_level, loader.noise_seed(batch.step), labels=y_b)     # add_noisy_edges + remove_interclass_edges
    output, out_adj, _ = model(x_b, edited.adj);  adjacency_mse_loss(out_adj, edited.target)

with_noise is the reference's per-batch edit (train_large_graphs.py:230-236) on the device (ops.batch_graph_edit,
include/dgg_hip_batch_graph.h): two kernels, two torch.cumsum and ONE more read-back (the edited graphs' entry counts).  Its noise is
a counter-based law keyed by noise_seed(step), a fixed function of (seed, epoch, step): every batch gets its own noise, where the
reference re-seeds numpy to 0 for every batch, and the realisation is that law's, not numpy's stream.

Not built (the reference loop never reads them, or the data is not available): GraphSAINT's node_norm / edge_norm coverage estimates
(sample_coverage), METIS partitioning (ClusterData) -- `parts` is the caller's, contiguous_parts is a stand-in that is NOT METIS --
and num_workers (the sampling runs on the device, on the caller's stream)."""
import torch

from . import ops
from .adjacency import CsrAdjacency, _cached, _seed_cache, csr_pattern

NOISE_STREAM = 0x6E6F6973          # folded into s1 by noise_seed: the noise of a step is not the stream its walks used


class SubgraphBatch:
    """One mini-batch: the sub-graph induced by `nodes`.
    nodes int64 [n] original ids, ascending (PyG's node_idx.unique() order) -- batch node i is original node nodes[i];
    adj sparse COO float32 [n, n], coalesced by construction (sorted unique indices), values = the graph's stored values: what the
    models take as in_adj; edge_index int64 [2, e] = adj.indices(); eid int64 [e] the position of every batch edge among the graph's
    coalesced entries (gathers edge weights or per-edge features: w[eid]); sub: the ops.InducedSubgraph it was built from (CSR arrays,
    bdeg = the prior degrees csr_candidates would compute for adj); step: the batch's number in its epoch (None when built by hand)."""

    def __init__(self, sub, values, step=None):
        self.sub = sub
        self.step = step
        self.nodes = sub.orig.long()
        self.eid = sub.beid
        self.edge_index = torch.stack([sub.brow.long(), sub.bcol.long()])
        self.adj = torch.sparse_coo_tensor(self.edge_index, values[sub.beid], (sub.n, sub.n), is_coalesced=True)
        self.num_nodes, self.num_edges = sub.n, sub.e

    def take(self, t):
        """t[nodes]: the batch's rows of a per-node tensor of the whole graph (features, labels, masks)"""
        return t[self.nodes]

    def with_noise(self, noise_level, seed, labels=None):
        """The batch with the reference's noisy edges, and the supervision target of its adjacency loss when `labels` (integer [n], the
        batch nodes' classes) are given -> EditedBatch.  Each off-diagonal pair that is not an edge becomes one of value 1 with
        probability 10 * noise_level (the reference's factor, utils.py:93; clipped to [0, 1]), a fixed function of seed = (s0, s1): a
        sampler's noise_seed(batch.step).  On the device, on the caller's stream, one read-back (ops.batch_graph_edit)."""
        p = min(max(10.0 * float(noise_level), 0.0), 1.0)
        return EditedBatch(self, ops.batch_graph_edit(self.sub.browptr, self.sub.bcol, self.adj._values(), p, seed, labels))


class EditedBatch:
    """A SubgraphBatch after with_noise.  nodes, take, num_nodes, step as there; num_edges counts the noisy entries too.
    adj sparse COO float32 [n, n], coalesced by construction: the batch's stored entries with their values plus the noisy entries with
    value 1; edge_index int64 [2, e] = adj.indices(); is_noise bool [e]; eid int64 [e]: the position of a stored entry among the whole
    graph's coalesced entries (the source batch's eid), -1 for a noisy entry; target: the CsrAdjacency of the entries of adj between
    nodes of one label, every value 1 (remove_interclass_edges(adj, labels); adjacency_mse_loss takes it as it is), None without
    labels; edit: the ops.EditedBatchGraph.
    csr_pattern(adj) and csr_candidates(adj) (and the float32 values) are seeded with the kernel's own CSR arrays: the first use of adj
    coalesces and converts nothing."""

    def __init__(self, batch, edit):
        self.source, self.edit = batch, edit
        self.nodes, self.step = batch.nodes, batch.step
        self.num_nodes, self.num_edges = edit.n, edit.e
        self.edge_index = torch.stack([edit.nrow.long(), edit.ncol.long()])
        self.adj = torch.sparse_coo_tensor(self.edge_index, edit.nval, (edit.n, edit.n), is_coalesced=True)
        self.is_noise = edit.nsrc < 0
        if batch.eid.shape[0] == 0:                    # (nothing to gather from: every entry is noise)
            self.eid = torch.full_like(edit.nsrc, -1)
        else:
            self.eid = torch.where(self.is_noise, edit.nsrc, batch.eid[edit.nsrc.clamp(min=0)])
        self.target = None
        if edit.trowptr is not None:
            self.target = CsrAdjacency(edit.trowptr, edit.tcol, edit.trow, torch.ones(edit.e_t, device=edit.nval.device), edit.n)
        # row sums as csr_candidates forms them: differences of a float64 running sum (deterministic)
        cs = torch.cat([edit.nval.new_zeros(1, dtype=torch.float64), edit.nval.double().cumsum(0)])
        deg = (cs[edit.nrowptr[1:]] - cs[edit.nrowptr[:-1]]).float()
        _seed_cache("pattern", self.adj, (edit.nrowptr, edit.ncol, edit.nrow))
        _seed_cache("candidates", self.adj, (edit.nrowptr, edit.ncol, deg))
        _seed_cache("values_f32", self.adj, edit.nval)

    def take(self, t):
        return t[self.nodes]


def _graph_csr(graph, who):
    """-> (rowptr int64 [N+1], col int32 [E], values float32 [E], N), converted once per graph object"""
    if not (torch.is_tensor(graph) and graph.is_sparse):
        raise TypeError(f"{who}: graph must be a sparse COO tensor [N, N] (the whole graph), got "
                        f"{'a dense tensor' if torch.is_tensor(graph) else type(graph).__name__}")
    if graph.ndim != 2 or graph.shape[0] != graph.shape[1]:
        raise ValueError(f"{who}: graph must be square [N, N], got {tuple(graph.shape)}")
    rowptr, col, _ = csr_pattern(graph)
    values = _cached("values_f32", graph, lambda: graph.coalesce().values().detach().to(torch.float32).contiguous())
    return rowptr, col, values, graph.shape[0]


def _generator(*key):
    """a CPU torch.Generator seeded from a tuple of non-negative ints (the same batches on every machine)"""
    s = 0
    for k_ in key:
        s = (s * 1000003 + int(k_) + 1) % (1 << 62)
    return torch.Generator().manual_seed(s)


class RandomWalkSampler:
    """GraphSAINTRandomWalkSampler(data, batch_size, walk_length, num_steps) (train_large_graphs.py:406-414): an iterable of `num_steps`
    batches per epoch.  A batch draws batch_size roots uniformly (with replacement, torch.Generator seeded from (seed, epoch, step)),
    walks walk_length steps from each on the device and takes the sub-graph induced by every visited node.  The batches are a fixed
    function of (seed, epoch, step); call set_epoch(e) before each epoch, or every epoch repeats the first."""

    def __init__(self, graph, batch_size, walk_length, num_steps, seed=0):
        self.rowptr, self.col, self.values, self.N = _graph_csr(graph, "RandomWalkSampler")
        if int(batch_size) < 1:
            raise ValueError(f"RandomWalkSampler: batch_size must be >= 1, got {batch_size}")
        if int(walk_length) < 0:
            raise ValueError(f"RandomWalkSampler: walk_length must be >= 0, got {walk_length}")
        if int(num_steps) < 1:
            raise ValueError(f"RandomWalkSampler: num_steps must be >= 1, got {num_steps}")
        if self.N < 1:
            raise ValueError("RandomWalkSampler: graph has no nodes")
        self.graph = graph                                 # (keeps the cached conversion alive)
        self.batch_size, self.walk_length, self.num_steps, self.seed, self.epoch = int(batch_size), int(walk_length), int(num_steps), int(seed), 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.num_steps

    def roots(self, step):
        """int32 [batch_size] on the CPU"""
        return torch.randint(0, self.N, (self.batch_size,), generator=_generator(self.seed, self.epoch, step), dtype=torch.int32)

    def walk_seed(self, step):
        """the (s0, s1) of the step's walks"""
        return self.seed & 0xffffffff, (self.epoch * 0x10001 + step) & 0xffffffff

    def noise_seed(self, step):
        """the (s0, s1) of the step's noisy edges (SubgraphBatch.with_noise): a fixed function of (seed, epoch, step), another stream
        than walk_seed's"""
        return self.seed & 0xffffffff, ((self.epoch * 0x10001 + step) ^ NOISE_STREAM) & 0xffffffff

    def batch(self, step):
        walk = ops.random_walk_nodes(self.rowptr, self.col, self.roots(step).to(self.rowptr.device), self.walk_length, self.walk_seed(step))
        # the node set is the walk's unique nodes: duplicates are left to the mark phase of the cut
        return SubgraphBatch(ops.induced_subgraph(self.rowptr, self.col, walk.reshape(-1), self.values), self.values, step=step)

    def __iter__(self):
        return (self.batch(step) for step in range(self.num_steps))


def contiguous_parts(N, num_parts):
    """The documented stand-in for ClusterData's METIS partition: node v belongs to part v * num_parts // N, i.e. num_parts runs of
    consecutive ids whose sizes differ by at most one.  It is NOT METIS: it minimises no edge cut, and is only as good as the locality
    of the node numbering.  -> int64 [N] on the CPU"""
    N, num_parts = int(N), int(num_parts)
    if num_parts < 1 or num_parts > max(N, 1):
        raise ValueError(f"contiguous_parts: num_parts must be in 1..N = {N}, got {num_parts}")
    return torch.arange(N, dtype=torch.int64) * num_parts // max(N, 1)


class ClusterSampler:
    """ClusterLoader(cluster_data, batch_size, shuffle) (train_large_graphs.py:416-421).  parts: int tensor [N], the cluster id of every
    node (the caller's partition; contiguous_parts is the stand-in where METIS is not available).  An epoch visits the clusters once, in
    a shuffled order (torch.Generator seeded from (seed, epoch)) or ascending id order; a batch is the union of `batch_size` of them
    (the last one of fewer) and, like ClusterLoader, keeps the edges BETWEEN its clusters."""

    def __init__(self, graph, parts, batch_size, shuffle=True, seed=0):
        self.rowptr, self.col, self.values, self.N = _graph_csr(graph, "ClusterSampler")
        if not torch.is_tensor(parts) or parts.dtype.is_floating_point or parts.ndim != 1 or parts.shape[0] != self.N:
            raise ValueError(f"ClusterSampler: parts must be an int tensor [N] = [{self.N}] of cluster ids, got "
                             f"{tuple(parts.shape) if torch.is_tensor(parts) else type(parts).__name__}")
        if int(batch_size) < 1:
            raise ValueError(f"ClusterSampler: batch_size must be >= 1, got {batch_size}")
        self.graph = graph
        self.batch_size, self.shuffle, self.seed, self.epoch = int(batch_size), bool(shuffle), int(seed), 0
        # once, on the host: the nodes sorted by cluster, and where each cluster starts
        p = parts.detach().cpu().long()
        order = torch.argsort(p, stable=True)
        _, counts = torch.unique_consecutive(p[order], return_counts=True)
        self.offsets = [0] + torch.cumsum(counts, 0).tolist()
        self.order = order.to(torch.int32).to(self.rowptr.device)
        self.num_clusters = len(self.offsets) - 1

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return (self.num_clusters + self.batch_size - 1) // self.batch_size

    def cluster_order(self):
        if not self.shuffle:
            return list(range(self.num_clusters))
        return torch.randperm(self.num_clusters, generator=_generator(self.seed, self.epoch)).tolist()

    def noise_seed(self, step):
        """the (s0, s1) of the noisy edges of the epoch's batch number `step` (by position in the epoch): RandomWalkSampler's function"""
        return self.seed & 0xffffffff, ((self.epoch * 0x10001 + step) ^ NOISE_STREAM) & 0xffffffff

    def batch_nodes(self, clusters):
        """int32 [M] on the graph's device: the members of the given clusters (slices of one device array: nothing is read back)"""
        return torch.cat([self.order[self.offsets[c]:self.offsets[c + 1]] for c in clusters])

    def __iter__(self):
        order = self.cluster_order()
        for step, s in enumerate(range(0, self.num_clusters, self.batch_size)):
            nodes = self.batch_nodes(order[s:s + self.batch_size])
            yield SubgraphBatch(ops.induced_subgraph(self.rowptr, self.col, nodes, self.values), self.values, step=step)
