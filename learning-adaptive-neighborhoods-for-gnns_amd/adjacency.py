"""Sparse adjacency containers exchanged between the DGG and the graph-conv layers.

The reference passes torch sparse COO [N,N] tensors and densifies them at every hand-over
(model.py:1249-1251, 1264, 1274; dgm.py:1298).  Here the learned graph stays in a fixed-width ELL layout
(idx int32 [N,K], values fp32 [N,K]) end to end; `.to_dense()` / `.to_sparse()` exist so that reference-style
callers (`unnorm_adj.to_dense()`, model.py:1274) keep working on small graphs.
"""
import torch

from . import ops


class AllPairs:
    """Candidate set = every ordered pair (the reference equivalent is a complete in_adj whose row sums are the
    prior degrees): carries the prior-degree vector read by the k-net (dgm.py:1568).

    prior (optional): the input graph itself, a sparse COO [N, N] tensor (a dense one is converted once) -- the reference equivalent
    is then the complete in_adj whose stored values are the prior's, zero for non-edges, so what reads the graph (the scorer
    u-v-A_uv, dgm.py:1628-1644; the k-net gcn-x-deg, dgm.py:1528-1540) runs on all-pairs candidates: the generator may pick edges
    outside the graph and still sees, for every pair, whether the graph has it.  A stored value of exactly 0 means the same as an
    absent entry.  The prior is coalesced here (duplicates summed) and kept in CSR form on the object (prior_csr()), and it is used AS
    GIVEN: the models pass an AllPairs through unchanged, without adding self loops (from_graph(..., self_loops=True) adds them)."""

    def __init__(self, prior_degree, prior=None):
        self.prior_degree = prior_degree
        n = prior_degree.shape[0]
        self.shape = (n, n)
        self.device = prior_degree.device
        self.prior = None
        self._prior_csr = None
        if prior is not None:
            if tuple(prior.shape) != (n, n):
                raise ValueError(f"AllPairs: prior must be [N, N] = {(n, n)} for prior_degree of shape {tuple(prior_degree.shape)}, "
                                 f"got {tuple(prior.shape)}")
            if prior.device != prior_degree.device:
                raise ValueError(f"AllPairs: prior is on {prior.device} but prior_degree (shape {tuple(prior_degree.shape)}; prior shape "
                                 f"{tuple(prior.shape)}) is on {prior_degree.device}")
            self.prior = (prior if prior.is_sparse else prior.to_sparse()).detach().coalesce()
            self.prior_csr()

    @classmethod
    def from_graph(cls, in_adj, self_loops=False):
        """All-pairs candidates that see the graph `in_adj` (sparse COO or dense [N, N]): prior = in_adj, plus the identity when
        self_loops (the reference's in_adj + I, model.py:1249-1251); prior_degree = the prior's row sums as csr_candidates computes
        them."""
        a = (in_adj if in_adj.is_sparse else in_adj.to_sparse()).detach()
        if self_loops:
            n = a.shape[0]
            eye = torch.arange(n, device=a.device)
            a = a + torch.sparse_coo_tensor(torch.stack([eye, eye]), torch.ones(n, device=a.device, dtype=a.dtype), a.shape)
        a = a.coalesce()
        return cls(csr_candidates(a)[2], prior=a)

    def prior_csr(self):
        """the prior as (rowptr int64 [N+1], col int32 [E] strictly ascending within a row, values float32 [E], erow int32 [E]);
        built on first use and cached on the object: a later forward launches nothing for it"""
        if self.prior is None:
            return None
        if self._prior_csr is None:
            ind = self.prior.indices()
            rowptr = torch._convert_indices_from_coo_to_csr(ind[0], self.shape[0], out_int32=False)
            col, val = ind[1].to(torch.int32).contiguous(), self.prior.values().to(torch.float32).contiguous()
            if col.shape[0] == 0:                # (an empty tensor has no data pointer: one entry that no row points into)
                col, val = col.new_zeros(1), val.new_zeros(1)
            self._prior_csr = (rowptr, col, val, ind[0].to(torch.int32).contiguous())
        return self._prior_csr


class EllAdjacency:
    """Row-major fixed-width sparse matrix: entry (i, idx[i,r]) = values[i,r]; idx == -1 marks padding.
    layout (ops.ChunkLayout, optional): CHUNKED rows -- the learned degrees of an all-pairs graph outgrew the 64-rank list, so row i is
    the chunks [cptr[i], cptr[i+1]) of idx / values [chunks,64] (rank r of the row = entry r % 64 of its chunk r / 64); the reference
    has no width limit (dense [N,N] rows, dgm.py:1402-1421)."""

    def __init__(self, idx, values, n_cols, rs=None, k=None, score=None, normalized=False, part=None, owner=None, partp=None, layout=None):
        self.idx, self._values, self.n_cols = idx, values, n_cols
        self.layout = layout if (layout is not None and layout.wide) else None
        # (payload partition, row sums of the unnormalised weights) when `values` are the normalised values that partition was
        # built with (DGG_LearnableK_debug.forward_conv): the backward of A @ X then runs by destination, without atomics
        self.partp = partp
        self.owner = owner          # the DGG module that produced it (its ELL-width bound is checked when the matrix is densified)
        self.rs, self.k, self.score, self.normalized = rs, k, score, normalized
        self.part = part            # destination-ordered partition of the active entries (ops.part_build), if one was built
        self.shape = (idx.shape[0] if self.layout is None else self.layout.rows, n_cols)
        self.device = idx.device

    # --- reference-style accessors ---------------------------------------------------------------------------
    def values(self):
        return self._values

    def ell(self):
        return self.idx, self._values

    def coalesce(self):
        return self

    def to_dense(self):
        """Differentiable densification (small graphs / tests only)."""
        if self.owner is not None:
            self.owner.check_ell_bound()
        valid = self.idx >= 0
        cols = self.idx.clamp(min=0).long()
        out = torch.zeros(self.shape, device=self.device, dtype=self._values.dtype)
        vals = torch.where(valid, self._values, torch.zeros_like(self._values))
        if self.layout is not None:              # chunked rows: a chunk's entries land in the row of its node
            rows = self._chunk_rows().unsqueeze(1).expand_as(self.idx)
            return out.index_put((rows.reshape(-1), cols.reshape(-1)), vals.reshape(-1), accumulate=True)
        return out.scatter_add(1, cols, vals)

    def _chunk_rows(self):
        return self.layout.cnode.long()[:self.idx.shape[0]]

    def to_sparse(self):
        if self.owner is not None:
            self.owner.check_ell_bound()
        valid = self.idx >= 0
        base = torch.arange(self.shape[0], device=self.device) if self.layout is None else self._chunk_rows()
        rows = base.unsqueeze(1).expand_as(self.idx)[valid]
        return torch.sparse_coo_tensor(torch.stack([rows, self.idx[valid].long()]), self._values[valid], self.shape)

    def to_csr(self):
        """CsrAdjacency with the stored entries (idx >= 0) as its pattern and the same (differentiable) values: rows of any width for
        the layers that take the learned graph as a separate module"""
        valid = self.idx >= 0
        base = torch.arange(self.idx.shape[0], device=self.device) if self.layout is None else self._chunk_rows()
        erow = base.unsqueeze(1).expand_as(self.idx)[valid]
        rowptr = torch.zeros(self.shape[0] + 1, device=self.device, dtype=torch.int64)
        rowptr[1:] = torch.bincount(erow, minlength=self.shape[0]).cumsum(0)
        return CsrAdjacency(rowptr, self.idx[valid].contiguous(), erow.to(torch.int32).contiguous(), self._values[valid], self.shape[0], k=self.k)

    # --- fast path -------------------------------------------------------------------------------------------
    def row_sums(self):
        if self.rs is None:
            per = self._values.detach().sum(1)
            self.rs = per if self.layout is None else torch.zeros(self.shape[0], device=self.device, dtype=per.dtype).index_add_(0, self._chunk_rows(), per)
        return self.rs

    def normalize(self):
        """D^-1/2 A D^-1/2 with ROW sums on both sides (normalize_adj, model.py:1205-1219)."""
        if self.layout is not None:              # chunked rows as a separate module: the CSR kernels (rows of any width)
            return self.to_csr().normalize()
        rs = self.row_sums()
        ahat = ops.EllNormalizeFn.apply(self._values, self.idx, rs, self.part)
        return EllAdjacency(self.idx, ahat, self.n_cols, rs=None, k=self.k, score=self.score, normalized=True, part=self.part,
                            owner=self.owner)

    def matmul(self, X, act=ops.ACT_NONE):
        """act(A @ X) (torch.mm(adj, x), model.py:594; act = ReLU fuses GCNConv's activation into the aggregation)."""
        # weights produced by the DGG ramp: an exact zero is a saturated ramp whose gradient vanishes too
        if self.layout is not None and self.partp is None:
            if not ops.backward_will_follow(self._values, X):      # inference (no_grad / a hipGraph capture): the chunked aggregation kernel
                return ops.spmm_fwd(self.idx, self._values.detach(), X.detach().contiguous(), act, layout=self.layout)
            out = self.to_csr().matmul(X)
            return torch.relu(out) if act == ops.ACT_RELU else out
        return ops.EllSpmmFn.apply(self._values, self.idx, X, self.k is not None, self.part, act, self.partp, self.layout)

    __matmul__ = matmul


class CsrAdjacency:
    """Sparse matrix with the pattern of a coalesced COO in_adj (rowptr int64 [N+1], col int32 [E], erow int32 [E]) and
    its own values [E]: what the `DGG` class returns (every candidate edge kept, dgm.py:1804-1815), rows of any width.
    row0 / n_rows: the rows [row0, row0 + n_rows) of such a matrix as a row shard holds them (csr_pattern_rows): shape (n_rows, n),
    rowptr [n_rows + 1] from 0, col and erow GLOBAL; to_dense() / to_sparse() place row erow - row0."""

    def __init__(self, rowptr, col, erow, values, n, k=None, row0=0, n_rows=None):
        self.rowptr, self.col, self.erow, self._values, self.k = rowptr, col, erow, values, k
        self.row0 = int(row0)
        self.shape = (n if n_rows is None else int(n_rows), n)
        self.device = values.device

    def values(self):
        return self._values

    def coalesce(self):
        return self

    def indices(self):
        return torch.stack([self.erow.long() - self.row0, self.col.long()])

    def to_sparse(self):
        return torch.sparse_coo_tensor(self.indices(), self._values, self.shape)

    def to_dense(self):
        out = torch.zeros(self.shape, device=self.device, dtype=self._values.dtype)
        return out.index_put((self.erow.long() - self.row0, self.col.long()), self._values, accumulate=True)

    def normalize(self):
        if self.shape[0] != self.shape[1]:
            raise NotImplementedError("CsrAdjacency.normalize: a row shard needs the other shards' row sums (dgg_amd.distributed)")
        return CsrAdjacency(self.rowptr, self.col, self.erow, ops.CsrNormalizeFn.apply(self._values, self.rowptr, self.col),
                            self.shape[0], k=self.k)

    def matmul(self, X):
        return ops.CsrSpmmFn.apply(self._values, self.rowptr, self.col, X)

    __matmul__ = matmul


# The candidate graph is DATA: the same sparse tensor object comes in on every forward (train_small_graphs.py builds it once), and
# turning it into the CSR arrays costs ~15 tiny launches (coalesce, coo -> csr, casts, a float64 cumsum, two index ops) -- a sixth of
# the Pubmed-shape step.  Both conversions are cached per tensor OBJECT (weak reference) and version of its values: a new tensor,
# or one modified in place, is converted again.  Not during a hipGraph capture of an unseen tensor (nothing is cached from there).
_CSR_CACHE = {}


def _cached(kind, in_adj, make):
    import weakref
    key = (kind, id(in_adj))
    ver = in_adj._values()._version if in_adj.is_sparse else in_adj._version
    ent = _CSR_CACHE.get(key)
    if ent is not None and ent[0]() is in_adj and ent[1] == ver:
        return ent[2]
    out = make()
    if not torch.cuda.is_available() or not torch.cuda.is_current_stream_capturing():
        for k_ in [k_ for k_, v in _CSR_CACHE.items() if v[0]() is None]:
            del _CSR_CACHE[k_]
        _CSR_CACHE[key] = (weakref.ref(in_adj), ver, out)
    return out


def _seed_cache(kind, in_adj, value):
    """Enters `value` as what _cached(kind, in_adj, ...) returns for this tensor object and version of its values: for a producer that
    already holds the converted arrays (a sampler's kernels build the batch graph in CSR form; dgg_amd.sampling.EditedBatch)."""
    _cached(kind, in_adj, lambda: value)
    return value


def csr_pattern(in_adj):
    """coalesced sparse COO -> (rowptr int64, col int32, erow int32)"""
    def make():
        a = in_adj.coalesce()
        ind = a.indices()
        rowptr = torch._convert_indices_from_coo_to_csr(ind[0], a.shape[0], out_int32=False)
        return rowptr, ind[1].to(torch.int32).contiguous(), ind[0].to(torch.int32).contiguous()
    return _cached("pattern", in_adj, make)


def csr_pattern_rows(in_adj, rows):
    """rows [r0, r1) of csr_pattern(in_adj) as a row shard takes them -> ((rowptr int64 [r1-r0+1] REBASED to start at 0, col int32
    [E_loc] global, erow int32 [E_loc] global), (e0, e1)): per-edge arrays of the whole graph are sliced to [e0, e1).  Cached with the
    graph (one host read of two offsets per graph object and row range)."""
    r0, r1 = int(rows[0]), int(rows[1])

    def make():
        rowptr, col, erow = csr_pattern(in_adj)
        e0, e1 = (int(v) for v in rowptr[[r0, r1]].tolist())
        return ((rowptr[r0:r1 + 1] - e0).contiguous(), col[e0:e1], erow[e0:e1]), (e0, e1)
    return _cached(("pattern_rows", r0, r1), in_adj, make)


def ell_from_dense(A, K=ops.DEFAULT_K):
    """Dense [N,N] -> ELL keeping the K largest entries per row (exact when every row has <= K non-zeros)."""
    assert (A != 0).sum(1).max() <= K, "row has more non-zeros than the ELL width"
    idx, val = ops.select_scores(A.abs().contiguous(), K)
    vals = torch.gather(A, 1, idx.clamp(min=0).long())
    valid = (idx >= 0) & (vals != 0)
    idx = torch.where(valid, idx, torch.full_like(idx, -1))
    return EllAdjacency(idx, torch.where(valid, vals, torch.zeros_like(vals)), A.shape[1])


def csr_candidates(in_adj):
    """torch sparse COO [N,N] (coalesced, self loops included by the caller as in model.py:1249-1264) ->
    (rowptr int64 [N+1], col int32 [E], deg fp32 [N] = row sums of the stored values)."""
    def make():
        a = in_adj.coalesce()
        N = a.shape[0]
        ind = a.indices()
        rowptr = torch._convert_indices_from_coo_to_csr(ind[0], N, out_int32=False)
        col = ind[1].to(torch.int32).contiguous()
        # row sums, deterministic (index_add_ uses float atomics: the last bit would change from call to call, and the raw
        # degrees are an input of the u-v-deg scorers): differences of a float64 running sum at the row boundaries
        cs = torch.cat([a.values().new_zeros(1, dtype=torch.float64), a.values().double().cumsum(0)])
        deg = (cs[rowptr[1:]] - cs[rowptr[:-1]]).float()
        return rowptr, col, deg
    return _cached("candidates", in_adj, make)


def _target_csr(target):
    """the supervision target as (rowptr int64, col int32, values float32): a CsrAdjacency's own arrays, or a sparse COO tensor through
    csr_pattern and its cache (the same object every step is converted once)"""
    if isinstance(target, CsrAdjacency):
        if target.shape[0] != target.shape[1]:
            raise NotImplementedError("adjacency_mse_loss: the target is a row shard; the loss is taken on the whole graph only")
        return target.rowptr, target.col, target.values().detach().to(torch.float32), target.shape
    if not (torch.is_tensor(target) and target.is_sparse):
        raise TypeError(f"adjacency_mse_loss: target must be a sparse COO tensor or a CsrAdjacency, got {type(target).__name__}")
    rowptr, col, _ = csr_pattern(target)
    gval = _cached("values_f32", target, lambda: target.coalesce().values().detach().to(torch.float32).contiguous())
    return rowptr, col, gval, tuple(target.shape)


def adjacency_mse_loss(out_adj, target, reduction="mean"):
    """F.mse_loss(out_adj.to_dense(), target.to_dense().float(), reduction=reduction) without either dense operand: the reference's
    supervision of the learned adjacency (train_reddit.py:236-251, `loss_2`), at any N.
    out_adj: the EllAdjacency (64-rank list or chunked rows) or CsrAdjacency of the WHOLE graph that a generator returned; a row shard
    raises NotImplementedError.  target: a sparse COO tensor [N,N] (coalesced and converted once per tensor object; integer or bool
    values are cast to float32) or a CsrAdjacency.  -> 0-dim float32 tensor on out_adj's device, differentiable with respect to
    out_adj.values() (one kernel pair; the backward is an elementwise product)."""
    if not isinstance(out_adj, (EllAdjacency, CsrAdjacency)):
        raise TypeError(f"adjacency_mse_loss: out_adj must be an EllAdjacency or a CsrAdjacency, got {type(out_adj).__name__}")
    if reduction not in ops.ADJ_LOSS_REDUCTIONS:
        raise ValueError(f"adjacency_mse_loss: reduction must be 'mean' or 'sum', got {reduction!r}")
    if out_adj.shape[0] != out_adj.shape[1]:
        raise NotImplementedError(f"adjacency_mse_loss: out_adj is a row shard {tuple(out_adj.shape)}; the loss is taken on the whole "
                                  "graph only (rows == columns)")
    rowptr, col, gval, tshape = _target_csr(target)
    if tuple(tshape) != tuple(out_adj.shape):
        raise ValueError(f"adjacency_mse_loss: target is {tuple(tshape)}, out_adj is {tuple(out_adj.shape)}")
    if gval.device != out_adj.device:
        raise ValueError(f"adjacency_mse_loss: target is on {gval.device}, out_adj on {out_adj.device}")
    if isinstance(out_adj, CsrAdjacency):
        index = (out_adj.rowptr, out_adj.col)
    else:
        if out_adj.owner is not None:
            out_adj.owner.check_ell_bound()
        index = (out_adj.idx,) if out_adj.layout is None else (out_adj.idx, out_adj.layout)
    return ops.AdjMseLossFn.run(out_adj.values(), index, (rowptr, col, gval), reduction).reshape(())
