"""Row-sharded training of GCN_DGG across the GPUs of one node through the nn.Module API (one process per GPU).

    net = ShardedGCN_DGG(model)                     # shares model's parameters, state_dict and optimiser groups
    logp, adj, _ = net(x, AllPairs(deg))            # x [N, d] and deg [N] replicated; logp = this rank's rows net.rows
    logp, adj, _ = net(x, in_adj)                   # or edge-list candidates: in_adj the whole sparse [N, N] graph, replicated
    loss = global_nll_loss(logp, labels, idx_train, net.rows)
    loss.backward()                                 # every rank now holds the full-graph gradient of every parameter

Layer 1 (generator + normalize_adj + GCNConv) is the fused node of DGG_LearnableK_debug.forward_conv over a row shard of
dgg_amd.parallel.ShardedDGGConv on replicated features with the hybrid exchange; layer 2 is relu(Â_local (x1 W2)) over all N columns
with x1 W2 (or x1) all-gathered and its cotangent reduce-scattered (_ShardedConvFn).  Both layers sum the replicated weight gradients
over the ranks inside their autograd nodes, so identical optimisers keep the ranks' parameters bit-identical.

Edge-list candidates (a sparse in_adj, the reference's own configuration: dgm.py:1613-1614) run on several ranks with the u-v-dist scorer
and the edge-MLP scorers of the fused layer (u-v-deg, u-v-A_uv, u-v-deg-dist, edge_conv, A_uv), under no / hash / symmetric hash noise:
every rank scores its own rows' candidates through the row-range kernels, and the scorer's gradients are summed with the layer's.

All-pairs candidates run with the u-v-dist scorer and with the edge-MLP scorers that read the end nodes and their prior degrees only
(u-v-deg, the reference training script's default, u-v-deg-dist, edge_conv -- an opt-in, args.dgg_allpairs_mlp_fused = True, as for the
fused layer on one GPU; without it the wrapper raises as before; no / hash / symmetric hash noise -- the ranked generators give
way to the per-pair hash of the same law, as on one GPU): every rank scores all N columns of its own rows through the row range of
dgg_allpairs_mlp_topk, or of dgg_allpairs_mlp_topk_wide on chunked rows under args.dgg_allpairs_mlp_rows = "chunked", and the adjacency
returned is the rank's rows with global columns (`layout` set for chunked rows).  The N^2 scoring is row-parallel, so this is the
configuration a row shard divides best; no run on several GPUs has been timed.
u-v-A_uv, which reads the input graph's stored values, runs the same way on all-pairs candidates that carry a prior graph --
AllPairs(deg, prior=P) / AllPairs.from_graph -- under an opt-in of its own, args.dgg_allpairs_prior_fused = True (enough alone; without it,
or without a prior, the wrapper raises as before; A_uv stays refused): every rank gets the whole prior, as it gets the whole prior_degree,
and the row range of dgg_allpairs_mlp_topk_prior / dgg_allpairs_mlp_topk_wide_prior looks up the stored value of every pair of its rows.

Edge-list rows wider than the 64-rank list whose learned degree needs more ranks than that leave the fused layer for the CSR form
(DGG_LearnableK_debug._csr_soft_adjacency -> CsrAdjacency.normalize -> GCNConv on a CsrAdjacency), on one GPU and, as an OPT-IN, on a row
shard: args.dgg_wide_rows = "csr" (the CSR form from the first forward) or "csr_auto" (the fused layer until the collective wide-row flag
first fires, the CSR form for that forward -- recomputed -- and every later one on that graph).  Under the default "auto" such a forward
still raises NotImplementedError on every rank at once (the flag is ORed over the ranks).  Under args.dgg_edgelist_rows = "chunked"
(opt-in; with args.dgg_wide_rows "auto" / "chunked") such rows never leave the fused layer, on one GPU or on a row shard: every rank lays the
clamped degrees min(k_i, n_i - 9.5) of its own rows out in chunks of 64 ranks (one read-back of the chunk count per forward and rank, no
collective: edge lists draw the per-pair hash keyed on global ids) and ranks them with dgg_edgelist_topk_chunked /
dgg_edgelist_topk_p_chunked; the adjacency returned carries `layout`, and neither the sticky CSR decision nor that NotImplementedError
applies.  The sharded CSR form (_CsrForm) keeps the
one-GPU operation order, so its forward has the one-GPU bits: every rank computes the projection, the edge-MLP scorer's per-node products
and the k-net on the whole graph (the k-net normalises with the mean and std of all N prior degrees), scores its own rows' entries
through the _rows entries of the dgg_csr_* kernels (noise keyed on the global pair), and the step costs, beside the loss's scalar: two
all-gathers (row sums [N], hidden rows [N, h]), one reduce-scatter (the hidden rows' cotangent), one all-reduce of the normalisation
backward's workspace [N] and one all-reduce of all parameter gradients in a flat buffer.  No timing of this path exists, and how any of
the steps scales with the number of GPUs has not been measured.

The reference has no distributed code; its loss is F.nll_loss(out[idx], labels[idx])
(train_small_graphs.py:226), which global_nll_loss splits over the ranks.
"""
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .adjacency import AllPairs, CsrAdjacency, csr_candidates
from .dgm import _capturing
from .model import GCN_DGG, _with_self_loops
from .parallel import ShardedDGGConv, _all_gather_rows, shard_bounds


def _world(group):
    return (dist.get_world_size(group), dist.get_rank(group)) if dist.is_initialized() else (1, 0)


def _reduce_scatter_rows(t, eng):
    """[N, c] partial sums on every rank -> the rank's own rows [r1 - r0, c], summed over the ranks (fresh buffers: the result is an
    autograd gradient)"""
    pad = eng.world * eng.per - eng.N
    src = torch.cat([t, t.new_zeros((pad, t.shape[1]))]) if pad else t.contiguous()
    out = t.new_empty((eng.per, t.shape[1]))
    dist.reduce_scatter_tensor(out, src, group=eng.group)
    return out[:eng.r1 - eng.r0]


class _ShardedConvFn(torch.autograd.Function):
    """GCN_DGG's second GCNConv on a row shard: relu(Â_local (x1 W)) with Â_local [rows, N] the normalised adjacency of layer 1's rows
    (global columns).  The order follows GCNConv.forward: x1 W first when out <= in and out is a width of the per-destination backward,
    (Â x1) W otherwise; the all-gathered operand is the narrower one.  The kernels are those GCNConv runs on one GPU (spmm_fwd,
    conv_bwd_cols_p on layer 1's payload partition, linear_fwd / linear_bwd); at one rank without collectives the bits are the same."""

    @staticmethod
    def forward(ctx, x1, ahat, W, eng, idx, layout, partp):
        fin, fout = W.shape
        gather = (lambda t_: _all_gather_rows(t_, eng.N, eng.per, eng.group)) if eng.coll else (lambda t_: t_)
        ctx.eng, ctx.idx, ctx.layout, ctx.partp = eng, idx, layout, partp
        ctx.first = fout <= fin and fout in ops.CONV_BWD_WIDTHS
        if ctx.first:
            H_loc = ops.linear_fwd(x1, W, None, ops.ACT_NONE, 1)
            H = gather(H_loc)
            Y = ops.spmm_fwd(idx, ahat, H, ops.ACT_RELU, layout=layout)
            ctx.save_for_backward(x1, W, H_loc, H, Y)
        else:
            X = gather(x1)
            AX = ops.spmm_fwd(idx, ahat, X, ops.ACT_NONE, layout=layout)
            Y = ops.linear_fwd(AX, W, None, ops.ACT_RELU, 1)
            ctx.save_for_backward(x1, W, X, AX, Y)
        return Y

    @staticmethod
    def backward(ctx, dY):
        eng, idx, partp = ctx.eng, ctx.idx, ctx.partp
        if partp is None:
            raise RuntimeError("ShardedGCN_DGG: this forward ran without a backward to follow (torch.no_grad() or frozen parameters), "
                               "so layer 1 did not sort the partition the second layer's backward runs on")
        dY = dY.contiguous()
        if ctx.first:
            x1, W, H_loc, H, Y = ctx.saved_tensors
            G = ops.act_bwd(Y, dY, ops.ACT_RELU)
            got = ops.conv_bwd_cols_p(idx, H, G, partp[0], partp[1], zero_dA=True)
            if got is None:
                raise RuntimeError("ShardedGCN_DGG: the second layer's shape is outside the per-destination backward (conv_bwd_cols_p)")
            dA, _, dH, _ = got
            if eng.coll:
                dH = _reduce_scatter_rows(dH, eng)
            dx1, dW, _ = ops.linear_bwd(x1, W, H_loc, dH, ops.ACT_NONE, 1, need_dx=ctx.needs_input_grad[0], need_db=False)
        else:
            x1, W, X, AX, Y = ctx.saved_tensors
            dAX, dW, _ = ops.linear_bwd(AX, W, Y, dY, ops.ACT_RELU, 1, need_dx=True, need_db=False)
            got = ops.conv_bwd_cols_p(idx, X, dAX.contiguous(), partp[0], partp[1], zero_dA=True)
            if got is None:
                raise RuntimeError("ShardedGCN_DGG: the second layer's shape is outside the per-destination backward (conv_bwd_cols_p)")
            dA, _, dx1, _ = got
            if eng.coll:
                dx1 = _reduce_scatter_rows(dx1, eng)
        if eng.coll:
            dist.all_reduce(dW, group=eng.group)
        return dx1, dA, dW, None, None, None, None


class _SumGradsFn(torch.autograd.Function):
    """The replicated parameters as the sharded CSR form reads them: identity forward; the backward runs once every use of every
    parameter has delivered its share and sums all of them over the ranks in ONE all-reduce of a flat buffer, so every rank leaves
    backward() with the same bits of the full-graph gradient.  A parameter no use reaches gets no gradient, as on one GPU (which ones is
    a property of the configuration, the same on every rank)."""

    @staticmethod
    def forward(ctx, group, *params):
        ctx.group = group
        ctx.set_materialize_grads(False)
        return tuple(p_.view_as(p_) for p_ in params)

    @staticmethod
    def backward(ctx, *grads):
        have = [g for g in grads if g is not None]
        if have:
            flat = torch.cat([g.reshape(-1) for g in have])
            dist.all_reduce(flat, group=ctx.group)
            parts = iter(flat.split([g.numel() for g in have]))
            grads = tuple(None if g is None else next(parts).view(g.shape) for g in grads)
        return (None,) + grads


class _GatherRowsFn(torch.autograd.Function):
    """the ranks' rows [r1 - r0, c] -> all N rows on every rank; the cotangent -- every rank's partial [N, c] -- is reduce-scattered"""

    @staticmethod
    def forward(ctx, t, sh):
        ctx.sh = sh
        return _all_gather_rows(t, sh.N, sh.per, sh.group)

    @staticmethod
    def backward(ctx, g):
        return _reduce_scatter_rows(g, ctx.sh), None


class _ShardedCsrNormalizeFn(torch.autograd.Function):
    """ops.CsrNormalizeFn on a row shard's slice: the shard's row sums are all-gathered (columns name other ranks' rows); the backward
    runs dgg_csr_norm_bwd's two kernels with the workspace [N] summed over the ranks in between, which also carries the gather's
    cotangent."""

    @staticmethod
    def forward(ctx, w, rowptr, col, sh):
        rs = _all_gather_rows(ops.csr_row_sum(w, rowptr), sh.N, sh.per, sh.group)
        ahat = ops.csr_normalize_fwd_rows(rowptr, col, w, rs, (sh.r0, sh.r1))
        ctx.sh = sh
        ctx.save_for_backward(w, rowptr, col, rs)
        return ahat

    @staticmethod
    def backward(ctx, dA):
        w, rowptr, col, rs = ctx.saved_tensors
        sh = ctx.sh
        dA = dA.contiguous()
        da = ops.csr_norm_bwd_acc_rows(rowptr, col, w, rs, dA, (sh.r0, sh.r1))
        dist.all_reduce(da, group=sh.group)
        return ops.csr_norm_bwd_apply_rows(rowptr, col, rs, dA, da, (sh.r0, sh.r1)), None, None, None


class _Shard:
    """rows [r0, r1) of N on rank `rank` of `group` (the fields _reduce_scatter_rows reads from an engine)"""

    def __init__(self, N, world, rank, group):
        self.N, self.world, self.rank, self.group = N, world, rank, group
        self.r0, self.r1, self.per = shard_bounds(N, world, rank)


class _CsrForm(nn.Module):
    """The one-GPU CSR form of GCN_DGG (_csr_soft_adjacency -> normalize -> relu((A x) W1) -> dropout -> relu((A x1) W2)) on a row
    shard, in that operation order.  A module of its own so that torch.func.functional_call can hand it the parameters behind
    _SumGradsFn: the code below reads them off `model` like any other forward."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x, in_adj, sh):
        m = self.model
        dgg = m.dggs[0]
        _, _, deg = csr_candidates(in_adj)
        noise_mode, _, seed = dgg._noise_now(x, all_pairs=False)    # (edge-list candidates: every candidate is scored, per-pair hash noise)
        mode = ops.MODE_K_TIMES_EDGE_PROB if dgg.k_select_mode == "k_times_edge_prob" else ops.MODE_K_ONLY
        # replicated: the k-net on the whole graph (its degree normalisation reads all N prior degrees); the shard keeps its rows' k
        k = dgg._knet_feat(dgg._project_for_k(x)[1], deg)
        unnorm = dgg._csr_soft_adjacency(x, in_adj, k[sh.r0:sh.r1], noise_mode, None, seed, mode, rows=(sh.r0, sh.r1))
        rowptr, col = unnorm.rowptr, unnorm.col
        ahat = _ShardedCsrNormalizeFn.apply(unnorm.values(), rowptr, col, sh)
        z = ops.LinearFn.apply(ops.CsrSpmmFn.apply(ahat, rowptr, col, x), m.conv1.W, None, ops.ACT_RELU, 1)
        z = _GatherRowsFn.apply(F.dropout(z, training=m.training), sh)
        out = ops.LinearFn.apply(ops.CsrSpmmFn.apply(ahat, rowptr, col, z), m.conv2.W, None, ops.ACT_RELU, 1)
        adj = CsrAdjacency(rowptr, col, unnorm.erow, unnorm.values().detach(), sh.N, k=unnorm.k, row0=sh.r0, n_rows=sh.r1 - sh.r0)
        return F.log_softmax(out, dim=-1), adj, None


_SHARDED_CSR_POLICIES = ("csr", "csr_auto")


class ShardedGCN_DGG(nn.Module):
    """GCN_DGG (reference model.py:1183-1311) on a row shard of the graph: rank r of `group` computes rows [r0, r1) = `.rows`
    (parallel.shard_bounds) of the log-probabilities against all N columns.

    The wrapper owns no parameters of its own: it holds `model` (whose parameters it broadcasts from the group's first rank when
    there are several), and `state_dict()` / `load_state_dict()` / `params1` / `params2` are the model's, so checkpoints and the
    optimiser groups of train_small_graphs.py are unchanged.  forward(x, in_adj) takes the FULL features x [N, d] (data, replicated on
    every rank) and in_adj = AllPairs(prior degrees of all N nodes) or the whole graph's sparse [N, N] adjacency (edge-list candidates,
    replicated like x; self loops are added as GCN_DGG.forward adds them); it returns (log_probs of the rank's rows, the DETACHED unnormalised
    EllAdjacency of those rows with global column indices, None).  After backward() every rank holds the full-graph gradient of every
    parameter when the loss is global_nll_loss (or any loss whose per-rank parts sum to the whole).

    Edge-list candidates on several ranks with args.dgg_wide_rows = "csr" / "csr_auto" (opt-in): the sharded CSR form for rows wider than
    the 64-rank list whose learned degrees outgrow it -- from the first forward ("csr"), or from the forward in which the collective
    wide-row flag first fires ("csr_auto": that forward is recomputed in CSR form, and the switch is sticky per graph object; all ranks
    switch in the same forward).  The adjacency returned is then the DETACHED unnormalised CsrAdjacency of the rank's rows
    (shape (rows, N), global columns); coverage and refusals are those of the fused layer on edge lists (_fused_outside).

    Every rank must draw the same noise: seed the CPU generator identically on every rank (torch.manual_seed) or call
    model.dggs[0].set_seed.  The dropout between the layers draws each rank's mask from its own CUDA generator.
    Outside its coverage the wrapper raises (no silent fall-back), before any collective: on several ranks, edge-list candidates whose
    rows need the CSR form under the default args.dgg_wide_rows = 'auto' and args.dgg_edgelist_rows = 'list' (raised by every rank in the
    same forward; args.dgg_edgelist_rows = 'chunked' keeps such rows in the fused layer as chunked rows), a writer, configurations the fused layer declines, a hipGraph capture on several ranks, args.dgg_hard_literal,
    args.dgg_differentiable_adj, args.dgg_wide_rows other than 'auto' / 'chunked' (edge lists on several ranks: or 'csr' / 'csr_auto'), and on several ranks args.dgg_sym_generator = 'auto'
    (a generator switch decided from one rank's rows)."""

    def __init__(self, model, group=None):
        super().__init__()
        if not isinstance(model, GCN_DGG):
            raise TypeError(f"ShardedGCN_DGG wraps a GCN_DGG, not {type(model).__name__}")
        self.module = model
        self.group = group
        self.world, self.rank = _world(group)
        self._engine = None
        self._rows = None
        if self.world > 1:
            src = 0 if group is None else dist.get_global_rank(group, 0)
            with torch.no_grad():
                for p_ in model.parameters():
                    dist.broadcast(p_.data, src=src, group=group)

    # --- the model's parameters, checkpoints and optimiser groups ------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):
        return self.module.state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        return self.module.load_state_dict(state_dict, strict=strict, assign=assign)

    @property
    def params1(self):
        return self.module.params1

    @property
    def params2(self):
        return self.module.params2

    @property
    def rows(self):
        """(r0, r1): the rows of the graph this rank computes (known from the first forward on)"""
        if self._rows is None:
            raise RuntimeError("ShardedGCN_DGG.rows: the node count is known from the first forward on")
        return self._rows

    # ------------------------------------------------------------------------------------------------------------------------------
    def _edge_lists(self, in_adj):
        """edge-list candidates on several ranks: the row shard's own path (one rank: the model's step)"""
        return self.world > 1 and not isinstance(in_adj, AllPairs)

    def _check(self, x, in_adj, writer):
        m = self.module
        dgg, a = m.dggs[0], m.dggs[0].args
        # (every refusal of edge-list candidates on several ranks names them)
        what = "ShardedGCN_DGG (edge-list candidates on several ranks)" if self._edge_lists(in_adj) else "ShardedGCN_DGG"
        if writer is not None:
            raise NotImplementedError(f"{what}: a writer (histograms of the whole graph) is not supported on a row shard")
        if self.world > 1 and _capturing():
            raise NotImplementedError(f"{what}: a hipGraph capture of a step on several ranks is not supported")
        if getattr(a, "dgg_hard_literal", False):
            raise NotImplementedError(f"{what}: args.dgg_hard_literal is not supported")
        if m.differentiable_adj:
            raise NotImplementedError(f"{what}: args.dgg_differentiable_adj needs the separate modules (one GPU: the model itself)")
        if x.requires_grad:
            raise ValueError(f"{what}: the features are data replicated on every rank; they cannot take a gradient")
        if self._edge_lists(in_adj):
            if not isinstance(in_adj, torch.Tensor) or in_adj.dim() != 2 or in_adj.shape[0] != x.shape[0] or in_adj.shape[1] != x.shape[0]:
                raise NotImplementedError(f"{what}: in_adj must be AllPairs(prior_degree) or the whole graph's [N, N] adjacency "
                                          f"(N = {x.shape[0]}, got {type(in_adj).__name__} {tuple(getattr(in_adj, 'shape', ()))})")
            policy = getattr(a, "dgg_wide_rows", "auto")
            if policy not in ("auto", "chunked") + _SHARDED_CSR_POLICIES:
                raise NotImplementedError(f"{what}: args.dgg_wide_rows = {policy!r} (a row shard keeps the 64-rank list, or takes the CSR "
                                          "form of rows wider than it under 'csr' / 'csr_auto')")
            dgg._edgelist_chunked()                          # (args.dgg_edgelist_rows: an unknown value or a combination it refuses raises)
            why = dgg._fused_outside(x, in_adj, m.conv1.W)
            if why is not None:
                raise NotImplementedError(f"{what}: the fused layer does not cover this configuration ({why})")
            return
        if not isinstance(in_adj, AllPairs):
            return
        if in_adj.prior_degree.shape[0] != x.shape[0]:
            raise ValueError(f"ShardedGCN_DGG: in_adj carries {in_adj.prior_degree.shape[0]} prior degrees for {x.shape[0]} nodes "
                             "(both are the whole graph's)")
        policy = getattr(a, "dgg_wide_rows", "auto")
        if policy not in ("auto", "chunked"):
            raise NotImplementedError(f"ShardedGCN_DGG: args.dgg_wide_rows = {policy!r} (rows wider than the list need the chunked form)")
        # (the edge-MLP scorers score every pair under the per-pair hash generators: no ranked generator, nothing to switch)
        if self.world > 1 and getattr(a, "dgg_sym_generator", "ranked") == "auto" and dgg.edge_prob_net_mode == "u-v-dist":
            raise NotImplementedError("ShardedGCN_DGG: args.dgg_sym_generator = 'auto' switches generators from one rank's rows; "
                                      "choose 'ranked' or 'hash' on several ranks")
        why = dgg._fused_outside(x, in_adj, m.conv1.W)
        if why is not None:
            raise NotImplementedError(f"ShardedGCN_DGG: the fused layer does not cover this configuration ({why})")

    def forward(self, x, in_adj, noise=True, epoch=None, writer=None):
        m = self.module
        self._check(x, in_adj, writer)
        N = x.shape[0]
        self._rows = shard_bounds(N, self.world, self.rank)[:2]
        edge_lists = self._edge_lists(in_adj)
        if not isinstance(in_adj, AllPairs) and not edge_lists:     # (one rank: edge-list candidates are the model's own step)
            return m(x, in_adj, noise=noise, epoch=epoch, writer=writer)
        policy = getattr(m.dggs[0].args, "dgg_wide_rows", "auto")
        if edge_lists:
            in_adj = _with_self_loops(in_adj)                # (as GCN_DGG.forward: cached per graph object)
            if policy == "csr":
                return self._csr_form(x, in_adj)
        eng = self._engine
        if eng is None or eng.N != N:
            eng = self._engine = ShardedDGGConv(ops, N, group=self.group, K=64, t=ops.T_DIST, x_full=x, hybrid=True)
        got = m.dggs[0]._forward_conv(x, in_adj, m.conv1.W, True, engine=eng)
        if got is None and edge_lists and policy == "csr_auto" and m.dggs[0]._wide_rows_state(in_adj, csr_candidates(in_adj)[0]) is True:
            # (decided collectively and sticky per graph: every rank is here in the same forward, and in every later one before any kernel)
            return self._csr_form(x, in_adj)
        if got is None and edge_lists:
            # (decided collectively: _wide_rows ORs the ranks' flags, so every rank raises here in the same forward)
            raise NotImplementedError("ShardedGCN_DGG (edge-list candidates on several ranks): a row wider than the 64-rank list has a "
                                      "learned degree beyond it; the CSR form of such rows is not sharded under args.dgg_wide_rows = "
                                      f"{policy!r} (opt in with 'csr' or 'csr_auto', or keep such rows in the fused layer as chunked rows "
                                      f"with args.dgg_edgelist_rows = 'chunked') ({m.dggs[0].__dict__.get('fused_fallback', {})})")
        if got is None:
            raise NotImplementedError("ShardedGCN_DGG: this forward left the fused layer's coverage "
                                      f"({m.dggs[0].__dict__.get('fused_fallback', {})})")
        z, unnorm, norm = got
        z = F.dropout(z, training=m.training)
        out = _ShardedConvFn.apply(z, norm.values(), m.conv2.W, eng, norm.idx, norm.layout, norm.partp)
        return F.log_softmax(out, dim=-1), unnorm, None


    def _csr_form(self, x, in_adj):
        """this forward in the sharded CSR form (edge-list candidates with self loops, several ranks): every rank enters every
        collective, whether or not it owns a wide row"""
        m = self.module
        sh = _Shard(x.shape[0], self.world, self.rank, self.group)
        named = [(n_, p_) for n_, p_ in m.named_parameters() if p_.requires_grad]
        params = {}
        if named and torch.is_grad_enabled():
            synced = _SumGradsFn.apply(self.group, *[p_ for _, p_ in named])
            params = {"model." + n_: s_ for (n_, _), s_ in zip(named, synced)}
        # (tie_weights=False: GCN_DGG lists each GCNConv under two names -- conv1 and convs[0] are ONE module, so the one name
        #  named_parameters() yields reaches both, and the tie logic would swap that module's slot twice and restore it wrongly)
        return torch.func.functional_call(_CsrForm(m), params, (x, in_adj, sh), tie_weights=False)


_SEL_CACHE = {}


def _local_selection(labels, idx, rows, device):
    """-> (own positions of the rank's share of idx [n], their labels [n], global count).  labels and idx are data: the selection is
    cached per tensor OBJECT and version (one synchronisation per new pair), as adjacency._cached does for the candidate graph."""
    import weakref
    key = (id(labels), id(idx), tuple(rows), str(device))
    ent = _SEL_CACHE.get(key)
    if ent is not None and ent[0]() is labels and ent[1]() is idx and ent[2] == (labels._version, idx._version):
        return ent[3]
    r0, r1 = rows
    i_ = idx.to(device)
    if i_.dtype == torch.bool:
        own, total = torch.nonzero(i_[r0:r1]).reshape(-1), int(i_.sum())
    else:
        i_ = i_.long()
        own, total = i_[(i_ >= r0) & (i_ < r1)] - r0, int(i_.numel())
    got = (own, labels.to(device)[own + r0].long(), total)
    for k_ in [k_ for k_, v in _SEL_CACHE.items() if v[0]() is None or v[1]() is None]:
        del _SEL_CACHE[k_]
    _SEL_CACHE[key] = (weakref.ref(labels), weakref.ref(idx), (labels._version, idx._version), got)
    return got


def global_nll_loss(log_probs_local, labels, idx, rows, group=None):
    """F.nll_loss(out[idx], labels[idx]) of the whole graph (reference train_small_graphs.py:226) from each rank's rows: the rank's
    share of idx, summed and divided by the GLOBAL count.  The value returned is the whole loss on every rank (one scalar all-reduce);
    its gradient is the rank's share only -- the collectives inside ShardedGCN_DGG's backward sum the shares.
    labels [N] (all nodes), idx: indices into the N nodes (duplicates count twice, as in the reference) or a boolean mask [N]."""
    own, lab, total = _local_selection(labels, idx, rows, log_probs_local.device)
    part = -log_probs_local[own, lab].sum() / total
    world, _ = _world(group)
    if world == 1:
        return part
    whole = part.detach().clone()
    dist.all_reduce(whole, group=group)
    return whole + (part - part.detach())                     # (the value of the whole, the gradient of the share)
