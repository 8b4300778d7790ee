"""Node-range sharding of the DGG hot path across the GPUs of one node (one process per GPU, RCCL over xGMI).

The reference has no distributed code; the all-pairs similarity shards by rows: every
output row i needs x_i, all candidate x_j, k_i and the row sums rs_j of its selected neighbours, and nothing else
(sort / ramp act on dim=-1, reference dgm.py:1404-1420).  Rank r owns rows [r*ceil(N/G), ...) of X, of the ELL
adjacency and of the conv output.

The graph conv is evaluated as relu(A (x W)) instead of the reference's relu((A x) W) (model.py:594-598; equal up to
fp32 reassociation): the aggregation gathers the out_features-wide projected rows H = X Wc, not the d-wide inputs, and
the backward's three column-walking terms (SDDMM, transposed SpMM, neighbour side of the normalisation backward) share
ONE gathered cotangent row per edge (ops.conv_bwd_cols).  Every per-node array a rank gathers from is therefore a
PROJECTION of the features: xp (scoring) and H (aggregation).

Two exchange schemes:

REPLICATED FEATURES (`x_full=`): when the DGG input is DATA (GCN_DGG / SAGE_DGG / GCNII_DGG all feed it the raw node
features, model.py:1266, 720) it never changes between steps, so it is placed on every GPU once at load (N*d*4 bytes:
0.4 GB of the 288 GB for 800k nodes) and NO feature tensor crosses the fabric per step: every rank projects all N rows
itself ([xp | H] = one GEMM that reads X once) and forms the weight gradients from its PARTIAL [dxp | dH] against the
full X (summed by the weight all-reduce).  Per-step collectives: all-gather of the row sums (N*4 B), all-reduce of da
(N*4 B), one flat all-reduce of the replicated weight gradients (~35k floats).

HYBRID (`x_full=` with `hybrid=True`; bench.py's default for several GPUs): as REPLICATED FEATURES for the scoring side -- every
rank projects xp of all N nodes itself (the search needs it at once, and N*d*h*2 flop is cheaper than receiving 7/8 of it over
xGMI) and forms dWe from its partial dxp against the full X -- but the AGGREGATION side is sharded: every rank projects H = X Wc
for its own rows only and all-gathers it ASYNCHRONOUSLY (H is first read by the aggregation, after the k-net, the search and the
partition: ~0.3 ms of kernels at 62 500 rows per rank to hide N*F*4 bytes behind), and the partial dH [N,F] -- complete after the
first backward kernel, needed only by the last -- is reduce-scattered behind the score backward, so that dWc is a product over
the rank's own rows.  Half of the replicated full-N GEMM work (projection and weight gradient) leaves the critical path.

GATHERED PROJECTIONS (inputs that are activations, `x_grad`; or data that is not replicated): every rank projects its
own rows and all-gathers [xp | H] (xp first -- the top-k waits for it -- H asynchronously behind it: it is needed only
by the aggregation, so it crosses xGMI while the top-k, soft-k, partition and normalisation kernels run); the backward
reduce-scatters the partial [dxp | dH] (the adjoint of that all-gather) and forms weight and input gradients from the
rank's own rows.

`kern` is the kernel namespace (dgg_amd.ops on the GPU; tests substitute a CPU stand-in built on the oracle so
that the partition / collective logic is exercised with gloo, world_size 2 and 3, without a GPU).  What the engine may call on it
beyond the baseline entries is written down in KernelContract.
"""
import os
import types
import weakref

import torch
import torch.distributed as dist

from .ops import KERNEL_WIDTHS, RSYM_WIDTHS        # (constants only: the kernels themselves come in through `kern`)


def shard_bounds(N, world, rank):
    per = (N + world - 1) // world
    r0 = min(rank * per, N)
    return r0, min(r0 + per, N), per


def csr_rows(rowptr, col, rows):
    """-> (rowptr [r1-r0+1] from 0, col of rows [r0, r1), (e0, e1)): the rebased CSR slice the row-shard entries of the edge-list kernels
    take (include/dgg_hip.h, dgg_edgelist_topk_softk_rows); per-edge arrays are sliced to [e0, e1).  One host read of two offsets."""
    r0, r1 = int(rows[0]), int(rows[1])
    e0, e1 = (int(v) for v in rowptr[[r0, r1]].tolist())
    return (rowptr[r0:r1 + 1] - e0).contiguous(), col[e0:e1], (e0, e1)


class _Gather:
    """A (possibly still running) all-gather of row shards: .get() waits and returns the [N, ...] tensor.  On RCCL the
    wait is a stream dependency (no host block); shards are padded to `per` rows for the fixed-size collective.  `bufs`
    (a dict owned by the layer) keeps the padded source and the gathered output between steps: no allocation, no
    torch.cat per step."""

    def __init__(self, t_local, N, per, group, async_op, bufs=None, key=None):
        world = dist.get_world_size(group)
        tail = tuple(t_local.shape[1:])
        n_loc = t_local.shape[0]
        if n_loc == per:
            src = t_local.contiguous()
        else:
            src = self._buf(bufs, (key, "src"), (per,) + tail, t_local)
            src[:n_loc].copy_(t_local)
            src[n_loc:].zero_()
        self.out = self._buf(bufs, (key, "out"), (world * per,) + tail, t_local)
        self.N = N
        self.work = dist.all_gather_into_tensor(self.out, src, group=group, async_op=async_op)

    @staticmethod
    def _buf(bufs, key, shape, like):
        if bufs is None or key[0] is None:
            return like.new_empty(shape)
        b = bufs.get(key)
        if b is None or tuple(b.shape) != tuple(shape) or b.device != like.device:
            b = bufs[key] = like.new_empty(shape)
        return b

    def get(self):
        if self.work is not None:
            self.work.wait()
            self.work = None
        return self.out[:self.N]


def _all_gather_rows(t_local, N, per, group, bufs=None, key=None):
    """[n_loc, ...] -> [N, ...]"""
    if dist.get_world_size(group) == 1 and os.environ.get("DGG_FORCE_COLLECTIVES") != "1":
        return t_local
    return _Gather(t_local, N, per, group, False, bufs, key).get()


class KernelContract:
    """What ShardedDGGConv may call on its kernel namespace BEYOND the baseline entries (linear_fwd / linear_bwd, degree_stats,
    knet_x_fwd / knet_x_bwd, allpairs_topk, edgelist_topk, edgelist_topk_p, edge_mlp_fwd / edge_mlp_bwd, softk_fwd / softk_bwd,
    normalize_fwd, spmm_fwd / spmm_bwd, act_bwd, norm_bwd_da, edge_bwd, csr_uvdist_bwd), written down once.  Every optional entry answers None --
    what dgg_amd.ops answers for "does not cover this shape" -- and every optional flag is off, so the engine calls them
    unconditionally and takes its fallback where it takes the shape fallback.  dgg_amd.ops provides every name with these parameter
    names (tests/test_kernel_contract.py); a test stand-in inherits from this class and defines the baseline entries only."""

    KNET_MFMA_WIDTHS = ()       # latent widths of the matrix-core k-net (knet_x_fwd_slim / knet_x_bwd_fused)
    PREMASK = False             # softk_edge_bwd_p / knet_x_bwd_fused can return gradients of the pre-activation (out_act)
    DA_MAP = False              # conv_bwd_cols_p(want_dA=False): the row kernel reads dA through the partition's slot -> record map
    EMLP_BWD_PARTP = False      # edge_mlp_bwd takes the payload partition for its neighbour-side sums

    def linear_fwd_multi(self, x, layers):
        return None

    def linear_bwd_multi(self, x, layers):
        return None

    # linear_fwd_multi + knet_x_fwd_slim on layer knet_seg's output in one launch -> ([y_s], k, u)
    def project_knet(self, x, layers, knet_seg, deg, mu_sd, W1, b1, Wmu, bmu, Wp, bp):
        return None

    def zero_pool(self, device, nfloats):
        return None

    def knet_x_fwd_slim(self, xk, deg, mu_sd, W1, b1, Wmu, bmu, Wp, bp):
        return None

    def knet_x_bwd_fused(self, xk, deg, mu_sd, W1, b1, Wmu, bmu, Wp, u, dk, out_act=0):
        return None

    def edgelist_topk_softk(self, xp, rowptr, col, k, mode, K, t, noise_mode, G, seed, overflow=None, rows=None):
        return None

    def allpairs_topk_softk(self, xp, k, mode, t, seed, rows=None, lpub=None):
        return None

    def allpairs_topk_wide(self, xp, k, layout, mode, t, seed, rows=None, ramp=True, noise_mode=None, lpub=None):
        return None

    def chunk_layout(self, k, maxm=None, ccap=None, ncols=None, sticky=None):
        return None

    # the edge-MLP scorer on ALL-PAIRS candidates: scorer + perturbation + top-K of every pair in one kernel, on the 64-rank list and on
    # chunked rows, and the ramp + normalisation backward of the chunked rows of a row shard.  An engine whose scorer needs them raises
    # when the namespace answers None: every pair has to be scored, and there is no other evaluator to fall back to
    def allpairs_mlp_topk(self, AB, xp, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, K, noise_mode, G, seed, rows=None):
        return None

    def allpairs_mlp_topk_wide(self, AB, xp, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, k, layout, mode, noise_mode, G, seed, rows=None):
        return None

    def softk_bwd_rows_chunked(self, idx, val, k, rs, dA, da_cols, ahat, layout, row0=0, mode=0):
        return None

    # edge-list candidates on chunked rows (rows of any width): search + ramp of u-v-dist, and perturbation + ranking + ramp of the
    # edge-MLP scorers' probabilities.  An engine that has laid wide rows out raises when the namespace answers None
    def edgelist_topk_chunked(self, xp, rowptr, col, k, layout, mode, t, noise_mode, seed, rows=None):
        return None

    def edgelist_topk_p_chunked(self, p_edge, N, rowptr, col, k, layout, mode, noise_mode, seed, ex_edge=None, rows=None):
        return None

    def rowmin_logp_bound(self, xp, t, rows=None):
        return None

    def ranked_probe(self, xp, k_limit, t, seed, rows=None, stride=1, max_blocks=0):
        return None

    def ranked_cost_estimate(self, probe, N, rows=None):
        return None

    # rsym_status is never called by the engine (a diagnostic that synchronises).  It stands for the one capability that is not "call
    # it, see None": the real namespace's allpairs_topk takes `status=` and reports the ranked symmetric generator's flags through it,
    # a stand-in's has no such parameter.  One boolean in ShardedDGGConv.__init__: the namespace is not built on this class.
    def rsym_status(self, ws, N, rows=None):
        return None

    def partp_build(self, idx, w, val, rs_rows, ncols, rs_all=None, phase=0, layout=None, want_ahat=True):
        return None

    def spmm_norm_fwd(self, idx, w, rs_rows, partp, X, act=0, layout=None):
        return None

    def partp_sort(self, part):
        return None

    def partp_has_map(self, rows):
        return None

    def part_build(self, idx, w, ncols):
        return None

    def conv_bwd_cols(self, idx, ahat, H, G, part, rs=None, want_da=False):
        return None

    def conv_bwd_cols_p(self, idx, H, G, partp, rs, zero_dA=True, dA_ext=None, want_dA=True):
        return None

    def softk_edge_bwd(self, xp, idx, val, k, dA, rs=None, da=None, row0=0, t=-0.05, perturb=False, mode=0, normalized=False, part=None,
                       want_dval=False, ahat_rows=None):
        return None

    def softk_edge_bwd_p(self, xp, idx, val, k, dA, dA_rec, rs, da, row0, t, perturb, mode, normalized, partp, ahat_rows=None, out_act=0,
                         phase=0, state=None, ainv_table=None):
        return None


def uvdist_score_bwd(kern, xp, idx, val, k, dA, rs, da, row0, t, perturb, mode, normalized, part=None, ahat_rows=None):
    """Ramp (+ normalisation, if `normalized`) + u-v-dist score backward on an ELL block with an optional index partition -> dxp, dk.
    Inside the row kernel of the score backward when the partition is there and the entry covers the shape, else the two calls."""
    fused = None
    if part is not None:
        fused = kern.softk_edge_bwd(xp, idx, val, k, dA, rs, da, row0, t, perturb, mode, normalized, part, ahat_rows=ahat_rows)
    if fused is not None:
        return fused[0], fused[1]
    assert ahat_rows is None
    dval, dk = kern.softk_bwd(idx, val, k, dA, rs, da, row0, mode, normalized)
    pk = {} if part is None else {"part": part}
    return kern.edge_bwd(xp, idx, val, dval, row0, t, perturb, **pk), dk


def edge_mlp_score_bwd(kern, sc, xp, AB, idx, eid, val, dval, sdeg, ex, perturb, **kw):
    """Backward of the edge-MLP scorer from d loss / d score: the MLP's backward on the entries (dgg_edge_mlp_bwd: per-node dAB,
    parameter sums), then AB's GEMM backward -> dxp (WITHOUT the ex_mode == 2 distance term, whose form -- ELL or CSR -- is the
    caller's), dex (None unless ex_mode == 2), {Wcat, wdu, wdv, wex, b1, w2, b2}.  sc: the scorer's terms (ShardedDGGConv.scorer);
    kw: edge_mlp_bwd's rows / rowptr / partp / w / nrec_max."""
    dAB, dpar, dex = kern.edge_mlp_bwd(AB, idx, eid, val, dval, sdeg, ex, sc["wdu"], sc["wdv"], sc["wex"], sc["b1"], sc["w2"], sc["b2"],
                                       sc["act"], perturb, need_dex=sc["ex_mode"] == 2, **kw)
    dxp, dWcat, _ = kern.linear_bwd(xp, sc["Wcat"], AB, dAB, 0, 0, True, False)
    hw = sc["Wcat"].shape[0] // 2
    pick = lambda t_, a: None if t_ is None else dpar[a * hw:(a + 1) * hw]  # noqa: E731
    return dxp, dex, dict(Wcat=dWcat, wdu=pick(sc["wdu"], 0), wdv=pick(sc["wdv"], 1), wex=pick(sc["wex"], 2), b1=dpar[3 * hw:4 * hw],
                          w2=dpar[4 * hw:5 * hw], b2=dpar[5 * hw:5 * hw + 1])


class ShardedDGGConv:
    """One DGG (all-pairs or edge-list candidates; u-v-dist or an edge-MLP scorer / x / k_times_edge_prob) + normalise + GCNConv layer,
    forward and backward, on a row shard.  Parameters are a dict with the reference's names (dgm.py:1097-1143, model.py:583).
    Edge-list candidates, and an edge-MLP scorer on any candidates, need replicated features (x_full) on several ranks: every rank
    projects xp (and the edge-MLP scorer's AB) for all N nodes, scores its own rows' candidates and sums the scorer's gradients with the
    layer's in one all-reduce.
    Edge-list rows wider than the 64-rank list whose learned degrees need more keep every weighted rank in chunked rows under
    wide_rows = "auto" (_chunk_layout_edge_list; edgelist_topk_chunked, or edge_mlp_fwd + edgelist_topk_p_chunked with a scorer) and run
    the backward of chunked all-pairs rows; the default "off" keeps the list, whose bound the caller enforces.
    An edge-MLP scorer on ALL-PAIRS candidates (u-v-deg / u-v-deg-dist / edge_conv: they read the two end nodes and their prior degrees
    only) scores all N columns of the rank's rows in one kernel (allpairs_mlp_topk; chunked rows under wide_rows: allpairs_mlp_topk_wide)
    under no / hash / symmetric hash noise keyed on the global pair; DESIGN.md has the step's kernel sequence.  u-v-A_uv joins them when
    the candidates carry a prior graph (scorer["prior"], replicated like the prior degrees): the same two kernels' _prior entries look a
    pair's stored value up on the rank's row range and return it per kept slot, which is all the backward reads."""

    PARAM_KEYS = ("We", "be", "Wk", "bk", "W1", "b1", "Wmu", "bmu", "Wp", "bp", "Wc")

    def __init__(self, kern, N, group=None, K=64, t=-0.05, noise_mode=2, seed=(1234, 0), mode=0, algo=0, x_grad=False, x_full=None,
                 hybrid=False, cand=None):
        if not isinstance(kern, (KernelContract, types.ModuleType)):
            # an OBJECT that does not inherit the contract (a stand-in written before there was one; the earlier version of this
            # project's host tests has such a class): the contract becomes a base of its class, behind its own names.  A module --
            # dgg_amd.ops -- is never touched: a contract name it lacks raises AttributeError where it is called.
            kern.__class__ = type(type(kern).__name__, (type(kern), KernelContract), {})
        self.kern, self.N, self.group = kern, N, group
        # cand = (rowptr int64 [N+1], col int32 [E]): the candidates of row i are the stored entries of in_adj (edge-list mode, the
        # live class's semantics dgm.py:1613-1614) instead of all N columns; every candidate is scored (per-pair hash noise), the rest
        # of the step is the same.  The WHOLE graph's candidates: on a row shard the step slices its rows' part once per graph
        # (_cand_rows) and runs the row-range forms of the edge-list kernels with replicated features.  A citation graph's step is
        # launch-bound (Pubmed: 0.29 ms fused on one GPU) and gains nothing from a shard; where larger edge lists stop being
        # launch-bound has not been measured.
        self.cand = cand
        # scorer: None = exp(t ||xp_i - xp_j||) (u-v-dist), or a dict with the edge-MLP scorer's terms in the per-node / per-edge form
        # of dgg_edge_mlp_fwd (reference dgm.py:1628-1719): Wcat [2hw,h], wdu / wdv / wex [hw] or None, b1 [hw], w2 [hw], b2 [1],
        # ex_mode, t_ex, act and, on edge-list candidates, erow int32 [E] and ex_in [E] or None (all-pairs candidates have no per-edge
        # inputs: ex_mode 0 or 2, or ex_mode 1 with prior = (rowptr int64 [N+1], col int32, val float32), the whole prior graph's CSR
        # arrays, in which the search looks up the extra of a pair -- u-v-A_uv; hw and h in {16, 32, 64, 128}).  backward() then also
        # returns g["scorer"] = {Wcat, wdu, wdv, wex, b1, w2, b2} (the rest of the step is the same; the prior's values get no gradient)
        self.scorer = None
        assert cand is None or noise_mode in (0, 2, 3), "edge-list candidates: noise_mode none / hash / symmetric hash"
        assert x_full is None or not x_grad, "replicated features are data: they cannot take a gradient"
        assert not hybrid or x_full is not None, "the hybrid scheme replicates the features for the scoring side"
        self.x_full = x_full                                 # [N,d] static node features present on every rank, or None
        self.hybrid = bool(hybrid)                           # replicated xp, all-gathered H, reduce-scattered dH (module docstring)
        # Two independent kernels of the step run beside their neighbours on a SECOND stream (captured into the same hipGraph): the
        # partition's sort (read by the backward only) beside the forward aggregation, and the k-net backward (needs only dk, MFMA-
        # bound) beside the per-destination kernel of the score backward (gather-bound).  DGG_OVERLAP=0 keeps everything on one stream.
        # DGG_OVERLAP: 2 (default) = only the k-net backward beside the score backward's column kernel; 1 = also the partition's sort
        # beside the aggregation; 3 = only the sort; 0 = one stream.  Round 6, same box, ms per step: 1.233 (2), 1.234-1.237 (1),
        # 1.244-1.246 (0), 1.252-1.255 (3): the sort beside the gather-bound aggregation LOSES 8 us (it stretched from 36 to 168 us and
        # took the aggregation with it), the MFMA-bound k-net backward beside the gather-bound column kernel wins 11
        ov = os.environ.get("DGG_OVERLAP", "2")
        self.overlap = ov != "0"
        self.overlap_sort, self.overlap_knet = ov in ("1", "3"), ov in ("1", "2")
        self._side = None
        # normalize_adj inside the forward aggregation (partp_build(want_ahat=False) + spmm_norm_fwd) instead of the partition's fill
        # pass; DGG_NORM_IN_SPMM=0 keeps the fill pass's ahat + spmm_fwd
        self.norm_in_spmm = os.environ.get("DGG_NORM_IN_SPMM", "1") != "0"
        # the k-net inside the projection kernel (_project_knet); DGG_FUSE_KNET=0 keeps linear_fwd_multi + knet_x_fwd_slim
        self.fuse_knet = os.environ.get("DGG_FUSE_KNET", "1") != "0"
        self.K, self.t, self.noise_mode, self.seed, self.mode, self.algo, self.x_grad = K, t, noise_mode, seed, mode, algo, x_grad
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        # DGG_FORCE_COLLECTIVES=1 issues every collective even in a 1-rank group (exercises the RCCL calls on a 1-GPU box)
        self.coll = self.world > 1 or (dist.is_initialized() and os.environ.get("DGG_FORCE_COLLECTIVES") == "1")
        self.emulate = None
        self.r0, self.r1, self.per = shard_bounds(N, self.world, self.rank)
        assert cand is None or self.world == 1 or x_full is not None, "edge-list candidates on several ranks: replicated features (x_full)"
        self._cand_cache = None                              # (rows, weakrefs of rowptr / col, their slice): _cand_rows
        self._lens_cache = None                              # (weakref of the rows' rowptr, their n_i - 9.5): _chunk_layout_edge_list
        self.bufs = {}                                       # collective staging buffers, kept between steps
        # Rows wider than the 64-rank list (all-pairs candidates, ranked noise): the learned degree is unbounded (dgm.py:1580-1584) and
        # the reference ramps over the whole dense row (dgm.py:1402-1421).  wide_rows: "off" = the [rows,64] list whatever k (exact
        # while k_i + 9.5 <= 64; callers enforce the bound), "auto" = chunked rows (ops.chunk_layout: ceil(k_i + 8.5) + 1 ranks of every
        # row in chunks of 64) from the forward in which some row needs them -- ONE readback of the chunk count per forward --, "on" =
        # chunked rows always.  wide_cap = (chunks, lists per wavefront): a FIXED capacity instead of the readback (hipGraph capture;
        # the flags of the last forward are in self.wide_meta, read by check_wide()).
        self.wide_rows = "off"
        self.wide_cap = None
        self.wide_meta = None
        self.wide_sticky = None                              # int32[1] on the device: overflow flags of every forward under wide_cap
        # symmetric noise (noise_mode 5, the ranked symmetric generator): sym_fallback = redo a forward it cannot settle under the
        # symmetric per-pair hash (noise_mode 3) and stay there (sym_hash); off by default for the bare engine (bench.py times the
        # generator it names), on for the nn.Module mirror
        self.sym_fallback = False
        self.sym_hash = False
        # force_chunked: rows that fit the 64-rank list go through the chunked rows' evaluator as well (one chunk per row).  Set by the module
        # once the ranked symmetric generator has failed on its data -- latents spread over several noise scales -- because the 64-rank
        # entry of the per-pair hash noise guesses ONE threshold for the graph from the noise law alone and loses every row to its
        # exhaustive fallback on such data (145-170 ms at N = 100 000, features x4), while the chunked rows' front end filters on
        # G + lpub_i with a threshold per row (6-9 ms on the same data; 2-3x the 64-rank entry where that one works)
        self.force_chunked = False
        self.tight_bound = "off"                             # ranked search: row-minimum distance bound in its stop tests (_row_bound)
        self._tight_on, self._tight_n, self.tight_probe = False, 0, None
        # allpairs_topk takes `status=` (KernelContract.rsym_status): true of dgg_amd.ops, not of a stand-in built on the contract
        self._rsym_status = not isinstance(kern, KernelContract)
        self.overflow = None                                 # int32[1] device flag the caller owns: the K-wide edge list dropped a weighted rank
        self.want_backward = True                            # False (the autograd node, no backward can follow): the partition is not sorted
        self.rsym_err = None                                 # ranked symmetric generator out of workspace: device flags since check_generator()
        self.rsym_last = None                                # ... and all status words of the last forward that ran it
        self.last_layout = None                              # (chunks, widest row) of the last chunk layout that was read back
        self.saved = None                                    # the last forward's state (keys: the stages' docstrings); read by backward()
        self._fwd_gen = 0                                    # forwards so far: saved["gen"] ties a backward to its forward
        self._stats_ref, self._stats_ver, self._stats = None, None, None     # degree statistics of the last prior-degree tensor (_learned_degree)

    def check_generator(self):
        """raises if the ranked symmetric noise generator (noise_mode 5) could not settle every row inside its workspace in any
        forward since the last call (one synchronisation; the rows concerned came back empty)"""
        err, self.rsym_err = self.rsym_err, None
        if err is not None and bool(err.any()):
            raise RuntimeError("ShardedDGGConv: the ranked symmetric noise generator ran out of workspace for its dense tier; "
                               "use noise_mode 3 (per-pair hash) for this data")

    def check_wide(self):
        """raises if a forward under a fixed chunk capacity (wide_cap) could not hold every row's ranks since the last call (one
        synchronisation).  The flags come from a device word that the layout kernel only ever ORs into (`wide_sticky`): every replay of a
        captured step is covered, not just the last one.  An overflowing forward is memory-safe -- the layout is cut to the capacity on
        the device -- but its cut rows are wrong: re-capture with a larger wide_cap."""
        st = self.wide_sticky
        meta, self.wide_meta = self.wide_meta, None
        if st is None:
            return
        flags = int(st.item())
        if flags:
            st.zero_()
            total, widest = (int(v) for v in meta[:2].cpu()) if meta is not None else (-1, -1)
            raise RuntimeError(f"ShardedDGGConv: the chunked rows outgrew their fixed capacity {self.wide_cap} (flags {flags}: 2 = more chunks than "
                               f"the capacity, 1 = a row wider than its lists, 4 = a learned degree is NaN; last forward: {total} chunks needed, "
                               f"widest row {widest}): re-capture with a larger wide_cap")

    WIDE_NOISE = {0: 0, 2: 2, 3: 3, 4: 4, 5: 3}      # noise_mode -> the generator wide rows are evaluated under (ranked symmetric: the
                                                     # symmetric per-pair hash -- same law, another realisation; no wide-row form of its own)

    def _chunk_layout(self, k):
        """-> ops.ChunkLayout for this forward's learned degrees, or None: every row fits the 64-rank list (or wide_rows is off).
        Edge-list candidates: _chunk_layout_edge_list"""
        kern = self.kern
        if self.wide_rows == "off" or self.noise_mode not in self.WIDE_NOISE or self.K != 64:
            return None
        if self.cand is not None:
            return self._chunk_layout_edge_list(k)
        if self.wide_cap is not None:
            if self.wide_sticky is None or self.wide_sticky.device != k.device:
                # (allocated by the first forward that runs with a capacity -- normally an eager warm-up; inside a capture the fill below
                #  would be replayed, i.e. the word would only cover one replay)
                self.wide_sticky = torch.zeros((1,), device=k.device, dtype=torch.int32)
            lay = kern.chunk_layout(k, maxm=int(self.wide_cap[1]), ccap=int(self.wide_cap[0]), sticky=self.wide_sticky)
            if lay is not None:
                self.wide_meta = lay.meta
            return lay
        assert not (k.is_cuda and torch.cuda.is_current_stream_capturing()), \
            "ShardedDGGConv: chunked rows inside a hipGraph capture need a fixed capacity (wide_cap = (chunks, lists))"
        lay = kern.chunk_layout(k, ncols=self.N)
        if lay is None:
            return None
        self.last_layout = (lay.chunks, lay.maxm)
        chunked = lay.wide or self.force_chunked
        if self.coll and self.noise_mode == 5:
            # the ranked symmetric generator has no wide-row form: chunked rows are evaluated under the symmetric per-pair hash
            # (WIDE_NOISE), and G_ij of one rank must be G_ji of the other -- so every rank takes the generator of the rank that needs
            # it (one MAX all-reduce of the deciding flags; the readback above has synchronised already)
            flags = torch.tensor([int(lay.wide), int(self.force_chunked), int(self.sym_hash)], dtype=torch.int32, device=k.device)
            dist.all_reduce(flags, op=dist.ReduceOp.MAX, group=self.group)
            wide_any, force_any, sym_hash_any = (bool(v) for v in flags.tolist())
            chunked = wide_any or force_any
            self.sym_hash = sym_hash_any
        if not chunked and self.wide_rows == "auto":
            return None
        return lay

    def _chunk_layout_edge_list(self, k):
        """_chunk_layout on edge-list candidates (wide_rows "auto" only; no fixed capacity, so not inside a capture): the layout of the
        CLAMPED degrees min(k_i, n_i - 9.5) of the rank's rows -- row i gets the chunks of its min(n_i, ceil(k_i + 8.5) + 1) ranks that can
        carry weight, so a row with 3 candidates and k = 1000 gets one chunk -- or None while every row fits the 64-rank list (the list
        kernels then run, unchanged).  The kernels, the ramp and every backward keep the true k.  Each rank decides from its own rows:
        edge lists always use the per-pair hash keyed on global ids, and no collective depends on the layout."""
        if self.wide_rows != "auto" or self.wide_cap is not None or (k.is_cuda and torch.cuda.is_current_stream_capturing()):
            return None
        rowptr = self._cand_rows()[0]
        ent = self._lens_cache                               # (n_i - 9.5 of the rank's rows, cached on the candidate slice's identity)
        if ent is None or ent[0]() is not rowptr:
            ent = self._lens_cache = (weakref.ref(rowptr), (rowptr[1:] - rowptr[:-1]).to(torch.float32) - 9.5)
        lay = self.kern.chunk_layout(torch.minimum(k, ent[1]), ncols=self.N)
        if lay is None:
            return None
        self.last_layout = (lay.chunks, lay.maxm)
        return lay if lay.wide else None

    def _row_bound(self, xp, k):
        """-> lpub [own rows] or None.  The ranked search bounds the score of the ranks it has not reached by their noise alone, i.e. as
        if they sat at distance 0; on latents whose distances spread over several noise scales it then walks ~ exp(spread / 0.3) times
        deeper than it has to (bench.py data_regimes: 2 blocks of 64 ranks per row on unit-scale features, 2 000 at x16).  With a
        lower bound of the distance to the row's nearest OTHER node (kern.rowmin_logp_bound: one fp16-MFMA sweep over all pairs, ~1.4 ms
        at N = 100 000) the same stop test uses G + log p_max(i).  tight_bound: "off" | "on" | "auto" = on when a pilot walk (~1000
        sampled rows, 64-block budget, every 16th forward and never inside a capture) puts the search's cost above 2.5 x the sweep's."""
        kern = self.kern
        if self.tight_bound == "off" or xp.shape[1] not in KERNEL_WIDTHS or self.t >= 0:
            return None
        if self.tight_bound == "auto":
            capturing = xp.is_cuda and torch.cuda.is_current_stream_capturing()
            if not capturing and self._tight_n % 16 == 0:
                seed = self.seed
                if torch.is_tensor(seed):
                    sd = seed.cpu()
                    seed = (int(sd[0]) & 0xFFFFFFFF, int(sd[1]) & 0xFFFFFFFF)
                pr = kern.ranked_probe(xp, k, self.t, seed, rows=(self.r0, self.r1), stride=max(1, (self.r1 - self.r0) // 1024), max_blocks=64)
                if pr is None:
                    return None
                est = kern.ranked_cost_estimate(pr, self.N, rows=self.r1 - self.r0)
                sweep_us = 1400.0 * (self.N / 1e5) * ((self.r1 - self.r0) / 1e5) * (xp.shape[1] + 16) / 80.0
                self._tight_on = est > 2.5 * sweep_us and self.N >= 8192
                self.tight_probe = dict(pr, ranked_us_estimate=est, sweep_us_estimate=sweep_us)
            if not capturing:
                self._tight_n += 1
            if not self._tight_on:
                return None
        return kern.rowmin_logp_bound(xp, self.t, rows=(self.r0, self.r1))

    def _cand_rows(self):
        """-> (rowptr, col, (e0, e1)) of the rank's rows: the whole graph's own tensors when the rank holds every row, else the rebased
        CSR slice (csr_rows), made on the device once per graph -- cached on the candidate tensors' identity (adjacency._cached keeps one
        pair per graph object) -- so that a step reads nothing back"""
        rowptr, col = self.cand
        if (self.r0, self.r1) == (0, self.N):
            return rowptr, col, (0, int(col.shape[0]))
        ent = self._cand_cache
        if ent is not None and ent[0] == (self.r0, self.r1) and ent[1]() is rowptr and ent[2]() is col:
            return ent[3]
        got = csr_rows(rowptr, col, (self.r0, self.r1))
        self._cand_cache = ((self.r0, self.r1), weakref.ref(rowptr), weakref.ref(col), got)
        return got

    def emulate_rank(self, world, rank):
        """TIMING DIAGNOSTIC (bench.py --emulate-world): do the work of `rank` of `world` in a single process -- own row range
        against all N columns, replicated features -- with the collectives left out and the other ranks' row sums faked by
        tiling the own ones.  Results are not meaningful; the kernel sequence and sizes are those of the real rank."""
        assert self.x_full is not None and not dist.is_initialized()
        self.world, self.rank, self.coll, self.emulate = world, rank, False, (world, rank)
        self.r0, self.r1, self.per = shard_bounds(self.N, world, rank)

    # ------------------------------------------------------------------------------------------------------------------
    def _linear_fwd_multi(self, x, layers):
        """several layers on one input: one GEMM that reads x once when the kernel namespace offers it (ops.linear_fwd_multi; the
        multi entry reaches the persistent register kernel for large N), one plain call per layer otherwise"""
        got = self.kern.linear_fwd_multi(x, layers)
        if got is None:
            got = [self.kern.linear_fwd(x, W, b, act, lay) for W, b, act, lay in layers]
        return got

    def _project(self, x_local, P):
        """-> xp (rows of `Xall`), H (rows of `Xall`; hybrid: the rank's OWN rows), xk (own rows)"""
        repl = self.x_full is not None
        Xall = self.x_full if repl else x_local
        le, lk, lc = (P["We"], P["be"], 1, 0), (P["Wk"], P["bk"], 1, 0), (P["Wc"], None, 0, 1)
        if not repl or (self.world == 1 and self.emulate is None):           # the own rows are all the rows that are projected
            xp, xk, H = self._linear_fwd_multi(Xall, [le, lk, lc])
        elif self.hybrid:
            (xp,) = self._linear_fwd_multi(Xall, [le])
            xk, H = self._linear_fwd_multi(x_local, [lk, lc])
        else:
            xp, H = self._linear_fwd_multi(Xall, [le, lc])
            xk = self.kern.linear_fwd(x_local, *lk)
        return xp, H, xk

    def _side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream()
        return self._side

    def _hyb(self):
        """the hybrid exchange is live: several ranks (or their single-process emulation) on replicated features"""
        return self.hybrid and self.x_full is not None and (self.coll or self.emulate is not None)

    def forward(self, x_local, deg_full, P):
        """One forward per backward: `saved` holds views of the persistent collective buffers (the gathered xp / H / row sums),
        which the next forward overwrites."""
        s = {}
        self._fwd_gen += 1
        fused = self._project_knet(s, x_local, deg_full, P)
        if fused is None:
            xp, H, xk = self._project(x_local, P)
        else:
            xp, H, xk = fused
        s["xp_loc"], s["H_loc"], s["xk"] = xp, H, xk
        g_xp, g_H = self._start_gathers(xp, H)
        if fused is None:
            self._learned_degree(s, deg_full, P)
        s["xp"] = xp if g_xp is None else g_xp.get()
        s["idx"], s["val"], s["w"], rs_local = self._search(s, deg_full)
        s["rs"] = self._gather_row_sums(rs_local)
        self._partition(s, rs_local)
        s["H"] = self._gathered_H(H, g_H)
        lkw = {} if s["layout"] is None else {"layout": s["layout"]}
        got = None
        if s["ahat"] is None:                       # the partition kept rs_j^-1/2 only: the aggregation normalises and returns ahat
            got = self.kern.spmm_norm_fwd(s["idx"], s["w"], rs_local, s["partp"], s["H"], 2, **lkw)
            if got is None:                         # (e.g. a gathered H that is not 16-byte aligned: the normalisation kernel, then the pair)
                s["ahat"] = self.kern.normalize_fwd(s["idx"], s["w"], s["rs"], self.r0)
        if got is not None:
            s["Z"], s["ahat"] = got
        else:
            s["Z"] = self.kern.spmm_fwd(s["idx"], s["ahat"], s["H"], 2, **lkw)    # relu(A (x Wc))
        s["gen"] = self._fwd_gen
        self.saved = s
        return s["Z"]

    def _start_gathers(self, xp, H):
        """-> (gather of xp or None, gather of H or None), both running"""
        if self.coll and self.x_full is None:       # xp first (the top-k waits for it), H streams in behind it
            return (_Gather(xp, self.N, self.per, self.group, True, self.bufs, "xp"),
                    _Gather(H, self.N, self.per, self.group, True, self.bufs, "H"))
        if self._hyb() and self.coll:               # H of the own rows only: gathered behind the k-net, the search and the partition
            return None, _Gather(H, self.N, self.per, self.group, True, self.bufs, "H")
        return None, None

    def _degree_stats(self, s, deg_full):
        """Writes s: mu_sd (cached on the degree tensor), deg_local -> both"""
        # mean / std of the prior degrees (dgm.py:1569-1570): an INPUT statistic -- recomputed only when the degree tensor changes
        # (keyed on the tensor OBJECT and its version counter, not on its address: a new tensor is always re-read)
        ref = self._stats_ref
        if ref is None or ref() is not deg_full or self._stats_ver != deg_full._version:
            self._stats_ref, self._stats_ver, self._stats = weakref.ref(deg_full), deg_full._version, self.kern.degree_stats(deg_full)
        s["mu_sd"] = self._stats
        s["deg_local"] = deg_full[self.r0:self.r1].contiguous()
        return s["mu_sd"], s["deg_local"]

    def _project_knet(self, s, x_local, deg_full, P):
        """The three projections AND the learned degree in one kernel (kern.project_knet) -> xp, H, xk with s: mu_sd, deg_local, k, u,
        z, feat written as _learned_degree writes them; None = this route takes _project + _learned_degree.  Only where all three
        projections read the rank's own rows (the first branch of _project) and the k-net is the matrix-core one; DGG_FUSE_KNET=0
        keeps the two calls."""
        if not self.fuse_knet or not (self.x_full is None or (self.world == 1 and self.emulate is None)):
            return None
        if P["Wk"].shape[0] not in self.kern.KNET_MFMA_WIDTHS:
            return None
        Xall = self.x_full if self.x_full is not None else x_local
        mu_sd, deg_local = self._degree_stats(s, deg_full)
        got = self.kern.project_knet(Xall, [(P["We"], P["be"], 1, 0), (P["Wk"], P["bk"], 1, 0), (P["Wc"], None, 0, 1)], 1, deg_local, mu_sd,
                                     P["W1"], P["b1"], P["Wmu"], P["bmu"], P["Wp"].reshape(-1), P["bp"])
        if got is None:
            return None
        (xp, xk, H), s["k"], s["u"] = got
        s["z"] = s["feat"] = None
        return xp, H, xk

    def _learned_degree(self, s, deg_full, P):
        """prior-degree statistics (cached on the degree tensor) + k-net.  Reads s: xk.  Writes s: mu_sd, deg_local, k, u and z, feat
        (None on the matrix-core k-net, whose backward re-runs layer 1)."""
        kern, xk = self.kern, s["xk"]
        mu_sd, deg_local = self._degree_stats(s, deg_full)
        if xk.shape[1] in kern.KNET_MFMA_WIDTHS:
            # k-net on the matrix cores: the forward saves only u; the backward re-runs layer 1 from xk and forms every gradient in one pass
            s["k"], s["u"] = kern.knet_x_fwd_slim(xk, deg_local, mu_sd, P["W1"], P["b1"], P["Wmu"], P["bmu"], P["Wp"].reshape(-1), P["bp"])
            s["z"] = s["feat"] = None
        else:
            s["k"], s["z"], s["u"], s["feat"] = kern.knet_x_fwd(xk, deg_local, mu_sd, P["W1"], P["b1"], P["Wmu"], P["bmu"],
                                                              P["Wp"].reshape(-1), P["bp"])

    def _search(self, s, deg_full):
        """scores + perturbation + top-K + ramp of the rank's rows -> idx, val, w, rs_local.  Reads s: xp (all N rows), k.  Writes s:
        layout (the chunk layout of rows wider than 64 ranks, or None) and, on edge lists, ncand, with a scorer also AB, sdeg, ex, eid."""
        kern, xp, k = self.kern, s["xp"], s["k"]
        s["layout"] = None
        if self.cand is not None:
            return self._search_edge_list(s, deg_full)
        if self.scorer is not None:
            return self._search_allpairs_mlp(s, deg_full)
        if self.noise_mode == 4 and self.K == 64 and xp.shape[1] in RSYM_WIDTHS:
            # ranked noise: the ramp is applied inside the search kernel, while the settled list is still in registers
            s["layout"] = lay = self._chunk_layout(k) if xp.shape[1] in KERNEL_WIDTHS else None
            lkw_ = {}
            lp = self._row_bound(xp, k)             # upper bounds of log p over a row's other nodes, when the walk is deep enough to pay for them
            if lp is not None:
                lkw_["lpub"] = lp
            if lay is not None:                     # rows wider than 64 ranks: ceil(k_i + 8.5) + 1 ranks of every row, in chunks of 64
                got = kern.allpairs_topk_wide(xp, k, lay, self.mode, self.t, self.seed, rows=(self.r0, self.r1), **lkw_)
            else:
                got = kern.allpairs_topk_softk(xp, k, self.mode, self.t, self.seed, rows=(self.r0, self.r1), **lkw_)
            if got is not None:
                return got
        # the generators without a row-wise early-stopping search (unperturbed scores, per-pair hash noise, the ranked symmetric
        # generator).  Rows wider than 64 ranks: chunked rows through the threshold-buffer evaluator (any width; the reference's
        # defaults symmetric_noise=True / perturb_edge_prob=False train into this regime like every other configuration)
        s["layout"] = lay = self._chunk_layout(k) if (xp.shape[1] in KERNEL_WIDTHS and self.mode in (0, 1)) else None
        if lay is not None:
            return kern.allpairs_topk_wide(xp, k, lay, self.mode, self.t, self.seed, rows=(self.r0, self.r1),
                                           noise_mode=self.WIDE_NOISE[self.noise_mode])
        nm = 3 if (self.noise_mode == 5 and self.sym_hash) else self.noise_mode
        # sym_fallback: a forward the ranked symmetric generator cannot settle (its dense tier overflows: data-dependent)
        # is redone under the symmetric per-pair hash, and the layer stays with it (one flag read back per forward; not
        # inside a capture, not across ranks -- every rank would have to take the same decision)
        # (st None under noise_mode 5: a stand-in kernel namespace without the status plumbing)
        st = {"sym_fallback": self.sym_fallback and self.world == 1} if (nm == 5 and self._rsym_status) else None
        kw = {} if st is None else {"status": st}
        idx, val = kern.allpairs_topk(xp, self.K, self.t, nm, None, self.seed, rows=(self.r0, self.r1), algo=self.algo, k_limit=k, **kw)
        if st and st.get("rsym_fell_back"):
            self.sym_hash = True
        if st and st.get("rsym_err") is not None:      # ranked symmetric generator out of workspace: device flag, read by check_generator()
            self.rsym_err = st["rsym_err"] if self.rsym_err is None else (self.rsym_err | st["rsym_err"])
            self.rsym_last = st                     # (all three status words of this forward: the module mirror keeps its own tally)
        return (idx, val) + tuple(kern.softk_fwd(idx, val, k, self.mode))

    def _search_edge_list(self, s, deg_full):
        """_search on edge-list candidates (cand), u-v-dist or the edge-MLP scorer, on the 64-rank list or on chunked rows.  Writes s:
        layout, ncand and with a scorer AB, sdeg, ex (per candidate on the list, per kept slot -- flat -- on chunked rows), eid (None on
        chunked rows, whose backward runs in CSR form on the flattened chunks)"""
        kern, xp, k = self.kern, s["xp"], s["k"]
        # a row shard: its rows' rebased CSR slice and the row-range entries (rows=); the whole graph: exactly the one-rank calls
        rowptr, col, (e0, e1) = self._cand_rows()
        rk = {} if (self.r0, self.r1) == (0, self.N) else {"rows": (self.r0, self.r1)}
        s["ncand"] = int(col.numel())
        # rows wider than 64 ranks whose learned degrees need them (wide_rows "auto"): min(n_i, ceil(k_i + 8.5) + 1) ranks of every row in
        # chunks of 64, the ramp fused into the search; None: every row fits the list, and the list kernels run as they always have
        s["layout"] = lay = self._chunk_layout(k) if (xp.shape[1] in KERNEL_WIDTHS and self.mode in (0, 1)) else None
        if self.scorer is not None:
            # edge-MLP scorer: first layer split into per-node products AB = xp [Wa | Wb]^T (MFMA GEMM, all N nodes) + per-edge terms
            sc = self.scorer
            erow, ex_in = sc["erow"], sc["ex_in"]
            if rk:                                  # (views: the shard's entries of the per-edge inputs)
                erow, ex_in = erow[e0:e1], (None if ex_in is None else ex_in[e0:e1])
            s["AB"] = AB = kern.linear_fwd(xp, sc["Wcat"], None, 0, 0)
            s["sdeg"] = sdeg = deg_full if sc["wdu"] is not None else None
            p_edge, s["ex"] = kern.edge_mlp_fwd(AB, xp, erow, col, sdeg, ex_in, sc["ex_mode"], sc["t_ex"], sc["wdu"], sc["wdv"],
                                                sc["wex"], sc["b1"], sc["w2"], sc["b2"], sc["act"])
            if lay is not None:
                # (ex per kept slot, flat; no eid: the backward runs in CSR form on the flattened chunks, _scorer_backward_chunked)
                got = kern.edgelist_topk_p_chunked(p_edge, self.N, rowptr, col, k, lay, self.mode, self.noise_mode, self.seed, ex_edge=s["ex"], **rk)
                if got is None:
                    raise NotImplementedError("ShardedDGGConv: the kernel namespace has no edgelist_topk_p_chunked (edge-list candidates, "
                                              "edge-MLP scorer, chunked rows)")
                idx, val, ex, w, rs_local = got
                s["ex"], s["eid"] = (None if ex is None else ex.reshape(-1)), None
                return idx, val, w, rs_local
            idx, val, s["eid"] = kern.edgelist_topk_p(p_edge, self.N, rowptr, col, self.K, self.noise_mode, None, self.seed, **rk)
            return (idx, val) + tuple(kern.softk_fwd(idx, val, k, self.mode))
        if lay is not None:
            got = kern.edgelist_topk_chunked(xp, rowptr, col, k, lay, self.mode, self.t, self.noise_mode, self.seed, **rk)
            if got is None:
                raise NotImplementedError("ShardedDGGConv: the kernel namespace has no edgelist_topk_chunked (edge-list candidates, chunked rows)")
            return got
        got = kern.edgelist_topk_softk(xp, rowptr, col, k, self.mode, self.K, self.t, self.noise_mode, None, self.seed,
                                       overflow=self.overflow, **rk)
        if got is not None:                         # search + ramp in one launch
            return got
        idx, val = kern.edgelist_topk(xp, rowptr, col, self.K, self.t, self.noise_mode, None, self.seed, **rk)
        return (idx, val) + tuple(kern.softk_fwd(idx, val, k, self.mode))

    MLP_NOISE = {0: 0, 2: 2, 3: 3, 4: 2, 5: 3}       # noise_mode -> the generator an edge-MLP scorer's all-pairs rows are evaluated under:
                                                     # every pair is scored, so the ranked generators (an early-stopping search) give way
                                                     # to the per-pair hash of the same law, as in the separate modules

    def _search_allpairs_mlp(self, s, deg_full):
        """_search with an edge-MLP scorer on all-pairs candidates: AB for all N nodes, then scorer + perturbation + top-K of the rank's
        rows against all N columns in one kernel.  Writes s: AB, sdeg, ex (per slot, flat), eid (the slot index; None on chunked rows,
        whose backward runs in CSR form on the flattened chunks), layout."""
        kern, xp, k, sc = self.kern, s["xp"], s["k"], self.scorer
        assert self.world == 1 or self.x_full is not None, "an edge-MLP scorer on several ranks: replicated features (x_full)"
        assert self.noise_mode in self.MLP_NOISE, "edge-MLP scorer on all-pairs candidates: counter-based noise or none"
        nm = self.MLP_NOISE[self.noise_mode]
        rows = (self.r0, self.r1)
        s["AB"] = AB = kern.linear_fwd(xp, sc["Wcat"], None, 0, 0)
        s["sdeg"] = sdeg = deg_full if sc["wdu"] is not None else None
        terms = (AB, xp, sdeg, sc["ex_mode"], sc["t_ex"], sc["wdu"], sc["wdv"], sc["wex"], sc["b1"], sc["w2"], sc["b2"], sc["act"])
        # u-v-A_uv against a prior graph: the WHOLE graph's CSR arrays on every rank (the kernel looks up the pairs of its row range);
        # handed on only when the scorer carries one -- the contract's entries, and a stand-in written to them, take no prior=
        pk = {} if sc.get("prior") is None else {"prior": sc["prior"]}
        s["layout"] = lay = self._chunk_layout(k) if (xp.shape[1] in KERNEL_WIDTHS and self.mode in (0, 1)) else None
        if lay is not None:                         # rows wider than 64 ranks: ceil(k_i + 8.5) + 1 ranks of every row, the ramp fused
            got = kern.allpairs_mlp_topk_wide(*terms, k, lay, self.mode, nm, None, self.seed, rows=rows, **pk)
            if got is None:
                raise NotImplementedError("ShardedDGGConv: the kernel namespace has no allpairs_mlp_topk_wide (edge-MLP scorer, chunked rows)")
            idx, val, ex, w, rs_local = got
            s["ex"], s["eid"] = (None if ex is None else ex.reshape(-1)), None
            return idx, val, w, rs_local
        got = kern.allpairs_mlp_topk(*terms, self.K, nm, None, self.seed, rows=rows, **pk)
        if got is None:
            raise NotImplementedError("ShardedDGGConv: the kernel namespace has no allpairs_mlp_topk (edge-MLP scorer on all-pairs candidates)")
        idx, val, ex = got
        s["ex"] = None if ex is None else ex.reshape(-1)
        eid = self.bufs.get("eid")                  # (an entry's extra is at its slot: the same arange every step)
        if eid is None or eid.shape != idx.shape or eid.device != idx.device:
            eid = self.bufs["eid"] = torch.arange(idx.numel(), device=idx.device, dtype=torch.int32).view(idx.shape)
        s["eid"] = eid
        return (idx, val) + tuple(kern.softk_fwd(idx, val, k, self.mode))

    def _gather_row_sums(self, rs_local):
        """-> the row sums of all N nodes (emulation: the other ranks' faked by tiling the own ones)"""
        if self.emulate is not None:
            return rs_local.repeat(self.world)[:self.N].contiguous()
        return _all_gather_rows(rs_local, self.N, self.per, self.group, self.bufs, "rs") if self.coll else rs_local

    def _partition(self, s, rs_local):
        """destination-bucket partition of the active entries: the backward's column-side terms run on it (no atomics).  Reads s: idx,
        w, val, rs, layout, xp, H_loc.  Writes s: partp (payload form -- records carry w rs_i^-1/2 and the score, no slot map,
        normalize_adj fused into its fill pass -- when the namespace offers it and covers the shape), else part (index form), ahat,
        partp_sorted (False: want_backward was off and the sort was not launched), side_join (the sort runs on the side stream).
        With norm_in_spmm, where the namespace normalises inside the aggregation (spmm_norm_fwd; 64-rank lists or chunked rows, conv
        width 16 / 32 / 64), ahat stays None for forward() to take from spmm_norm_fwd.  DGG_NORM_IN_SPMM=0: ahat from the fill pass."""
        kern, rs, lay = self.kern, s["rs"], s["layout"]
        use_p = s["xp"].shape[1] in KERNEL_WIDTHS and s["H_loc"].shape[1] in KERNEL_WIDTHS and self.mode in (0, 1)
        use_n = use_p and self.norm_in_spmm and s["idx"].shape[1] == 64 and s["H_loc"].shape[1] in (16, 32, 64)
        ov = use_p and self.overlap and self.overlap_sort and s["idx"].is_cuda
        # want_backward = False (set by the autograd node under torch.no_grad() / frozen parameters): the per-bucket sort of the
        # partition -- read by the backward's column kernels only -- is not launched at all (an eval forward used to
        # leave it running on the side stream with nothing ever joining it)
        nobwd = use_p and not self.want_backward
        lkw = {} if lay is None else {"layout": lay}
        # two independent choices.  Who normalises: the fill pass (ahat comes back) or the aggregation (records only).  Which stages:
        # all three (0); count + fill (1: the sort runs on the side stream, or never -- the fill pass must still write ahat); the
        # count pass alone (3: no backward follows and the aggregation normalises from the rs_j^-1/2 table)
        want_ahat = not use_n
        stages = 3 if (use_n and nobwd) else (1 if (ov or nobwd) else 0)
        got = kern.partp_build(s["idx"], s["w"], s["val"], rs_local, self.N, rs, phase=stages, want_ahat=want_ahat, **lkw) if use_p else None
        assert lay is None or use_p, "chunked rows run on the payload partition (latent / conv widths 16, 32, 64, 128; soft modes)"
        s["partp"], s["ahat"] = got if got is not None else (None, None)
        s["side_join"] = False
        s["partp_sorted"] = not (nobwd and got is not None)
        if nobwd and got is not None:
            s["partp"].skip_sort()                  # (the records, if filled at all, stay in bucket order, unread)
        elif ov and got is not None:                # the sort runs beside the aggregation; the backward joins before its first column kernel
            main, side = torch.cuda.current_stream(), self._side_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                kern.partp_sort(s["partp"])
            if not torch.cuda.is_current_stream_capturing():
                s["partp"].ws.record_stream(side)
            s["side_join"] = True
        s["part"] = kern.part_build(s["idx"], s["w"], self.N) if s["partp"] is None else None
        if s["ahat"] is None and not (use_n and got is not None):
            s["ahat"] = kern.normalize_fwd(s["idx"], s["w"], rs, self.r0)

    def _gathered_H(self, H, g_H):
        """-> H of all N nodes: the finished gather, the projection itself, or under emulation the own rows in stale filler"""
        if g_H is not None:
            return g_H.get()
        if not self._hyb():
            return H
        Hf = _Gather._buf(self.bufs, ("H", "emu"), (self.N, H.shape[1]), H)     # (the other ranks' rows: a persistent buffer)
        if not self.bufs.get(("H", "emu_init")):
            Hf.copy_(H.repeat((self.N + H.shape[0] - 1) // H.shape[0], 1)[:self.N])
            self.bufs[("H", "emu_init")] = True
        Hf[self.r0:self.r1].copy_(H)
        return Hf

    def backward(self, dZ, x_local, P, dA_ext=None):
        """-> dict of parameter gradients (summed over ranks) and, if x_grad, 'x' = d loss / d x_local.
        dA_ext [rows,K] (optional): cotangent of the NORMALISED adjacency (saved["ahat"]) from consumers other than this layer's own
        aggregation (GCN_DGG's second layer reads the same adjacency); added to the aggregation's own before the score backward."""
        kern, s = self.kern, self.saved
        assert s is not None and s["gen"] == self._fwd_gen, "ShardedDGGConv: backward() must follow the forward() it differentiates " \
            "(a second forward has overwritten the gathered buffers)"
        assert s["partp_sorted"], "ShardedDGGConv: this forward ran with want_backward = False (its partition was not sorted)"
        # every zero-initialised accumulator of the backward from ONE filled buffer, where the namespace has such a pool
        ncols, h, F = s["xp"].shape[0], s["xp"].shape[1], s["H"].shape[1]
        rows = s["idx"].shape[0]
        # (payload path: dH / da / dxp / dA are written by their owner wavefronts, only the weight gradients are accumulated into)
        need = 3 * sum(int(v.numel()) for v in P.values()) + 65536
        if s["partp"] is None:
            need += rows * self.K + ncols * (h + F + 2)
        if self.scorer is not None:                  # row-major dA (zero outside the partition), dAB + parameter sums, dWcat, dxp
            need += rows * self.K + ncols * (2 * self.scorer["Wcat"].shape[0] + h) + 4 * int(self.scorer["Wcat"].numel()) + 4096
        pool = kern.zero_pool(s["xp"].device, need)
        if pool is None:
            return self._backward(dZ, x_local, P, dA_ext)
        with pool:
            return self._backward(dZ, x_local, P, dA_ext)

    def _reduce_scatter_rows(self, t, key, async_op=False):
        """[N, c] partial sums on every rank -> the rank's own rows [r1-r0, c], summed over ranks.  async_op: returns a callable
        that waits (a stream dependency on RCCL) and yields the rows -- the transfer runs behind the kernels issued meanwhile."""
        pad = self.world * self.per - self.N
        src = t
        if pad:
            src = _Gather._buf(self.bufs, (key, "rs_src"), (self.world * self.per, t.shape[1]), t)
            src[:self.N].copy_(t)
            src[self.N:].zero_()
        out = _Gather._buf(self.bufs, (key, "rs_out"), (self.per, t.shape[1]), t)
        src = src.contiguous()
        work = dist.reduce_scatter_tensor(out, src, group=self.group, async_op=async_op)
        if not async_op:
            return out[: self.r1 - self.r0]

        def get(_keep=src):
            work.wait()
            return out[: self.r1 - self.r0]
        return get

    def _backward(self, dZ, x_local, P, dA_ext=None):
        kern, s = self.kern, self.saved
        g = {}
        G = kern.act_bwd(s["Z"], dZ, 2)                  # cotangent of A H
        dA, dA_rec, dH, da, ahat_rows = self._conv_backward(G, dA_ext)
        # (da first: both collectives share one RCCL stream and da is an operand of the very next kernel; behind the 25-128 MB
        #  reduce-scatter it would wait for that transfer -- ADVICE round 4)
        if self.coll:
            dist.all_reduce(da, group=self.group)
        if self._hyb() and self.coll:               # dH [N,F] partial is complete here and needed only by the last kernel of the step
            dH = self._reduce_scatter_rows(dH, "dH", async_op=True)
        if self.scorer is not None:
            dxp, dk = self._scorer_backward(g, dA, da, ahat_rows)
            return self._weight_grads(g, dxp, dH, dk, x_local, P)
        if s["partp"] is None:
            dxp, dk = uvdist_score_bwd(kern, s["xp"], s["idx"], s["val"], s["k"], dA, s["rs"], da, self.r0, self.t, self.noise_mode != 0,
                                       self.mode, True, s["part"], ahat_rows)
            return self._weight_grads(g, dxp, dH, dk, x_local, P)
        dxp, dk, pre, kn = self._uvdist_backward_p(dA, dA_rec, da, P)
        return self._weight_grads(g, dxp, dH, dk, x_local, P, premasked=pre, knet=kn)

    def _conv_backward(self, G, dA_ext):
        """backward of Z = A H and the neighbour side of the normalisation backward, on whichever partition the forward built
        -> dA [rows,K] (None: read through the partition's map), dA_rec (payload form only), dH [N,F] partial, da [N], ahat_rows.
        ahat_rows = saved ahat: `da` holds the neighbour-side sums only and the consumer forms the row side (sqrt(rs_i) sum_r dA_ir
        ahat_ir) itself; None: `da` is d loss / d (rs^-1/2), both sides.  Reads s: idx, H, rs, w, ahat, partp, part, layout, side_join."""
        kern, s = self.kern, self.saved
        # one gather of G per edge for SDDMM + transposed SpMM + neighbour side of da; its companion is the fused score backward
        # (which adds the row side of da in registers), so both must cover the shape
        partp, part = s["partp"], s["part"]
        if partp is not None:                       # payload partition
            if s["side_join"]:                      # the partition's sort ran on the side stream
                torch.cuda.current_stream().wait_stream(self._side_stream())
                s["side_join"] = False
            # (dA of the entries outside the partition is masked by the row kernel -- ahat_rows is 0 there -- so it is not zero-filled)
            # Small graphs (the record-ordered dA fits an XCD's L2: Pubmed, 5 MB): no row-major dA -- the row kernel gathers the
            # record-ordered copy through the slot -> record map the partition's sort left (Pubmed step 0.359 -> 0.349 ms).  At
            # N = 100 000 (25.6 MB) the 4.1 M four-byte gathers cost the row kernel more (+70 us) than the scattered stores cost the
            # node kernel (-47 us): 1.264 -> 1.285 ms, so large graphs keep the scattered row-major copy.  DGG_DA_MAP=0/1 forces one.
            use_map = kern.DA_MAP and kern.partp_has_map(s["idx"].shape[0]) and self.scorer is None and s["layout"] is None
            kw = {"want_dA": False} if use_map else {}
            if dA_ext is not None:
                kw["dA_ext"] = dA_ext
            pc = kern.conv_bwd_cols_p(s["idx"], s["H"], G, partp, s["rs"], zero_dA=self.scorer is not None, **kw)
            assert pc is not None
            return pc + (s["ahat"],)
        cols = None
        if self.scorer is None and dA_ext is None and part is not None and s["xp"].shape[1] in KERNEL_WIDTHS and self.mode in (0, 1):
            cols = kern.conv_bwd_cols(s["idx"], s["ahat"], s["H"], G, part, s["rs"], True)
        if cols is not None:                        # index partition
            dA, dH, da = cols
            return dA, None, dH, da, s["ahat"]
        dA, dH = kern.spmm_bwd(s["idx"], s["ahat"], s["H"], G, True, True)      # atomic baseline
        if dA_ext is not None:                       # (the slot-wise total; the masked entries carry no weight either way)
            dA = dA + torch.where(s["idx"] >= 0, dA_ext, torch.zeros_like(dA_ext))
        pk = () if part is None else (part,)
        return dA, None, dH, kern.norm_bwd_da(s["idx"], s["w"], s["rs"], dA, self.r0, *pk), None

    def _uvdist_backward_p(self, dA, dA_rec, da, P):
        """ramp + normalisation + u-v-dist score backward on the payload partition -> dxp, dk, premasked, the k-net's gradients when
        its backward already ran beside the column kernel (else None).  Reads s: xp, idx, val, k, rs, ahat, partp, xk, deg_local,
        mu_sd, u, z."""
        kern, s = self.kern, self.saved
        # the activation derivative of the two LeakyReLU projections is applied by the kernels that PRODUCE dxp / dxk (they hold
        # xp_j / xk in registers): the fused weight-gradient product then reads no forward output for the mask (51 MB less)
        pre = self._premask()
        args = (s["xp"], s["idx"], s["val"], s["k"], dA, dA_rec, s["rs"], da, self.r0, self.t, self.noise_mode != 0, self.mode, True, s["partp"])
        kw = dict(ahat_rows=s["ahat"], out_act=1 if pre else 0)
        if not (self.overlap and self.overlap_knet and self.mode == 0 and s["z"] is None and s["idx"].is_cuda):
            dxp, dk = kern.softk_edge_bwd_p(*args, **kw)
            return dxp, dk, pre, None
        # row kernel -> dk; then the k-net backward on the side stream beside the per-destination kernel on this one
        dxp, dk, st = kern.softk_edge_bwd_p(*args, **kw, phase=1)
        main, side = torch.cuda.current_stream(), self._side_stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            kn = kern.knet_x_bwd_fused(s["xk"], s["deg_local"], s["mu_sd"], P["W1"], P["b1"], P["Wmu"], P["bmu"],
                                       P["Wp"].reshape(-1), s["u"], dk, out_act=1 if pre else 0)
        kern.softk_edge_bwd_p(*args, **kw, phase=2, state=st)
        main.wait_stream(side)
        if not torch.cuda.is_current_stream_capturing():
            dk.record_stream(side)
            for t_ in kn:
                t_.record_stream(main)
        return dxp, dk, pre, kn

    def _scorer_backward(self, g, dA, da, ahat_rows):
        """score backward of the edge-MLP scorer: ramp + normalisation backward by rows, then edge_mlp_score_bwd on the selected
        edges -> dxp, dk; writes g["scorer"].  da [N]: d loss / d (rs^-1/2), both sides (dgg_norm_bwd_da), or with ahat_rows the
        neighbour-side sums (the row side is then formed inside the row kernel, dgg_softk_bwd_rows).  Reads s: idx, val, k, rs, xp, AB,
        eid, sdeg, ex, layout and, for the payload form of the MLP's backward (edge-list candidates), partp, w, ncand."""
        kern, s, sc = self.kern, self.saved, self.scorer
        kw = {} if (self.r0, self.r1) == (0, self.N) else {"rows": (self.r0, self.r1)}
        if s["layout"] is not None:
            return self._scorer_backward_chunked(g, dA, da, ahat_rows, kw)
        akw = {} if ahat_rows is None else {"ahat_rows": ahat_rows}
        dval, dk = kern.softk_bwd(s["idx"], s["val"], s["k"], dA, s["rs"], da, self.r0, self.mode, True, **akw)
        # (all-pairs candidates keep the MLP backward's atomic form: the payload form sizes its scratch by the number of candidate
        #  edges, which is rows x N there -- and the separate modules run the atomic form too)
        if s["partp"] is not None and self.cand is not None and kern.EMLP_BWD_PARTP:
            kw.update(partp=s["partp"], w=s["w"], nrec_max=s["ncand"])       # (a selected entry is one of the rows' candidate edges)
        dxp, dex, g["scorer"] = edge_mlp_score_bwd(kern, sc, s["xp"], s["AB"], s["idx"], s["eid"], s["val"], dval, s["sdeg"], s["ex"],
                                                   self.noise_mode != 0, **kw)
        if sc["ex_mode"] == 2:                              # exp(t ||xp_u - xp_v||) as an edge feature also depends on the projection
            dxp = dxp + kern.edge_bwd(s["xp"], s["idx"], s["val"], dex, self.r0, sc["t_ex"], False)
        return dxp, dk

    def _scorer_backward_chunked(self, g, dA, da, ahat_rows, kw):
        """_scorer_backward on chunked rows (all-pairs or edge-list candidates: a chunked row does not say where it came from): ramp +
        normalisation backward by node over the row's chunks
        (softk_bwd_rows_chunked; da = the neighbour-side sums), then the MLP's backward in its CSR form on the flattened chunks -- row i's
        entries are [64 cptr[i], 64 cptr[i+1]), empty slots carry idx = -1 and are skipped; parameter sums in a fixed order -- and the
        distance term of u-v-deg-dist through csr_uvdist_bwd on the same pattern.  kw: rows= of a row shard."""
        kern, s, sc = self.kern, self.saved, self.scorer
        lay = s["layout"]
        assert ahat_rows is not None, "chunked rows run on the payload partition"
        got = kern.softk_bwd_rows_chunked(s["idx"], s["val"], s["k"], s["rs"], dA, da, ahat_rows, lay, self.r0, self.mode)
        if got is None:
            raise NotImplementedError("ShardedDGGConv: the kernel namespace has no softk_bwd_rows_chunked (edge-MLP scorer, chunked rows)")
        dval, dk = got
        rowptr = lay.cptr.to(torch.int64) * 64
        col = s["idx"].reshape(-1)
        dxp, dex, g["scorer"] = edge_mlp_score_bwd(kern, sc, s["xp"], s["AB"], col, None, s["val"].reshape(-1), dval.reshape(-1), s["sdeg"],
                                                   s["ex"], self.noise_mode != 0, rowptr=rowptr, **kw)
        if sc["ex_mode"] == 2:
            # (empty slots: ex = 0 from the forward and dex = 0 from the MLP backward's CSR form, so csr_uvdist_bwd skips them before it
            #  reads the column; the clamp only keeps a column it never uses inside the graph)
            dxp = dxp + kern.csr_uvdist_bwd(s["xp"], rowptr, col.clamp(min=0), s["ex"], dex, sc["t_ex"], **kw)
        return dxp, dk

    def _premask(self):
        """True when the step's weight gradients go through linear_bwd_multi (no input gradient) and the producers of dxp / dxk can
        apply LeakyReLU' themselves (ranked / k_times_edge_prob path on the HIP kernels)"""
        return bool(self.kern.PREMASK) and not self.x_grad and self.mode == 0 and self.saved["z"] is None and \
            not (self.coll and self.x_full is None)

    def _linear_bwd_multi(self, X, layers):
        """weight (and bias) gradients of layers that share the input X -> [(dW, db or None)]: one pass over X (leaky masks applied on
        the operand load) when the kernel namespace offers it, one linear_bwd per layer otherwise"""
        got = self.kern.linear_bwd_multi(X, layers)
        if got is None:
            got = [self.kern.linear_bwd(X, W, y, dy, act, lay, False, need_db)[1:] for W, y, dy, act, lay, need_db in layers]
        return got

    def _weight_grads(self, g, dxp, dH, dk, x_local, P, premasked=False, knet=None):
        """k-net backward (unless `knet` already holds it), weight gradients of the three projections, their all-reduce, d loss / dx.
        Reads s: xp, xp_loc, xk, deg_local, mu_sd, u, z, feat."""
        kern, s = self.kern, self.saved
        repl = self.x_full is not None
        # weight gradients of the two projections.  Replicated features: partial [dxp | dH] of all N nodes against the full X (the
        # weight all-reduce sums the ranks); gathered projections: reduce-scatter the partials, then the rank's own rows only.
        if self.coll and not repl:
            both = self._reduce_scatter_rows(torch.cat([dxp, dH], 1), "dproj")
            h = dxp.shape[1]
            dxp_g, dH_g, Xg, xp_g = both[:, :h].contiguous(), both[:, h:].contiguous(), x_local, s["xp_loc"]
        else:
            dxp_g, dH_g, Xg, xp_g = dxp, dH, (self.x_full if repl else x_local), s["xp"]
        if knet is not None:                         # already run (beside the score backward's column kernel)
            dxk, g["W1"], g["b1"], g["Wmu"], g["bmu"], dWp, g["bp"] = knet
        elif s["z"] is None:
            okw = {"out_act": 1} if premasked else {}
            dxk, g["W1"], g["b1"], g["Wmu"], g["bmu"], dWp, g["bp"] = kern.knet_x_bwd_fused(
                s["xk"], s["deg_local"], s["mu_sd"], P["W1"], P["b1"], P["Wmu"], P["bmu"], P["Wp"].reshape(-1), s["u"], dk, **okw)
        else:
            dxk, g["W1"], g["b1"], g["Wmu"], g["bmu"], dWp, g["bp"] = kern.knet_x_bwd(
                s["xk"].shape[1], s["mu_sd"], P["W1"], P["Wmu"], P["bmu"], P["Wp"].reshape(-1), s["z"], s["u"], s["feat"], dk)
        g["Wp"] = dWp.reshape(P["Wp"].shape)
        same_rows = Xg.shape[0] == x_local.shape[0] and (not repl or self.world == 1) and self.emulate is None
        ym, am = (None, 0) if premasked else (True, 1)          # premasked: dxp / dxk already carry LeakyReLU'
        le = (P["We"], xp_g if ym else None, dxp_g, am, 0, True)
        lk = (P["Wk"], s["xk"] if ym else None, dxk, am, 0, True)
        dX1 = dX2 = dX3 = None
        if self._hyb():
            # hybrid: dWe from the rank's PARTIAL dxp of all N nodes against the full X (summed by the weight all-reduce); dWk and dWc
            # from the rank's own rows -- dH_own = the reduce-scattered sum over ranks (emulation: the rank's own rows of its partial)
            dH_own = dH_g() if callable(dH_g) else dH_g[self.r0:self.r1]
            ((g["We"], g["be"]),) = self._linear_bwd_multi(Xg, [le])
            (g["Wk"], g["bk"]), (g["Wc"], _) = self._linear_bwd_multi(x_local, [lk, (P["Wc"], None, dH_own, 0, 1, False)])
            # (dWc comes from the ALREADY SUMMED dH of the own rows: in the flat weight all-reduce below every rank's part is its share
            # of the total, so the sum over ranks is the whole gradient -- as for every other weight)
        elif not self.x_grad and same_rows:
            # one pass over X for the three weight gradients
            (g["We"], g["be"]), (g["Wk"], g["bk"]), (g["Wc"], _) = self._linear_bwd_multi(Xg, [le, lk, (P["Wc"], None, dH_g, 0, 1, False)])
        elif not self.x_grad:
            (g["We"], g["be"]), (g["Wc"], _) = self._linear_bwd_multi(Xg, [le, (P["Wc"], None, dH_g, 0, 1, False)])
            _, g["Wk"], g["bk"] = kern.linear_bwd(x_local, *lk[:5], False, True)
        else:
            dX1, g["We"], g["be"] = kern.linear_bwd(Xg, P["We"], xp_g, dxp_g, 1, 0, True, True)
            dX3, g["Wc"], _ = kern.linear_bwd(Xg, P["Wc"], None, dH_g, 0, 1, True, False)
            dX2, g["Wk"], g["bk"] = kern.linear_bwd(x_local, P["Wk"], s["xk"], dxk, 1, 0, True, True)
        if self.coll:
            # (the edge-MLP scorer's gradients -- g["scorer"], every rank's share of the selected edges -- ride in the same bucket)
            sg = g.get("scorer")
            parts = [(g, k) for k in self.PARAM_KEYS] + ([] if sg is None else [(sg, k) for k in sorted(sg) if sg[k] is not None])
            flat = _Gather._buf(self.bufs, ("wgrad", "flat"), (sum(int(d_[k].numel()) for d_, k in parts),), g["We"])
            o = 0
            for d_, k in parts:
                n = d_[k].numel()
                flat[o:o + n].copy_(d_[k].reshape(-1))
                o += n
            dist.all_reduce(flat, group=self.group)
            o = 0
            for d_, k in parts:                    # (copies: `flat` is a persistent bucket, overwritten by the next step's all-reduce)
                n = d_[k].numel()
                d_[k] = flat[o:o + n].view_as(d_[k]).clone()
                o += n
        if self.x_grad:
            g["x"] = dX1 + dX3 + dX2                     # all three on the rank's own rows
        return g
