/* dgg_hip_next.h -- entry points of libdgg_hip.so added SINCE ABI v6.
 *
 * include/dgg_hip.h is the recorded ABI (dgg_abi_version() == 6): its prototypes do not change between bumps.  What the library has
 * gained since is declared here.  The header is purely additive -- it changes no declaration of dgg_hip.h, which it includes, and every
 * entry point keeps that header's conventions (int return: DGG_OK or a DGG_ERR_* code with dgg_last_error(); device pointers; `stream` a
 * hipStream_t) -- and it is folded into dgg_hip.h at the next ABI bump.  The library's definitions are compiled against this file and the
 * ctypes binding parses it into tables of its own (dgg_amd._lib.NEXT_PROTOTYPES / NEXT_RESTYPES).
 */
#ifndef DGG_HIP_NEXT_H
#define DGG_HIP_NEXT_H
#include "dgg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- edge-list candidates on CHUNKED rows (rows of any width) --------------------------------------------------------------------
 * The live class takes the candidates of row i from the stored entries of in_adj (dgm.py:1613-1623), perturbs them (dgm.py:1211-1229)
 * and ramps over the whole sorted row with an unbounded learned degree (select_top_k, dgm.py:1402-1421).  dgg_edgelist_topk_softk keeps
 * the 64 best candidates of a row, exact while k_i + 8.5 <= 64 or the row has no more candidates than that; here row i keeps its
 * L_i = min(n_i, ceil(k_i + 8.5) + 1) best candidates (n_i = its candidates: every rank that can carry weight) in the chunks
 * [cptr[i], cptr[i+1]) of idx / val / w [ccap,64], rank r at entry r % 64 of chunk r / 64 (dgg_hip.h, "CHUNKED rows").
 * cptr [row1-row0+1] = dgg_chunk_layout of the CLAMPED degrees min(k_i, n_i - 9.5), which gives exactly ceil(L_i / 64) chunks per row (a
 * row of 3 candidates with k = 1000 owns one chunk); k [row1-row0] stays the TRUE learned degree: the ramp and every backward read it.
 * rowptr [row1-row0+1] / col: the rebased CSR slice of the rows asked for with global columns, xp [N,h] every node, the noise keyed on
 * the global pair (row0 + i, j) -- as dgg_edgelist_topk_softk_rows.  noise_mode DGG_NOISE_NONE / HASH / HASH_SYM (an explicit noise
 * tensor is outside the fused layer).  One wavefront per row; score chain, key order (score descending, lower column first) and bits of
 * dgg_edgelist_topk_softk[_rows] at h in {16, 32, 64, 128}: with every M_i = 1 the ranks below L_i are its output at K = 64.
 * w = the ramp of dgg_allpairs_topk_ranked_wide (mode 0 score x ramp, 1 the ramp, 3 the straight-through forward value); rs [row1-row0] =
 * lane-wise sums over a row's chunks in chunk order, then the wavefront butterfly -- a one-chunk row sums as dgg_edgelist_topk_softk does.
 * Every other slot of a row's chunks and every chunk in [cptr[rows], ccap) is written EMPTY (idx -1, val 0, w 0); nothing outside the
 * arrays is written.  A wavefront settles 8 chunks of a row per pass over its candidates; rows of more chunks take ceil(maxm / 8)
 * passes launched from the host integer maxm >= max M_i (no device read-back), each continuing strictly below the last key the previous
 * one wrote.
 * DGG_ERR_UNSUPPORTED and nothing written: h outside {16, 32, 64, 128} or xp not 16-byte aligned, a noise_mode other than 0 / 2 / 3.
 * DGG_ERR_ARG and nothing written: mode outside {0, 1, 3}, rows outside 0 <= row0 <= row1 <= N < 2^31, maxm outside 1..2^20, ccap
 * outside 0 <= ccap < 2^25, a NULL array.  row0 == row1 returns 0 without a launch. */
int dgg_edgelist_topk_chunked(const float *xp, int64_t N, int h, int64_t row0, int64_t row1, const int64_t *rowptr, const int32_t *col,
                              float t, int noise_mode, uint32_t s0, uint32_t s1, const float *k, int mode, int maxm, const int32_t *cptr,
                              int64_t ccap, int32_t *idx, float *val, float *w, float *rs, void *stream);
/* The same from given edge probabilities p_edge [E] (CSR order of the slice, the columns of a row ascending): the edge-MLP scorers' path
 * (dgm.py:1628-1725 through dgg_edge_mlp_fwd), in place of dgg_edgelist_topk_p[_rows] + dgg_softk_fwd.  Perturbation and key order are
 * dgg_edgelist_topk_p's (dgm.py:1211-1229, 1404; ties: the earlier candidate of the row first); ramp, row sums, empty slots, passes and
 * layout as above (dgm.py:1402-1421).  ex_edge (nullable, [E]): the per-candidate extra -- the stored value a_uv of u-v-A_uv / A_uv, or
 * the distance extra dgg_edge_mlp_fwd returned -- gathered to ex_out [ccap,64] per kept slot, 0 on empty slots (ex_out is required with
 * ex_edge and ignored without).  eid (nullable, [ccap,64]): the kept candidate's index in the slice's per-edge arrays, -1 on empty slots.
 * Refusals as above (there is no latent width here: p_edge is already the score). */
int dgg_edgelist_topk_p_chunked(const float *p_edge, int64_t N, int64_t row0, int64_t row1, const int64_t *rowptr, const int32_t *col,
                                int noise_mode, uint32_t s0, uint32_t s1, const float *k, int mode, int maxm, const int32_t *cptr,
                                int64_t ccap, const float *ex_edge, int32_t *idx, float *val, float *ex_out, int32_t *eid, float *w,
                                float *rs, void *stream);

/* ==== block norm_spmm ==== (dgg_amd._lib.NEXT_BLOCKS["norm_spmm"]; the declarations above are NEXT_PROTOTYPES) */

/* ---- normalize_adj inside the forward aggregation ----------------------------------------------------------------------------------
 * dgg_partp_build_phase / dgg_partp_build_chunked take three more values of `phase` (no prototype changes; phases 0..2 are as recorded,
 * rs_all and ahat going together).  Phases 4 / 5 = phases 1 / 0 called with rs_all != NULL and ahat == NULL (required): the count pass
 * still leaves ainv [ncols] = rs_all_j^-1/2 in the workspace, the fill pass writes the records only (no a_j gathers, no ahat stores);
 * phase 2 finishes a phase 4.  Phase 3 runs the count pass alone (rs_all required; val / rs_rows / cnode are not read): the ainv table
 * is complete, nothing else of the workspace is -- what a forward without a backward needs.
 *
 * Y [rows,F] = act(A H) AND ahat [rows,64] = rs_i^-1/2 w rs_j^-1/2 from the unnormalised weights: idx / w [rows,64] (K = 64), rs_rows
 * [rows] the own rows' sums, partp_ws a payload workspace of (rows, 64, ncols) whose count pass ran with rs_all (its ainv table is
 * read; no other part of it), X [ncols,F], F in {16, 32, 64}, X / Y 16-byte aligned.  ahat has the bits of dgg_partp_build_norm
 * (a_i = 1 / sqrt(rs_i), (a_i * w) * ainv_j, 0 where idx < 0 or w == 0), Y the bits of dgg_ell_spmm_act_fwd on that ahat for finite X.
 * act 0 / 2 as dgg_ell_spmm_act_fwd.  DGG_ERR_UNSUPPORTED: another F or alignment, no payload partition for the shape; DGG_ERR_ARG: a
 * NULL array, act outside {0, 2}.  rows == 0 returns 0 without a launch. */
int dgg_ell_spmm_norm_act_fwd(const int32_t *idx, const float *w, const float *rs_rows, const void *partp_ws, int64_t ncols, const float *X,
                              int64_t rows, int F, int act, float *Y, float *ahat, void *stream);
/* The same on chunked rows: idx / w / ahat [chunks,64], node i = the chunks [cptr[i], cptr[i+1]), rs_nodes [rows], partp_ws a workspace
 * of (chunks, 64, ncols) (dgg_partp_build_chunked), Y [rows,F].  Chunks in [cptr[rows], chunks) get ahat = 0. */
int dgg_ell_spmm_norm_act_fwd_chunked(const int32_t *idx, const float *w, const float *rs_nodes, const void *partp_ws, int64_t ncols,
                                      const float *X, int64_t rows, const int32_t *cptr, int64_t chunks, int F, int act, float *Y,
                                      float *ahat, void *stream);

/* dgg_softk_edge_bwd_partp_phase / dgg_softk_edge_bwd_partp_chunked with ainv_table: 1 = the row kernel takes a_j = rs_j^-1/2 from the
 * partition's ainv table (the partition was built with rs_all = rs: the same bits) instead of a division and a square root per lane;
 * 0 = those entries.  Every other argument, refusal and result as theirs. */
int dgg_softk_edge_bwd_partp_tab(const float *xp, int64_t rows, int h, const int32_t *idx, const float *val, const float *k, const float *rs,
                                 const float *dA, const float *dA_rec, const float *da, const float *ahat_rows, int K, int64_t row0, float t,
                                 int perturb, int mode, int normalized, const void *partp_ws, int64_t ncols, float *rowinfo_ws, float *dk,
                                 float *dxp, int out_act, int phase, int ainv_table, void *stream);
int dgg_softk_edge_bwd_partp_chunked_tab(const float *xp, int64_t rows, const int32_t *cptr, int64_t chunks, int h, const int32_t *idx,
                                         const float *val, const float *k, const float *rs, const float *dA, const float *dA_rec,
                                         const float *da, const float *ahat_rows, int64_t row0, float t, int perturb, int mode,
                                         int normalized, const void *partp_ws, int64_t ncols, float *rowinfo_ws, float *dk, float *dxp,
                                         int out_act, int phase, int ainv_table, void *stream);

/* ==== block project_knet ==== (dgg_amd._lib.NEXT_BLOCKS["project_knet"]) */

/* ---- the dense prologue of the forward in one launch: several layers on one input + the learned degree ---------------------------
 * y_s [N, out_s] = act_s(x W_s^T + b_s) for nseg <= 8 layers that read x [N,d] (dgg_linear_fwd_multi), each weight read from its OWN tensor
 * -- W / b / y are HOST arrays of nseg device pointers, b or b[s] may be NULL, seg_layout[s] 0: W_s [out_s,d], 1: W_s [d,out_s] -- and
 * k [N], u [N] (u nullable) = dgg_knet_x_fwd_mfma on layer knet_seg's output (h = 64: W1 [32,65], b1 [32], Wmu [16,32], bmu [16], Wp [16],
 * bp [1]; deg [N], mu_sd [2]), taken from the projection's accumulators instead of a second pass over y_knet_seg.  Every output has the
 * bits of dgg_linear_pack_weights + dgg_linear_fwd_multi + dgg_knet_x_fwd_mfma: the same k-ordered fmaf chains.
 * force: -1 = the fused kernel where dgg_linear_fwd_multi takes its persistent kernel (N >= 32768), 0 = never, 1 = at any N.
 * DGG_ERR_UNSUPPORTED and nothing written -- the caller runs the pair --: force says so; d != 128; a width that is no multiple of 32 or
 * more than 6 column blocks of 32; a k-net layer that is not 64 wide; layers arranged other than xp | xk | H, xp | xk, xk | H or xk
 * (64-wide neighbours); x, a y_s or a weight not 16-byte aligned.  DGG_ERR_ARG: a NULL array, nseg / knet_seg / force out of
 * range.  N == 0 returns 0 without a launch. */
int dgg_project_knet_fwd(const float *x, int64_t N, int d, int nseg, const float *const *W, const float *const *b, const int *seg_out,
                         const int *seg_layout, const int *seg_act, float *const *y, int knet_seg, const float *deg, const float *mu_sd,
                         const float *W1, const float *b1, const float *Wmu, const float *bmu, const float *Wp, const float *bp, float *k,
                         float *u, int force, void *stream);

/* ==== block adj_stats ==== (dgg_amd._lib.NEXT_BLOCKS["adj_stats"]) */

/* ---- get_adj_diff_stats on sparse data: the reference's train_stats scalars (dgm.py:1313-1350) --------------------------------------
 * How far the learned SOFT adjacency (the value before any straight-through replacement: dgm.py:1288 runs before return_hard_or_soft)
 * has moved from the input graph, and the learned degree from the input degree, of the WHOLE graph (rows [0, rows): row shards refuse a
 * writer).  The learned rows: cptr == NULL: idx / w [rows,K], K <= 64; cptr [rows+1] given: chunked rows, idx / w [chunks,64] (K = 64),
 * row i = the chunks [cptr[i], cptr[i+1]), chunks in [cptr[rows], chunks) are not read.  idx < 0 marks an empty slot; the columns of a
 * row's other slots are distinct.  The input graph in CSR (csr_pattern / AllPairs.prior_csr): rowptr int64 [rows+1], col int32 strictly
 * ascending within a row, aval float32; k [rows] the learned degrees.  With a_ij the stored input value (0 where nothing is stored) and
 * w_ij the learned value (0 where not selected, at an empty slot or outside the row's chunks):
 *   on-edge population   the pairs with a_ij > 0, d = a_ij - w_ij, kept iff d != 0 as a float32 subtraction -- input edges the generator
 *                        did not select are in it with d = a_ij (dgm.py:1321-1326);
 *   off-edge population  the pairs with a_ij == 0 (absent, or stored as exactly 0), d = -w_ij, kept iff d != 0 (dgm.py:1322-1328);
 *                        a stored negative value belongs to neither.
 * out [10] float32, the layout below: n, mean = sum d / n and the UNBIASED std (n - 1) of either population; in_deg_mean = mean_i sum_j
 * a_ij; mean and unbiased std of k_diff_i = k_i - sum_j a_ij; k_mean = mean_i k_i.  n == 0 gives a NaN mean and std, n == 1 a NaN std, as
 * torch.mean / torch.std on what the reference indexes; rows == 0 writes those results (n = 0, the other eight NaN) without a row launch,
 * and only `out` is read from the arguments.  The counts are exact up to 2^24.
 * One wavefront per row; moments as (n, mean, M2) in double, merged by Chan's formula in a fixed order (wavefront butterfly, the 16 rows
 * of a workgroup in ascending order, then one block folds the workgroups' records in a fixed tree); no floating-point atomics: the same
 * input gives the same bits.  Rounded to float32 only when stored.  ws: 96 * ceil(rows / 16) bytes, 8-byte aligned (those records).
 * DGG_ERR_ARG and nothing written: K outside 1..64 (K != 64 on chunked rows), rows outside 0 <= rows < 2^31, chunks outside
 * 0 <= chunks < 2^31, a NULL array (rows > 0) or a NULL out, ws not 8-byte aligned. */
#define DGG_ADJ_STATS_ON_N 0
#define DGG_ADJ_STATS_ON_MEAN 1
#define DGG_ADJ_STATS_ON_STD 2
#define DGG_ADJ_STATS_OFF_N 3
#define DGG_ADJ_STATS_OFF_MEAN 4
#define DGG_ADJ_STATS_OFF_STD 5
#define DGG_ADJ_STATS_IN_DEG_MEAN 6
#define DGG_ADJ_STATS_K_DIFF_MEAN 7
#define DGG_ADJ_STATS_K_DIFF_STD 8
#define DGG_ADJ_STATS_K_MEAN 9
#define DGG_ADJ_STATS_COUNT 10
int dgg_adj_diff_stats(const int32_t *idx, const float *w, int64_t rows, int K, const int32_t *cptr, int64_t chunks, const int64_t *rowptr,
                       const int32_t *col, const float *aval, const float *k, void *ws, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DGG_HIP_NEXT_H */
