/* dgg_hip_adj_loss.h -- the adjacency supervision loss of libdgg_hip.so on sparse rows.
 *
 * The reference's large-graph training loops supervise the learned adjacency directly (train_reddit.py:236-251,
 * train_large_graphs.py:236-251):
 *     batch_gt_adj = remove_interclass_edges(batch_adj, batch_label)
 *     loss_2 = F.mse_loss(out_adj.to_dense(), batch_gt_adj.to_dense().float())
 * which forms two dense [N,N] operands.  dgg_adj_mse_loss computes the same number from the stored entries of both matrices.
 *
 * The header is purely additive: it changes no declaration of dgg_hip.h (the recorded ABI, which it includes) or of dgg_hip_next.h, and
 * the entry keeps their conventions (int return: DGG_OK or a DGG_ERR_* code with dgg_last_error(); device pointers; `stream` a
 * hipStream_t).  The library's definition is compiled against this file and the ctypes binding parses it into tables of its own
 * (dgg_amd._lib.ADJ_LOSS_PROTOTYPES / ADJ_LOSS_RESTYPES).
 */
#ifndef DGG_HIP_ADJ_LOSS_H
#define DGG_HIP_ADJ_LOSS_H
#include "dgg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DGG_ADJ_LOSS_MEAN 0
#define DGG_ADJ_LOSS_SUM 1

/* ---- dense-equivalent squared error of a learned adjacency A against a target graph G ------------------------------------------------
 * A [rows, rows] (the WHOLE graph: rows == columns) in ONE of three row forms:
 *   list     idx / val [rows,K], 1 <= K <= 64 (cptr, rowptr_l, col_l NULL);
 *   chunked  idx / val [chunks,64] (K = 64), cptr [rows+1] given: row i = the chunks [cptr[i], cptr[i+1]) clamped to [0, chunks]
 *            (dgg_hip.h, "CHUNKED rows"; rowptr_l, col_l NULL);
 *   CSR      rowptr_l int64 [rows+1] and col_l int32 [E] given, val [E]: row i = the entries [rowptr_l[i], rowptr_l[i+1]), of any width
 *            (idx, cptr NULL; K and chunks are not read).
 * A column < 0 marks an empty (padding) slot.  A row holds each column at most once -- true of everything the generator returns; it is
 * NOT checked, and a row that breaks it counts the column's error once per slot.
 * G in CSR: rowptr int64 [rows+1], col int32 strictly ascending within a row, gval float32 (csr_pattern / AllPairs.prior_csr).
 * With a_ij the stored learned value and g_ij the stored target value (0 where G stores nothing):
 *     S = sum over the stored (i,j) of A of (a_ij - g_ij)^2  +  sum over the (i,j) stored in G and not in A of g_ij^2
 *     out[0] = S / (rows * rows)   reduction DGG_ADJ_LOSS_MEAN  (F.mse_loss of the two dense matrices)
 *     out[0] = S                   reduction DGG_ADJ_LOSS_SUM
 * d = a_ij - g_ij is one float32 subtraction, as the dense reference forms it; the square, the row sums and every fold are double.
 * One wavefront per row, the 16 rows of a workgroup in ascending order, then one block folds the workgroups' records in a fixed tree:
 * no floating-point atomics, the same input gives the same bits.  out[0] is rounded to float32 only when it is stored; nothing is read
 * back.  rows == 0 stores 0 (SUM) or NaN (MEAN, as torch's mean of nothing) without a row launch; only `out` is read then.
 * dval (nullable; the shape of val): dval[e] = scale * 2 * (a_e - g_e) in float32, exactly 0.0f at every padding slot (chunked rows:
 * also in the chunks past cptr[rows]).  scale = 1 / (rows * rows) (MEAN) or 1 (SUM), computed in double by the caller and passed as
 * one float: the gradient of out[0] with respect to val is then grad_out * dval, with no second join.
 * ws: 8 * ceil(rows / 16) bytes, 8-byte aligned (one double per workgroup).
 * DGG_ERR_ARG and nothing written: rows outside 0 <= rows < 2^31; K outside 1..64 (list / chunked); chunked rows with K != 64 or chunks
 * outside 0 <= chunks < 2^31; more than one row form given at once (rowptr_l or col_l together with idx or cptr); a reduction other than
 * the two; a NULL array (rows > 0); ws not 8-byte aligned (rows > 0); a NULL out. */
int dgg_adj_mse_loss(const int32_t *idx, const float *val, int64_t rows, int K, const int32_t *cptr, int64_t chunks,
                     const int64_t *rowptr_l, const int32_t *col_l, const int64_t *rowptr, const int32_t *col, const float *gval,
                     int reduction, float scale, void *ws, float *dval, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DGG_HIP_ADJ_LOSS_H */
