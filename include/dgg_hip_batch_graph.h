/* dgg_hip_batch_graph.h -- batch preparation of libdgg_hip.so: the noisy edges and the same-class target of one mini-batch graph.
 *
 * The reference's mini-batch loop edits every training batch before the model sees it (train_large_graphs.py:230-236, with the script's
 * default --edge_noise_level 0.00014, train_large_graphs.py:77-81):
 *     adj = to_scipy(batch.edge_index); adj = add_noisy_edges(adj, noise_level)           (numpy, on the host: rand(n, n) < 10 * level)
 *     gt_adj = remove_interclass_edges(adj, batch.y)                                       (the supervision target of the adjacency loss)
 * The one entry here does both on the device, on the batch graph's CSR arrays (dgg_amd.ops.batch_graph_edit binds it,
 * dgg_amd.sampling.SubgraphBatch.with_noise dresses the result).
 *
 * The header is purely additive: it changes no declaration of dgg_hip.h (the recorded ABI, which it includes), of dgg_hip_next.h, of
 * dgg_hip_adj_loss.h or of dgg_hip_sampling.h, and the entry keeps their conventions (int return: DGG_OK or a DGG_ERR_* code with
 * dgg_last_error(); device pointers; `stream` a hipStream_t).  The library's definition is compiled against this file and the ctypes
 * binding parses it into tables of its own (dgg_amd._lib.BATCH_GRAPH_PROTOTYPES / BATCH_GRAPH_RESTYPES).
 *
 * INPUT: a batch graph in CSR with local ids 0..n-1: rowptr int64 [n+1] ascending from 0 to E, col int32 [E] STRICTLY ascending within a
 * row, values float32 [E]; optionally labels int32 [n]; a seed (s0, s1); a threshold thr in [0, 2^32].
 *
 * THE LAW (a CPU restatement is bit-exact; all uint32 arithmetic wraps, mix32 is the finaliser of csrc/dgg_common.h, the one the walk
 * law of dgg_hip_sampling.h uses:  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16):
 *     x(i,j)     = mix32( mix32((uint32)i ^ s0) ^ s1 ^ ((uint32)j * 0x9E3779B9u) )
 *     noisy(i,j) = i != j  and  (uint64)x(i,j) < thr  and  (i,j) is not a stored entry
 * The host computes thr = min(2^32, (uint64)(p * 2^32)) in double, p = 10 * noise_level clipped to [0, 1]: the factor 10 is the
 * reference's (utils.py:93).  thr = 0: no noisy pair; thr = 2^32: every off-diagonal pair.
 *
 * OUTPUT: two coalesced graphs, columns strictly ascending within a row.
 *     the NOISY GRAPH  every stored entry plus every noisy pair: nrowptr int64 [n+1], ncol int32 [E'], nrow int32 [E'], nval float32 [E'],
 *                      nsrc int64 [E'].  A stored entry: nval = its stored value, nsrc = its position in col.  A noisy entry: nval = 1.0f,
 *                      nsrc = -1.  A stored diagonal entry is kept (no NEW diagonal entry is ever made).
 *     the TARGET       only with labels: the entries (i,j) of the noisy graph with labels[i] == labels[j], every one of value 1
 *                      (remove_interclass_edges of the noisy batch graph): trowptr int64 [n+1], tcol int32 [E_t], trow int32 [E_t].
 *
 * TWO DEVIATIONS from the reference, both deliberate:
 *   * every batch gets its own noise: the caller derives (s0, s1) from (seed, epoch, step).  The reference calls np.random.seed(0) inside
 *     add_noisy_edges, so every batch there gets the top-left corner of one and the same noise matrix;
 *   * the realisation is the counter-based law above, not numpy's Mersenne stream (the same trade that
 *     dgg_amd.data.add_noisy_edges(reference_stream=False) makes): the distribution is the reference's -- each off-diagonal pair that is
 *     not stored, independently, with probability thr / 2^32 -- the bits are not.
 *
 * COST: every row evaluates the hash of every column, n^2 / 64 window iterations of one wavefront (pure integer vector work; the stored
 * entries are merged in on the way, with no search list and no scratch).  That is the right trade for BATCH graphs (n of a few thousand:
 * microseconds) and still 1.6e8 iterations at n = 100 000; it is not meant for whole graphs of millions of nodes.
 *
 * status (int32 [1], device): what a kernel finds wrong in DEVICE data, which the host-side checks cannot see.  A kernel never reads or
 * writes out of bounds because of it: it skips the offending row or slot and stores the code (plain stores of one value).
 *     DGG_BATCH_EDIT_BAD_GRAPH  a row range outside 0 <= rowptr[i] <= rowptr[i+1] <= E, a column outside [0, n), a row whose columns are
 *                               not strictly ascending (the whole row is skipped: it counts 0 entries and fills none), or a fill slot
 *                               outside the row's range [nrowptr[i], nrowptr[i+1]) within [0, E') (trowptr, E_t likewise): the prefix
 *                               sums do not belong to this graph, seed and threshold
 * The caller zeroes it before the first call and reads it back when it reads anything back; the entry never clears it.
 */
#ifndef DGG_HIP_BATCH_GRAPH_H
#define DGG_HIP_BATCH_GRAPH_H
#include "dgg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DGG_BATCH_EDIT_BAD_GRAPH 1

/* One entry, two values of `phase`; the caller's two exclusive prefix sums (torch.cumsum) run between them.  Every phase reads only the
 * arguments listed for it; the others may be NULL / 0.  No kernel uses an atomic and every store lands at an index that exactly one lane
 * computes: the same input gives the same output, bit for bit, on every run.
 *
 *   DGG_BATCH_EDIT_COUNT  rowptr, col, n, E, labels (nullable), s0, s1, thr  ->  ndeg_i int32 [n]: the entries of every row of the noisy
 *                         graph; with labels also tdeg_i int32 [n]: those of the target.
 *       caller: nrowptr / trowptr int64 [n+1] = EXCLUSIVE prefix sums of ndeg_i / tdeg_i; E' = nrowptr[n], E_t = trowptr[n];
 *               the ONE read-back of the edit: (E', E_t, status) in one copy
 *   DGG_BATCH_EDIT_FILL   rowptr, col, values, n, E, labels (nullable), s0, s1, thr, nrowptr, E_n (= E'), trowptr and E_t (with labels)
 *                         ->  ncol, nrow, nval, nsrc [E_n]; with labels tcol, trow [E_t].  The same sweep: one wavefront per row walks the
 *                         columns in windows of 64, lane l owning column c0 + l; the occupied lanes of a window (stored, or noisy) take
 *                         the slots base + (occupied lanes below l), a STABLE merge of the two ascending sets by ballot prefix.
 *
 * DGG_ERR_ARG and nothing launched: a phase outside the two; n outside 0 <= n < 2^31; E, E_n or E_t < 0; thr > 2^32; a NULL status; a NULL
 * array that the phase reads or writes on a non-empty problem (COUNT: rowptr, ndeg_i; col with E > 0.  FILL: rowptr, nrowptr; col and values
 * with E > 0; ncol, nrow, nval, nsrc with E_n > 0; with labels trowptr, and tcol, trow with E_t > 0); labels without the phase's target
 * arrays (COUNT: tdeg_i; FILL: trowptr), or a target array (tdeg_i; trowptr, tcol, trow) without labels.
 * n == 0: DGG_OK, nothing launched, no pointer read. */
#define DGG_BATCH_EDIT_COUNT 0
#define DGG_BATCH_EDIT_FILL 1

int dgg_batch_graph_edit(int phase, const int64_t *rowptr, const int32_t *col, const float *values, int64_t n, int64_t E,
                         const int32_t *labels, uint32_t s0, uint32_t s1, uint64_t thr, int32_t *ndeg_i, int32_t *tdeg_i,
                         const int64_t *nrowptr, int64_t E_n, int32_t *ncol, int32_t *nrow, float *nval, int64_t *nsrc,
                         const int64_t *trowptr, int64_t E_t, int32_t *tcol, int32_t *trow, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DGG_HIP_BATCH_GRAPH_H */
