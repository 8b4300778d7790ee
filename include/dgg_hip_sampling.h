/* dgg_hip_sampling.h -- mini-batch sampling of libdgg_hip.so: random-walk node sets and induced sub-graphs of a CSR graph.
 *
 * The reference's large-graph loops train on sub-graphs of one big graph (train_large_graphs.py:402-421):
 *     GraphSAINTRandomWalkSampler(data, batch_size=args.graphsaint_bs, walk_length=args.graphsaint_wl, num_steps=5, ...)
 *     ClusterLoader(cluster_data, batch_size=5, shuffle=True, ...)
 * Both come down to "a node set -> the sub-graph it induces"; the random-walk sampler finds its node set by walking.  The two entries
 * here are those two steps on the device (dgg_amd.sampling builds the samplers on them).
 *
 * The header is purely additive: it changes no declaration of dgg_hip.h (the recorded ABI, which it includes), of dgg_hip_next.h or of
 * dgg_hip_adj_loss.h, and the entries keep their conventions (int return: DGG_OK or a DGG_ERR_* code with dgg_last_error(); device
 * pointers; `stream` a hipStream_t).  The library's definitions are compiled against this file and the ctypes binding parses it into
 * tables of its own (dgg_amd._lib.SAMPLING_PROTOTYPES / SAMPLING_RESTYPES).
 *
 * The graph is CSR throughout: rowptr int64 [N+1] ascending from 0 to E, col int32 [E] (csr_pattern gives both).  Neither entry uses an
 * atomic: the same input gives the same output, bit for bit, on every run.
 *
 * status (int32 [1], device): what a kernel finds wrong in DEVICE data, which the host-side checks of an entry cannot see.  A kernel
 * never reads or writes out of bounds because of it: it skips the offending item and stores a code there (plain stores of one value).
 *     DGG_SAMPLING_BAD_NODE   a root / a member of `nodes` outside [0, N)
 *     DGG_SAMPLING_BAD_GRAPH  a row range outside 0 <= rowptr[v] <= rowptr[v+1] <= E, a column outside [0, N), or a fill position outside
 *                             [0, E_b) (browptr does not belong to this node set)
 * The caller zeroes it before the first call and reads it back when it reads anything back; no entry ever clears it.
 */
#ifndef DGG_HIP_SAMPLING_H
#define DGG_HIP_SAMPLING_H
#include "dgg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DGG_SAMPLING_BAD_NODE 1
#define DGG_SAMPLING_BAD_GRAPH 2

/* ---- the nodes a GraphSAINT random-walk sampler visits -----------------------------------------------------------------------------
 * roots int32 [B]; walk int32 [B, L+1] row-major; L >= 0 steps; seed (s0, s1).  THE LAW (a CPU restatement is bit-exact; all uint32
 * arithmetic wraps, mix32 is the finaliser of csrc/dgg_common.h:
 *     x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16):
 *     walk[b,0] = roots[b]
 *     for t = 1..L, from v = walk[b,t-1] with d = rowptr[v+1] - rowptr[v]:
 *         d == 0:  walk[b,t] = v                                    (the walk stays on a node without neighbours)
 *         else     x = mix32(mix32((uint32)b ^ s0) ^ s1 ^ ((uint32)t * 0x9E3779B9u))
 *                  walk[b,t] = col[rowptr[v] + (((uint64)x * (uint64)d) >> 32)]       (a pick in [0, d): d < 2^32)
 * One thread per walk: a walk is a dependent chain of gathers, there is nothing to share between its steps.
 * A root outside [0, N): the whole row walk[b,:] = -1 and status = DGG_SAMPLING_BAD_NODE.  A broken row range or column: the walk stays
 * where it is for that step and status = DGG_SAMPLING_BAD_GRAPH.
 * DGG_ERR_ARG and nothing launched: N outside 0 <= N < 2^31; E outside 0 <= E < 2^32 (no row can then reach d = 2^32, which the pick
 * could not address); B outside 0 <= B < 2^31; L < 0; B > 0 with N == 0; a NULL rowptr, roots, walk or status (B > 0); a NULL col with
 * E > 0 (B > 0, L > 0).  B == 0: DGG_OK, nothing launched, no pointer read. */
int dgg_random_walk_nodes(const int64_t *rowptr, const int32_t *col, int64_t N, int64_t E, const int32_t *roots, int64_t B, int L,
                          uint32_t s0, uint32_t s1, int32_t *walk, int32_t *status, void *stream);

/* ---- the sub-graph a node set induces ----------------------------------------------------------------------------------------------
 * One entry, four values of `phase`; the host sizes the outputs between them (the pattern of dgg_partp_build_phase).  The exclusive
 * prefix sums between the phases are NOT written here: they are left to the caller (torch.cumsum), as marked below.  Every phase reads
 * only the arguments listed for it; the others may be NULL / 0.
 *
 *   DGG_SUBGRAPH_MARK     nodes int32 [M] (duplicates allowed), N  ->  flag int32 [N] = 1 for the members of `nodes`, 0 elsewhere;
 *                         status = DGG_SAMPLING_BAD_NODE if a member is outside [0, N) (it is skipped).
 *                         Duplicates store the same value twice: plain stores, no atomic.
 *       caller: rank int32 [N] = INCLUSIVE prefix sum of flag; n_b = rank[N-1], which may stay on the device
 *   DGG_SUBGRAPH_RELABEL  flag, rank, N, rows  ->  newid int32 [N] = rank[v] - 1 where flag[v], else -1: the rank of v among the set nodes in
 *                         ascending original id (the order of PyG's node_idx.unique(); monotone).  orig int32 [rows], rows >= n_b (min(M, N)
 *                         always is): orig[newid[v]] = v; entries n_b <= r < rows are not written.
 *   DGG_SUBGRAPH_COUNT    rowptr, col, values (nullable float32 [E]), N, E, rank, newid, orig, rows  ->  bdeg_i int32 [rows], bdeg float32
 *                         [rows] (only with values).  rows is an UPPER bound of n_b (min(M, N) always is one): n_b is read from rank[N-1] on
 *                         the device, so the caller has not had to read it back yet.  One wavefront per row r < n_b walks the CSR row of
 *                         v = orig[r] in strides of 64 and counts the neighbours u with newid[u] >= 0: bdeg_i[r].  bdeg[r] = the sum of
 *                         the values of those entries, FIXED ORDER: lane l adds its entries (positions rowptr[v] + l, + 64, ...) in
 *                         ascending order in double, the 64 lane sums fold by the xor butterfly 32, 16, .., 1 in double, one rounding to
 *                         float32 at the store.  Rows n_b <= r < rows store 0 in both.
 *       caller: browptr int64 [rows+1] = EXCLUSIVE prefix sum of bdeg_i; E_b = browptr[n_b]; the ONE read-back: (n_b, E_b, status)
 *   DGG_SUBGRAPH_FILL     rowptr, col, N, E, newid, orig, rows (= n_b now), browptr int64 [>= rows+1], E_b  ->  bcol int32 [E_b] the
 *                         relabelled neighbour, beid int64 [E_b] the position of the entry in col (to gather values, edge weights or
 *                         per-edge features), brow int32 [E_b] the relabelled row.  The same walk; a kept entry of lane l lands at
 *                         browptr[r] + (kept entries of earlier strides) + (kept entries of lanes < l in this stride): a STABLE compaction
 *                         by ballot prefix, so with col strictly ascending within a row and the relabelling monotone, bcol is strictly
 *                         ascending within a row and (brow, bcol) are the sorted, unique indices of a coalesced COO matrix.
 *
 * DGG_ERR_ARG and nothing launched: a phase outside the four; N outside 0 <= N < 2^31; M, E, rows, E_b < 0; rows > N; a NULL array
 * that the phase reads or writes on a non-empty problem; a NULL status (every phase writes it).  An empty problem launches nothing and
 * returns DGG_OK: MARK with N == 0 (M == 0 still clears flag); RELABEL with N == 0; COUNT with rows == 0 or N == 0; FILL with rows == 0 or
 * E_b == 0. */
#define DGG_SUBGRAPH_MARK 0
#define DGG_SUBGRAPH_RELABEL 1
#define DGG_SUBGRAPH_COUNT 2
#define DGG_SUBGRAPH_FILL 3

int dgg_induced_subgraph(int phase, const int64_t *rowptr, const int32_t *col, const float *values, int64_t N, int64_t E,
                         const int32_t *nodes, int64_t M, int32_t *flag, const int32_t *rank, int32_t *newid, int32_t *orig, int64_t rows,
                         int32_t *bdeg_i, float *bdeg, const int64_t *browptr, int64_t E_b, int32_t *bcol, int64_t *beid, int32_t *brow,
                         int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DGG_HIP_SAMPLING_H */
