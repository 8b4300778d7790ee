// dgg_batch_graph.hip -- batch preparation on the device: the noisy edges of a mini-batch graph and its same-class target (reference
// train_large_graphs.py:230-236 does both on the host, add_noisy_edges in numpy and remove_interclass_edges after it).  The contract --
// the noise law, the two output graphs, the two phases and what the caller's prefix sums do between them, the status word -- is the
// comment of include/dgg_hip_batch_graph.h; this file only says how the kernel keeps it.
//
// One wavefront per row sweeps the columns 0..n-1 in windows of 64; lane l owns column c0 + l and evaluates the hash of the pair (pure
// integer vector work, the row key hoisted).  The row's stored entries are strictly ascending (checked first, 64 at a time), so those of
// a window are consecutive in col and at most 64: the wavefront keeps one position `sp` into the row, loads the 64 entries from there
// (one coalesced load, only in windows that hold a stored entry) and every lane finds its own column among them by a lower bound over
// the lanes' registers (six shuffles, no LDS array and no memory search).  occupied = stored | (hit & off the diagonal): COUNT adds
// popcount(ballot), FILL gives lane l the slot base + mbcnt(ballot) -- a stable merge of the two ascending sets, the ballot-prefix idiom
// of subgraph_fill_k.  The target runs the same ballot with `& labels equal` and a base of its own; labels are read by occupied lanes only.
// No atomic; every store lands at an index that one lane of one wavefront computes (the status word stores one value from several
// lanes), so the output is the same bits on every run.
// Nothing is read or written out of bounds whatever the DEVICE data holds: the row range is checked against E, every column against n,
// every fill slot against the row's range clamped to the output arrays; a row or slot that fails is skipped and reported.
#include "dgg_api_internal.h"
#include "../../include/dgg_hip_batch_graph.h"
#include "dgg_common.h"

namespace dgg {

constexpr int BG_WAVES = 4;           // rows (wavefronts) per workgroup
constexpr int64_t BG_NONE = INT64_MAX;  // the column of "no stored entry left in the row": right of every window

__device__ __forceinline__ int bg_below(unsigned long long m) {               // set bits of m in the lanes below this one
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// row i as a checked range of strictly ascending columns inside [0, n): false when it is none (wave-uniform)
__device__ __forceinline__ bool bg_row_ok(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t i, int64_t n, int64_t E, int lane,
                                          int64_t &p0, int64_t &p1) {
    p0 = rowptr[i];
    p1 = rowptr[i + 1];
    if (p0 < 0 || p0 > p1 || p1 > E) return false;
    bool bad = false;
    for (int64_t t = p0; t < p1; t += 64) {
        const int64_t p = t + lane;
        if (p < p1) {
            const int32_t c = col[p];
            if (c < 0 || c >= n) bad = true;
            else if (p > p0 && col[p - 1] >= c) bad = true;
        }
    }
    return __ballot(bad) == 0ull;
}

template <bool FILL>
__global__ __launch_bounds__(BG_WAVES * 64) void batch_edit_k(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                              const float *__restrict__ values, int64_t n, int64_t E,
                                                              const int32_t *__restrict__ labels, uint32_t s0, uint32_t s1, uint64_t thr,
                                                              int32_t *__restrict__ ndeg_i, int32_t *__restrict__ tdeg_i,
                                                              const int64_t *__restrict__ nrowptr, int64_t E_n, int32_t *__restrict__ ncol,
                                                              int32_t *__restrict__ nrow, float *__restrict__ nval, int64_t *__restrict__ nsrc,
                                                              const int64_t *__restrict__ trowptr, int64_t E_t, int32_t *__restrict__ tcol,
                                                              int32_t *__restrict__ trow, int32_t *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * BG_WAVES + wave_id();
    if (i >= n) return;                                                       // (wave-uniform, as every branch on i, sp and nxt below)
    const bool with_t = labels != nullptr;
    int64_t p0, p1;
    if (!bg_row_ok(rowptr, col, i, n, E, lane, p0, p1)) {                     // the row is skipped: no entry counted, none filled
        status[0] = DGG_BATCH_EDIT_BAD_GRAPH;
        if (!FILL && lane == 0) {
            ndeg_i[i] = 0;
            if (with_t) tdeg_i[i] = 0;
        }
        return;
    }
    int64_t at = 0, q0 = 0, q1 = 0, tat = 0, t0 = 0, t1 = 0;                  // FILL: the next slot and the row's slots, clamped to the arrays
    if (FILL) {
        at = q0 = nrowptr[i];
        q1 = nrowptr[i + 1];
        if (q0 < 0) q0 = 0;
        if (q1 > E_n) q1 = E_n;
        if (with_t) {
            tat = t0 = trowptr[i];
            t1 = trowptr[i + 1];
            if (t0 < 0) t0 = 0;
            if (t1 > E_t) t1 = E_t;
        }
    }
    const uint32_t key = mix32((uint32_t)i ^ s0) ^ s1;
    const int32_t li = with_t ? labels[i] : 0;
    int cnt = 0, tcnt = 0;
    int64_t sp = p0;                                                          // the row's first stored entry at or right of the window
    int64_t nxt = sp < p1 ? (int64_t)__builtin_amdgcn_readfirstlane(col[sp]) : BG_NONE;      // ... and its column
    for (int64_t c0 = 0; c0 < n; c0 += 64) {
        const int64_t c = c0 + lane;
        bool stored = false;
        int64_t pos = 0;
        if (nxt < c0 + 64) {                                                  // the window holds stored entries: col[sp .. sp + nw), nw <= 64
            const int64_t pe = sp + lane;
            const int32_t cl = pe < p1 ? col[pe] : 0x7fffffff;                // ascending over the lanes (columns are < n <= 2^31 - 1)
            const int nw = __popcll(__ballot(pe < p1 && (int64_t)cl < c0 + 64));
            int k = 0;                                                        // lower bound of c among the 64 lanes' cl
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1)
                if ((int64_t)__shfl(cl, k + s - 1, 64) < c) k += s;
            stored = c < n && (int64_t)__shfl(cl, k, 64) == c;
            pos = sp + k;
            sp += nw;
            nxt = sp < p1 ? (int64_t)__builtin_amdgcn_readfirstlane(col[sp]) : BG_NONE;
        }
        const uint32_t x = mix32(key ^ ((uint32_t)c * 0x9E3779B9u));
        const bool occ = c < n && (stored || ((uint64_t)x < thr && c != i));
        const unsigned long long m = __ballot(occ);
        bool same = false;
        if (with_t && occ) same = labels[c] == li;
        const unsigned long long mt = with_t ? __ballot(same) : 0ull;
        if (FILL) {
            if (occ) {
                const int64_t q = at + bg_below(m);
                if (q >= q0 && q < q1) {
                    ncol[q] = (int32_t)c;
                    nrow[q] = (int32_t)i;
                    nval[q] = stored ? values[pos] : 1.0f;
                    nsrc[q] = stored ? pos : (int64_t)-1;
                } else {                                                      // (nrowptr was not counted from this graph, seed and threshold)
                    status[0] = DGG_BATCH_EDIT_BAD_GRAPH;
                }
            }
            if (same) {
                const int64_t q = tat + bg_below(mt);
                if (q >= t0 && q < t1) {
                    tcol[q] = (int32_t)c;
                    trow[q] = (int32_t)i;
                } else {
                    status[0] = DGG_BATCH_EDIT_BAD_GRAPH;
                }
            }
            at += __popcll(m);
            tat += __popcll(mt);
        } else {
            cnt += __popcll(m);
            tcnt += __popcll(mt);
        }
    }
    if (!FILL && lane == 0) {
        ndeg_i[i] = cnt;
        if (with_t) tdeg_i[i] = tcnt;
    }
}

}  // namespace dgg

extern "C" int dgg_batch_graph_edit(int phase, const int64_t *rowptr, const int32_t *col, const float *values, int64_t n, int64_t E,
                                    const int32_t *labels, uint32_t s0, uint32_t s1, uint64_t thr, int32_t *ndeg_i, int32_t *tdeg_i,
                                    const int64_t *nrowptr, int64_t E_n, int32_t *ncol, int32_t *nrow, float *nval, int64_t *nsrc,
                                    const int64_t *trowptr, int64_t E_t, int32_t *tcol, int32_t *trow, int32_t *status, void *stream) {
    using namespace dgg;
    hipStream_t st = (hipStream_t)stream;
    if (phase != DGG_BATCH_EDIT_COUNT && phase != DGG_BATCH_EDIT_FILL)
        return dgg_set_error(DGG_ERR_ARG, "dgg_batch_graph_edit: phase is neither DGG_BATCH_EDIT_COUNT nor DGG_BATCH_EDIT_FILL");
    if (n < 0 || n >= ((int64_t)1 << 31)) return dgg_set_error(DGG_ERR_ARG, "dgg_batch_graph_edit: n outside 0 <= n < 2^31");
    if (E < 0 || E_n < 0 || E_t < 0) return dgg_set_error(DGG_ERR_ARG, "dgg_batch_graph_edit: E, E_n or E_t < 0");
    if (thr > ((uint64_t)1 << 32)) return dgg_set_error(DGG_ERR_ARG, "dgg_batch_graph_edit: thr > 2^32 (a probability above 1)");
    if (status == nullptr) return dgg_set_error(DGG_ERR_ARG, "dgg_batch_graph_edit: status is NULL");
    if (n == 0) return DGG_OK;
    const dim3 grid((unsigned)((n + BG_WAVES - 1) / BG_WAVES)), block(BG_WAVES * 64);
    if (phase == DGG_BATCH_EDIT_COUNT) {
        if ((labels != nullptr) != (tdeg_i != nullptr))
            return dgg_set_error(DGG_ERR_ARG, "dgg_batch_graph_edit: labels and tdeg_i go together (COUNT: the target is counted with labels only)");
        if (rowptr == nullptr || ndeg_i == nullptr || (col == nullptr && E > 0))
            return dgg_set_error(DGG_ERR_ARG, "dgg_batch_graph_edit: a NULL array (COUNT: rowptr, col, ndeg_i)");
        hipLaunchKernelGGL(batch_edit_k<false>, grid, block, 0, st, rowptr, col, values, n, E, labels, s0, s1, thr, ndeg_i, tdeg_i, nrowptr, E_n, ncol,
                           nrow, nval, nsrc, trowptr, E_t, tcol, trow, status);
        return dgg_check_launch("dgg_batch_graph_edit (COUNT)");
    }
    if (labels == nullptr ? (trowptr != nullptr || tcol != nullptr || trow != nullptr) : trowptr == nullptr)
        return dgg_set_error(DGG_ERR_ARG, "dgg_batch_graph_edit: labels and the target arrays go together (FILL: trowptr, tcol, trow with labels only)");
    if (rowptr == nullptr || nrowptr == nullptr || ((col == nullptr || values == nullptr) && E > 0) ||
        ((ncol == nullptr || nrow == nullptr || nval == nullptr || nsrc == nullptr) && E_n > 0) ||
        (labels != nullptr && (tcol == nullptr || trow == nullptr) && E_t > 0))
        return dgg_set_error(DGG_ERR_ARG, "dgg_batch_graph_edit: a NULL array (FILL: rowptr, col, values, nrowptr, ncol, nrow, nval, nsrc; trowptr, tcol, trow)");
    hipLaunchKernelGGL(batch_edit_k<true>, grid, block, 0, st, rowptr, col, values, n, E, labels, s0, s1, thr, ndeg_i, tdeg_i, nrowptr, E_n, ncol, nrow,
                       nval, nsrc, trowptr, E_t, tcol, trow, status);
    return dgg_check_launch("dgg_batch_graph_edit (FILL)");
}
