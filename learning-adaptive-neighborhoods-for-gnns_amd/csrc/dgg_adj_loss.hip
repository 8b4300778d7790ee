// dgg_adj_loss.hip -- F.mse_loss(out_adj.to_dense(), gt_adj.to_dense()) (reference train_reddit.py:236-251, train_large_graphs.py:236-251)
// on sparse data: the squared error of the learned adjacency A against a target graph G over ALL N x N pairs, without either dense
// operand, and the per-entry gradient of it in the same pass.
//
// One wavefront per row joins the learned row with the target's CSR row, as adj_stats_rows does.  The learned row is a range of
// entries [e0, e1) walked 64 at a time (lane r owns entry r of a piece) whatever its form: entries [i K, (i+1) K) of a [rows,K] list,
// the chunks [cptr[i], cptr[i+1]) of chunked rows, or the CSR segment [rowptr_l[i], rowptr_l[i+1]) -- one kernel, templated on how the
// range is found.
//   1. every learned entry looks its target value up by binary search (prior_value_at): d = a - g as ONE float32 subtraction, as the
//      dense reference forms it elementwise; d * d in double; dval = scale * 2 * d when the gradient is asked for (0.0f at padding).
//   2. the target entries that no learned slot holds add g^2.  Of the two ways to take this term, this file takes (a): the target row
//      is walked 64 entries at a time against the learned row's lanes, as adj_stats_rows step 2 does.  Every term of S is then a
//      square: nothing cancels, so the 2^-22 bound on the loss holds for any data -- (b), sum_G g^2 - sum_{A and G} g^2, would lose it
//      exactly where training drives the loss (A close to G, S far below sum_G g^2).
// A learned row must hold each column at most once (true of everything the generator returns): a column held twice is counted twice
// in step 1.  This is not checked.
// Sums are double and folded in a FIXED order: the wavefront butterfly (addition commutes: both partners compute the same bits), the 16
// rows of a workgroup in ascending order, then the workgroups' records by one block (thread t folds records t, t + 256, ... in ascending
// order; the 256 partials in a binary tree).  No floating-point atomics: two launches on the same input give the same bits.  The result
// is rounded to float32 only when it is stored.
#include "dgg_api_internal.h"
#include "../../include/dgg_hip_adj_loss.h"
#include "dgg_common.h"
#include "dgg_prior_lookup.h"

namespace dgg {

constexpr int LOSS_WAVES = 16;        // rows per workgroup of the row kernel
constexpr int LOSS_FOLD = 256;        // threads of the fold kernel
enum { LOSS_LIST = 0, LOSS_CHUNKED = 1, LOSS_CSR = 2 };

__device__ __forceinline__ double loss_shfl_xor_f64(double v, int mask) {
    return __longlong_as_double((long long)shfl_xor_u64((uint64_t)__double_as_longlong(v), mask));
}

// idx: the learned columns (col_l for LOSS_CSR); ends: cptr (LOSS_CHUNKED, int32) or rowptr_l (LOSS_CSR, int64), unused for LOSS_LIST
template <int FORM>
__global__ __launch_bounds__(LOSS_WAVES * 64) void adj_loss_rows(const int32_t *__restrict__ idx, const float *__restrict__ val, int64_t rows, int K,
                                                                 const void *__restrict__ ends, int64_t chunks,
                                                                 const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                 const float *__restrict__ gval, float scale, float *__restrict__ dval,
                                                                 double *__restrict__ rec) {
    __shared__ double sh[LOSS_WAVES];
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * LOSS_WAVES + wave_id();
    if (row < rows) {                                                     // (wave-uniform)
        const PriorCsr P = prior_csr(rowptr, col, gval);
        // the learned row: entries [e0, e1), piece t holds entries t + lane
        int64_t e0, e1;
        if (FORM == LOSS_CHUNKED) {
            const int32_t *cptr = (const int32_t *)ends;
            int64_t c0 = cptr[row], c1 = cptr[row + 1];
            if (c0 < 0) c0 = 0;
            if (c1 > chunks) c1 = chunks;
            e0 = c0 * 64;
            e1 = c1 * 64;
        } else if (FORM == LOSS_CSR) {
            const int64_t *rp = (const int64_t *)ends;
            e0 = rp[row];
            e1 = rp[row + 1];
        } else {
            e0 = row * K;
            e1 = e0 + K;
        }
        const float scale2 = 2.0f * scale;                                // (exact)
        double s = 0.0;
        // 1. the learned entries: the target value of each by binary search in the target row
        for (int64_t t = e0; t < e1; t += 64) {
            const int64_t e = t + lane;
            const bool in = e < e1;
            const int32_t j = in ? idx[e] : -1;
            float dv = 0.0f;
            if (j >= 0) {
                const float d = __fsub_rn(val[e], prior_value_at(P, row, j));
                s += (double)d * (double)d;
                dv = scale2 * d;
            }
            if (dval != nullptr && in) dval[e] = dv;
        }
        // 2. the target row, 64 entries at a time: the entries that no learned slot holds (a_ij = 0: d = -g_ij)
        const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
        for (int64_t t = p0; t < p1; t += 64) {
            const int64_t p = t + lane;
            const bool in = p < p1;
            const int32_t cj = in ? col[p] : -1;
            const float g = in ? gval[p] : 0.0f;
            bool held = false;
            if (__ballot(in && g != 0.0f) != 0ull) {                          // (wave-uniform: a tile of zeros adds nothing)
                for (int64_t u = e0; u < e1; u += 64) {
                    const int32_t j = u + lane < e1 ? idx[u + lane] : -1;
                    const int nr = e1 - u < 64 ? (int)(e1 - u) : 64;          // (wave-uniform)
                    for (int r = 0; r < nr; r++) {
                        const int32_t jr = bcast(j, r);
                        held = held || (jr >= 0 && jr == cj);
                    }
                }
            }
            if (in && !held) s += (double)g * (double)g;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += loss_shfl_xor_f64(s, off);
        if (lane == 0) sh[wave_id()] = s;
        // chunked rows: the chunks past the last row belong to no wavefront's range; they are padding, shared out over the rows
        if (FORM == LOSS_CHUNKED && dval != nullptr) {
            int64_t ct = ((const int32_t *)ends)[rows];
            if (ct < 0) ct = 0;
            for (int64_t c = ct + row; c < chunks; c += rows) dval[c * 64 + lane] = 0.0f;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                               // the workgroup's rows, in ascending order
        double f = 0.0;
        for (int v = 0; v < LOSS_WAVES && (int64_t)blockIdx.x * LOSS_WAVES + v < rows; v++) f += sh[v];
        rec[blockIdx.x] = f;
    }
}

__global__ __launch_bounds__(LOSS_FOLD) void adj_loss_fold(const double *__restrict__ rec, int64_t nrec, int64_t rows, int reduction,
                                                           float *__restrict__ out) {
    __shared__ double part[LOSS_FOLD];
    const int t = threadIdx.x;
    double f = 0.0;
    for (int64_t i = t; i < nrec; i += LOSS_FOLD) f += rec[i];
    part[t] = f;
    __syncthreads();
    for (int s = LOSS_FOLD / 2; s >= 1; s >>= 1) {
        if (t < s) part[t] = part[t] + part[t + s];
        __syncthreads();
    }
    if (t == 0) {
        const double n = (double)rows;
        double S = part[0];
        if (reduction == DGG_ADJ_LOSS_MEAN) S = rows > 0 ? S / (n * n) : __longlong_as_double(0x7ff8000000000000ll);
        out[0] = (float)S;
    }
}

}  // namespace dgg

extern "C" int dgg_adj_mse_loss(const int32_t *idx, const float *val, int64_t rows, int K, const int32_t *cptr, int64_t chunks,
                                const int64_t *rowptr_l, const int32_t *col_l, const int64_t *rowptr, const int32_t *col, const float *gval,
                                int reduction, float scale, void *ws, float *dval, float *out, void *stream) {
    using namespace dgg;
    hipStream_t st = (hipStream_t)stream;
    const bool csr = rowptr_l != nullptr || col_l != nullptr;
    if (rows < 0 || rows >= ((int64_t)1 << 31)) return dgg_set_error(DGG_ERR_ARG, "dgg_adj_mse_loss: rows outside 0 <= rows < 2^31");
    if (csr && (idx != nullptr || cptr != nullptr))
        return dgg_set_error(DGG_ERR_ARG, "dgg_adj_mse_loss: more than one row form (rowptr_l / col_l together with idx / cptr)");
    if (!csr && (K < 1 || K > 64)) return dgg_set_error(DGG_ERR_ARG, "dgg_adj_mse_loss: K outside 1..64 (wider rows arrive as chunked or CSR rows)");
    if (cptr != nullptr && (K != 64 || chunks < 0 || chunks >= ((int64_t)1 << 31)))
        return dgg_set_error(DGG_ERR_ARG, "dgg_adj_mse_loss: chunked rows have K = 64 and 0 <= chunks < 2^31");
    if (reduction != DGG_ADJ_LOSS_MEAN && reduction != DGG_ADJ_LOSS_SUM)
        return dgg_set_error(DGG_ERR_ARG, "dgg_adj_mse_loss: reduction is neither DGG_ADJ_LOSS_MEAN nor DGG_ADJ_LOSS_SUM");
    if (out == nullptr) return dgg_set_error(DGG_ERR_ARG, "dgg_adj_mse_loss: out is NULL");
    if (rows > 0) {
        if (val == nullptr || rowptr == nullptr || col == nullptr || gval == nullptr || ws == nullptr ||
            (csr ? (rowptr_l == nullptr || col_l == nullptr) : idx == nullptr))
            return dgg_set_error(DGG_ERR_ARG, "dgg_adj_mse_loss: a NULL array");
        if (((uintptr_t)ws & 7) != 0) return dgg_set_error(DGG_ERR_ARG, "dgg_adj_mse_loss: ws is not 8-byte aligned");
        const dim3 grid((unsigned)((rows + LOSS_WAVES - 1) / LOSS_WAVES)), block(LOSS_WAVES * 64);
        if (csr)
            hipLaunchKernelGGL(adj_loss_rows<LOSS_CSR>, grid, block, 0, st, col_l, val, rows, K, (const void *)rowptr_l, chunks, rowptr, col, gval,
                               scale, dval, (double *)ws);
        else if (cptr != nullptr)
            hipLaunchKernelGGL(adj_loss_rows<LOSS_CHUNKED>, grid, block, 0, st, idx, val, rows, K, (const void *)cptr, chunks, rowptr, col, gval,
                               scale, dval, (double *)ws);
        else
            hipLaunchKernelGGL(adj_loss_rows<LOSS_LIST>, grid, block, 0, st, idx, val, rows, K, (const void *)nullptr, chunks, rowptr, col, gval,
                               scale, dval, (double *)ws);
        const int rc = dgg_check_launch("dgg_adj_mse_loss (rows)");
        if (rc != DGG_OK) return rc;
    }
    hipLaunchKernelGGL(adj_loss_fold, dim3(1), dim3(LOSS_FOLD), 0, st, (const double *)ws, (rows + LOSS_WAVES - 1) / LOSS_WAVES, rows, reduction, out);
    return dgg_check_launch("dgg_adj_mse_loss (fold)");
}
