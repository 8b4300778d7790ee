// dgg_adj_stats.hip -- get_adj_diff_stats (reference dgm.py:1313-1350) on sparse data: how far the learned soft adjacency has moved from
// the input graph, and the learned degree from the input degree, without the six dense [N,N] temporaries of the reference.
//
// One wavefront per row joins the learned row (64-rank list or chunked rows; lane r owns entry r of a chunk) with the input graph's CSR
// row: every learned entry looks its input value up by binary search (prior_value_at), and the input row is walked 64 entries at a time
// against the learned row's lanes for the input edges the generator did not select.  Moments are carried as (n, mean, M2) in double
// and merged with Chan's formula in a FIXED order -- lane partials by the xor butterfly with the lower lane as the left operand, the 16
// rows of a workgroup in ascending order, then the workgroups' records by one block (thread t folds records t, t + 256, ... in ascending
// order; the 256 partials in a binary tree with the lower thread as the left operand).  No floating-point atomics: two launches on the
// same input give the same bits.  The ten results are rounded to float32 only when they are stored.
#include "dgg_api_internal.h"
#include "../../include/dgg_hip_next.h"
#include "dgg_common.h"
#include "dgg_prior_lookup.h"

namespace dgg {

constexpr int STATS_WAVES = 16;       // rows per workgroup of the row kernel
constexpr int STATS_FOLD = 256;       // threads of the fold kernel
constexpr int STATS_ROW = 8;          // doubles a row leaves in LDS: on (n, mean, M2), off (n, mean, M2), sum_j a_ij, k_i
constexpr int STATS_REC = 12;         // doubles per workgroup record: on, off, k_diff (n, mean, M2 each), sum of sum_j a_ij, sum of k_i, pad

struct Moments {                      // n values with mean `mean` and sum of squared deviations M2
    double n, mean, M2;
};

__device__ __forceinline__ void mom_add(Moments &m, double d) {           // Welford: one more value
    m.n += 1.0;
    const double delta = d - m.mean;
    m.mean += delta / m.n;
    m.M2 += delta * (d - m.mean);
}

// Chan et al.: a then b.  Not bitwise symmetric in (a, b): every caller fixes which operand is the left one.
__device__ __forceinline__ Moments mom_merge(const Moments &a, const Moments &b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    Moments r;
    r.n = a.n + b.n;
    const double delta = b.mean - a.mean;
    r.mean = a.mean + delta * (b.n / r.n);
    r.M2 = (a.M2 + b.M2) + (delta * delta) * (a.n * (b.n / r.n));
    return r;
}

__device__ __forceinline__ double shfl_xor_f64(double v, int mask) {
    return __longlong_as_double((long long)shfl_xor_u64((uint64_t)__double_as_longlong(v), mask));
}

// every lane ends with the wavefront's moments: the lane whose `off` bit is clear is the left operand, so both partners compute the same bits
__device__ __forceinline__ Moments wave_moments(Moments m, int lane) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Moments o;
        o.n = shfl_xor_f64(m.n, off);
        o.mean = shfl_xor_f64(m.mean, off);
        o.M2 = shfl_xor_f64(m.M2, off);
        m = (lane & off) ? mom_merge(o, m) : mom_merge(m, o);
    }
    return m;
}

__device__ __forceinline__ double wave_sum_f64(double v) {                // (addition commutes: no operand order to fix)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += shfl_xor_f64(v, off);
    return v;
}

// the pair (i, c) with input value a and learned value w (dgm.py:1321-1328): on-edge where a > 0, off-edge where a == 0, kept iff the
// float32 difference is not zero; a stored negative (or NaN) value is in neither population
__device__ __forceinline__ void pair_add(Moments &on, Moments &off, float a, float w) {
    const float d = __fadd_rn(a, -w);
    if (a > 0.0f) {
        if (d != 0.0f) mom_add(on, (double)d);
    } else if (a == 0.0f) {
        if (d != 0.0f) mom_add(off, (double)d);
    }
}

struct Fold {                         // what one thread of the fold kernel carries
    Moments on, off, kd;
    double asum, ksum;
};

__device__ __forceinline__ Fold fold_merge(const Fold &a, const Fold &b) {
    Fold r;
    r.on = mom_merge(a.on, b.on);
    r.off = mom_merge(a.off, b.off);
    r.kd = mom_merge(a.kd, b.kd);
    r.asum = a.asum + b.asum;
    r.ksum = a.ksum + b.ksum;
    return r;
}

__device__ __forceinline__ void fold_store(double *o, const Fold &f) {
    o[0] = f.on.n; o[1] = f.on.mean; o[2] = f.on.M2;
    o[3] = f.off.n; o[4] = f.off.mean; o[5] = f.off.M2;
    o[6] = f.kd.n; o[7] = f.kd.mean; o[8] = f.kd.M2;
    o[9] = f.asum; o[10] = f.ksum;
}
__device__ __forceinline__ Fold fold_load(const double *r) {
    return Fold{{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, {r[6], r[7], r[8]}, r[9], r[10]};
}

// CHUNKED: the learned row i is the chunks [cptr[i], cptr[i+1]) of idx / w [chunks,64]; otherwise entries [i K, (i+1) K) of idx / w [rows,K]
template <bool CHUNKED>
__global__ __launch_bounds__(STATS_WAVES * 64) void adj_stats_rows(const int32_t *__restrict__ idx, const float *__restrict__ w, int64_t rows,
                                                                  int K, const int32_t *__restrict__ cptr, int64_t chunks,
                                                                  const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                  const float *__restrict__ aval, const float *__restrict__ k,
                                                                  double *__restrict__ rec) {
    __shared__ double sh[STATS_WAVES][STATS_ROW];
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * STATS_WAVES + wave_id();
    if (row < rows) {                                                     // (wave-uniform)
        const PriorCsr P = prior_csr(rowptr, col, aval);
        // the learned row as 64-entry pieces [c0, c1): piece c holds entries base(c) + lane, the lanes below `width` being real slots
        int64_t c0 = row, c1 = row + 1;
        if (CHUNKED) {
            c0 = cptr[row];
            c1 = cptr[row + 1];
            if (c0 < 0) c0 = 0;
            if (c1 > chunks) c1 = chunks;
        }
        const int width = CHUNKED ? 64 : K;
        Moments on{0.0, 0.0, 0.0}, off{0.0, 0.0, 0.0};
        // 1. the learned entries: the input value of each by binary search in the input row
        for (int64_t c = c0; c < c1; c++) {
            const int64_t e = c * width + lane;
            const int32_t j = lane < width ? idx[e] : -1;
            if (j >= 0) pair_add(on, off, prior_value_at(P, row, j), w[e]);
        }
        // 2. the input row, 64 entries at a time: its sum, and the edges that no learned slot holds (w_ij = 0: d = a_ij)
        const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
        double asum = 0.0;
        for (int64_t t = p0; t < p1; t += 64) {
            const int64_t p = t + lane;
            const bool in = p < p1;
            const int32_t cj = in ? col[p] : -1;
            const float a = in ? aval[p] : 0.0f;
            asum += (double)a;
            bool held = false;
            if (__ballot(in && a > 0.0f) != 0ull) {                           // (wave-uniform: a tile without a positive value adds nothing)
                for (int64_t c = c0; c < c1; c++) {
                    const int32_t j = lane < width ? idx[c * width + lane] : -1;
#pragma unroll 8
                    for (int r = 0; r < 64; r++) {
                        const int32_t jr = bcast(j, r);
                        held = held || (jr >= 0 && jr == cj);
                    }
                }
            }
            if (in && !held) pair_add(on, off, a, 0.0f);                      // (a == 0 gives d = 0: never kept)
        }
        on = wave_moments(on, lane);
        off = wave_moments(off, lane);
        asum = wave_sum_f64(asum);
        if (lane == 0) {
            double *o = sh[wave_id()];
            o[0] = on.n; o[1] = on.mean; o[2] = on.M2;
            o[3] = off.n; o[4] = off.mean; o[5] = off.M2;
            o[6] = asum; o[7] = (double)k[row];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                               // the workgroup's rows, in ascending order
        Fold f{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, 0.0};
        for (int v = 0; v < STATS_WAVES && (int64_t)blockIdx.x * STATS_WAVES + v < rows; v++) {
            const double *r = sh[v];
            f.on = mom_merge(f.on, Moments{r[0], r[1], r[2]});
            f.off = mom_merge(f.off, Moments{r[3], r[4], r[5]});
            mom_add(f.kd, r[7] - r[6]);                                   // k_i - sum_j a_ij (dgm.py:1331)
            f.asum += r[6];
            f.ksum += r[7];
        }
        fold_store(rec + (int64_t)blockIdx.x * STATS_REC, f);
    }
}

__device__ __forceinline__ float mom_mean(const Moments &m) { return (float)(m.n > 0.0 ? m.mean : __longlong_as_double(0x7ff8000000000000ll)); }
// unbiased; NaN for n < 2 as torch.std
__device__ __forceinline__ float mom_std(const Moments &m) {
    return (float)(m.n > 1.0 ? sqrt(m.M2 / (m.n - 1.0)) : __longlong_as_double(0x7ff8000000000000ll));
}

__global__ __launch_bounds__(STATS_FOLD) void adj_stats_fold(const double *__restrict__ rec, int64_t nrec, int64_t rows, float *__restrict__ out) {
    __shared__ Fold part[STATS_FOLD];
    const int t = threadIdx.x;
    Fold f{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, 0.0};
    for (int64_t i = t; i < nrec; i += STATS_FOLD) f = fold_merge(f, fold_load(rec + i * STATS_REC));
    part[t] = f;
    __syncthreads();
    for (int s = STATS_FOLD / 2; s >= 1; s >>= 1) {
        if (t < s) part[t] = fold_merge(part[t], part[t + s]);
        __syncthreads();
    }
    if (t == 0) {
        const Fold g = part[0];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const double n = (double)rows;
        out[DGG_ADJ_STATS_ON_N] = (float)g.on.n;
        out[DGG_ADJ_STATS_ON_MEAN] = mom_mean(g.on);
        out[DGG_ADJ_STATS_ON_STD] = mom_std(g.on);
        out[DGG_ADJ_STATS_OFF_N] = (float)g.off.n;
        out[DGG_ADJ_STATS_OFF_MEAN] = mom_mean(g.off);
        out[DGG_ADJ_STATS_OFF_STD] = mom_std(g.off);
        out[DGG_ADJ_STATS_IN_DEG_MEAN] = (float)(rows > 0 ? g.asum / n : nan);
        out[DGG_ADJ_STATS_K_DIFF_MEAN] = mom_mean(g.kd);
        out[DGG_ADJ_STATS_K_DIFF_STD] = mom_std(g.kd);
        out[DGG_ADJ_STATS_K_MEAN] = (float)(rows > 0 ? g.ksum / n : nan);
    }
}

}  // namespace dgg

extern "C" int dgg_adj_diff_stats(const int32_t *idx, const float *w, int64_t rows, int K, const int32_t *cptr, int64_t chunks,
                                  const int64_t *rowptr, const int32_t *col, const float *aval, const float *k, void *ws, float *out,
                                  void *stream) {
    using namespace dgg;
    hipStream_t st = (hipStream_t)stream;
    if (rows < 0 || rows >= ((int64_t)1 << 31)) return dgg_set_error(DGG_ERR_ARG, "dgg_adj_diff_stats: rows outside 0 <= rows < 2^31");
    if (K < 1 || K > 64) return dgg_set_error(DGG_ERR_ARG, "dgg_adj_diff_stats: K outside 1..64 (wider rows arrive as chunked rows)");
    if (cptr != nullptr && (K != 64 || chunks < 0 || chunks >= ((int64_t)1 << 31)))
        return dgg_set_error(DGG_ERR_ARG, "dgg_adj_diff_stats: chunked rows have K = 64 and 0 <= chunks < 2^31");
    if (out == nullptr) return dgg_set_error(DGG_ERR_ARG, "dgg_adj_diff_stats: out is NULL");
    if (rows > 0) {
        if (idx == nullptr || w == nullptr || rowptr == nullptr || col == nullptr || aval == nullptr || k == nullptr || ws == nullptr)
            return dgg_set_error(DGG_ERR_ARG, "dgg_adj_diff_stats: a NULL array");
        if (((uintptr_t)ws & 7) != 0) return dgg_set_error(DGG_ERR_ARG, "dgg_adj_diff_stats: ws is not 8-byte aligned");
        const dim3 grid((unsigned)((rows + STATS_WAVES - 1) / STATS_WAVES)), block(STATS_WAVES * 64);
        if (cptr != nullptr)
            hipLaunchKernelGGL(adj_stats_rows<true>, grid, block, 0, st, idx, w, rows, K, cptr, chunks, rowptr, col, aval, k, (double *)ws);
        else
            hipLaunchKernelGGL(adj_stats_rows<false>, grid, block, 0, st, idx, w, rows, K, cptr, chunks, rowptr, col, aval, k, (double *)ws);
        const int rc = dgg_check_launch("dgg_adj_diff_stats (rows)");
        if (rc != DGG_OK) return rc;
    }
    hipLaunchKernelGGL(adj_stats_fold, dim3(1), dim3(STATS_FOLD), 0, st, (const double *)ws, (rows + STATS_WAVES - 1) / STATS_WAVES, rows, out);
    return dgg_check_launch("dgg_adj_diff_stats (fold)");
}
