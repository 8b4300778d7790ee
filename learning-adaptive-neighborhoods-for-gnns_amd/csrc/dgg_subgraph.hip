// dgg_subgraph.hip -- mini-batch sampling on the device: the node sets of GraphSAINT's random-walk sampler and the sub-graph a node set
// induces (reference train_large_graphs.py:402-421 draws both with PyG's GraphSAINTRandomWalkSampler / ClusterLoader on the host).
// The contract -- the walk law, the four phases of the cut and what the caller's prefix sums do between them, the status word -- is the
// comment of include/dgg_hip_sampling.h; this file only says how each kernel keeps it.
//
// Walk: one thread per walk.  Step t needs the node of step t - 1, so a walk is a chain of dependent gathers (rowptr, then col); the
// parallelism is across walks.
// Cut: one wavefront per selected node walks that node's CSR row 64 entries at a time (coalesced), and asks newid[] whether each
// neighbour is in the set.  COUNT takes popcount(ballot); FILL takes the ballot prefix below each lane (mbcnt) as the lane's slot, so
// the kept entries keep their order.  No kernel here uses an atomic, and every store lands at an index that only one lane of one
// wavefront computes (MARK's duplicate nodes and the status word store the same value from several lanes), so the output is the same
// bits on every run.
// Nothing is read or written out of bounds whatever the DEVICE data holds: nodes, row ranges, columns and fill positions are all checked
// against N, E, rows and E_b before they index anything; an item that fails is skipped and reported in the status word.
#include "dgg_api_internal.h"
#include "../../include/dgg_hip_sampling.h"
#include "dgg_common.h"

namespace dgg {

constexpr int SUB_THREADS = 256;      // threads of the elementwise kernels
constexpr int SUB_WAVES = 4;          // selected nodes (wavefronts) per workgroup of the row kernels

__global__ __launch_bounds__(SUB_THREADS) void random_walk_nodes_k(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t N,
                                                                   int64_t E, const int32_t *__restrict__ roots, int64_t B, int L, uint32_t s0,
                                                                   uint32_t s1, int32_t *__restrict__ walk, int32_t *__restrict__ status) {
    const int64_t b = (int64_t)blockIdx.x * SUB_THREADS + threadIdx.x;
    if (b >= B) return;
    int32_t *out = walk + b * ((int64_t)L + 1);
    int32_t v = roots[b];
    if (v < 0 || v >= N) {
        for (int t = 0; t <= L; t++) out[t] = -1;
        status[0] = DGG_SAMPLING_BAD_NODE;
        return;
    }
    out[0] = v;
    const uint32_t kb = mix32((uint32_t)b ^ s0) ^ s1;
    for (int t = 1; t <= L; t++) {
        const int64_t p0 = rowptr[v], p1 = rowptr[v + 1];
        if (p0 < 0 || p1 < p0 || p1 > E) {
            status[0] = DGG_SAMPLING_BAD_GRAPH;
        } else if (p1 > p0) {
            const uint64_t d = (uint64_t)(p1 - p0);                           // < 2^32: E is
            const uint32_t x = mix32(kb ^ ((uint32_t)t * 0x9E3779B9u));
            const int32_t u = col[p0 + (int64_t)(((uint64_t)x * d) >> 32)];
            if (u < 0 || u >= N) status[0] = DGG_SAMPLING_BAD_GRAPH;
            else v = u;
        }
        out[t] = v;
    }
}

__global__ __launch_bounds__(SUB_THREADS) void subgraph_mark_k(const int32_t *__restrict__ nodes, int64_t M, int64_t N, int32_t *__restrict__ flag,
                                                               int32_t *__restrict__ status) {
    const int64_t m = (int64_t)blockIdx.x * SUB_THREADS + threadIdx.x;
    if (m >= M) return;
    const int32_t v = nodes[m];
    if (v >= 0 && v < N) flag[v] = 1;
    else status[0] = DGG_SAMPLING_BAD_NODE;
}

__global__ __launch_bounds__(SUB_THREADS) void subgraph_relabel_k(const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, int64_t N,
                                                                  int64_t rows, int32_t *__restrict__ newid, int32_t *__restrict__ orig,
                                                                  int32_t *__restrict__ status) {
    const int64_t v = (int64_t)blockIdx.x * SUB_THREADS + threadIdx.x;
    if (v >= N) return;
    int32_t r = -1;
    if (flag[v] != 0) {
        r = rank[v] - 1;
        if (r >= 0 && r < rows) {
            orig[r] = (int32_t)v;
        } else {                                                              // (rank is not the prefix sum of flag)
            status[0] = DGG_SAMPLING_BAD_GRAPH;
            r = -1;
        }
    }
    newid[v] = r;
}

__device__ __forceinline__ double sub_shfl_xor_f64(double v, int mask) {
    return __longlong_as_double((long long)shfl_xor_u64((uint64_t)__double_as_longlong(v), mask));
}

// the CSR row of selected node r as a checked range: false (and the status word set) when the node or its range is not inside the graph
__device__ __forceinline__ bool sub_row_range(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ orig, int64_t r, int64_t N, int64_t E,
                                              int64_t &p0, int64_t &p1, int32_t *__restrict__ status) {
    const int32_t v = orig[r];
    if (v >= 0 && v < N) {
        p0 = rowptr[v];
        p1 = rowptr[v + 1];
        if (p0 >= 0 && p0 <= p1 && p1 <= E) return true;
    }
    status[0] = DGG_SAMPLING_BAD_GRAPH;
    return false;
}

// is the entry at position p (this lane's, when in) kept: its column a node of the set?  u: the column, nu: its new id
__device__ __forceinline__ bool sub_keep(const int32_t *__restrict__ col, const int32_t *__restrict__ newid, int64_t N, int64_t p, bool in, int32_t &nu,
                                         int32_t *__restrict__ status) {
    nu = -1;
    if (!in) return false;
    const int32_t u = col[p];
    if (u < 0 || u >= N) {
        status[0] = DGG_SAMPLING_BAD_GRAPH;
        return false;
    }
    nu = newid[u];
    return nu >= 0;
}

__global__ __launch_bounds__(SUB_WAVES * 64) void subgraph_count_k(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                   const float *__restrict__ values, int64_t N, int64_t E,
                                                                   const int32_t *__restrict__ rank, const int32_t *__restrict__ newid,
                                                                   const int32_t *__restrict__ orig, int64_t rows, int32_t *__restrict__ bdeg_i,
                                                                   float *__restrict__ bdeg, int32_t *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * SUB_WAVES + wave_id();
    if (r >= rows) return;                                                    // (wave-uniform, as every branch on r below)
    int cnt = 0;
    double s = 0.0;
    int64_t p0 = 0, p1 = 0;
    if (r < (int64_t)rank[N - 1] && sub_row_range(rowptr, orig, r, N, E, p0, p1, status)) {
        for (int64_t t = p0; t < p1; t += 64) {
            const int64_t p = t + lane;
            int32_t nu;
            const bool keep = sub_keep(col, newid, N, p, p < p1, nu, status);
            cnt += __popcll(__ballot(keep));
            if (values != nullptr && keep) s += (double)values[p];
        }
        if (values != nullptr) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) s += sub_shfl_xor_f64(s, off);
        }
    }
    if (lane == 0) {
        bdeg_i[r] = cnt;
        if (bdeg != nullptr) bdeg[r] = (float)s;
    }
}

__global__ __launch_bounds__(SUB_WAVES * 64) void subgraph_fill_k(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t N,
                                                                  int64_t E, const int32_t *__restrict__ newid, const int32_t *__restrict__ orig,
                                                                  int64_t rows, const int64_t *__restrict__ browptr, int64_t E_b,
                                                                  int32_t *__restrict__ bcol, int64_t *__restrict__ beid, int32_t *__restrict__ brow,
                                                                  int32_t *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * SUB_WAVES + wave_id();
    if (r >= rows) return;
    int64_t p0, p1;
    if (!sub_row_range(rowptr, orig, r, N, E, p0, p1, status)) return;
    int64_t q0 = browptr[r], q1 = browptr[r + 1];                             // this row's slots, clamped to the output arrays
    if (q0 < 0) q0 = 0;
    if (q1 > E_b) q1 = E_b;
    int64_t at = browptr[r];
    for (int64_t t = p0; t < p1; t += 64) {
        const int64_t p = t + lane;
        int32_t nu;
        const bool keep = sub_keep(col, newid, N, p, p < p1, nu, status);
        const unsigned long long m = __ballot(keep);
        const int64_t q = at + (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (keep) {
            if (q >= q0 && q < q1) {
                bcol[q] = nu;
                beid[q] = p;
                brow[q] = (int32_t)r;
            } else {                                                          // (browptr was not counted from this node set)
                status[0] = DGG_SAMPLING_BAD_GRAPH;
            }
        }
        at += __popcll(m);
    }
}

static inline unsigned sub_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace dgg

extern "C" int dgg_random_walk_nodes(const int64_t *rowptr, const int32_t *col, int64_t N, int64_t E, const int32_t *roots, int64_t B, int L,
                                     uint32_t s0, uint32_t s1, int32_t *walk, int32_t *status, void *stream) {
    using namespace dgg;
    if (N < 0 || N >= ((int64_t)1 << 31)) return dgg_set_error(DGG_ERR_ARG, "dgg_random_walk_nodes: N outside 0 <= N < 2^31");
    if (E < 0 || E >= ((int64_t)1 << 32))
        return dgg_set_error(DGG_ERR_ARG, "dgg_random_walk_nodes: E outside 0 <= E < 2^32 (a row degree d >= 2^32 cannot be addressed by the pick)");
    if (B < 0 || B >= ((int64_t)1 << 31)) return dgg_set_error(DGG_ERR_ARG, "dgg_random_walk_nodes: B outside 0 <= B < 2^31");
    if (L < 0) return dgg_set_error(DGG_ERR_ARG, "dgg_random_walk_nodes: L < 0");
    if (B == 0) return DGG_OK;
    if (N == 0) return dgg_set_error(DGG_ERR_ARG, "dgg_random_walk_nodes: B > 0 roots on a graph without nodes (N == 0)");
    if (rowptr == nullptr || roots == nullptr || walk == nullptr || status == nullptr || (col == nullptr && E > 0 && L > 0))
        return dgg_set_error(DGG_ERR_ARG, "dgg_random_walk_nodes: a NULL array");
    hipLaunchKernelGGL(random_walk_nodes_k, dim3(sub_blocks(B, SUB_THREADS)), dim3(SUB_THREADS), 0, (hipStream_t)stream, rowptr, col, N, E, roots, B, L,
                       s0, s1, walk, status);
    return dgg_check_launch("dgg_random_walk_nodes");
}

extern "C" int dgg_induced_subgraph(int phase, const int64_t *rowptr, const int32_t *col, const float *values, int64_t N, int64_t E,
                                    const int32_t *nodes, int64_t M, int32_t *flag, const int32_t *rank, int32_t *newid, int32_t *orig, int64_t rows,
                                    int32_t *bdeg_i, float *bdeg, const int64_t *browptr, int64_t E_b, int32_t *bcol, int64_t *beid, int32_t *brow,
                                    int32_t *status, void *stream) {
    using namespace dgg;
    hipStream_t st = (hipStream_t)stream;
    if (phase < DGG_SUBGRAPH_MARK || phase > DGG_SUBGRAPH_FILL)
        return dgg_set_error(DGG_ERR_ARG, "dgg_induced_subgraph: phase is none of DGG_SUBGRAPH_MARK / RELABEL / COUNT / FILL");
    if (N < 0 || N >= ((int64_t)1 << 31)) return dgg_set_error(DGG_ERR_ARG, "dgg_induced_subgraph: N outside 0 <= N < 2^31");
    if (M < 0 || E < 0 || rows < 0 || E_b < 0) return dgg_set_error(DGG_ERR_ARG, "dgg_induced_subgraph: M, E, rows or E_b < 0");
    if (rows > N) return dgg_set_error(DGG_ERR_ARG, "dgg_induced_subgraph: rows > N (a node set has at most N distinct members)");
    if (status == nullptr) return dgg_set_error(DGG_ERR_ARG, "dgg_induced_subgraph: status is NULL");
    if (N == 0) return DGG_OK;
    switch (phase) {
    case DGG_SUBGRAPH_MARK: {
        if (flag == nullptr || (nodes == nullptr && M > 0)) return dgg_set_error(DGG_ERR_ARG, "dgg_induced_subgraph: a NULL array (MARK: nodes, flag)");
        const int rc = dgg_check_hip(hipMemsetAsync(flag, 0, (size_t)N * sizeof(int32_t), st), "dgg_induced_subgraph (MARK: clearing flag)");
        if (rc != DGG_OK || M == 0) return rc;
        hipLaunchKernelGGL(subgraph_mark_k, dim3(sub_blocks(M, SUB_THREADS)), dim3(SUB_THREADS), 0, st, nodes, M, N, flag, status);
        return dgg_check_launch("dgg_induced_subgraph (MARK)");
    }
    case DGG_SUBGRAPH_RELABEL:
        if (flag == nullptr || rank == nullptr || newid == nullptr || (orig == nullptr && rows > 0))
            return dgg_set_error(DGG_ERR_ARG, "dgg_induced_subgraph: a NULL array (RELABEL: flag, rank, newid, orig)");
        hipLaunchKernelGGL(subgraph_relabel_k, dim3(sub_blocks(N, SUB_THREADS)), dim3(SUB_THREADS), 0, st, flag, rank, N, rows, newid, orig, status);
        return dgg_check_launch("dgg_induced_subgraph (RELABEL)");
    case DGG_SUBGRAPH_COUNT:
        if (rows == 0) return DGG_OK;
        if (rowptr == nullptr || (col == nullptr && E > 0) || rank == nullptr || newid == nullptr || orig == nullptr || bdeg_i == nullptr ||
            (values != nullptr && bdeg == nullptr))
            return dgg_set_error(DGG_ERR_ARG, "dgg_induced_subgraph: a NULL array (COUNT: rowptr, col, rank, newid, orig, bdeg_i; bdeg with values)");
        hipLaunchKernelGGL(subgraph_count_k, dim3(sub_blocks(rows, SUB_WAVES)), dim3(SUB_WAVES * 64), 0, st, rowptr, col, values, N, E, rank, newid, orig,
                           rows, bdeg_i, values != nullptr ? bdeg : (float *)nullptr, status);
        return dgg_check_launch("dgg_induced_subgraph (COUNT)");
    default:
        if (rows == 0 || E_b == 0) return DGG_OK;
        if (rowptr == nullptr || col == nullptr || newid == nullptr || orig == nullptr || browptr == nullptr || bcol == nullptr || beid == nullptr ||
            brow == nullptr)
            return dgg_set_error(DGG_ERR_ARG, "dgg_induced_subgraph: a NULL array (FILL: rowptr, col, newid, orig, browptr, bcol, beid, brow)");
        hipLaunchKernelGGL(subgraph_fill_k, dim3(sub_blocks(rows, SUB_WAVES)), dim3(SUB_WAVES * 64), 0, st, rowptr, col, N, E, newid, orig, rows, browptr,
                           E_b, bcol, beid, brow, status);
        return dgg_check_launch("dgg_induced_subgraph (FILL)");
    }
}
