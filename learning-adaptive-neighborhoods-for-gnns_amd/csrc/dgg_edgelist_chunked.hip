// dgg_edgelist_chunked.hip -- edge-list candidates ranked into CHUNKED rows (rows of any width): dgg_edgelist_topk_chunked (u-v-dist) and
// dgg_edgelist_topk_p_chunked (given edge probabilities: the edge-MLP scorers), declared in include/dgg_hip_next.h.
//
// The reference takes the candidates of row i from the stored entries of in_adj (dgm.py:1613-1623), perturbs their probabilities
// (dgm.py:1211-1229), sorts the row (dgm.py:1404) and ramps over ALL of it with an unbounded learned degree (dgm.py:1402-1421).  The list
// kernels (edgelist_row_full<H> of dgg_topk.hip, edgelist_topk_p_kernel of dgg_edgemlp.hip) keep 64 ranks of a row; here row i keeps
// L_i = min(n_i, ceil(k_i + 8.5) + 1) ranks -- every rank that can carry weight -- in the chunks [cptr[i], cptr[i+1]) of a dgg_chunk_layout
// run on the clamped degrees min(k_i, n_i - 9.5), with the ramp fused.  Score chain, perturbation and key order are those kernels', to the
// bit: 16-byte loads of the candidate's row, the ascending __fmaf_rn chain, c_sqrt, score_from_dist / perturb_p, pair_noise keyed on the
// global pair (row0 + i, j); the key's payload is the column (u-v-dist) or the candidate's place in its row (given probabilities).
//
// One wavefront per row, no LDS.  The structure for wide rows is dgg_allpairs_mlp_wide.hip's: a row keeps MR descending 64-lane lists in
// registers (list 0: ranks 0..63, list 1: ranks 64..127, ...); a batch of 64 candidates is sorted once and cascaded down the lists (one
// bitonic half-cleaner per list: the upper 64 stay, the lower 64 carry on; a list whose last key beats the carry's first is skipped) to
// the row's depth min(M_i, MR).  Rows of more than MR chunks are finished by CONTINUATION passes of the same kernel: pass p settles the
// chunks [MR p, MR (p + 1)) and admits only keys strictly below the row's ceiling = the key at rank 64 MR p - 1, read back from what pass
// p - 1 wrote (the key order is total, so "strictly below" is exact among tied scores too).  The host launches ceil(maxm / MR) passes
// from the integer maxm: no device read-back.  A one-chunk row runs the same body at depth 1, which is the list kernels' merge.
#include "dgg_common.h"
#include "dgg_edgemlp_score.h"
#include "dgg_api_internal.h"
#include "../../include/dgg_hip_next.h"

#include <cstdarg>
#include <cstdio>

using namespace dgg;

namespace {

constexpr int WAVES = 4;          // wavefronts (rows) per workgroup
constexpr int MR = 8;             // 64-lane register lists per row = chunks a pass settles

struct Args {
    const float *xp;              // u-v-dist: [N,H]
    const float *p_edge, *ex_edge;   // given probabilities: [E], the per-candidate extra (nullable)
    int64_t row0, rows;
    const int64_t *rowptr;
    const int32_t *col;
    float t;
    int noise_mode;
    uint32_t s0, s1;
    const float *k;
    int mode;
    const int32_t *cptr;
    int64_t ccap;
    int32_t *idx;
    float *val, *ex_out;
    int32_t *eid;
    float *w, *rs;
    int pass;                     // chunks [MR pass, MR (pass + 1)) of every row
    unsigned nrow_blocks;         // workgroups beyond these (pass 0) write the spare chunks [cptr[rows], ccap) empty
};

// the key of candidate e of row i (e0: the row's first candidate).  H > 0: exp(t ||xp_i - xp_j||), edgelist_row_full<H>'s chain, payload =
// the column; H == 0: p_edge[e], edgelist_topk_p_kernel's perturbation, payload = e - e0
template <int H>
__device__ __forceinline__ uint64_t cand_key(const Args &a, int64_t i, int64_t e0, int64_t e) {
    const bool sym = a.noise_mode == 3;
    const int32_t j = a.col[e];
    if constexpr (H > 0) {
        const float4 *xi4 = reinterpret_cast<const float4 *>(a.xp + (a.row0 + i) * H);
        const float4 *xj4 = reinterpret_cast<const float4 *>(a.xp + (int64_t)j * H);
        float d2 = 0.0f;
        constexpr int CH = H / 4 < 16 ? H / 4 : 16;      // float4s in flight per lane
#pragma unroll
        for (int c0 = 0; c0 < H / 4; c0 += CH) {
            float4 v[CH];
#pragma unroll
            for (int u = 0; u < CH; u++) v[u] = xj4[c0 + u];
#pragma unroll
            for (int u = 0; u < CH; u++) {
                const float4 b = xi4[c0 + u];
                float df = __fadd_rn(b.x, -v[u].x);
                d2 = __fmaf_rn(df, df, d2);
                df = __fadd_rn(b.y, -v[u].y);
                d2 = __fmaf_rn(df, df, d2);
                df = __fadd_rn(b.z, -v[u].z);
                d2 = __fmaf_rn(df, df, d2);
                df = __fadd_rn(b.w, -v[u].w);
                d2 = __fmaf_rn(df, df, d2);
            }
        }
        const float dist = c_sqrt(d2);
        float g = 0.0f;
        if (a.noise_mode >= 2) g = pair_noise(a.s0, a.s1, (uint32_t)(a.row0 + i), (uint32_t)j, sym);
        return make_key(score_from_dist(dist, a.t, a.noise_mode != 0, g), j);
    } else {
        float v = a.p_edge[e];
        if (a.noise_mode != 0) v = perturb_p(v, pair_noise(a.s0, a.s1, (uint32_t)(a.row0 + i), (uint32_t)j, sym));
        return make_key(v, (int32_t)(e - e0));
    }
}

// the lists of one row of this pass -> its chunks [c0 + m0, c0 + m0 + depth): idx / val (/ ex_out / eid), the ramp, and in the row's
// last pass rs = the lane-wise sums over ALL of its chunks in chunk order (the earlier passes' weights are read back), then the butterfly
template <int H>
__device__ __forceinline__ void write_row(const Args &a, const uint64_t (&list)[MR], int64_t i, int64_t e0, int c0, int Mi, int m0, int depth,
                                          int L, float ki, int lane) {
    float rsum = 0.0f;
    for (int mg = 0; mg < m0 && (int64_t)c0 + mg < a.ccap; mg++) {
        const float wv = a.w[((int64_t)c0 + mg) * 64 + lane];
        rsum = mg == 0 ? wv : __fadd_rn(rsum, wv);
    }
    for (int m = 0; m < depth && (int64_t)c0 + m0 + m < a.ccap; m++) {          // (wave-uniform)
        uint64_t key = list[0];
#pragma unroll
        for (int q = 1; q < MR; q++)
            if (q == m) key = list[q];
        const int mg = m0 + m, rk = 64 * mg + lane;
        const bool empty = key == DGG_EMPTY_KEY || rk >= L;
        const int64_t s = ((int64_t)c0 + mg) * 64 + lane;
        const float sv = empty ? 0.0f : key_val(key);
        if constexpr (H > 0) {
            a.idx[s] = empty ? -1 : key_col(key);
        } else {
            const int64_t e = e0 + (empty ? 0 : key_col(key));                   // (an empty slot reads nothing)
            a.idx[s] = empty ? -1 : a.col[e];
            if (a.ex_out) a.ex_out[s] = empty ? 0.0f : a.ex_edge[e];            // (ex_out is there with ex_edge only)
            if (a.eid) a.eid[s] = empty ? -1 : (int32_t)e;
        }
        a.val[s] = sv;
        const float wv = empty ? 0.0f : ramp_weight(rk, ki, sv, a.mode);
        a.w[s] = wv;
        rsum = mg == 0 ? wv : __fadd_rn(rsum, wv);
    }
    if (m0 + depth == Mi) {
        const float s_ = wave_sum_butterfly(rsum);
        if (lane == 0) a.rs[i] = s_;
    }
}

template <int H>
__global__ __launch_bounds__(WAVES * 64) void edgelist_topk_chunked_kernel(const Args a) {
    const int lane = threadIdx.x & 63, wave = dgg::wave_id();
    if (blockIdx.x >= a.nrow_blocks) {
        const int64_t q = (int64_t)a.cptr[a.rows] + (int64_t)(blockIdx.x - a.nrow_blocks) * WAVES + wave;
        if (q < a.ccap) {
            a.idx[q * 64 + lane] = -1;
            a.val[q * 64 + lane] = 0.0f;
            a.w[q * 64 + lane] = 0.0f;
            if constexpr (H == 0) {
                if (a.ex_out) a.ex_out[q * 64 + lane] = 0.0f;
                if (a.eid) a.eid[q * 64 + lane] = -1;
            }
        }
        return;
    }
    const int64_t i = (int64_t)blockIdx.x * WAVES + wave;         // the row inside the range (everything below is wave-uniform)
    if (i >= a.rows) return;
    const int m0 = a.pass * MR;
    const int c0 = __builtin_amdgcn_readfirstlane(a.cptr[i]);
    const int Mi = __builtin_amdgcn_readfirstlane(a.cptr[i + 1]) - c0;
    if (Mi <= 0) {                                                // (a fixed capacity ran out before this row: it owns no chunk)
        if (a.pass == 0 && lane == 0) a.rs[i] = 0.0f;
        return;
    }
    if (Mi <= m0) return;                                         // settled by an earlier pass
    const int depth = Mi - m0 < MR ? Mi - m0 : MR;
    const float ki = a.k[i];
    const int L = __builtin_amdgcn_readfirstlane(klimit_len(ki, 64 * Mi));
    const int64_t e0 = a.rowptr[i], e1 = a.rowptr[i + 1];

    uint64_t ceil_key = ~0ull, thr = DGG_EMPTY_KEY, list[MR];
#pragma unroll
    for (int m = 0; m < MR; m++) list[m] = DGG_EMPTY_KEY;
    if (a.pass > 0) {                                             // the last key the previous pass settled; none there: the candidates ran out
        const int64_t s = ((int64_t)c0 + m0 - 1) * 64 + 63;
        const int32_t cj = (int64_t)c0 + m0 <= a.ccap ? a.idx[s] : -1;
        ceil_key = DGG_EMPTY_KEY;
        if (cj >= 0) {
            if constexpr (H > 0) {
                ceil_key = make_key(a.val[s], cj);
            } else {                                              // its place in the row: the one candidate with that column
                for (int64_t eb = e0; eb < e1; eb += 64) {
                    const int64_t e = eb + lane;
                    const unsigned long long hit = __ballot(e < e1 && a.col[e] == cj);
                    if (hit != 0ull) {
                        ceil_key = make_key(a.val[s], (int32_t)(eb - e0) + __ffsll(hit) - 1);
                        break;
                    }
                }
            }
        }
    }

    for (int64_t eb = e0; eb < e1; eb += 64) {
        const int64_t e = eb + lane;
        const uint64_t key = e < e1 ? cand_key<H>(a, i, e0, e) : DGG_EMPTY_KEY;
        const bool pass = key > thr && key < ceil_key;
        if (__ballot(pass) == 0ull) continue;                     // wave-uniform
        uint64_t carry = wave_sort_desc(pass ? key : DGG_EMPTY_KEY, lane);
        bool more = true;                                         // (wave-uniform: false once nothing is left to place)
#pragma unroll
        for (int m = 0; m < MR; m++) {
            if (more && m < depth) {
                const uint64_t cmax = readlane_u64(carry, 0);
                more = cmax != DGG_EMPTY_KEY;
                if (cmax > readlane_u64(list[m], 63)) {           // (else: list m keeps all of its entries, the carry goes on whole)
                    const uint64_t rc = shfl_u64(carry, 63 - lane);          // ascending
                    const uint64_t hi = list[m] > rc ? list[m] : rc, lo = list[m] > rc ? rc : list[m];
                    list[m] = bitonic_block<64, 32, true>(hi, lane);
                    carry = bitonic_block<64, 32, true>(lo, lane);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < MR; m++)
            if (m == depth - 1) thr = readlane_u64(list[m], 63);
    }
    write_row<H>(a, list, i, e0, c0, Mi, m0, depth, L, ki, lane);
}

template <int H>
void launch_passes(Args a, int maxm, hipStream_t st) {
    a.nrow_blocks = (unsigned)((a.rows + WAVES - 1) / WAVES);
    const int64_t tail = a.ccap > a.rows ? a.ccap - a.rows : 0;   // (every row has at least one chunk, or the capacity is used up)
    for (int p = 0; p * MR < maxm; p++) {
        a.pass = p;
        const unsigned grid = a.nrow_blocks + (p == 0 ? (unsigned)((tail + WAVES - 1) / WAVES) : 0u);
        hipLaunchKernelGGL(edgelist_topk_chunked_kernel<H>, dim3(grid), dim3(WAVES * 64), 0, st, a);
    }
}

int fail(int code, const char *fmt, ...) {
    char msg[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    return dgg_set_error(code, msg);
}

// the checks of the two entry points, in the order of dgg_allpairs_mlp_sweep.h's validate.  h: the latent width, 0 for given
// probabilities; ins_ok: the entry's own pointers are there.  -> run = false with DGG_OK: no rows, nothing to launch
int validate(const char *n, const Args &a, int64_t N, int h, int64_t row1, int maxm, bool ins_ok, bool *run) {
    *run = false;
    if (h != 0 && ((h != 16 && h != 32 && h != 64 && h != 128) || (reinterpret_cast<uintptr_t>(a.xp) & 15) != 0))
        return fail(DGG_ERR_UNSUPPORTED, "%s: latent_dim must be 16, 32, 64 or 128 (16-byte aligned rows)", n);
    if (a.noise_mode != 0 && a.noise_mode != 2 && a.noise_mode != 3)
        return fail(DGG_ERR_UNSUPPORTED, "%s: noise_mode must be none / hash / symmetric hash (an explicit noise tensor is outside the "
                                         "fused layer; the ranked generators score every candidate under the per-pair hash)", n);
    if (a.mode != 0 && a.mode != 1 && a.mode != 3)
        return fail(DGG_ERR_ARG, "%s: mode must be 0 (k_times_edge_prob), 1 (k_only) or 3 (straight-through forward)", n);
    if (a.row0 < 0 || row1 < a.row0 || row1 > N || N >= ((int64_t)1 << 31))
        return fail(DGG_ERR_ARG, "%s: rows must satisfy 0 <= row0 <= row1 <= N < 2^31", n);
    if (maxm < 1 || maxm > DGG_CHUNK_MAXM_ANY || a.ccap < 0 || a.ccap >= ((int64_t)1 << 25))
        return fail(DGG_ERR_ARG, "%s: maxm in 1..2^20, 0 <= ccap < 2^25 chunks", n);
    if (a.row0 == row1) return DGG_OK;
    if (!ins_ok || !a.rowptr || !a.col || !a.k || !a.cptr || !a.idx || !a.val || !a.w || !a.rs)
        return fail(DGG_ERR_ARG, "%s: missing inputs / layout / outputs", n);
    *run = true;
    return DGG_OK;
}

}  // namespace

extern "C" int dgg_edgelist_topk_chunked(const float *xp, int64_t N, int h, int64_t row0, int64_t row1, const int64_t *rowptr,
                                         const int32_t *col, float t, int noise_mode, uint32_t s0, uint32_t s1, const float *k, int mode,
                                         int maxm, const int32_t *cptr, int64_t ccap, int32_t *idx, float *val, float *w, float *rs,
                                         void *stream) {
    const Args a = {xp, nullptr, nullptr, row0, row1 - row0, rowptr, col, t, noise_mode, s0, s1, k, mode, cptr, ccap, idx, val, nullptr, nullptr,
                    w, rs, 0, 0u};
    bool go;
    if (const int rc = validate("edgelist_topk_chunked", a, N, h ? h : -1, row1, maxm, xp != nullptr, &go); rc != DGG_OK || !go) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (h == 16) launch_passes<16>(a, maxm, st);
    else if (h == 32) launch_passes<32>(a, maxm, st);
    else if (h == 64) launch_passes<64>(a, maxm, st);
    else launch_passes<128>(a, maxm, st);
    return dgg_check_launch("edgelist_topk_chunked");
}

extern "C" int dgg_edgelist_topk_p_chunked(const float *p_edge, int64_t N, int64_t row0, int64_t row1, const int64_t *rowptr,
                                           const int32_t *col, int noise_mode, uint32_t s0, uint32_t s1, const float *k, int mode, int maxm,
                                           const int32_t *cptr, int64_t ccap, const float *ex_edge, int32_t *idx, float *val, float *ex_out,
                                           int32_t *eid, float *w, float *rs, void *stream) {
    const Args a = {nullptr, p_edge, ex_edge, row0, row1 - row0, rowptr, col, 0.0f, noise_mode, s0, s1, k, mode, cptr, ccap, idx, val,
                    ex_edge ? ex_out : nullptr, eid, w, rs, 0, 0u};
    bool go;
    if (const int rc = validate("edgelist_topk_p_chunked", a, N, 0, row1, maxm, p_edge != nullptr && !(ex_edge && !ex_out), &go);
        rc != DGG_OK || !go)
        return rc;
    launch_passes<0>(a, maxm, (hipStream_t)stream);
    return dgg_check_launch("edgelist_topk_p_chunked");
}
