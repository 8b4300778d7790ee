// dgg_allpairs_mlp_wide.hip -- dgg_allpairs_mlp_topk (dgg_allpairs_mlp.hip) for rows of ANY width: the edge-MLP scorers u-v-deg /
// u-v-deg-dist / edge_conv (reference dgm.py:1645-1719) on ALL-PAIRS candidates, perturbation (dgm.py:1211-1229) and torch.sort
// (dgm.py:1404) kept to the L_i = ceil(k_i + 8.5) + 1 best columns of row i -- the support of the ramp of select_top_k over the dense row
// with an unbounded learned degree (dgm.py:1402-1421, 1580-1584) -- written into CHUNKED rows (dgg_chunk_layout) with the ramp fused.
//
// Structure of the list kernel: a workgroup owns a block of rows whose A_u (and xp_u) sit in LDS, 64-column tiles of B_v (and xp_v)
// stream through LDS, one key per lane, the score chain is the shared one of dgg_edgemlp_score.h (same bits).  A row keeps MR descending
// 64-lane lists in registers instead of one (list 0: ranks 0..63, list 1: ranks 64..127, ...): a tile's passing keys are sorted once and
// cascaded down the lists as in allpairs_topk_ranked_wide (one bitonic half-cleaner per list: the upper 64 stay, the lower 64 carry on; a
// list whose last key beats the carry's first is skipped) to the row's depth min(M_i, MR); the row's threshold is the last key of its
// deepest list.
//
// Rows of more than MR chunks are finished by CONTINUATION passes of the same kernel: pass p settles the chunks [MR p, MR (p + 1)) of the
// rows that have them and admits only keys strictly below the row's ceiling = the key at rank 64 MR p - 1, which pass p - 1 wrote to
// idx / val (the key order -- score descending, lower column first -- is total, so "strictly below" is exact among tied scores too).
// A later pass scores every pair of its open rows again: exact, because the score chain is the same, at the cost of one sweep per pass for
// the rows still open (a workgroup whose rows are all settled returns before its first barrier; a wavefront whose rows are settled stages
// tiles and keeps the barriers, but scores nothing).  The host launches ceil(maxm / MR) passes from the integer maxm: no device read-back.
//
// dgg_allpairs_mlp_topk_wide_prior: the same for u-v-A_uv (dgm.py:1628-1644) against a sparse PRIOR graph, as dgg_allpairs_mlp_topk_prior
// does it on the list (dgg_prior_lookup.h: one cursor per row and wavefront, a 64-float strip of LDS per wavefront).  Every pass opens
// the cursors of its open rows at the start of their CSR segments, so a continuation pass walks the prior again with the columns.
#include "dgg_common.h"
#include "dgg_edgemlp_score.h"
#include "dgg_prior_lookup.h"
#include "dgg_api_internal.h"

using namespace dgg;

namespace {

constexpr int WAVES = 4;          // wavefronts per workgroup
constexpr int TN = 64;            // columns per tile (one per lane)
constexpr int OB = 8;             // hidden units per pass over a wavefront's rows
constexpr int RW = 2;             // rows per wavefront
constexpr int MR = 8;             // 64-lane register lists per row = chunks a pass settles (ops.APMLP_WIDE_REG_CHUNKS repeats it)

struct Args {
    const float *AB, *xp;
    int64_t N;
    int h;
    int64_t row0, row1;
    const float *deg;
    int ex_mode;
    float t_ex;
    const float *wdu, *wdv, *wex, *b1, *w2, *b2;
    int act, noise_mode;
    const float *G;
    int64_t ldG;
    uint32_t s0, s1;
    const float *k;
    int mode;
    const int32_t *cptr;
    int64_t ccap;
    int32_t *idx;
    float *val, *ex_out, *w, *rs;
    int pass;                     // chunks [MR pass, MR (pass + 1)) of every row
    unsigned nrow_blocks;         // workgroups beyond these (pass 0) write the spare chunks [cptr[rows], ccap) empty
};

// the lists of one row of this pass -> its chunks [c0 + m0, c0 + m0 + depth): idx / val / ex_out, the ramp, and in the row's last pass
// rs = the lane-wise sums over ALL of its chunks in chunk order (the earlier passes' weights are read back), then the butterfly
// PRIOR: ex_out = the prior's stored value of (i, column) (binary search in the row's segment of prp / pci / pv)
template <bool PRIOR>
__device__ __forceinline__ void write_row(const Args &a, const uint64_t (&list)[MR], int64_t i, int c0, int Mi, int m0, int depth, int L, float ki,
                                          bool has_ex, int lane, const PriorCsr &P) {
    float rsum = 0.0f;
    if (a.w) {
        for (int mg = 0; mg < m0 && (int64_t)c0 + mg < a.ccap; mg++) {
            const float wv = a.w[((int64_t)c0 + mg) * 64 + lane];
            rsum = mg == 0 ? wv : __fadd_rn(rsum, wv);
        }
    }
    for (int m = 0; m < depth && (int64_t)c0 + m0 + m < a.ccap; m++) {          // (wave-uniform)
        uint64_t key = list[0];
#pragma unroll
        for (int q = 1; q < MR; q++)
            if (q == m) key = list[q];
        const int mg = m0 + m, rk = 64 * mg + lane;
        const bool empty = key == DGG_EMPTY_KEY || rk >= L;
        const int32_t c = key_col(key);
        const int64_t e = ((int64_t)c0 + mg) * 64 + lane;
        const float sv = empty ? 0.0f : key_val(key);
        a.idx[e] = empty ? -1 : c;
        a.val[e] = sv;
        if constexpr (PRIOR) {
            if (a.ex_out) a.ex_out[e] = empty ? 0.0f : prior_value_at(P, i, c);
        } else {
            if (a.ex_out) a.ex_out[e] = (has_ex && !empty) ? edge_mlp_dist_extra(a.xp + i * a.h, a.xp + (int64_t)c * a.h, a.h, a.t_ex) : 0.0f;
        }
        if (a.w) {
            const float wv = empty ? 0.0f : ramp_weight(rk, ki, sv, a.mode);
            a.w[e] = wv;
            rsum = mg == 0 ? wv : __fadd_rn(rsum, wv);
        }
    }
    if (a.w && m0 + depth == Mi) {
        const float s_ = wave_sum_butterfly(rsum);
        if (lane == 0) a.rs[i - a.row0] = s_;
    }
}

// VAR as in dgg_allpairs_mlp.hip -- 0: u-v-deg, 1: u-v-deg-dist, 2: edge_conv, 3: whatever the arguments say.  LDS (dynamic) as there:
// rowsA [RB][HW] | rowsX [RB][h] (extra only) | tile (xp_v rows of h + 1 floats, then B_v transposed [HW][TN]).
// VAR 4 / 5 (dgg_allpairs_mlp_topk_wide_prior): the extra is the prior's stored value of the pair -- 4: LeakyReLU, no degree term
// (u-v-A_uv); 5: whatever degree term / activation the arguments say.  LDS: rowsA | tile (B_v transposed) | strips [WAVES][64].  Every
// pass opens its rows' cursors at the start of their segments: a continuation pass sweeps the columns, and the prior, again.  The CSR
// arrays are the trailing arguments PR = (rowptr, col, val); the pack is empty for VAR 0..3, whose kernels are what they were.
template <int HW, int VAR, class... PR>
__global__ __launch_bounds__(WAVES * 64) void allpairs_mlp_topk_wide_kernel(const Args a, PR... pr) {
    constexpr int RB = RW * WAVES;
    constexpr bool PRIOR = VAR >= 4;
    static_assert(sizeof...(PR) == (PRIOR ? 3 : 0), "the prior variants, and only they, take the prior's CSR arrays");
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = dgg::wave_id();
    const int64_t rows = a.row1 - a.row0;
    if (blockIdx.x >= a.nrow_blocks) {
        const int64_t q = (int64_t)a.cptr[rows] + (int64_t)(blockIdx.x - a.nrow_blocks) * WAVES + wave;
        if (q < a.ccap) {
            a.idx[q * 64 + lane] = -1;
            a.val[q * 64 + lane] = 0.0f;
            if (a.ex_out) a.ex_out[q * 64 + lane] = 0.0f;
            if (a.w) a.w[q * 64 + lane] = 0.0f;
        }
        return;
    }
    const bool has_deg = (VAR == 3 || VAR == 5) ? a.deg != nullptr : (VAR != 2 && VAR != 4);
    const bool has_ex = VAR == 3 ? a.ex_mode == 2 : VAR == 1;     // the distance extra
    const bool any_ex = has_ex || PRIOR;
    const int act = (VAR == 3 || VAR == 5) ? a.act : (VAR == 2 ? 0 : 1);
    const int h = a.h, hx = h + 1;
    const int64_t N = a.N;
    float *rowsA = lds;
    float *rowsX = rowsA + RB * HW;
    float *tile = rowsX + (has_ex ? RB * h : 0);
    const int64_t rbase = a.row0 + (int64_t)blockIdx.x * RB;
    const int m0 = a.pass * MR;

    // this wavefront's rows (everything here is wave-uniform): first chunk, chunks in all, lists of this pass, rank limit, ceiling
    int c0[RW], Mi[RW], depth[RW], L[RW];
    float ki[RW], du[RW];
    uint64_t ceil_key[RW], thr[RW], list[RW][MR];
    bool wave_open = false;
#pragma unroll
    for (int r = 0; r < RW; r++) {
        const int64_t gi = rbase + wave * RW + r, lrow = gi - a.row0;
        c0[r] = 0; Mi[r] = 0; depth[r] = 0; L[r] = 0; ki[r] = 0.0f; du[r] = 0.0f;
        ceil_key[r] = ~0ull;
        thr[r] = DGG_EMPTY_KEY;
#pragma unroll
        for (int m = 0; m < MR; m++) list[r][m] = DGG_EMPTY_KEY;
        if (gi >= a.row1) continue;
        c0[r] = __builtin_amdgcn_readfirstlane(a.cptr[lrow]);
        Mi[r] = __builtin_amdgcn_readfirstlane(a.cptr[lrow + 1]) - c0[r];
        if (Mi[r] <= 0) {                                       // (a fixed capacity ran out before this row: it owns no chunk)
            if (a.pass == 0 && a.w && lane == 0) a.rs[lrow] = 0.0f;
            continue;
        }
        ki[r] = a.k[lrow];
        L[r] = __builtin_amdgcn_readfirstlane(klimit_len(ki[r], 64 * Mi[r]));
        if (Mi[r] <= m0) continue;                              // settled by an earlier pass
        depth[r] = Mi[r] - m0 < MR ? Mi[r] - m0 : MR;
        du[r] = has_deg ? a.deg[gi] : 0.0f;
        wave_open = true;
        if (a.pass > 0) {                                       // the last key the previous pass settled; none there: the columns ran out
            const int64_t e = ((int64_t)c0[r] + m0 - 1) * 64 + 63;
            const int32_t cj = (int64_t)c0[r] + m0 <= a.ccap ? a.idx[e] : -1;
            ceil_key[r] = cj < 0 ? DGG_EMPTY_KEY : make_key(a.val[e], cj);
        }
    }
    bool open = false;                                          // any row of the WORKGROUP (uniform over it: no barrier before the return)
    for (int q = 0; q < RB; q++) {
        const int64_t lrow = rbase + q - a.row0;
        if (lrow < rows && a.cptr[lrow + 1] - a.cptr[lrow] > m0) open = true;
    }
    if (!open) return;
    const PriorCsr P = prior_csr(pr...);
    float *strip = tile + HW * TN + wave * 64;                  // (PRIOR only) this wavefront's 64 floats of prior_tile_extra
    PriorCursor pc[PRIOR ? RW : 1];
    if constexpr (PRIOR) {
#pragma unroll
        for (int r = 0; r < RW; r++) pc[r] = prior_cursor_open(P, rbase + wave * RW + r, depth[r] > 0);
        strip[lane] = 0.0f;
        DGG_PRIOR_WAVE_FENCE();
    }

    for (int e = tid; e < RB * HW; e += WAVES * 64) {
        const int r = e / HW, c = e % HW;
        const int64_t gi = rbase + r;
        rowsA[e] = gi < a.row1 ? a.AB[gi * 2 * HW + c] : 0.0f;
    }
    if (has_ex) {
        for (int e = tid; e < RB * h; e += WAVES * 64) {
            const int r = e / h, c = e % h;
            const int64_t gi = rbase + r;
            rowsX[e] = gi < a.row1 ? a.xp[gi * h + c] : 0.0f;
        }
    }
    const bool sym = a.noise_mode == 3;
    const float b2v = a.b2[0];

    for (int64_t j0 = 0; j0 < N; j0 += TN) {
        const int64_t j = j0 + lane;
        const bool jvalid = j < N;
        float ex[RW];
#pragma unroll
        for (int r = 0; r < RW; r++) ex[r] = 0.0f;
        __syncthreads();                                        // (the previous tile has been read; the first: the rows are staged)
        if (has_ex) {
            for (int e = tid; e < TN * h; e += WAVES * 64) {
                const int jj = e / h, c = e % h;
                const int64_t gj = j0 + jj;
                tile[jj * hx + c] = gj < N ? a.xp[gj * h + c] : 0.0f;
            }
            __syncthreads();
            if (wave_open) {
#pragma unroll
                for (int r = 0; r < RW; r++) ex[r] = edge_mlp_dist_extra(rowsX + (wave * RW + r) * h, tile + lane * hx, h, a.t_ex);
            }
            __syncthreads();
        }
        for (int e = tid; e < TN * (HW / 4); e += WAVES * 64) {
            const int jj = e % TN, c4 = (e / TN) * 4;
            const int64_t gj = j0 + jj;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (gj < N) v = *reinterpret_cast<const float4 *>(a.AB + gj * 2 * HW + HW + c4);
            tile[(c4 + 0) * TN + jj] = v.x; tile[(c4 + 1) * TN + jj] = v.y;
            tile[(c4 + 2) * TN + jj] = v.z; tile[(c4 + 3) * TN + jj] = v.w;
        }
        const float dv = (has_deg && jvalid) ? a.deg[j] : 0.0f;
        if constexpr (PRIOR) {
#pragma unroll
            for (int r = 0; r < RW; r++) ex[r] = prior_tile_extra(pc[r], P, j0, strip, lane);
        }
        __syncthreads();
        if (!wave_open) continue;                               // (wave-uniform; the barriers above are the loop's only ones)

        float s[RW];
#pragma unroll
        for (int r = 0; r < RW; r++) s[r] = 0.0f;
#pragma unroll 2
        for (int o0 = 0; o0 < HW; o0 += OB) {
            float b[OB], p_du[OB], p_dv[OB], p_ex[OB], p_b1[OB], p_w2[OB];
#pragma unroll
            for (int q = 0; q < OB; q++) {
                b[q] = tile[(o0 + q) * TN + lane];
                p_du[q] = has_deg ? a.wdu[o0 + q] : 0.0f;        // (wave-uniform)
                p_dv[q] = has_deg ? a.wdv[o0 + q] : 0.0f;
                p_ex[q] = any_ex ? a.wex[o0 + q] : 0.0f;
                p_b1[q] = a.b1[o0 + q];
                p_w2[q] = a.w2[o0 + q];
            }
#pragma unroll
            for (int r = 0; r < RW; r++) {
                const float *ar = rowsA + (wave * RW + r) * HW + o0;  // wave-uniform address: LDS broadcast
#pragma unroll
                for (int q = 0; q < OB; q++)
                    s[r] = edge_mlp_unit(ar[q], b[q], q, has_deg, du[r], dv, p_du, p_dv, any_ex, ex[r], p_ex, p_b1, p_w2, act, s[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RW; r++) {
            if (depth[r] == 0) continue;                        // wave-uniform
            const int64_t i = rbase + wave * RW + r;
            float v = edge_mlp_prob(s[r], b2v);
            if (a.noise_mode != 0) {
                float g = 0.0f;
                if (a.noise_mode == 1) g = jvalid ? a.G[i * a.ldG + j] : 0.0f;
                else g = pair_noise(a.s0, a.s1, (uint32_t)i, (uint32_t)j, sym);
                v = perturb_p(v, g);
            }
            const uint64_t key = jvalid ? make_key(v, (int32_t)j) : DGG_EMPTY_KEY;
            const bool pass = key > thr[r] && key < ceil_key[r];
            if (__ballot(pass) != 0ull) {                       // wave-uniform
                uint64_t carry = wave_sort_desc(pass ? key : DGG_EMPTY_KEY, lane);
                bool more = true;                                // (wave-uniform: false once nothing is left to place)
#pragma unroll
                for (int m = 0; m < MR; m++) {
                    if (more && m < depth[r]) {
                        const uint64_t cmax = readlane_u64(carry, 0);
                        more = cmax != DGG_EMPTY_KEY;
                        if (cmax > readlane_u64(list[r][m], 63)) {   // (else: list m keeps all of its entries, the carry goes on whole)
                            const uint64_t rc = shfl_u64(carry, 63 - lane);          // ascending
                            const uint64_t hi = list[r][m] > rc ? list[r][m] : rc, lo = list[r][m] > rc ? rc : list[r][m];
                            list[r][m] = bitonic_block<64, 32, true>(hi, lane);
                            carry = bitonic_block<64, 32, true>(lo, lane);
                        }
                    }
                }
#pragma unroll
                for (int m = 0; m < MR; m++)
                    if (m == depth[r] - 1) thr[r] = readlane_u64(list[r][m], 63);
            }
        }
    }

#pragma unroll
    for (int r = 0; r < RW; r++)
        if (depth[r] > 0) write_row<PRIOR>(a, list[r], rbase + wave * RW + r, c0[r], Mi[r], m0, depth[r], L[r], ki[r], has_ex, lane, P);
}

size_t lds_bytes(int hw, int h, bool has_ex) {
    const size_t rb = (size_t)RW * WAVES;
    size_t tile = (size_t)hw * TN;
    if (has_ex && (size_t)TN * (h + 1) > tile) tile = (size_t)TN * (h + 1);
    return (rb * hw + (has_ex ? rb * h : 0) + tile) * sizeof(float);
}

size_t lds_bytes_prior(int hw) { return ((size_t)RW * WAVES * hw + (size_t)hw * TN + (size_t)WAVES * 64) * sizeof(float); }

struct Prior {                    // the prior's CSR arrays (dgg_allpairs_mlp_topk_wide_prior; NULL otherwise)
    const int64_t *prp;
    const int32_t *pci;
    const float *pv;
};

template <int HW, int VAR>
void launch_passes(Args a, int maxm, hipStream_t st, const Prior &pr = Prior{nullptr, nullptr, nullptr}) {
    constexpr int RB = RW * WAVES;
    const int64_t rows = a.row1 - a.row0;
    a.nrow_blocks = (unsigned)((rows + RB - 1) / RB);
    const int64_t tail = a.ccap > rows ? a.ccap - rows : 0;     // (every row has at least one chunk, or the capacity is used up)
    const size_t lds = VAR >= 4 ? lds_bytes_prior(HW) : lds_bytes(HW, a.h, a.ex_mode == 2);
    for (int p = 0; p * MR < maxm; p++) {
        a.pass = p;
        const unsigned grid = a.nrow_blocks + (p == 0 ? (unsigned)((tail + WAVES - 1) / WAVES) : 0u);
        if constexpr (VAR >= 4)
            hipLaunchKernelGGL((allpairs_mlp_topk_wide_kernel<HW, VAR, const int64_t *, const int32_t *, const float *>), dim3(grid), dim3(WAVES * 64), lds, st, a, pr.prp, pr.pci, pr.pv);
        else
            hipLaunchKernelGGL((allpairs_mlp_topk_wide_kernel<HW, VAR>), dim3(grid), dim3(WAVES * 64), lds, st, a);
    }
}

template <int HW>
void launch_var(const Args &a, int maxm, hipStream_t st) {
    const bool leaky = a.act == 1;
    if (a.deg && leaky && a.ex_mode == 0) launch_passes<HW, 0>(a, maxm, st);
    else if (a.deg && leaky && a.ex_mode == 2) launch_passes<HW, 1>(a, maxm, st);
    else if (!a.deg && !leaky && a.ex_mode == 0) launch_passes<HW, 2>(a, maxm, st);
    else launch_passes<HW, 3>(a, maxm, st);
}

template <int HW>
void launch_var_prior(const Args &a, int maxm, hipStream_t st, const Prior &pr) {
    if (!a.deg && a.act == 1) launch_passes<HW, 4>(a, maxm, st, pr);
    else launch_passes<HW, 5>(a, maxm, st, pr);
}

bool width_ok(int w) { return w == 16 || w == 32 || w == 64 || w == 128; }

}  // namespace

extern "C" int dgg_allpairs_mlp_topk_wide(const float *AB, const float *xp, int64_t N, int h, int hw, int64_t row0, int64_t row1,
                                          const float *deg, int ex_mode, float t_ex, const float *wdu, const float *wdv, const float *wex,
                                          const float *b1, const float *w2, const float *b2, int act, int noise_mode, const float *G,
                                          int64_t ldG, uint32_t s0, uint32_t s1, const float *k, int mode, int maxm, const int32_t *cptr,
                                          int64_t ccap, int32_t *idx, float *val, float *ex_out, float *w, float *rs, void *stream) {
    if (!width_ok(hw) || !width_ok(h))
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk_wide: hidden width hw and latent_dim h must be 16, 32, 64 or 128");
    if (ex_mode == 1)
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk_wide: a per-edge extra array (u-v-A_uv, A_uv) does not exist for "
                                                  "all-pairs candidates; supported: u-v-deg, u-v-deg-dist, edge_conv");
    if (noise_mode == 4 || noise_mode == 5)
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk_wide: noise_mode must be none / explicit / hash / symmetric hash (every "
                                                  "pair is scored: the ranked generators have nothing to stop early)");
    if (ex_mode != 0 && ex_mode != 2) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide: ex_mode must be 0 (none) or 2 (exp(t dist))");
    if (noise_mode < 0 || noise_mode > 5) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide: unknown noise_mode");
    if (act != 0 && act != 1) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide: act must be 0 (identity) or 1 (LeakyReLU)");
    if (mode != 0 && mode != 1 && mode != 3)
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide: mode must be 0 (k_times_edge_prob), 1 (k_only) or 3 (straight-through forward)");
    if (noise_mode == 1 && (!G || ldG < N)) return dgg_set_error(DGG_ERR_ARG, "explicit noise requested but G is NULL (or ldG < N)");
    if (row0 < 0 || row1 < row0 || row1 > N || N >= ((int64_t)1 << 31))
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide: rows must satisfy 0 <= row0 <= row1 <= N < 2^31");
    if (maxm < 1 || maxm > DGG_CHUNK_MAXM_ANY || ccap < 0 || ccap >= ((int64_t)1 << 25))
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide: maxm in 1..2^20, 0 <= ccap < 2^25 chunks");
    if (row0 == row1) return 0;
    if (!AB || !b1 || !w2 || !b2 || !k || !cptr || !idx || !val || (w && !rs) || (ex_mode == 2 && (!xp || !wex)) || (deg && (!wdu || !wdv)))
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide: missing inputs / weights / layout for the requested mode");
    if ((reinterpret_cast<uintptr_t>(AB) & 15) != 0) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide: AB must be 16-byte aligned");
    const Args a{AB, xp, N, h, row0, row1, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, noise_mode, G, ldG, s0, s1, k, mode, cptr, ccap,
                 idx, val, ex_out, w, rs, 0, 0u};
    const hipStream_t st = (hipStream_t)stream;
    switch (hw) {
        case 16: launch_var<16>(a, maxm, st); break;
        case 32: launch_var<32>(a, maxm, st); break;
        case 64: launch_var<64>(a, maxm, st); break;
        default: launch_var<128>(a, maxm, st); break;
    }
    return dgg_check_launch("allpairs_mlp_topk_wide");
}

extern "C" int dgg_allpairs_mlp_topk_wide_prior(const float *AB, const float *xp, int64_t N, int h, int hw, int64_t row0, int64_t row1,
                                                const float *deg, int ex_mode, float t_ex, const float *wdu, const float *wdv,
                                                const float *wex, const float *b1, const float *w2, const float *b2, int act, int noise_mode,
                                                const float *G, int64_t ldG, uint32_t s0, uint32_t s1, const float *k, int mode, int maxm,
                                                const int32_t *cptr, int64_t ccap, int32_t *idx, float *val, float *ex_out, float *w, float *rs,
                                                const int64_t *prior_rowptr, const int32_t *prior_col, const float *prior_val, void *stream) {
    if (!width_ok(hw) || !width_ok(h))
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk_wide_prior: hidden width hw and latent_dim h must be 16, 32, 64 or 128");
    if (ex_mode != 1)
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk_wide_prior: ex_mode must be 1 (the extra of a pair is the prior's stored "
                                                  "value); ex_mode 0 / 2 are dgg_allpairs_mlp_topk_wide's");
    if (noise_mode == 4 || noise_mode == 5)
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk_wide_prior: noise_mode must be none / explicit / hash / symmetric hash "
                                                  "(every pair is scored: the ranked generators have nothing to stop early)");
    if (noise_mode < 0 || noise_mode > 5) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide_prior: unknown noise_mode");
    if (act != 0 && act != 1) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide_prior: act must be 0 (identity) or 1 (LeakyReLU)");
    if (mode != 0 && mode != 1 && mode != 3)
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide_prior: mode must be 0 (k_times_edge_prob), 1 (k_only) or 3 (straight-through forward)");
    if (noise_mode == 1 && (!G || ldG < N)) return dgg_set_error(DGG_ERR_ARG, "explicit noise requested but G is NULL (or ldG < N)");
    if (row0 < 0 || row1 < row0 || row1 > N || N >= ((int64_t)1 << 31))
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide_prior: rows must satisfy 0 <= row0 <= row1 <= N < 2^31");
    if (maxm < 1 || maxm > DGG_CHUNK_MAXM_ANY || ccap < 0 || ccap >= ((int64_t)1 << 25))
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide_prior: maxm in 1..2^20, 0 <= ccap < 2^25 chunks");
    if (!prior_rowptr || !prior_col || !prior_val)
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide_prior: the prior's CSR arrays (rowptr, col, val) must not be NULL");
    if (row0 == row1) return 0;
    if (!AB || !wex || !b1 || !w2 || !b2 || !k || !cptr || !idx || !val || (w && !rs) || (deg && (!wdu || !wdv)))
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide_prior: missing inputs / weights / layout for the requested mode");
    if ((reinterpret_cast<uintptr_t>(AB) & 15) != 0) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_wide_prior: AB must be 16-byte aligned");
    const Args a{AB, xp, N, h, row0, row1, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, noise_mode, G, ldG, s0, s1, k, mode, cptr, ccap,
                 idx, val, ex_out, w, rs, 0, 0u};
    const Prior pr{prior_rowptr, prior_col, prior_val};
    const hipStream_t st = (hipStream_t)stream;
    switch (hw) {
        case 16: launch_var_prior<16>(a, maxm, st, pr); break;
        case 32: launch_var_prior<32>(a, maxm, st, pr); break;
        case 64: launch_var_prior<64>(a, maxm, st, pr); break;
        default: launch_var_prior<128>(a, maxm, st, pr); break;
    }
    return dgg_check_launch("allpairs_mlp_topk_wide_prior");
}
