// dgg_allpairs_mlp_wide.hip -- dgg_allpairs_mlp_topk (dgg_allpairs_mlp.hip) for rows of ANY width: the edge-MLP scorers u-v-deg /
// u-v-deg-dist / edge_conv (reference dgm.py:1645-1719) on ALL-PAIRS candidates, perturbation (dgm.py:1211-1229) and torch.sort
// (dgm.py:1404) kept to the L_i = ceil(k_i + 8.5) + 1 best columns of row i -- the support of the ramp of select_top_k over the dense row
// with an unbounded learned degree (dgm.py:1402-1421, 1580-1584) -- written into CHUNKED rows (dgg_chunk_layout) with the ramp fused.
//
// The sweep of the list kernel, literally: dgg_allpairs_mlp_sweep.h holds what the two share (a workgroup owns a block of rows whose A_u
// (and xp_u) sit in LDS, 64-column tiles of B_v (and xp_v) stream through LDS, one key per lane, the score chain of dgg_edgemlp_score.h;
// the entry points' checks and dispatch); this file holds the passes, the ceiling, the cascade and write_row.  A row keeps MR descending
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
#include "dgg_allpairs_mlp_sweep.h"

using namespace dgg;
using namespace dgg::apmlp;

namespace {

constexpr int RW = 2;             // rows per wavefront
constexpr int MR = 8;             // 64-lane register lists per row = chunks a pass settles (ops.APMLP_WIDE_REG_CHUNKS repeats it)

struct Args {
    Scorer sc;
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
            if (a.ex_out) a.ex_out[e] = (has_ex && !empty) ? edge_mlp_dist_extra(a.sc.xp + i * a.sc.h, a.sc.xp + (int64_t)c * a.sc.h, a.sc.h, a.sc.t_ex) : 0.0f;
        }
        if (a.w) {
            const float wv = empty ? 0.0f : ramp_weight(rk, ki, sv, a.mode);
            a.w[e] = wv;
            rsum = mg == 0 ? wv : __fadd_rn(rsum, wv);
        }
    }
    if (a.w && m0 + depth == Mi) {
        const float s_ = wave_sum_butterfly(rsum);
        if (lane == 0) a.rs[i - a.sc.row0] = s_;
    }
}

// The sweep of dgg_allpairs_mlp_sweep.h (VAR, the LDS layout and the stages of a tile are documented there) into MR lists per row, one pass.
// Every pass opens its rows' prior cursors at the start of their segments: a continuation pass sweeps the columns, and the prior, again.
template <int HW, int VAR, class... PR>
__global__ __launch_bounds__(WAVES * 64) void allpairs_mlp_topk_wide_kernel(const Args a, PR... pr) {
    constexpr int RB = RW * WAVES;
    constexpr bool PRIOR = var_prior(VAR);
    static_assert(sizeof...(PR) == (PRIOR ? 3 : 0), "the prior variants, and only they, take the prior's CSR arrays");
    extern __shared__ float lds[];
    const Scorer &sc = a.sc;
    const int tid = threadIdx.x, lane = tid & 63, wave = dgg::wave_id();
    const int64_t rows = sc.row1 - sc.row0;
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
    const Switches sw = resolve<VAR>(sc);
    const Lds L = lds_layout<HW, RB>(lds, sc.h, sw.has_ex, wave);
    const int64_t rbase = sc.row0 + (int64_t)blockIdx.x * RB;
    const int m0 = a.pass * MR;

    // this wavefront's rows (everything here is wave-uniform): first chunk, chunks in all, lists of this pass, rank limit, ceiling
    int c0[RW], Mi[RW], depth[RW], Lk[RW];
    float ki[RW], du[RW];
    uint64_t ceil_key[RW], thr[RW], list[RW][MR];
    bool wave_open = false;
#pragma unroll
    for (int r = 0; r < RW; r++) {
        const int64_t gi = rbase + wave * RW + r, lrow = gi - sc.row0;
        c0[r] = 0; Mi[r] = 0; depth[r] = 0; Lk[r] = 0; ki[r] = 0.0f; du[r] = 0.0f;
        ceil_key[r] = ~0ull;
        thr[r] = DGG_EMPTY_KEY;
#pragma unroll
        for (int m = 0; m < MR; m++) list[r][m] = DGG_EMPTY_KEY;
        if (gi >= sc.row1) continue;
        c0[r] = __builtin_amdgcn_readfirstlane(a.cptr[lrow]);
        Mi[r] = __builtin_amdgcn_readfirstlane(a.cptr[lrow + 1]) - c0[r];
        if (Mi[r] <= 0) {                                       // (a fixed capacity ran out before this row: it owns no chunk)
            if (a.pass == 0 && a.w && lane == 0) a.rs[lrow] = 0.0f;
            continue;
        }
        ki[r] = a.k[lrow];
        Lk[r] = __builtin_amdgcn_readfirstlane(klimit_len(ki[r], 64 * Mi[r]));
        if (Mi[r] <= m0) continue;                              // settled by an earlier pass
        depth[r] = Mi[r] - m0 < MR ? Mi[r] - m0 : MR;
        du[r] = sw.has_deg ? sc.deg[gi] : 0.0f;
        wave_open = true;
        if (a.pass > 0) {                                       // the last key the previous pass settled; none there: the columns ran out
            const int64_t e = ((int64_t)c0[r] + m0 - 1) * 64 + 63;
            const int32_t cj = (int64_t)c0[r] + m0 <= a.ccap ? a.idx[e] : -1;
            ceil_key[r] = cj < 0 ? DGG_EMPTY_KEY : make_key(a.val[e], cj);
        }
    }
    bool open = false;                                          // any row of the WORKGROUP (uniform over it: no barrier before the return)
    for (int q = 0; q < RB; q++) {
        const int64_t lrow = rbase + q - sc.row0;
        if (lrow < rows && a.cptr[lrow + 1] - a.cptr[lrow] > m0) open = true;
    }
    if (!open) return;
    const PriorCsr P = prior_csr(pr...);
    PriorCursor pc[PRIOR ? RW : 1];
    if constexpr (PRIOR) {
#pragma unroll
        for (int r = 0; r < RW; r++) pc[r] = prior_cursor_open(P, rbase + wave * RW + r, depth[r] > 0);
        L.strip[lane] = 0.0f;
        DGG_PRIOR_WAVE_FENCE();
    }
    stage_rows<HW, RB>(sc, L, rbase, sw.has_ex, tid);
    const float b2v = sc.b2[0];

    for (int64_t j0 = 0; j0 < sc.N; j0 += TN) {
        const int64_t j = j0 + lane;
        float ex[RW];
#pragma unroll
        for (int r = 0; r < RW; r++) ex[r] = 0.0f;
        __syncthreads();                                        // (the previous tile has been read; the first: the rows are staged)
        if (sw.has_ex) dist_extra_tile<RW>(sc, L, j0, wave, lane, tid, wave_open, ex);      // (every wavefront: it holds barriers)
        stage_b_tile<HW>(sc, L, j0, tid);
        const float dv = (sw.has_deg && j < sc.N) ? sc.deg[j] : 0.0f;
        if constexpr (PRIOR) {
#pragma unroll
            for (int r = 0; r < RW; r++) ex[r] = prior_tile_extra(pc[r], P, j0, L.strip, lane);
        }
        __syncthreads();
        if (!wave_open) continue;                               // (wave-uniform; the barriers above are the loop's only ones)

        float s[RW];
        score_tile<HW, RW>(sc, sw, L, wave, lane, du, dv, ex, s);
#pragma unroll
        for (int r = 0; r < RW; r++) {
            if (depth[r] == 0) continue;                        // wave-uniform
            const uint64_t key = pair_key(sc, s[r], b2v, rbase + wave * RW + r, j);
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
        if (depth[r] > 0) write_row<PRIOR>(a, list[r], rbase + wave * RW + r, c0[r], Mi[r], m0, depth[r], Lk[r], ki[r], sw.has_ex, lane, P);
}

template <int HW, int VAR>
void launch_passes(Args a, int maxm, const Prior &pr, hipStream_t st) {
    constexpr int RB = RW * WAVES;
    const int64_t rows = a.sc.row1 - a.sc.row0;
    a.nrow_blocks = (unsigned)((rows + RB - 1) / RB);
    const int64_t tail = a.ccap > rows ? a.ccap - rows : 0;     // (every row has at least one chunk, or the capacity is used up)
    const size_t lds = lds_bytes(HW, RB, a.sc.h, a.sc.ex_mode == 2, var_prior(VAR));
    for (int p = 0; p * MR < maxm; p++) {
        a.pass = p;
        const unsigned grid = a.nrow_blocks + (p == 0 ? (unsigned)((tail + WAVES - 1) / WAVES) : 0u);
        if constexpr (var_prior(VAR))
            hipLaunchKernelGGL((allpairs_mlp_topk_wide_kernel<HW, VAR, const int64_t *, const int32_t *, const float *>), dim3(grid), dim3(WAVES * 64), lds, st, a, pr.rp, pr.ci, pr.v);
        else
            hipLaunchKernelGGL((allpairs_mlp_topk_wide_kernel<HW, VAR>), dim3(grid), dim3(WAVES * 64), lds, st, a);
    }
}

int run(const Entry &e, const Args &a, int hw, int maxm, const Prior &pr, void *stream) {
    bool go;
    const bool outs_ok = a.k && a.cptr && a.idx && a.val && !(a.w && !a.rs);
    if (const int rc = validate(e, a.sc, hw, 0, a.mode, maxm, a.ccap, outs_ok, pr, &go); rc != DGG_OK || !go) return rc;
    dispatch(hw, scorer_var(a.sc, e.prior), [&](auto HW, auto VAR) { launch_passes<HW(), VAR()>(a, maxm, pr, (hipStream_t)stream); });
    return dgg_check_launch(e.name);
}

}  // namespace

extern "C" int dgg_allpairs_mlp_topk_wide(const float *AB, const float *xp, int64_t N, int h, int hw, int64_t row0, int64_t row1,
                                          const float *deg, int ex_mode, float t_ex, const float *wdu, const float *wdv, const float *wex,
                                          const float *b1, const float *w2, const float *b2, int act, int noise_mode, const float *G,
                                          int64_t ldG, uint32_t s0, uint32_t s1, const float *k, int mode, int maxm, const int32_t *cptr,
                                          int64_t ccap, int32_t *idx, float *val, float *ex_out, float *w, float *rs, void *stream) {
    return run({"allpairs_mlp_topk_wide", true, false},
               {{AB, xp, N, h, row0, row1, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, noise_mode, G, ldG, s0, s1}, k, mode, cptr, ccap, idx, val,
                ex_out, w, rs, 0, 0u},
               hw, maxm, {nullptr, nullptr, nullptr}, stream);
}

extern "C" int dgg_allpairs_mlp_topk_wide_prior(const float *AB, const float *xp, int64_t N, int h, int hw, int64_t row0, int64_t row1,
                                                const float *deg, int ex_mode, float t_ex, const float *wdu, const float *wdv,
                                                const float *wex, const float *b1, const float *w2, const float *b2, int act, int noise_mode,
                                                const float *G, int64_t ldG, uint32_t s0, uint32_t s1, const float *k, int mode, int maxm,
                                                const int32_t *cptr, int64_t ccap, int32_t *idx, float *val, float *ex_out, float *w, float *rs,
                                                const int64_t *prior_rowptr, const int32_t *prior_col, const float *prior_val, void *stream) {
    return run({"allpairs_mlp_topk_wide_prior", true, true},
               {{AB, xp, N, h, row0, row1, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, noise_mode, G, ldG, s0, s1}, k, mode, cptr, ccap, idx, val,
                ex_out, w, rs, 0, 0u},
               hw, maxm, {prior_rowptr, prior_col, prior_val}, stream);
}
