// dgg_allpairs_mlp.hip -- the edge-MLP scorers u-v-deg / u-v-deg-dist / edge_conv (reference dgm.py:1645-1719) on ALL-PAIRS candidates:
// score + perturbation (dgm.py:1211-1229) + torch.sort kept to the K <= 64 best per row (dgm.py:1404) in one kernel.
//
// These three scorers are functions of the two end nodes and their prior degrees only, and their first layer splits into per-node
// products AB = xp [Wa | Wb]^T (dgg_edgemlp.hip), so a pair costs O(hw) vector work and nothing is gathered.  The structure is that of
// allpairs_topk_exhaustive (dgg_topk.hip): a workgroup owns a block of rows whose A_u (and xp_u) sit in LDS, column tiles of B_v (and
// xp_v) stream through LDS, every wavefront keeps the running top-64 of its rows in registers (one key per lane) and merges a tile only
// when one of its keys passes the row's threshold.  The N x N probabilities of the composed path (dgg_edge_mlp_fwd on the complete
// pattern + dgg_edgelist_topk_p) never exist; the result has the same bits: the score chain is the shared one of dgg_edgemlp_score.h.
//
// dgg_allpairs_mlp_topk_prior: the same sweep for u-v-A_uv (dgm.py:1628-1644) against a sparse PRIOR graph -- the extra of pair (i, j) is
// the prior's stored value, 0.0f where it stores nothing (the complete in_adj whose values are the prior's, zero for non-edges).  The
// tiles ascend and so do a row's CSR entries: a wavefront keeps one cursor per row and touches the prior only in tiles that hold an
// entry of the row (dgg_prior_lookup.h); ex_out of a kept entry comes from a binary search in the row's segment at write-out.
#include "dgg_common.h"
#include "dgg_edgemlp_score.h"
#include "dgg_prior_lookup.h"
#include "dgg_api_internal.h"

#include <cstdlib>
#include <cstring>

using namespace dgg;

namespace {

constexpr int WAVES = 4;          // wavefronts per workgroup
constexpr int TN = 64;            // columns per tile (one per lane)
constexpr int OB = 8;             // hidden units per pass over a wavefront's rows

// VAR: the scorer's switches as compile-time constants -- 0: degrees, LeakyReLU (u-v-deg); 1: degrees, LeakyReLU, exp(t dist) extra
// (u-v-deg-dist); 2: neither, no activation (edge_conv); 3: whatever the arguments say (any other combination)
//
// LDS (dynamic): rowsA [RB][HW] | rowsX [RB][h] (extra only) | tile.  The tile holds, one after the other, xp_v NOT transposed with
// rows of h + 1 floats (a lane walks its own row: bank = lane + c, conflict-free) and then B_v transposed [HW][TN] (lane-strided reads).
//
// VAR 4 / 5 (dgg_allpairs_mlp_topk_prior): the extra of a pair is the stored value of a sparse prior graph (dgg_prior_lookup.h), whose CSR
// arrays are the kernel's trailing arguments PR = (rowptr, col, val) -- the pack is empty for VAR 0..3, whose kernels take the same
// arguments and compile to the same code as without these variants.  4: LeakyReLU, no degree term (u-v-A_uv); 5: whatever degree term
// and activation the arguments say.  LDS: rowsA | tile (B_v transposed) | strips [WAVES][64].
template <int HW, int RW, int VAR, class... PR>
__global__ __launch_bounds__(WAVES * 64) void allpairs_mlp_topk_kernel(
    const float *__restrict__ AB, const float *__restrict__ xp, int64_t N, int h, int64_t row0, int64_t row1,
    const float *__restrict__ deg, int ex_mode, float t_ex, const float *__restrict__ wdu, const float *__restrict__ wdv,
    const float *__restrict__ wex, const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2, int act_rt,
    int noise_mode, const float *__restrict__ G, int64_t ldG, uint32_t s0, uint32_t s1, int K, int32_t *__restrict__ idx,
    float *__restrict__ val, float *__restrict__ ex_out, PR... pr) {
    constexpr int RB = RW * WAVES;
    constexpr bool PRIOR = VAR >= 4;
    static_assert(sizeof...(PR) == (PRIOR ? 3 : 0), "the prior variants, and only they, take the prior's CSR arrays");
    extern __shared__ float lds[];
    const bool has_deg = (VAR == 3 || VAR == 5) ? deg != nullptr : (VAR != 2 && VAR != 4);
    const bool has_ex = VAR == 3 ? ex_mode == 2 : VAR == 1;     // the distance extra
    const bool any_ex = has_ex || PRIOR;
    const int act = (VAR == 3 || VAR == 5) ? act_rt : (VAR == 2 ? 0 : 1);
    float *rowsA = lds;
    float *rowsX = rowsA + RB * HW;
    float *tile = rowsX + (has_ex ? RB * h : 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = dgg::wave_id();
    const int64_t rbase = row0 + (int64_t)blockIdx.x * RB;
    const int hx = h + 1;

    for (int e = tid; e < RB * HW; e += WAVES * 64) {
        const int r = e / HW, c = e % HW;
        const int64_t gi = rbase + r;
        rowsA[e] = gi < row1 ? AB[gi * 2 * HW + c] : 0.0f;
    }
    if (has_ex) {
        for (int e = tid; e < RB * h; e += WAVES * 64) {
            const int r = e / h, c = e % h;
            const int64_t gi = rbase + r;
            rowsX[e] = gi < row1 ? xp[gi * h + c] : 0.0f;
        }
    }
    float du[RW];
    uint64_t list[RW], thr[RW];
#pragma unroll
    for (int r = 0; r < RW; r++) {
        const int64_t gi = rbase + wave * RW + r;               // wave-uniform
        du[r] = (has_deg && gi < row1) ? deg[gi] : 0.0f;
        list[r] = DGG_EMPTY_KEY;
        thr[r] = DGG_EMPTY_KEY;
    }
    const PriorCsr P = prior_csr(pr...);
    float *strip = tile + HW * TN + wave * 64;                  // (PRIOR only) this wavefront's 64 floats of prior_tile_extra
    PriorCursor pc[PRIOR ? RW : 1];
    if constexpr (PRIOR) {
#pragma unroll
        for (int r = 0; r < RW; r++) {
            const int64_t gi = rbase + wave * RW + r;
            pc[r] = prior_cursor_open(P, gi, gi < row1);
        }
        strip[lane] = 0.0f;
        DGG_PRIOR_WAVE_FENCE();
    }
    const bool sym = noise_mode == 3;
    const float b2v = b2[0];

    for (int64_t j0 = 0; j0 < N; j0 += TN) {
        const int64_t j = j0 + lane;
        const bool jvalid = j < N;
        float ex[RW];
#pragma unroll
        for (int r = 0; r < RW; r++) ex[r] = 0.0f;
        __syncthreads();                                        // (the previous tile has been read; the first: the rows are staged)
        if (has_ex) {
            for (int e = tid; e < TN * h; e += WAVES * 64) {    // coalesced read of TN rows of h floats
                const int jj = e / h, c = e % h;
                const int64_t gj = j0 + jj;
                tile[jj * hx + c] = gj < N ? xp[gj * h + c] : 0.0f;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < RW; r++) ex[r] = edge_mlp_dist_extra(rowsX + (wave * RW + r) * h, tile + lane * hx, h, t_ex);
            __syncthreads();
        }
        // B_v of the tile, transposed: a lane fetches 16 bytes of ITS column's row (lanes differ in the column: the LDS writes of a
        // wavefront go to 64 consecutive words)
        for (int e = tid; e < TN * (HW / 4); e += WAVES * 64) {
            const int jj = e % TN, c4 = (e / TN) * 4;
            const int64_t gj = j0 + jj;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (gj < N) v = *reinterpret_cast<const float4 *>(AB + gj * 2 * HW + HW + c4);
            tile[(c4 + 0) * TN + jj] = v.x; tile[(c4 + 1) * TN + jj] = v.y;
            tile[(c4 + 2) * TN + jj] = v.z; tile[(c4 + 3) * TN + jj] = v.w;
        }
        const float dv = (has_deg && jvalid) ? deg[j] : 0.0f;
        if constexpr (PRIOR) {
#pragma unroll
            for (int r = 0; r < RW; r++) ex[r] = prior_tile_extra(pc[r], P, j0, strip, lane);
        }
        __syncthreads();

        float s[RW];
#pragma unroll
        for (int r = 0; r < RW; r++) s[r] = 0.0f;
#pragma unroll 2
        for (int o0 = 0; o0 < HW; o0 += OB) {
            float b[OB], p_du[OB], p_dv[OB], p_ex[OB], p_b1[OB], p_w2[OB];
#pragma unroll
            for (int q = 0; q < OB; q++) {
                b[q] = tile[(o0 + q) * TN + lane];
                p_du[q] = has_deg ? wdu[o0 + q] : 0.0f;          // (wave-uniform)
                p_dv[q] = has_deg ? wdv[o0 + q] : 0.0f;
                p_ex[q] = any_ex ? wex[o0 + q] : 0.0f;
                p_b1[q] = b1[o0 + q];
                p_w2[q] = w2[o0 + q];
            }
#pragma unroll
            for (int r = 0; r < RW; r++) {
                const float *a = rowsA + (wave * RW + r) * HW + o0;   // wave-uniform address: LDS broadcast
#pragma unroll
                for (int q = 0; q < OB; q++)
                    s[r] = edge_mlp_unit(a[q], b[q], q, has_deg, du[r], dv, p_du, p_dv, any_ex, ex[r], p_ex, p_b1, p_w2, act, s[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RW; r++) {
            const int64_t i = rbase + wave * RW + r;
            if (i >= row1) continue;                            // wave-uniform
            float v = edge_mlp_prob(s[r], b2v);
            if (noise_mode != 0) {
                float g = 0.0f;
                if (noise_mode == 1) g = jvalid ? G[i * ldG + j] : 0.0f;
                else g = pair_noise(s0, s1, (uint32_t)i, (uint32_t)j, sym);
                v = perturb_p(v, g);
            }
            const uint64_t key = jvalid ? make_key(v, (int32_t)j) : DGG_EMPTY_KEY;
            const bool pass = key > thr[r];
            if (__ballot(pass) != 0ull) {                       // wave-uniform
                uint64_t cand = pass ? key : DGG_EMPTY_KEY;
                cand = wave_sort_desc(cand, lane);
                list[r] = wave_merge_top64(list[r], cand, lane);
                thr[r] = shfl_u64(list[r], 63);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RW; r++) {
        const int64_t i = rbase + wave * RW + r;
        if (i >= row1) continue;
        if (lane < K) {
            const bool empty = list[r] == DGG_EMPTY_KEY;
            const int32_t c = key_col(list[r]);
            const int64_t o = (i - row0) * K + lane;
            idx[o] = empty ? -1 : c;
            val[o] = empty ? 0.0f : key_val(list[r]);
            if constexpr (PRIOR) {
                if (ex_out) ex_out[o] = empty ? 0.0f : prior_value_at(P, i, c);
            } else {
                if (ex_out) ex_out[o] = (has_ex && !empty) ? edge_mlp_dist_extra(xp + i * h, xp + (int64_t)c * h, h, t_ex) : 0.0f;
            }
        }
    }
}

size_t lds_bytes(int hw, int rw, int h, bool has_ex) {
    const size_t rb = (size_t)rw * WAVES;
    size_t tile = (size_t)hw * TN;
    if (has_ex && (size_t)TN * (h + 1) > tile) tile = (size_t)TN * (h + 1);
    return (rb * hw + (has_ex ? rb * h : 0) + tile) * sizeof(float);
}

size_t lds_bytes_prior(int hw, int rw) { return ((size_t)rw * WAVES * hw + (size_t)hw * TN + (size_t)WAVES * 64) * sizeof(float); }

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
    int K;
    int32_t *idx;
    float *val, *ex_out;
    hipStream_t st;
    const int64_t *prp;           // the prior's CSR arrays (dgg_allpairs_mlp_topk_prior; NULL otherwise)
    const int32_t *pci;
    const float *pv;
};

template <int HW, int RW, int VAR>
void launch_one(const Args &a) {
    const int64_t rows = a.row1 - a.row0;
    constexpr int RB = RW * WAVES;
    if constexpr (VAR >= 4) {
        hipLaunchKernelGGL((allpairs_mlp_topk_kernel<HW, RW, VAR, const int64_t *, const int32_t *, const float *>), dim3((unsigned)((rows + RB - 1) / RB)), dim3(WAVES * 64),
                           lds_bytes_prior(HW, RW), a.st, a.AB, a.xp, a.N, a.h, a.row0, a.row1, a.deg, a.ex_mode, a.t_ex, a.wdu, a.wdv, a.wex,
                           a.b1, a.w2, a.b2, a.act, a.noise_mode, a.G, a.ldG, a.s0, a.s1, a.K, a.idx, a.val, a.ex_out, a.prp, a.pci, a.pv);
    } else {
        hipLaunchKernelGGL((allpairs_mlp_topk_kernel<HW, RW, VAR>), dim3((unsigned)((rows + RB - 1) / RB)), dim3(WAVES * 64),
                           lds_bytes(HW, RW, a.h, a.ex_mode == 2), a.st, a.AB, a.xp, a.N, a.h, a.row0, a.row1, a.deg, a.ex_mode, a.t_ex, a.wdu,
                           a.wdv, a.wex, a.b1, a.w2, a.b2, a.act, a.noise_mode, a.G, a.ldG, a.s0, a.s1, a.K, a.idx, a.val, a.ex_out);
    }
}

// rows per wavefront: RWBIG while that still gives every SIMD of the device a few wavefronts, else 2 (small graphs, row shards).
// DGG_APMLP_RW=big / small (read on every call: a host-side getenv) forces one of the two whatever the row count -- how the tests hold
// the RWBIG kernels to the CPU oracle at small N, and how the two are timed against each other.
template <int HW, int VAR>
void launch_rw(const Args &a) {
    constexpr int RWBIG = HW == 128 ? 4 : 8;                     // (hw = h = 128 with the extra: 16 rows + tile = 48.3 KB of LDS)
    const int64_t rows = a.row1 - a.row0;
    bool big = (rows + RWBIG * WAVES - 1) / (RWBIG * WAVES) >= 1024;
    if (const char *e = getenv("DGG_APMLP_RW")) {
        if (!strcmp(e, "big")) big = true;
        else if (!strcmp(e, "small")) big = false;
    }
    if (big) launch_one<HW, RWBIG, VAR>(a);
    else launch_one<HW, 2, VAR>(a);
}

template <int HW>
void launch_var(const Args &a) {
    const bool leaky = a.act == 1;
    if (a.deg && leaky && a.ex_mode == 0) launch_rw<HW, 0>(a);
    else if (a.deg && leaky && a.ex_mode == 2) launch_rw<HW, 1>(a);
    else if (!a.deg && !leaky && a.ex_mode == 0) launch_rw<HW, 2>(a);
    else launch_rw<HW, 3>(a);
}

template <int HW>
void launch_var_prior(const Args &a) {
    if (!a.deg && a.act == 1) launch_rw<HW, 4>(a);
    else launch_rw<HW, 5>(a);
}

bool width_ok(int w) { return w == 16 || w == 32 || w == 64 || w == 128; }

}  // namespace

extern "C" int dgg_allpairs_mlp_topk(const float *AB, const float *xp, int64_t N, int h, int hw, int64_t row0, int64_t row1, const float *deg,
                                     int ex_mode, float t_ex, const float *wdu, const float *wdv, const float *wex, const float *b1,
                                     const float *w2, const float *b2, int act, int noise_mode, const float *G, int64_t ldG, uint32_t s0,
                                     uint32_t s1, int K, int32_t *idx, float *val, float *ex_out, void *stream) {
    if (!width_ok(hw) || !width_ok(h))
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk: hidden width hw and latent_dim h must be 16, 32, 64 or 128");
    if (K < 1 || K > 64) return dgg_set_error(DGG_ERR_UNSUPPORTED, "ELL width K must be in [1,64]");
    if (ex_mode == 1)
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk: a per-edge extra array (u-v-A_uv, A_uv) does not exist for all-pairs "
                                                  "candidates; supported: u-v-deg, u-v-deg-dist, edge_conv");
    if (noise_mode == 4 || noise_mode == 5)
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk: noise_mode must be none / explicit / hash / symmetric hash (every "
                                                  "pair is scored: the ranked generators have nothing to stop early)");
    if (ex_mode != 0 && ex_mode != 2) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk: ex_mode must be 0 (none) or 2 (exp(t dist))");
    if (noise_mode < 0 || noise_mode > 5) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk: unknown noise_mode");
    if (act != 0 && act != 1) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk: act must be 0 (identity) or 1 (LeakyReLU)");
    if (noise_mode == 1 && (!G || ldG < N)) return dgg_set_error(DGG_ERR_ARG, "explicit noise requested but G is NULL (or ldG < N)");
    if (row0 < 0 || row1 < row0 || row1 > N || N >= ((int64_t)1 << 31))
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk: rows must satisfy 0 <= row0 <= row1 <= N < 2^31");
    if (row0 == row1) return 0;
    if (!AB || !b1 || !w2 || !b2 || !idx || !val || (ex_mode == 2 && (!xp || !wex)) || (deg && (!wdu || !wdv)))
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk: missing inputs / weights for the requested mode");
    if ((reinterpret_cast<uintptr_t>(AB) & 15) != 0) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk: AB must be 16-byte aligned");
    const Args a{AB, xp, N, h, row0, row1, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, noise_mode, G, ldG, s0, s1, K, idx, val, ex_out,
                 (hipStream_t)stream, nullptr, nullptr, nullptr};
    switch (hw) {
        case 16: launch_var<16>(a); break;
        case 32: launch_var<32>(a); break;
        case 64: launch_var<64>(a); break;
        default: launch_var<128>(a); break;
    }
    return dgg_check_launch("allpairs_mlp_topk");
}

extern "C" int dgg_allpairs_mlp_topk_prior(const float *AB, const float *xp, int64_t N, int h, int hw, int64_t row0, int64_t row1,
                                           const float *deg, int ex_mode, float t_ex, const float *wdu, const float *wdv, const float *wex,
                                           const float *b1, const float *w2, const float *b2, int act, int noise_mode, const float *G,
                                           int64_t ldG, uint32_t s0, uint32_t s1, int K, int32_t *idx, float *val, float *ex_out,
                                           const int64_t *prior_rowptr, const int32_t *prior_col, const float *prior_val, void *stream) {
    if (!width_ok(hw) || !width_ok(h))
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk_prior: hidden width hw and latent_dim h must be 16, 32, 64 or 128");
    if (K < 1 || K > 64) return dgg_set_error(DGG_ERR_UNSUPPORTED, "ELL width K must be in [1,64]");
    if (ex_mode != 1)
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk_prior: ex_mode must be 1 (the extra of a pair is the prior's stored "
                                                  "value); ex_mode 0 / 2 are dgg_allpairs_mlp_topk's");
    if (noise_mode == 4 || noise_mode == 5)
        return dgg_set_error(DGG_ERR_UNSUPPORTED, "allpairs_mlp_topk_prior: noise_mode must be none / explicit / hash / symmetric hash "
                                                  "(every pair is scored: the ranked generators have nothing to stop early)");
    if (noise_mode < 0 || noise_mode > 5) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_prior: unknown noise_mode");
    if (act != 0 && act != 1) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_prior: act must be 0 (identity) or 1 (LeakyReLU)");
    if (noise_mode == 1 && (!G || ldG < N)) return dgg_set_error(DGG_ERR_ARG, "explicit noise requested but G is NULL (or ldG < N)");
    if (row0 < 0 || row1 < row0 || row1 > N || N >= ((int64_t)1 << 31))
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_prior: rows must satisfy 0 <= row0 <= row1 <= N < 2^31");
    if (!prior_rowptr || !prior_col || !prior_val)
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_prior: the prior's CSR arrays (rowptr, col, val) must not be NULL");
    if (row0 == row1) return 0;
    if (!AB || !wex || !b1 || !w2 || !b2 || !idx || !val || (deg && (!wdu || !wdv)))
        return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_prior: missing inputs / weights for the requested mode");
    if ((reinterpret_cast<uintptr_t>(AB) & 15) != 0) return dgg_set_error(DGG_ERR_ARG, "allpairs_mlp_topk_prior: AB must be 16-byte aligned");
    const Args a{AB, xp, N, h, row0, row1, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, noise_mode, G, ldG, s0, s1, K, idx, val, ex_out,
                 (hipStream_t)stream, prior_rowptr, prior_col, prior_val};
    switch (hw) {
        case 16: launch_var_prior<16>(a); break;
        case 32: launch_var_prior<32>(a); break;
        case 64: launch_var_prior<64>(a); break;
        default: launch_var_prior<128>(a); break;
    }
    return dgg_check_launch("allpairs_mlp_topk_prior");
}
