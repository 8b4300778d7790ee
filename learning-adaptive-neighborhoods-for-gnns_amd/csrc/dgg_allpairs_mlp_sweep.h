// dgg_allpairs_mlp_sweep.h -- the sweep that the all-pairs edge-MLP kernels share: dgg_allpairs_mlp.hip (one 64-rank register list per
// row) and dgg_allpairs_mlp_wide.hip (chunked rows of any width) score the same pairs in the same order and must return the same bits as
// each other and as the CPU oracle, so everything up to the perturbed key of a pair exists once, here; what a kernel does with the key
// (its lists, passes and write-out) stays in its file.  The score chain itself is dgg_edgemlp_score.h's.
//
// A workgroup of WAVES wavefronts owns RB = RW * WAVES rows (RW per wavefront) whose A_u (and xp_u) sit in LDS; 64-column tiles of B_v
// (and xp_v) stream through LDS, one column per lane.
//
// VAR: the scorer's switches as compile-time constants (Switches, resolve<VAR>) --
//   0: degrees, LeakyReLU (u-v-deg)            1: degrees, LeakyReLU, exp(t dist) extra (u-v-deg-dist)
//   2: neither, no activation (edge_conv)      3: whatever the arguments say (any other combination without a prior)
//   4: prior extra, LeakyReLU, no degree term (u-v-A_uv)       5: prior extra, whatever degree term and activation the arguments say
// VAR 4 / 5 (the *_prior entry points): the extra of a pair is the stored value of a sparse prior graph (dgg_prior_lookup.h), whose CSR
// arrays are the kernel's TRAILING arguments, a pack that is empty for VAR 0..3 -- those kernels take no argument more than without.
//
// LDS (dynamic; lds_layout / lds_bytes): rowsA [RB][HW] | rowsX [RB][h] (distance extra only) | tile | strips [WAVES][64] (prior only).
// The tile holds, one after the other, xp_v NOT transposed with rows of h + 1 floats (a lane walks its own row: bank = lane + c,
// conflict-free) and then B_v transposed [HW][TN] (lane-strided reads).
//
// Contract of the device functions:
//  - Barriers.  dist_extra_tile is the only one that holds barriers (two); it is called under has_ex alone, which is uniform over the
//    workgroup, never under a wave-dependent condition: a wavefront with nothing to score passes live = false instead.  The others hold
//    none, so a kernel may gate them per wavefront (the wide kernel's wave_open / depth[r] == 0) and owns the loop's two barriers:
//    one before dist_extra_tile / stage_b_tile (the previous tile has been read; the first: the rows are staged), one after stage_b_tile.
//  - Operation order.  Every floating-point operation is in its __f*_rn form and place; the files build with -ffp-contract=off.
//  - Wave-uniform values (du, the rows' indices, the prior cursors) come in by value or by reference to a local array of a
//    __forceinline__ function, so they stay in scalar registers after inlining.
#pragma once
#include "dgg_common.h"
#include "dgg_edgemlp_score.h"
#include "dgg_prior_lookup.h"
#include "dgg_api_internal.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>

namespace dgg {
namespace apmlp {

constexpr int WAVES = 4;          // wavefronts per workgroup
constexpr int TN = 64;            // columns per tile (one per lane)
constexpr int OB = 8;             // hidden units per pass over a wavefront's rows

struct Scorer {                   // the scorer and noise arguments of the four entry points
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
};

constexpr bool var_prior(int VAR) { return VAR >= 4; }

struct Switches {
    bool has_deg, has_ex, any_ex; // degree term; the DISTANCE extra; any extra (distance or prior)
    int act;
};
template <int VAR>
__device__ __forceinline__ Switches resolve(const Scorer &sc) {
    constexpr bool RT = VAR == 3 || VAR == 5;
    Switches sw;
    sw.has_deg = RT ? sc.deg != nullptr : (VAR != 2 && VAR != 4);
    sw.has_ex = VAR == 3 ? sc.ex_mode == 2 : VAR == 1;
    sw.any_ex = sw.has_ex || var_prior(VAR);
    sw.act = RT ? sc.act : (VAR == 2 ? 0 : 1);
    return sw;
}

struct Lds {
    float *rowsA, *rowsX, *tile, *strip;   // strip: (prior only) this wavefront's 64 floats of prior_tile_extra
};
template <int HW, int RB>
__device__ __forceinline__ Lds lds_layout(float *lds, int h, bool has_ex, int wave) {
    Lds L;
    L.rowsA = lds;
    L.rowsX = L.rowsA + RB * HW;
    L.tile = L.rowsX + (has_ex ? RB * h : 0);
    L.strip = L.tile + HW * TN + wave * 64;
    return L;
}
inline size_t lds_bytes(int hw, int rb, int h, bool has_ex, bool prior) {
    size_t tile = (size_t)hw * TN;
    if (has_ex && (size_t)TN * (h + 1) > tile) tile = (size_t)TN * (h + 1);
    return ((size_t)rb * hw + (has_ex ? (size_t)rb * h : 0) + tile + (prior ? (size_t)WAVES * 64 : 0)) * sizeof(float);
}

// A_u (and xp_u with the distance extra) of the workgroup's rows [rbase, rbase + RB); rows past row1 are zero
template <int HW, int RB>
__device__ __forceinline__ void stage_rows(const Scorer &sc, const Lds &L, int64_t rbase, bool has_ex, int tid) {
    for (int e = tid; e < RB * HW; e += WAVES * 64) {
        const int r = e / HW, c = e % HW;
        const int64_t gi = rbase + r;
        L.rowsA[e] = gi < sc.row1 ? sc.AB[gi * 2 * HW + c] : 0.0f;
    }
    if (has_ex) {
        const int h = sc.h;
        for (int e = tid; e < RB * h; e += WAVES * 64) {
            const int r = e / h, c = e % h;
            const int64_t gi = rbase + r;
            L.rowsX[e] = gi < sc.row1 ? sc.xp[gi * h + c] : 0.0f;
        }
    }
}

// the distance extra of this wavefront's RW rows against the tile [j0, j0 + TN): stages xp_v (coalesced read of TN rows of h floats),
// BARRIER, ex[r] (live wavefronts only), BARRIER (the tile is free for B_v).  Every wavefront of the workgroup must call it.
template <int RW>
__device__ __forceinline__ void dist_extra_tile(const Scorer &sc, const Lds &L, int64_t j0, int wave, int lane, int tid, bool live, float (&ex)[RW]) {
    const int h = sc.h, hx = h + 1;
    for (int e = tid; e < TN * h; e += WAVES * 64) {
        const int jj = e / h, c = e % h;
        const int64_t gj = j0 + jj;
        L.tile[jj * hx + c] = gj < sc.N ? sc.xp[gj * h + c] : 0.0f;
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < RW; r++) ex[r] = edge_mlp_dist_extra(L.rowsX + (wave * RW + r) * h, L.tile + lane * hx, h, sc.t_ex);
    }
    __syncthreads();
}

// B_v of the tile, transposed: a lane fetches 16 bytes of ITS column's row (lanes differ in the column: the LDS writes of a wavefront
// go to 64 consecutive words)
template <int HW>
__device__ __forceinline__ void stage_b_tile(const Scorer &sc, const Lds &L, int64_t j0, int tid) {
    for (int e = tid; e < TN * (HW / 4); e += WAVES * 64) {
        const int jj = e % TN, c4 = (e / TN) * 4;
        const int64_t gj = j0 + jj;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gj < sc.N) v = *reinterpret_cast<const float4 *>(sc.AB + gj * 2 * HW + HW + c4);
        L.tile[(c4 + 0) * TN + jj] = v.x; L.tile[(c4 + 1) * TN + jj] = v.y;
        L.tile[(c4 + 2) * TN + jj] = v.z; L.tile[(c4 + 3) * TN + jj] = v.w;
    }
}

// s[r] = the hidden layer's sum of pair (row r of this wavefront, the lane's column), OB hidden units at a time over the RW rows
template <int HW, int RW>
__device__ __forceinline__ void score_tile(const Scorer &sc, const Switches &sw, const Lds &L, int wave, int lane, const float (&du)[RW], float dv,
                                           const float (&ex)[RW], float (&s)[RW]) {
#pragma unroll
    for (int r = 0; r < RW; r++) s[r] = 0.0f;
#pragma unroll 2
    for (int o0 = 0; o0 < HW; o0 += OB) {
        float b[OB], p_du[OB], p_dv[OB], p_ex[OB], p_b1[OB], p_w2[OB];
#pragma unroll
        for (int q = 0; q < OB; q++) {
            b[q] = L.tile[(o0 + q) * TN + lane];
            p_du[q] = sw.has_deg ? sc.wdu[o0 + q] : 0.0f;         // (wave-uniform)
            p_dv[q] = sw.has_deg ? sc.wdv[o0 + q] : 0.0f;
            p_ex[q] = sw.any_ex ? sc.wex[o0 + q] : 0.0f;
            p_b1[q] = sc.b1[o0 + q];
            p_w2[q] = sc.w2[o0 + q];
        }
#pragma unroll
        for (int r = 0; r < RW; r++) {
            const float *a = L.rowsA + (wave * RW + r) * HW + o0;    // wave-uniform address: LDS broadcast
#pragma unroll
            for (int q = 0; q < OB; q++)
                s[r] = edge_mlp_unit(a[q], b[q], q, sw.has_deg, du[r], dv, p_du, p_dv, sw.any_ex, ex[r], p_ex, p_b1, p_w2, sw.act, s[r]);
        }
    }
}

// the key of pair (i, j): probability, perturbation, (score, column) key; the empty key for a column past N.  b2v = b2[0]
__device__ __forceinline__ uint64_t pair_key(const Scorer &sc, float s, float b2v, int64_t i, int64_t j) {
    const bool jvalid = j < sc.N;
    float v = edge_mlp_prob(s, b2v);
    if (sc.noise_mode != 0) {
        float g = 0.0f;
        if (sc.noise_mode == 1) g = jvalid ? sc.G[i * sc.ldG + j] : 0.0f;
        else g = pair_noise(sc.s0, sc.s1, (uint32_t)i, (uint32_t)j, sc.noise_mode == 3);
        v = perturb_p(v, g);
    }
    return jvalid ? make_key(v, (int32_t)j) : DGG_EMPTY_KEY;
}

// ---- host side of the entry points ---------------------------------------------------------------------------------------------------

struct Prior {                    // the prior's CSR arrays (the *_prior entry points)
    const int64_t *rp;
    const int32_t *ci;
    const float *v;
};

struct Entry {                    // what an entry point accepts
    const char *name;             // without "dgg_": the prefix of its messages
    bool wide;                    // chunked rows (k, mode, maxm, layout) instead of the [rows, K] list
    bool prior;                   // ex_mode 1 against the prior's CSR arrays instead of ex_mode 0 / 2
};

inline int fail(int code, const char *fmt, ...) {
    char msg[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    return dgg_set_error(code, msg);
}

inline bool width_ok(int w) { return w == 16 || w == 32 || w == 64 || w == 128; }

// the checks of the four entry points, in their order.  K: the list's width; mode, maxm, ccap: the chunked rows'; outs_ok: the entry's
// own pointers (outputs, layout) are there.  -> run = false with DGG_OK: no rows, nothing to launch.
inline int validate(const Entry &e, const Scorer &sc, int hw, int K, int mode, int maxm, int64_t ccap, bool outs_ok, const Prior &pr, bool *run) {
    const char *n = e.name;
    *run = false;
    if (!width_ok(hw) || !width_ok(sc.h)) return fail(DGG_ERR_UNSUPPORTED, "%s: hidden width hw and latent_dim h must be 16, 32, 64 or 128", n);
    if (!e.wide && (K < 1 || K > 64)) return fail(DGG_ERR_UNSUPPORTED, "ELL width K must be in [1,64]");
    if (e.prior && sc.ex_mode != 1)
        return fail(DGG_ERR_UNSUPPORTED, "%s: ex_mode must be 1 (the extra of a pair is the prior's stored value); ex_mode 0 / 2 are dgg_%.*s's", n,
                    (int)strlen(n) - 6, n);
    if (!e.prior && sc.ex_mode == 1)
        return fail(DGG_ERR_UNSUPPORTED, "%s: a per-edge extra array (u-v-A_uv, A_uv) does not exist for all-pairs candidates; supported: u-v-deg, "
                                         "u-v-deg-dist, edge_conv", n);
    if (sc.noise_mode == 4 || sc.noise_mode == 5)
        return fail(DGG_ERR_UNSUPPORTED, "%s: noise_mode must be none / explicit / hash / symmetric hash (every pair is scored: the ranked "
                                         "generators have nothing to stop early)", n);
    if (!e.prior && sc.ex_mode != 0 && sc.ex_mode != 2) return fail(DGG_ERR_ARG, "%s: ex_mode must be 0 (none) or 2 (exp(t dist))", n);
    if (sc.noise_mode < 0 || sc.noise_mode > 5) return fail(DGG_ERR_ARG, "%s: unknown noise_mode", n);
    if (sc.act != 0 && sc.act != 1) return fail(DGG_ERR_ARG, "%s: act must be 0 (identity) or 1 (LeakyReLU)", n);
    if (e.wide && mode != 0 && mode != 1 && mode != 3)
        return fail(DGG_ERR_ARG, "%s: mode must be 0 (k_times_edge_prob), 1 (k_only) or 3 (straight-through forward)", n);
    if (sc.noise_mode == 1 && (!sc.G || sc.ldG < sc.N)) return fail(DGG_ERR_ARG, "explicit noise requested but G is NULL (or ldG < N)");
    if (sc.row0 < 0 || sc.row1 < sc.row0 || sc.row1 > sc.N || sc.N >= ((int64_t)1 << 31))
        return fail(DGG_ERR_ARG, "%s: rows must satisfy 0 <= row0 <= row1 <= N < 2^31", n);
    if (e.wide && (maxm < 1 || maxm > DGG_CHUNK_MAXM_ANY || ccap < 0 || ccap >= ((int64_t)1 << 25)))
        return fail(DGG_ERR_ARG, "%s: maxm in 1..2^20, 0 <= ccap < 2^25 chunks", n);
    if (e.prior && (!pr.rp || !pr.ci || !pr.v)) return fail(DGG_ERR_ARG, "%s: the prior's CSR arrays (rowptr, col, val) must not be NULL", n);
    if (sc.row0 == sc.row1) return DGG_OK;
    if (!sc.AB || !sc.b1 || !sc.w2 || !sc.b2 || !outs_ok || (e.prior && !sc.wex) || (sc.ex_mode == 2 && (!sc.xp || !sc.wex)) ||
        (sc.deg && (!sc.wdu || !sc.wdv)))
        return fail(DGG_ERR_ARG, "%s: missing inputs / weights%s for the requested mode", n, e.wide ? " / layout" : "");
    if ((reinterpret_cast<uintptr_t>(sc.AB) & 15) != 0) return fail(DGG_ERR_ARG, "%s: AB must be 16-byte aligned", n);
    *run = true;
    return DGG_OK;
}

// (deg, act, ex_mode, prior) -> VAR
inline int scorer_var(const Scorer &sc, bool prior) {
    const bool leaky = sc.act == 1;
    if (prior) return (!sc.deg && leaky) ? 4 : 5;
    if (sc.deg && leaky && sc.ex_mode == 0) return 0;
    if (sc.deg && leaky && sc.ex_mode == 2) return 1;
    if (!sc.deg && !leaky && sc.ex_mode == 0) return 2;
    return 3;
}

// f(integral_constant HW, integral_constant VAR) for the hidden width hw (width_ok) and the VAR of scorer_var
template <class F>
void dispatch(int hw, int var, F &&f) {
    auto with_hw = [&](auto HW) {
        switch (var) {
            case 0: f(HW, std::integral_constant<int, 0>{}); break;
            case 1: f(HW, std::integral_constant<int, 1>{}); break;
            case 2: f(HW, std::integral_constant<int, 2>{}); break;
            case 3: f(HW, std::integral_constant<int, 3>{}); break;
            case 4: f(HW, std::integral_constant<int, 4>{}); break;
            default: f(HW, std::integral_constant<int, 5>{}); break;
        }
    };
    switch (hw) {
        case 16: with_hw(std::integral_constant<int, 16>{}); break;
        case 32: with_hw(std::integral_constant<int, 32>{}); break;
        case 64: with_hw(std::integral_constant<int, 64>{}); break;
        default: with_hw(std::integral_constant<int, 128>{}); break;
    }
}

}  // namespace apmlp
}  // namespace dgg
