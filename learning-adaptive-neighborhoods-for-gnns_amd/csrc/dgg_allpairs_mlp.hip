// dgg_allpairs_mlp.hip -- the edge-MLP scorers u-v-deg / u-v-deg-dist / edge_conv (reference dgm.py:1645-1719) on ALL-PAIRS candidates:
// score + perturbation (dgm.py:1211-1229) + torch.sort kept to the K <= 64 best per row (dgm.py:1404) in one kernel.
//
// These three scorers are functions of the two end nodes and their prior degrees only, and their first layer splits into per-node
// products AB = xp [Wa | Wb]^T (dgg_edgemlp.hip), so a pair costs O(hw) vector work and nothing is gathered.  The structure is that of
// allpairs_topk_exhaustive (dgg_topk.hip): a workgroup owns a block of rows whose A_u (and xp_u) sit in LDS, column tiles of B_v (and
// xp_v) stream through LDS, every wavefront keeps the running top-64 of its rows in registers (one key per lane) and merges a tile only
// when one of its keys passes the row's threshold.  The N x N probabilities of the composed path (dgg_edge_mlp_fwd on the complete
// pattern + dgg_edgelist_topk_p) never exist; the result has the same bits: the score chain is the shared one of dgg_edgemlp_score.h.
// The sweep up to a pair's key -- staging, score, perturbation -- and the entry points' checks and dispatch are shared with the wide
// kernel (dgg_allpairs_mlp_wide.hip) and live in dgg_allpairs_mlp_sweep.h; this file holds the register list and the [rows, K] write-out.
//
// dgg_allpairs_mlp_topk_prior: the same sweep for u-v-A_uv (dgm.py:1628-1644) against a sparse PRIOR graph -- the extra of pair (i, j) is
// the prior's stored value, 0.0f where it stores nothing (the complete in_adj whose values are the prior's, zero for non-edges).  The
// tiles ascend and so do a row's CSR entries: a wavefront keeps one cursor per row and touches the prior only in tiles that hold an
// entry of the row (dgg_prior_lookup.h); ex_out of a kept entry comes from a binary search in the row's segment at write-out.
#include "dgg_allpairs_mlp_sweep.h"

#include <cstdlib>

using namespace dgg;
using namespace dgg::apmlp;

namespace {

// The sweep of dgg_allpairs_mlp_sweep.h (VAR, the LDS layout and the stages of a tile are documented there) into ONE descending register
// list per row: a tile's keys that pass the row's threshold (its 64th best so far) are sorted and merged in, then the [rows, K] write-out.
template <int HW, int RW, int VAR, class... PR>
__global__ __launch_bounds__(WAVES * 64) void allpairs_mlp_topk_kernel(
    const float *__restrict__ AB, const float *__restrict__ xp, int64_t N, int h, int64_t row0, int64_t row1_,
    const float *__restrict__ deg, int ex_mode, float t_ex, const float *__restrict__ wdu, const float *__restrict__ wdv,
    const float *__restrict__ wex, const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2, int act_rt,
    int noise_mode, const float *__restrict__ G, int64_t ldG, uint32_t s0, uint32_t s1, int K, int32_t *__restrict__ idx,
    float *__restrict__ val, float *__restrict__ ex_out, PR... pr) {
    // (the scalars keep their __restrict__, which a struct argument would lose: the struct lives in registers)
    const Scorer sc{AB, xp, N, h, row0, row1_, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act_rt, noise_mode, G, ldG, s0, s1};
    constexpr int RB = RW * WAVES;
    constexpr bool PRIOR = var_prior(VAR);
    static_assert(sizeof...(PR) == (PRIOR ? 3 : 0), "the prior variants, and only they, take the prior's CSR arrays");
    extern __shared__ float lds[];
    const Switches sw = resolve<VAR>(sc);
    const int tid = threadIdx.x, lane = tid & 63, wave = dgg::wave_id();
    const Lds L = lds_layout<HW, RB>(lds, sc.h, sw.has_ex, wave);
    const int64_t rbase = sc.row0 + (int64_t)blockIdx.x * RB, row1 = sc.row1;

    stage_rows<HW, RB>(sc, L, rbase, sw.has_ex, tid);
    float du[RW];
    uint64_t list[RW], thr[RW];
#pragma unroll
    for (int r = 0; r < RW; r++) {
        const int64_t gi = rbase + wave * RW + r;               // wave-uniform
        du[r] = (sw.has_deg && gi < row1) ? sc.deg[gi] : 0.0f;
        list[r] = DGG_EMPTY_KEY;
        thr[r] = DGG_EMPTY_KEY;
    }
    const PriorCsr P = prior_csr(pr...);
    PriorCursor pc[PRIOR ? RW : 1];
    if constexpr (PRIOR) {
#pragma unroll
        for (int r = 0; r < RW; r++) {
            const int64_t gi = rbase + wave * RW + r;
            pc[r] = prior_cursor_open(P, gi, gi < row1);
        }
        L.strip[lane] = 0.0f;
        DGG_PRIOR_WAVE_FENCE();
    }
    const float b2v = sc.b2[0];

    for (int64_t j0 = 0; j0 < sc.N; j0 += TN) {
        const int64_t j = j0 + lane;
        float ex[RW];
#pragma unroll
        for (int r = 0; r < RW; r++) ex[r] = 0.0f;
        __syncthreads();                                        // (the previous tile has been read; the first: the rows are staged)
        if (sw.has_ex) dist_extra_tile<RW>(sc, L, j0, wave, lane, tid, true, ex);
        stage_b_tile<HW>(sc, L, j0, tid);
        const float dv = (sw.has_deg && j < sc.N) ? sc.deg[j] : 0.0f;
        if constexpr (PRIOR) {
#pragma unroll
            for (int r = 0; r < RW; r++) ex[r] = prior_tile_extra(pc[r], P, j0, L.strip, lane);
        }
        __syncthreads();

        float s[RW];
        score_tile<HW, RW>(sc, sw, L, wave, lane, du, dv, ex, s);
#pragma unroll
        for (int r = 0; r < RW; r++) {
            const int64_t i = rbase + wave * RW + r;
            if (i >= row1) continue;                            // wave-uniform
            const uint64_t key = pair_key(sc, s[r], b2v, i, j);
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
            const int64_t o = (i - sc.row0) * K + lane;
            idx[o] = empty ? -1 : c;
            val[o] = empty ? 0.0f : key_val(list[r]);
            if constexpr (PRIOR) {
                if (ex_out) ex_out[o] = empty ? 0.0f : prior_value_at(P, i, c);
            } else {
                if (ex_out) ex_out[o] = (sw.has_ex && !empty) ? edge_mlp_dist_extra(sc.xp + i * sc.h, sc.xp + (int64_t)c * sc.h, sc.h, sc.t_ex) : 0.0f;
            }
        }
    }
}

struct Out {                      // the entry points' own arguments
    int K;
    int32_t *idx;
    float *val, *ex_out;
};

template <int HW, int RW, int VAR>
void launch_one(const Scorer &sc, const Out &o, const Prior &pr, hipStream_t st) {
    constexpr int RB = RW * WAVES;
    const dim3 grid((unsigned)((sc.row1 - sc.row0 + RB - 1) / RB));
    const size_t lds = lds_bytes(HW, RB, sc.h, sc.ex_mode == 2, var_prior(VAR));
    auto go = [&](auto kernel, auto... prior) {
        hipLaunchKernelGGL(kernel, grid, dim3(WAVES * 64), lds, st, sc.AB, sc.xp, sc.N, sc.h, sc.row0, sc.row1, sc.deg, sc.ex_mode, sc.t_ex, sc.wdu, sc.wdv,
                           sc.wex, sc.b1, sc.w2, sc.b2, sc.act, sc.noise_mode, sc.G, sc.ldG, sc.s0, sc.s1, o.K, o.idx, o.val, o.ex_out, prior...);
    };
    if constexpr (var_prior(VAR)) go(allpairs_mlp_topk_kernel<HW, RW, VAR, const int64_t *, const int32_t *, const float *>, pr.rp, pr.ci, pr.v);
    else go(allpairs_mlp_topk_kernel<HW, RW, VAR>);
}

// rows per wavefront: RWBIG while that still gives every SIMD of the device a few wavefronts, else 2 (small graphs, row shards).
// DGG_APMLP_RW=big / small (read on every call: a host-side getenv) forces one of the two whatever the row count -- how the tests hold
// the RWBIG kernels to the CPU oracle at small N, and how the two are timed against each other.
template <int HW, int VAR>
void launch_rw(const Scorer &sc, const Out &o, const Prior &pr, hipStream_t st) {
    constexpr int RWBIG = HW == 128 ? 4 : 8;                     // (hw = h = 128 with the extra: 16 rows + tile = 48.3 KB of LDS)
    const int64_t rows = sc.row1 - sc.row0;
    bool big = (rows + RWBIG * WAVES - 1) / (RWBIG * WAVES) >= 1024;
    if (const char *e = getenv("DGG_APMLP_RW")) {
        if (!strcmp(e, "big")) big = true;
        else if (!strcmp(e, "small")) big = false;
    }
    if (big) launch_one<HW, RWBIG, VAR>(sc, o, pr, st);
    else launch_one<HW, 2, VAR>(sc, o, pr, st);
}

int run(const Entry &e, const Scorer &sc, int hw, const Out &o, const Prior &pr, void *stream) {
    bool go;
    if (const int rc = validate(e, sc, hw, o.K, 0, 0, 0, o.idx && o.val, pr, &go); rc != DGG_OK || !go) return rc;
    dispatch(hw, scorer_var(sc, e.prior), [&](auto HW, auto VAR) { launch_rw<HW(), VAR()>(sc, o, pr, (hipStream_t)stream); });
    return dgg_check_launch(e.name);
}

}  // namespace

extern "C" int dgg_allpairs_mlp_topk(const float *AB, const float *xp, int64_t N, int h, int hw, int64_t row0, int64_t row1, const float *deg,
                                     int ex_mode, float t_ex, const float *wdu, const float *wdv, const float *wex, const float *b1,
                                     const float *w2, const float *b2, int act, int noise_mode, const float *G, int64_t ldG, uint32_t s0,
                                     uint32_t s1, int K, int32_t *idx, float *val, float *ex_out, void *stream) {
    return run({"allpairs_mlp_topk", false, false}, {AB, xp, N, h, row0, row1, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, noise_mode, G, ldG, s0, s1},
               hw, {K, idx, val, ex_out}, {nullptr, nullptr, nullptr}, stream);
}

extern "C" int dgg_allpairs_mlp_topk_prior(const float *AB, const float *xp, int64_t N, int h, int hw, int64_t row0, int64_t row1,
                                           const float *deg, int ex_mode, float t_ex, const float *wdu, const float *wdv, const float *wex,
                                           const float *b1, const float *w2, const float *b2, int act, int noise_mode, const float *G,
                                           int64_t ldG, uint32_t s0, uint32_t s1, int K, int32_t *idx, float *val, float *ex_out,
                                           const int64_t *prior_rowptr, const int32_t *prior_col, const float *prior_val, void *stream) {
    return run({"allpairs_mlp_topk_prior", false, true}, {AB, xp, N, h, row0, row1, deg, ex_mode, t_ex, wdu, wdv, wex, b1, w2, b2, act, noise_mode, G, ldG, s0, s1},
               hw, {K, idx, val, ex_out}, {prior_rowptr, prior_col, prior_val}, stream);
}
