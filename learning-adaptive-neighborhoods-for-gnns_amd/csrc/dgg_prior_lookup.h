// dgg_prior_lookup.h -- the stored value of a pair (i, j) of a sparse PRIOR graph (CSR: rowptr int64 [N+1], columns int32 strictly
// ascending within a row, values float32) inside the all-pairs sweeps of dgg_allpairs_mlp.hip / dgg_allpairs_mlp_wide.hip: the per-edge
// extra a_uv of the scorer u-v-A_uv (reference dgm.py:1628-1644) on the complete candidate pattern, 0.0f where nothing is stored.
//
// The sweeps walk the columns in ascending 64-column tiles, and so do a row's entries: a wavefront keeps one wave-uniform cursor per
// row plus the column at the cursor.  A tile whose first column past the cursor is >= j0 + 64 holds no entry of the row: the extra
// is 0.0f without a memory access (almost every tile of a sparse prior).  Otherwise lane l loads entry cursor + l -- a tile has 64
// distinct columns, so one 64-entry load covers it -- the in-tile lanes write their value at column - j0 into a 64-float strip of LDS
// (one per wavefront, kept all-zero between uses), every lane reads its own column's slot, the written slots are zeroed again and
// the cursor advances by the number of in-tile entries.
#pragma once
#include "dgg_common.h"

namespace dgg {

constexpr int32_t PRIOR_NO_COL = 0x7fffffff;

struct PriorCsr {                 // the prior's CSR arrays
    const int64_t *rp;
    const int32_t *ci;
    const float *v;
};
__device__ __forceinline__ PriorCsr prior_csr() { return PriorCsr{nullptr, nullptr, nullptr}; }     // (a kernel variant without a prior)
__device__ __forceinline__ PriorCsr prior_csr(const int64_t *rp, const int32_t *ci, const float *v) { return PriorCsr{rp, ci, v}; }

struct PriorCursor {              // (wave-uniform)
    int64_t cur, end;             // entries [cur, end) of the row are still ahead of the sweep
    int32_t next;                 // column of entry cur; PRIOR_NO_COL past the row's end
};

#define DGG_PRIOR_WAVE_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

// the cursor at the start of row `row`; a row that is not `live` (outside the range, settled) has no entries
__device__ __forceinline__ PriorCursor prior_cursor_open(const PriorCsr &P, int64_t row, bool live) {
    PriorCursor pc;
    pc.cur = live ? P.rp[row] : 0;
    pc.end = live ? P.rp[row + 1] : 0;
    pc.next = pc.cur < pc.end ? P.ci[pc.cur] : PRIOR_NO_COL;
    return pc;
}

// the prior value of (row, j0 + lane) for the tile [j0, j0 + 64); advances the cursor past the tile.  strip: this wavefront's 64 floats
// of LDS, all zero on entry and on return.  An entry left of the tile (columns not ascending: outside the contract) is never written.
__device__ __forceinline__ float prior_tile_extra(PriorCursor &pc, const PriorCsr &P, int64_t j0, float *strip, int lane) {
    if ((int64_t)pc.next >= j0 + 64) return 0.0f;               // wave-uniform
    const int64_t p = pc.cur + lane;
    const bool in = p < pc.end;
    const int32_t c = in ? P.ci[p] : PRIOR_NO_COL;
    const bool hit = in && (int64_t)c >= j0 && (int64_t)c < j0 + 64;
    const int slot = hit ? (int)((int64_t)c - j0) : 0;
    if (hit) strip[slot] = P.v[p];
    DGG_PRIOR_WAVE_FENCE();
    const float ex = strip[lane];
    DGG_PRIOR_WAVE_FENCE();
    if (hit) strip[slot] = 0.0f;
    DGG_PRIOR_WAVE_FENCE();
    pc.cur += __popcll(__ballot(hit));
    pc.next = pc.cur < pc.end ? P.ci[pc.cur] : PRIOR_NO_COL;
    return ex;
}

// the prior value of (row, c) by binary search in the row's segment (write-out of a kept column); 0.0f where nothing is stored
__device__ __forceinline__ float prior_value_at(const PriorCsr &P, int64_t row, int32_t c) {
    const int64_t end = P.rp[row + 1];
    int64_t lo = P.rp[row], hi = end;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (P.ci[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && P.ci[lo] == c) ? P.v[lo] : 0.0f;
}

}  // namespace dgg
