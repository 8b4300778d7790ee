// dgg_edgemlp_score.h -- the score chain of the edge-MLP scorers (reference dgm.py:1628-1725), shared by every kernel that evaluates
// it (dgg_edgemlp.hip on a candidate edge list; dgg_allpairs_mlp_sweep.h, the sweep of dgg_allpairs_mlp.hip and dgg_allpairs_mlp_wide.hip
// on all-pairs candidates) so that they return the same bits:
//   z_o = A[u][o] + B[v][o] (+ deg_u wdu_o + deg_v wdv_o) (+ ex wex_o) + b1_o;  p = sigmoid(sum_o act(z_o) w2_o + b2)
// in exactly the operation order of oracle/dgg_oracle.c (mlp_edge_p); the sum over o ascends.
#pragma once
#include "dgg_common.h"

namespace dgg {

__device__ __forceinline__ float act_apply(float z, int act) { return act == 1 ? (z > 0.0f ? z : __fmul_rn(0.01f, z)) : z; }

// one hidden unit o: s + act(z_o) w2_o.  The weight arrays are indexed at o; those of a term that is switched off are not read (may be NULL).
__device__ __forceinline__ float edge_mlp_unit(float a, float b, int o, bool has_deg, float du, float dv, const float *__restrict__ wdu,
                                               const float *__restrict__ wdv, bool has_ex, float ex, const float *__restrict__ wex,
                                               const float *__restrict__ b1, const float *__restrict__ w2, int act, float s) {
    float z = __fadd_rn(a, b);
    if (has_deg) { z = __fmaf_rn(du, wdu[o], z); z = __fmaf_rn(dv, wdv[o], z); }
    if (has_ex) z = __fmaf_rn(ex, wex[o], z);
    z = __fadd_rn(z, b1[o]);
    return __fmaf_rn(act_apply(z, act), w2[o], s);
}

// the output layer's bias and the sigmoid
__device__ __forceinline__ float edge_mlp_prob(float s, float b2) {
    s = __fadd_rn(s, b2);
    return __fdiv_rn(1.0f, __fadd_rn(1.0f, c_exp(-s)));
}

// the per-edge extra of u-v-deg-dist: exp(t ||xp_u - xp_v||), canonical chain (dgm.py:1684-1686)
__device__ __forceinline__ float edge_mlp_dist_extra(const float *__restrict__ xu, const float *__restrict__ xv, int h, float t_ex) {
    return c_exp(__fmul_rn(t_ex, c_sqrt(pair_d2_thread(xu, xv, h))));
}

// Gumbel perturbation of an edge probability (dgm.py:1211-1229): exp(log(p + 1e-8) + g)
__device__ __forceinline__ float perturb_p(float p, float g) { return c_exp(__fadd_rn(c_log(__fadd_rn(p, 1e-8f)), g)); }

}  // namespace dgg
