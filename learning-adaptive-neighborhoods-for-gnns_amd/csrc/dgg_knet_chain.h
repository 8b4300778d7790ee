// dgg_knet_chain.h -- the forward chain of the learned-degree k-net on the fp32 matrix cores, ONE body for the two kernels that run it:
// knet_x_fwd_reg (dgg_knet.hip, layer-1 operands from xk in memory) and linear_fwd_reg<.., KS >= 0> (dgg_linear.hip, layer-1 operands out
// of the projection's xk accumulators).  Both hand it the SAME operand values in the same step order, so k and u agree bit for bit by
// construction.  Layout of the operands and accumulators: dgg_knet.hip, above knet_x_fwd_reg.
#pragma once
#include "dgg_common.h"

namespace dgg {

typedef float knet_f32x16 __attribute__((ext_vector_type(16)));

template <int H>
struct KnetChain {
    static constexpr int H2 = H / 2, H4 = H / 4, S1 = H / 2 + 1, S2 = H2 / 2 + 1;
    static constexpr int LDS_FLOATS = (S1 + S2) * 64;            // the two layers' weights in operand order

    // once per workgroup (NT threads, a barrier afterwards): lane (o, half) of step s holds W[o][2s + half]; the last step of
    // layer 1 carries the weight of nd and the bias, the last step of layer 2 its bias.  Every element is ONE unconditional load from a
    // clamped address, all of a thread's loads in flight at once, the zero padding applied at the LDS write (a rolled loop with the
    // loads behind their conditions paid one L2 round trip per pass: 13 of them at 256 threads, ~10 us of the fused projection).
    template <int NT>
    static __device__ __forceinline__ void stage(float *wsh, const float *__restrict__ W1, const float *__restrict__ b1,
                                                 const float *__restrict__ Wmu, const float *__restrict__ bmu, int tid) {
        constexpr int PASSES = (LDS_FLOATS + NT - 1) / NT;
        float v[PASSES];
#pragma unroll
        for (int it = 0; it < PASSES; it++) {
            const int e = tid + it * NT, l = e & 63, sI = e >> 6, o = l & 31, half = l >> 5;
            const float *p;
            if (sI < S1) {
                const int c = 2 * sI + half, oc = o < H2 ? o : 0;
                p = c <= H ? W1 + oc * (H + 1) + c : b1 + oc;
            } else {
                const int c = 2 * (sI - S1) + half, oc = o < H4 ? o : 0;
                p = c < H2 ? Wmu + oc * H2 + c : bmu + oc;
            }
            v[it] = *(e < LDS_FLOATS ? p : W1);
        }
#pragma unroll
        for (int it = 0; it < PASSES; it++) {
            const int e = tid + it * NT, l = e & 63, sI = e >> 6, o = l & 31, half = l >> 5;
            const bool live = sI < S1 ? o < H2 : (o < H4 && 2 * (sI - S1) + half <= H2);
            if (e < LDS_FLOATS) wsh[e] = live ? v[it] : 0.0f;
        }
    }

    // op1[s]: the layer-1 operand of step s on this lane = xk[node li][2s + half] (after the LeakyReLU of the projection);
    // dg = the node's prior degree; wp / bpv = k_project.  -> u (every lane of a node holds it); k = relu(u) + 1
    static __device__ __forceinline__ float run(const float (&op1)[H / 2], float dg, float mu, float sd, const float *wsh,
                                                const float (&wp)[H4], float bpv, int lane) {
        const int hh = lane >> 5;
        float w1[S1], w2[S2];
#pragma unroll
        for (int sI = 0; sI < S1; sI++) w1[sI] = wsh[sI * 64 + lane];
#pragma unroll
        for (int sI = 0; sI < S2; sI++) w2[sI] = wsh[(S1 + sI) * 64 + lane];
        const float nd = __fdiv_rn(__fadd_rn(dg, -mu), __fadd_rn(sd, 1e-5f));
        knet_f32x16 a1;
#pragma unroll
        for (int r = 0; r < 16; r++) a1[r] = 0.0f;
#pragma unroll
        for (int sI = 0; sI < S1 - 1; sI++) a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[sI], op1[sI], a1, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[S1 - 1], hh == 0 ? nd : 1.0f, a1, 0, 0, 0);      // k = H: nd, k = H + 1: the bias
        float zs[16];
#pragma unroll
        for (int r = 0; r < 16; r++) zs[r] = a1[r] > 0.0f ? a1[r] : __fmul_rn(0.01f, a1[r]);
        swap_pairs(zs);
        knet_f32x16 a2;
#pragma unroll
        for (int r = 0; r < 16; r++) a2[r] = 0.0f;
#pragma unroll
        for (int sI = 0; sI < S2 - 1; sI++) a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[sI], from_acc(zs, 2 * sI), a2, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[S2 - 1], hh == 0 ? 1.0f : 0.0f, a2, 0, 0, 0);     // k = H2: the bias
        // k_project: one lane per node gathers the h/4 values of m (its own rows and the other half's) and runs the ascending chain
        // (register r < 8 of half `hh` is output (r&3) + 8(r>>2) + 4 hh: output o lives in register (o&3) + 4(o>>3) of half (o>>2)&1 --
        // one select per output; indexing m[] by the lane's half made the compiler search the array: 256 compares + selects)
        float m[16];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const float other = __uint_as_float(xor_shfl<32>(__float_as_uint(a2[r]), lane));
            const int o = (r & 3) + 8 * (r >> 2);                // the lower half's output in this register; the upper half's is o + 4
            m[o] = hh == 0 ? a2[r] : other;
            m[o + 4] = hh == 0 ? other : a2[r];
        }
        float ak = 0.0f;
#pragma unroll
        for (int o = 0; o < H4; o++) ak = __fmaf_rn(m[o], wp[o], ak);
        const float kp = __fadd_rn(ak, bpv);
        return __fadd_rn(__fmul_rn(kp, sd), mu);
    }

    static __device__ __forceinline__ float k_of(float u) { return __fadd_rn(u > 0.0f ? u : 0.0f, 1.0f); }

    // A transposed 32x32 accumulator as the NEXT chain's second operand.  Lane (li, half) holds outputs o(r) = (r&3) + 8(r>>2) + 4 half of
    // node li; after one v_permlane32_swap per register pair (r, r+1), r even, the lower half holds o(r) and o(r) + 4, the upper half
    // o(r) + 1 and o(r) + 5 -- what the k-ordered chain wants from each half (step s: k = 2s below, 2s + 1 above).
    static __device__ __forceinline__ void swap_pairs(float (&zs)[16]) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(zs[r]), __float_as_uint(zs[r + 1]), false, false);
            zs[r] = __uint_as_float(q[0]);                       // lower half: o(r)      upper half: o(r) + 1
            zs[r + 1] = __uint_as_float(q[1]);                   // lower half: o(r) + 4  upper half: o(r) + 5
        }
    }
    // the operand of the step whose lower-half k is `o` (even, < 32), out of a swapped accumulator
    static __device__ __forceinline__ float from_acc(const float (&zs)[16], int o) {
        const int pr = 4 * (o >> 3) + (o & 2);
        return (o & 4) ? zs[pr + 1] : zs[pr];
    }
};

}  // namespace dgg
