// gemx_policy_dev.hpp -- the device helpers of the MLP actor that the policy rollout kernel (gemx_policy_kernel.hpp: the policy units and
// the complete policy units) and the evaluation pass (gemx_policy_eval.hip) share: the activations as register vectors, the 8-output FMA
// block on wave-uniform LDS reads, the activation functions.  What they are for is described at the head of gemx_policy_kernel.hpp.
#pragma once
#include "gemx_policy.hpp"

namespace gemx {

constexpr int PL_BLOCK_MAX = 256;

// The activations: eight 8-float vector VALUES per layer (struct members, never an array in memory), so that they are registers whatever
// the optimiser's passes make of the loops around them
typedef float pl_v8 __attribute__((ext_vector_type(8)));
struct PlAct { pl_v8 b0, b1, b2, b3, b4, b5, b6, b7; };
// one 8-output block's accumulators into its member, on the wave-uniform block index
__device__ __forceinline__ void pl_scatter(int jb, pl_v8 acc, PlAct &dst) {
    switch (jb) {
    case 0: dst.b0 = acc; break;
    case 1: dst.b1 = acc; break;
    case 2: dst.b2 = acc; break;
    case 3: dst.b3 = acc; break;
    case 4: dst.b4 = acc; break;
    case 5: dst.b5 = acc; break;
    case 6: dst.b6 = acc; break;
    default: dst.b7 = acc;
    }
}
// acc[q] = fmaf(w[q], x, acc[q]) for the 8 outputs of a block: w = 8 consecutive words of the blob in LDS, one address for the wave
__device__ __forceinline__ void pl_fma8(const float *w, float x, pl_v8 &acc) {
    const float4 w0 = *reinterpret_cast<const float4 *>(w), w1 = *reinterpret_cast<const float4 *>(w + 4);
    acc[0] = fmaf(w0.x, x, acc[0]); acc[1] = fmaf(w0.y, x, acc[1]); acc[2] = fmaf(w0.z, x, acc[2]); acc[3] = fmaf(w0.w, x, acc[3]);
    acc[4] = fmaf(w1.x, x, acc[4]); acc[5] = fmaf(w1.y, x, acc[5]); acc[6] = fmaf(w1.z, x, acc[6]); acc[7] = fmaf(w1.w, x, acc[7]);
}
// the 8 inputs of one input block of a later layer (x: that member of the previous layer's activations) into one output block's
// accumulators, in order; w: row 8 ib of that output block
__device__ __forceinline__ void pl_in_block(const float *w, pl_v8 x, pl_v8 &acc) {
#pragma unroll
    for (int q = 0; q < 8; ++q) pl_fma8(w + q * 8, x[q], acc);
}
__device__ __forceinline__ pl_v8 pl_pick(const PlAct &h, int ib) {
    switch (ib) {
    case 0: return h.b0;
    case 1: return h.b1;
    case 2: return h.b2;
    case 3: return h.b3;
    case 4: return h.b4;
    case 5: return h.b5;
    case 6: return h.b6;
    default: return h.b7;
    }
}
__device__ __forceinline__ pl_v8 pl_load8(const float *p) {
    const float4 v0 = *reinterpret_cast<const float4 *>(p), v1 = *reinterpret_cast<const float4 *>(p + 4);
    pl_v8 r = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    return r;
}
__device__ __forceinline__ void pl_activate(int activation, pl_v8 &acc) {
    if (activation == PL_ACT_TANH) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = tanhf(acc[q]);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = fmaxf(acc[q], 0.0f);
    }
}

}  // namespace gemx
