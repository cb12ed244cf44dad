// gemx_policy.hpp -- the device MLP actor of the policy rollout (gemx_rollout_policy): what the C ABI (gemx_capi.hip) and the policy
// rollout units (gemx_policy.hip; the kernel: gemx_policy_kernel.hpp) share -- the layout of the weight blob, the kernel's view of a policy
// and the unit's entry points.
//
// THE BLOB (float words, one hipMalloc per policy, rewritten in place by gemx_policy_set_weights): per layer l, weights then biases.
//   weights  [JB][n_rows][8]: output block jb = outputs 8 jb .. 8 jb + 7, row i = input i.  Layer 0 has n_rows = the policy's input width
//            (x = [obs_prev[columns], references[k]] in THAT order); a later layer n_rows = the previous layer's width rounded up to 8,
//            the rows past the true width zero.  JB = the layer's width rounded up to 8, / 8; the outputs past the true width have zero
//            weights and a zero bias, so they come out as act(0) = 0 and feed zero rows.
//   biases   [8 JB]
// A wave reads 8 weights of one input with two 16-byte LDS reads at one address for all its lanes.
#pragma once
#include "gemx_common.hpp"

namespace gemx {

constexpr int PL_MAX_LAYERS = 3, PL_MAX_WIDTH = 64, PL_MAX_INPUT = 48;
constexpr int PL_ACT_RELU = 0, PL_ACT_TANH = 1;
constexpr int PL_SQUASH_TANH = 0, PL_SQUASH_CLIP = 1;
constexpr int EP_LAUNCH_POLICY = 7;  // gemx_handle::LastLaunch::pipe of policy_rollout_kernel (gemx_envparams.hpp lists the others)
// policy_rollout_kernel's GEN, where the actor's references come from: the complete env's generators stepped in the lane (an all-Wiener
// gemx_refgen, a gemx_refprofile; LastLaunch::il of such a launch), or none -- row k of the call's tensor
constexpr int PC_GEN_WIENER = 0, PC_GEN_PROFILE = 1, PC_GEN_NONE = 2;

constexpr int pl_pad8(int n) { return (n + 7) & ~7; }
// rows of layer l's weight block, and the blob's size in words, for widths n_in -> width[0] -> ... -> width[L - 1]
inline int pl_rows(int l, int n_in, const int *width) { return l == 0 ? n_in : pl_pad8(width[l - 1]); }
inline int pl_blob_words(int n_layers, int n_in, const int *width) {
    int words = 0;
    for (int l = 0; l < n_layers; ++l) words += pl_pad8(width[l]) * (pl_rows(l, n_in, width) + 1);
    return words;
}
// pack one layer (W [out][in] row-major, b [out]) at `dst`; returns the words written
inline int pl_pack_layer(float *dst, int l, int n_in, const int *width, const float *W, const float *b) {
    const int rows = pl_rows(l, n_in, width), in = l == 0 ? n_in : width[l - 1], out = width[l], jb_n = pl_pad8(out) / 8;
    for (int jb = 0; jb < jb_n; ++jb)
        for (int i = 0; i < rows; ++i)
            for (int q = 0; q < 8; ++q) {
                const int j = 8 * jb + q;
                dst[((size_t)jb * rows + i) * 8 + q] = (j < out && i < in) ? W[(size_t)j * in + i] : 0.0f;
            }
    float *bias = dst + (size_t)jb_n * rows * 8;
    for (int j = 0; j < 8 * jb_n; ++j) bias[j] = j < out ? b[j] : 0.0f;
    return 8 * jb_n * (rows + 1);
}

// the kernel's view of one policy call (kernel argument, by value -> SGPRs)
struct PolicyDev {
    const float *blob;            // the policy's weight blob (above)
    int32_t blob_words;
    int32_t n_layers;
    int32_t n_in;                 // layer 0's rows: n_cols + n_ref
    int32_t width[PL_MAX_LAYERS];
    int32_t activation, squash;   // PL_ACT_*, PL_SQUASH_*
    int32_t n_cols, n_ref;
    int8_t pos[GEMX_MAX_OUT];     // observation column c is input pos[c] of layer 0; -1: not selected
    const float *reset_obs;       // [S_out]: the handle's normalised reset observation (what the masked reset writes)
    const float *obs0;            // [N][S_out] | [S_out][N]: the observation in front of step 0
    const float *refs;            // [K][N][n_ref], nullptr with n_ref = 0
    const float *noise;           // [K][N][out], nullptr: none
    void *actions_out;            // [K][N][A] float | [K][N] uint8
};

}  // namespace gemx

// the host's policy object (include/gemx.h: gemx_policy)
struct gemx_policy {
    int device;
    int n_layers, n_in, width[gemx::PL_MAX_LAYERS];
    int activation, squash;
    int blob_words;
    float *blob;  // device
};

// a policy rollout unit, libgemx_pl<S>_<C>.so (fp32): gemx_pl_unit_init as gemx_unit_init; gemx_pl_unit_launch runs K >= 1 control steps of
// every env, each on the action the MLP computes from the previous step's row, with the episode time limit inside the launch
// (policy_rollout_kernel; the other arguments as gemx_tl_unit_launch takes them).  gemx_pl_unit_tanh runs the unit's tanhf over n values.
typedef int (*gemx_pl_unit_launch_fn)(gemx_handle *h, const gemx::PolicyDev *pol, int K, const int32_t *length, int32_t max_steps, void *obs, uint8_t *terminated,
                                      uint8_t *truncated, uint8_t *ended, hipStream_t st, int *linmap_built);
typedef int (*gemx_pl_unit_tanh_fn)(const float *x, float *y, long long n, hipStream_t st);
