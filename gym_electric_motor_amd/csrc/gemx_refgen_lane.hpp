// gemx_refgen_lane.hpp -- the per-lane functions of the all-Wiener reference generators: the counter-based draws, the sub-episode, the
// restart and the clipped walk of ONE (column, env).  gemx_refgen.hip's kernels (refgen_normals_kernel, refgen_walk_kernel,
// refgen_step_kernel, the kinds and switched kernels) and the complete policy rollout units (gemx_policy_complete.hip), which step the
// generators in the lane that steps the env, call THESE functions: one definition, hence one sequence of draws and one arithmetic.
// Reference (paths relative to src/gym_electric_motor/reference_generators/): see the head of gemx_refgen.hip.
#pragma once
#include "gemx_common.hpp"

namespace gemx {
namespace refgen_lane {

enum { DRAW_STEP = 0, DRAW_SUB = 1, DRAW_RESET = 2 };

__device__ inline void refgen_block(uint64_t seed, int64_t env, int gen, int kind, uint64_t index, uint32_t (&r)[4]) {
    // key: seed; counter: (env lo, env hi | gen << 24 | kind << 28, index lo, index hi)
    const uint64_t env_word = (uint64_t)env | ((uint64_t)gen << 56) | ((uint64_t)kind << 60);
    uint32_t c[4] = {(uint32_t)env_word, (uint32_t)(env_word >> 32), (uint32_t)index, (uint32_t)(index >> 32)};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int i = 0; i < 10; ++i) {
        gemx::Philox::round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    for (int i = 0; i < 4; ++i) r[i] = c[i];
}

// the standard normal of step t of (env, generator): Box-Muller on two Philox words, rounded to the tensor's type
template <class R> __device__ inline R step_normal(uint64_t seed, int64_t global_env, int g, uint64_t t) {
    uint32_t r[4];
    refgen_block(seed, global_env, g, DRAW_STEP, t, r);  // (the GLOBAL env index keys the stream)
    const double u1 = gemx::Philox::u01(r[0]), u2 = gemx::Philox::u01(r[1]);
    return (R)(sqrt(-2.0 * log(u1)) * cos(gemx::kTwoPi * u2));
}

struct RefgenDev {
    int32_t n_ref, len_lo, len_hi;
    uint64_t seed;
    int64_t env_base;  // gemx_refgen_config.env_base
    double log_sig_lo[GEMX_MAX_REF], log_sig_hi[GEMX_MAX_REF], m_lo[GEMX_MAX_REF], m_hi[GEMX_MAX_REF], i_lo[GEMX_MAX_REF], i_hi[GEMX_MAX_REF];
};

// SubepisodedReferenceGenerator.get_reference_observation, lines 104-111: a new sub-episode draws its length and its sigma
__device__ inline void new_subepisode(const RefgenDev &G, int64_t env, int g, uint32_t &n_sub, int32_t &left, double &sigma) {
    uint32_t r[4];
    refgen_block(G.seed, G.env_base + env, g, DRAW_SUB, n_sub++, r);
    // int((hi - lo) * U + lo), _get_current_value lines 116-119; then 10 ** U(log10 sigma_range), wiener ... line 31
    left = (int32_t)((double)(G.len_hi - G.len_lo) * gemx::Philox::u01(r[0]) + (double)G.len_lo);
    sigma = pow(10.0, (G.log_sig_hi[g] - G.log_sig_lo[g]) * gemx::Philox::u01(r[1]) + G.log_sig_lo[g]);
}
// WienerProcessReferenceGenerator.reset, lines 43-49: initial reference ~ U(initial_range); SubepisodedReferenceGenerator.reset 86-93
__device__ inline void reset_generator(const RefgenDev &G, int64_t env, int g, uint32_t &n_reset, uint32_t &n_sub, int32_t &left, double &sigma,
                                       double &value) {
    uint32_t r[4];
    refgen_block(G.seed, G.env_base + env, g, DRAW_RESET, n_reset++, r);
    value = (G.i_hi[g] - G.i_lo[g]) * gemx::Philox::u01(r[0]) + G.i_lo[g];
    left = 0;  // `_current_episode_length = -1`: the next get_reference_observation starts a sub-episode
    (void)n_sub; (void)sigma;
}
// one step of the clipped walk, wiener_process_reference_generator.py:35-41
__device__ inline double walk_step(const RefgenDev &G, int g, double value, double sigma, double z) {
    value += sigma * z;
    if (value > G.m_hi[g]) value = G.m_hi[g];
    if (value < G.m_lo[g]) value = G.m_lo[g];
    return value;
}

}  // namespace refgen_lane

// The complete policy rollout's view of an all-Wiener gemx_refgen (a kernel argument, by value): its description and its per-(column, env)
// arrays [n_ref][N].  The step's standard normals are NOT drawn in the lane: refgen_policy_normals fills refs_out with them in a launch in
// front (as gemx_refgen_rollout_shell does), the lane reads z from refs_out[k] and writes the reference over it; the step counters t move
// by K in the epilogue
struct PcWienerDev {
    const refgen_lane::RefgenDev *G;  // in DEVICE memory (the handle's copy): the lane reads the column it is at, when it is at it
    double *value, *sigma;
    int32_t *left;
    uint32_t *n_sub, *n_reset;
    uint64_t *t;
};
// gemx_refgen.hip: the view of a handle the kernel serves (its first call makes the description's device copy), GEMX_ERR_ARG (naming `what`)
// for any other -- a kinds, mixed or switched gemx_refgen; a handle of another n_envs, dtype (fp32 only), device or env_base
int refgen_policy_view(gemx_refgen *r, const char *what, int64_t n_envs, int device, int64_t env_base, PcWienerDev *out, int *n_ref);
int refgen_policy_normals(gemx_refgen *r, int32_t K, void *refs_out_dev, hipStream_t st);  // K * N * n_ref standard normals at the handle's step counters
}  // namespace gemx
