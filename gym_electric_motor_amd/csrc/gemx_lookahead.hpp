// gemx_lookahead.hpp -- one-step finite-control-set predictive control inside the fused rollout launch (gemx_rollout_lookahead_complete):
// what the C ABI (gemx_capi.hip) and the lookahead units (gemx_lookahead.hip, libgemx_la<S>_<C>.so) share -- the part of a call the
// rollout call record (RolloutCall, gemx_common.hpp) does not carry, and the unit's entry point.
//
// The unit's kernel is episodic_rollout_kernel (gemx_episodic.hip) with the action of step k not read from a tensor but CHOSEN in the
// lane: every one of the converter's NACTIONS switching actions is stepped once from the state the step starts at, each outcome is scored
// with the env's own reward (reward_row, gemx_reward.hpp) against the references shown in front of step k, and the lowest index among the
// maxima of score + noise is taken -- the policy kernel's selection rule.  The generators are stepped in the lane as in the complete
// policy rollout (gemx_policy_complete.hip), so everything behind the launch is that rollout's too.
#pragma once
#include "gemx_policy_complete.hpp"

namespace gemx {

constexpr int EP_LAUNCH_LOOKAHEAD = 9;  // gemx_handle::LastLaunch::pipe of lookahead_rollout_kernel; LastLaunch::il: the generator kind (PC_GEN_*, gemx_policy.hpp)

// Beside a RolloutCall {K, obs [K][N][S_out], done = terminated [K][N], refs = the row shown in front of step 0 [N][n_ref]}:
struct LaCall {
    const int32_t *length;  // [N]: the episode stage's counters, read only
    int32_t max_steps;
    int32_t n_ref;
    uint8_t *truncated, *ended;  // [K][N]; may be null
    float *refs_out;             // [K][N][n_ref]
    uint8_t *actions_out;        // [K][N]: the flat action index taken
    float *scores_out;           // [K][N][NACTIONS]: the scores in front of `+ noise`; may be null
    const float *noise;          // [K][N][NACTIONS]; may be null
    const PcWienerDev *wiener;   // exactly one of the two generator views
    const PcProfileDev *profile;
    int *linmap_built;
};

}  // namespace gemx

// a lookahead unit, libgemx_la<S>_<C>.so (fp32, finite converters only): gemx_la_unit_init as gemx_unit_init; gemx_la_unit_launch runs
// K >= 1 control steps of every env, each on the best of the converter's actions one step ahead
typedef int (*gemx_la_unit_launch_fn)(gemx_handle *h, const gemx::RolloutCall *call, const gemx::LaCall *la, hipStream_t st);
