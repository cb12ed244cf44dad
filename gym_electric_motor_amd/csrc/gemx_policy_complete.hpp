// gemx_policy_complete.hpp -- the policy rollout of the COMPLETE env (gemx_rollout_policy_complete): what the C ABI (gemx_capi.hip), the
// generator units of libgemx.so (gemx_refgen.hip, gemx_refprofile.hip) and the complete policy rollout units (gemx_policy_complete.hip)
// share -- the kernel's by-value view of a generator handle, the functions that resolve it and the unit's entry point.
//
// The unit's kernel is policy_rollout_kernel (gemx_policy_kernel.hpp) with the reference generators stepped in the lane that steps the env: the actor of step k
// reads the reference row shown in front of step k (`shown` at k = 0, refs_out[k - 1] afterwards), and behind the row store of step k the
// lane restarts its generators where the episode ended, advances them and writes refs_out[k] -- the shell's order, which
// gemx_refgen_rollout_shell and gemx_refprofile_rollout_shell replay on the ENDED rows.  The generator state is not kept in registers
// across the actor: it is read from the handle's arrays behind the row store and written back at once (a lane touches its own words only).
#pragma once
#include "gemx_policy.hpp"
#include "gemx_refgen_lane.hpp"
#include "gemx_refprofile_lane.hpp"

namespace gemx {

constexpr int EP_LAUNCH_POLICY_COMPLETE = 8;  // gemx_handle::LastLaunch::pipe of policy_rollout_kernel with a generator; LastLaunch::il: the generator kind (PC_GEN_*, gemx_policy.hpp)

// (the kernel's views of the two generator handles, PcWienerDev and PcProfileDev, and the functions that resolve them stand beside the lane
// functions: gemx_refgen_lane.hpp, gemx_refprofile_lane.hpp)
struct PcRefs {
    const float *shown;  // [N][n_ref]: the references shown in front of step 0
    float *out;          // [K][N][n_ref]
};

}  // namespace gemx

// a complete policy rollout unit, libgemx_pc<S>_<C>.so (fp32): gemx_pc_unit_init as gemx_unit_init; gemx_pc_unit_launch as
// gemx_pl_unit_launch, with the references and exactly one of the two generator views (the other NULL)
typedef int (*gemx_pc_unit_launch_fn)(gemx_handle *h, const gemx::PolicyDev *pol, const gemx::PcRefs *refs, const gemx::PcWienerDev *wiener, const gemx::PcProfileDev *profile,
                                      int K, const int32_t *length, int32_t max_steps, void *obs, uint8_t *terminated, uint8_t *truncated, uint8_t *ended, hipStream_t st,
                                      int *linmap_built);
