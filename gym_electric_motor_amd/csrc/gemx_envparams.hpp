// gemx_envparams.hpp -- per-env motor / load / supply parameters (domain randomisation): what the C ABI (gemx_capi.hip) and the per-env
// kernel units (gemx_envparams.hip) share.
//
// A handle with a parameter TABLE steps every env with its own machine: the table is [F][N] R on the device, field-major (a wave's loads of
// one field are 64 consecutive words), and holds the DevParams members that depend on machine, load and supply, in this order:
//   m[0 .. n)        the system's packed model entries (pack_model: n = ep_model_entries(system))
//   tc0 .. tc3       torque coefficients
//   inv_j, la, lb, lc, omega_lim, lin_factor, inv_tau_decay      PolynomialStaticLoad
//   u_sup            IdealVoltageSupply
// Everything else of DevParams stays one value per handle (kernel argument -> SGPRs): tau, pole, inv_lim, dc_thr, init, the constraint kind,
// the solver settings, the action frame.
#pragma once
#include "gemx_common.hpp"

namespace gemx {

constexpr int EP_TAIL = 12;  // tc0..tc3, inv_j, la, lb, lc, omega_lim, lin_factor, inv_tau_decay, u_sup
constexpr int ep_model_entries(int sys) {
    return sys == GEMX_SYS_DC_PERMEX || sys == GEMX_SYS_DC_SERIES ? 3
           : sys == GEMX_SYS_DC_SHUNT || sys == GEMX_SYS_DC_EXTEX ? 5
           : sys == GEMX_SYS_SYNC                                  ? 7
           : sys == GEMX_SYS_DFIM                                  ? 18
                                                                   : 14;  // EESM, SCIM
}
constexpr int ep_fields(int sys) { return ep_model_entries(sys) + EP_TAIL; }

// gemx_handle::LastLaunch::pipe of the two per-env kernels (0 advance_kernel, 1 advance_pipe_kernel, 2 step_kernel, 3 dc_stream_kernel)
constexpr int EP_LAUNCH_STEP = 4, EP_LAUNCH_ROLLOUT = 5;
// ... and of the episodic rollout kernel (gemx_episodic.hip: K steps with the episode time limit inside the launch); LastLaunch::d is 1
// when the launch read the handle's parameter table, LastLaunch::s the time limit
constexpr int EP_LAUNCH_EPISODIC = 6;

}  // namespace gemx

// a per-env unit, libgemx_ep<S>_<C>.so (fp32): gemx_ep_unit_init as gemx_unit_init; gemx_ep_unit_launch runs K >= 1 control steps of every env
// with the parameters of the handle's table (gemx_handle::envp; K == 1 without a fused reward: envparams_step_kernel, else envparams_rollout_kernel), every step's row stored
typedef int (*gemx_ep_unit_launch_fn)(gemx_handle *h, const gemx::RolloutCall &call, hipStream_t st);

// an episodic rollout unit, libgemx_tl<S>_<C>.so (fp32): gemx_tl_unit_init as gemx_unit_init; gemx_tl_unit_launch runs K >= 1 control steps
// of every env with the episode time limit `max_steps` inside the launch (episodic_rollout_kernel): length [N] is read, never written;
// terminated / truncated / ended [K][N] may each be null.  With a table on the handle (gemx_handle::envp) every lane steps with its column.
// *linmap_built is set when this launch built the handle's one-step map (the caller's coverage note)
typedef int (*gemx_tl_unit_launch_fn)(gemx_handle *h, const void *actions, int K, const int32_t *length, int32_t max_steps, void *obs, uint8_t *terminated,
                                      uint8_t *truncated, uint8_t *ended, hipStream_t st, int *linmap_built);
