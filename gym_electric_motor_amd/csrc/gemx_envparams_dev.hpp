// gemx_envparams_dev.hpp -- the device helpers the per-env kernel units (gemx_envparams.hip) and the episodic rollout units
// (gemx_episodic.hip) share: the lane's column of a parameter table, its per-lane view of DevParams, the row store of a single-wave
// kernel, and the action stage + control step of one lane.  One definition, so that a lane with a table computes the same bits in every
// kernel that reads it.
#pragma once
#include "gemx_kernels.hpp"
#include "gemx_envparams.hpp"

namespace gemx {

// the lane's column of the table: F loads of consecutive words per wave and field, all issued before anything waits
template <int SYS, class R> __device__ __forceinline__ void ep_load(const R *__restrict__ tab, int64_t N, int64_t e, R (&c)[ep_fields(SYS)]) {
#pragma unroll
    for (int f = 0; f < ep_fields(SYS); ++f) c[f] = tab[(int64_t)f * N + e];
}
// ... into the per-lane view of the parameters.  P.kink_split carries the handle's FLAG here (GEMX_SOLVER_SPLIT_KINKS behind a
// PolynomialStaticLoad); whether a lane's load has a kink at all is that lane's omega_lim > 0, as fill_params decides it for a handle
template <int SYS, class R> __device__ __forceinline__ void ep_apply(const R (&c)[ep_fields(SYS)], DevParams<R> &PL) {
    constexpr int NM = ep_model_entries(SYS);
#pragma unroll
    for (int i = 0; i < NM; ++i) PL.m[i] = c[i];
    PL.tc0 = c[NM]; PL.tc1 = c[NM + 1]; PL.tc2 = c[NM + 2]; PL.tc3 = c[NM + 3];
    PL.inv_j = c[NM + 4]; PL.la = c[NM + 5]; PL.lb = c[NM + 6]; PL.lc = c[NM + 7];
    PL.omega_lim = c[NM + 8]; PL.lin_factor = c[NM + 9]; PL.inv_tau_decay = c[NM + 10];
    PL.u_sup = c[NM + 11];
    PL.kink_split = PL.kink_split != 0 && PL.omega_lim > R(0);
}

// one observation row from the lane's registers (step_kernel's stores: a row is NOUT * sizeof(R) contiguous bytes)
template <int NOUT, class R> __device__ __forceinline__ void ep_store_row(const DevParams<R> &P, R *obs_k, int64_t N, int64_t env, const R (&obs)[NOUT]) {
    if (P.obs_layout == GEMX_OBS_AOS) {
        R *row = obs_k + env * NOUT;
        constexpr int W = (NOUT * sizeof(R)) % 16 == 0 ? 16 / sizeof(R) : ((NOUT * sizeof(R)) % 8 == 0 ? 8 / sizeof(R) : 1);  // row alignment
        typedef R vec_t __attribute__((ext_vector_type(W)));
        if constexpr (W > 1) {
#pragma unroll
            for (int j = 0; j < NOUT; j += W) {
                vec_t v;
#pragma unroll
                for (int q = 0; q < W; ++q) v[q] = obs[j + q];
                *reinterpret_cast<vec_t *>(row + j) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NOUT; ++j) row[j] = obs[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) obs_k[(int64_t)j * N + env] = obs[j];
    }
}

// the action stage and the control step of one lane, exactly as step_kernel / compute_block do them (no DeadTimeProcessor, no RC supply)
template <int SYS, int CONV, int LOAD, int SOLVER, class R>
__device__ __forceinline__ bool ep_control_step(const DevParams<R> &P, const DevParams<R> &PL, R (&y)[SysTraits<SYS>::ND], typename Angle<R>::T &ang,
                                                R (&act)[MAX_ACT], uint32_t dact, uint32_t &bad_action, R (&obs)[SysTraits<SYS>::NOUT]) {
    constexpr int ND = SysTraits<SYS>::ND, NOUT = SysTraits<SYS>::NOUT;
    using ST = Stepper<SYS, conv_base<CONV>(), LOAD, SOLVER, false, R>;
    if (ConvTraits<CONV>::DISCRETE) { bad_action |= dact >= (uint32_t)ConvTraits<CONV>::NACTIONS; dact &= (uint32_t)(ConvTraits<CONV>::NACTIONS - 1); }
    if (conv_dq<CONV>()) dq_action_stage<SYS, CONV, R>(P, y, ang, act);  // (either frame: without a delay queue both orders are this one)
    uint32_t sw = 0;
    R hcar = R(0);
    full_step<ST, ND, NOUT, R, false>(PL, y, ang, sw, act, dact, obs, nullptr, &hcar);
    return constraint_done<ST, NOUT, R>(P, obs);
}

}  // namespace gemx
