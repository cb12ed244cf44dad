// gemx_refprofile_lane.hpp -- the per-lane functions of the profile references: the restart, the rows of a position, the 12 bytes of state
// of one env, and the declaration of THE row function (defined once, at the head of gemx_refprofile.hip).  gemx_refprofile.hip's kernels
// and the complete policy rollout units (gemx_policy_complete.hip), which show the profile in the lane that steps the env, call THESE
// functions: one definition each, hence the same rows bit for bit.  The rule itself is described at the head of gemx_refprofile.hip.
#pragma once
#include "gemx_common.hpp"

namespace gemx {
namespace profile_lane {

struct ProfileDev {  // uniform parameters, by value
    int32_t n_ref, T, per_env, interp, wrap, random;
    uint64_t seed;
    int64_t env_base, N;
    double ratio;  // tau / profile_tau
};

struct ProfileLane {
    int32_t k, s;
    uint32_t e;
};

constexpr uint32_t PROFILE_BLOCK_TAG = 0x50524F46u;  // "PROF": the block word of the start-row draw

__device__ __forceinline__ void profile_restart(const ProfileDev &P, int64_t env, ProfileLane &s) {
    s.k = 0;
    s.e += 1u;
    s.s = 0;
    if (P.random) {
        uint32_t r[4];
        gemx::Philox::block(P.seed, (uint64_t)(P.env_base + env), s.e, PROFILE_BLOCK_TAG, r);
        const int32_t row = (int32_t)(gemx::Philox::u01(r[0]) * (double)P.T);
        s.s = row < P.T - 1 ? row : P.T - 1;
    }
}

// the rows (ia, ib) in [0, T - 1] and the weight of the lane's position; whatever k and s hold (a counter that ran over, a foreign blob),
// the rows stay inside the table
__device__ __forceinline__ void profile_rows_of(const ProfileDev &P, const ProfileLane &s, int32_t &ia, int32_t &ib, double &w) {
    const double p = __dadd_rn((double)s.s, __dmul_rn((double)s.k, P.ratio));
    const int32_t last = P.T - 1;
    if (P.wrap) {
        const double fl = floor(p);
        w = p - fl;
        int64_t m = (int64_t)fl % (int64_t)P.T;
        if (m < 0) m += P.T;
        ia = (int32_t)m;
        ib = ia == last ? 0 : ia + 1;
    } else if (p >= (double)last) {
        ia = ib = last; w = 0.0;
    } else if (p >= 0.0) {
        const double fl = floor(p);
        w = p - fl;
        ia = (int32_t)fl;
        ib = ia + 1;
    } else {
        ia = ib = 0; w = 0.0;
    }
}

// one step of one env: the n_ref values at the lane's position into row[], then k += 1.  `active`: the lane has an env (all 64 lanes of a
// wave come here together: its vote needs them).  THE row function is DEFINED in gemx_refprofile.hip, once, in the section at that file's
// head; a unit outside libgemx.so that calls it includes this header and then that section (GEMX_REFPROFILE_ROW_ONLY)
template <class R>
__device__ __forceinline__ void profile_row(const ProfileDev &P, const R *__restrict__ tab, int64_t env, bool active, ProfileLane &s, R (&row)[GEMX_MAX_REF]);

__device__ __forceinline__ ProfileLane profile_load(const int32_t *__restrict__ st, int64_t N, int64_t env) {
    return {st[env], st[N + env], (uint32_t)st[2 * N + env]};
}
__device__ __forceinline__ void profile_save(int32_t *__restrict__ st, int64_t N, int64_t env, const ProfileLane &s) {
    st[env] = s.k; st[N + env] = s.s; st[2 * N + env] = (int32_t)s.e;
}

}  // namespace profile_lane

// The complete policy rollout's view of a gemx_refprofile (a kernel argument, by value): its description, its table and its state [3][N]
struct PcProfileDev {
    profile_lane::ProfileDev P;
    const float *tab;
    int32_t *state;
};
// gemx_refprofile.hip: the view of a handle the kernel serves, GEMX_ERR_ARG (naming `what`) for a handle of another n_envs, dtype (fp32
// only), device or env_base
int refprofile_policy_view(gemx_refprofile *p, const char *what, int64_t n_envs, int device, int64_t env_base, PcProfileDev *out);
}  // namespace gemx
