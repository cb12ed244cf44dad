// gemx_policy_complete.hip -- ONE complete policy rollout unit: policy_rollout_kernel (gemx_policy_kernel.hpp) with the env's own reference
// generators stepped in the lane that steps the env (gemx_rollout_policy_complete), for one (system, converter unit), fp32, built as its
// own shared object
//   hipcc -DGEMX_INST_SYS=<0..7> -DGEMX_INST_CONV=<0..11> -shared gemx_policy_complete.hip -o libgemx_pc<S>_<C>.so
// and loaded with dlopen by the first gemx_rollout_policy_complete of such a handle (gemx_capi.hip: load_pc_unit).  The policy units
// (libgemx_pl<S>_<C>.so) are untouched.
//
// The kernel and its launcher are the policy units' (gemx_policy_kernel.hpp), instantiated with a generator kind, GEN = PC_GEN_WIENER (an
// all-Wiener gemx_refgen) or PC_GEN_PROFILE (a gemx_refprofile).  What GEN changes in the kernel:
//   * the references the actor of step k reads are not row k of a given tensor but the row the env SHOWED in front of step k: `shown`
//     [N][n_ref] at k = 0, refs_out[k - 1] afterwards -- the fp32 words this lane stored, re-read;
//   * behind the row store of step k the lane restarts its generators if the step ended the episode, advances them and stores
//     refs_out[k] (pc_references, below) -- the shell's order (restart first, then advance), which gemx_refgen_rollout_shell and
//     gemx_refprofile_rollout_shell replay on the ENDED rows.  The lane functions are the generator units' own (gemx_refgen_lane.hpp,
//     gemx_refprofile_lane.hpp), so the rows and the state left behind are theirs bit for bit.
//
// Where the generator state lives: in the handle's arrays, not in registers.  The policy kernels already fill the register file
// (profiles/policy_rollout.md), so the 36 bytes per Wiener column (value, sigma, left, n_sub, n_reset; t is not needed, below) and the 12
// bytes per env of a profile are read behind the row store, used and written back at once; a lane touches its own words only, they stay
// in L2 between steps, and against the actor's FMAs the traffic is nothing.  A compiler barrier at the top of the step keeps the
// optimiser from promoting them to loop-carried registers.  The Wiener step's double log / sqrt / cos do not run here either:
// refgen_normals_kernel fills refs_out with the K * N * n_ref standard normals in a launch in front (what gemx_refgen_rollout_shell does),
// the lane reads z from refs_out[k] and writes the reference over it, and the step counters move by K in the epilogue.  The rare paths
// (new_subepisode's pow, reset_generator) stay in the lane.  The profile's wave-uniform table read is kept: tail lanes recompute env
// N - 1 (their stores masked), so all 64 lanes arrive at the vote.  What this compiles to: profiles/policy_complete_rollout.md.
#include "gemx_policy_kernel.hpp"
#include "gemx_policy_complete.hpp"
#define GEMX_REFPROFILE_ROW_ONLY  // the head section of gemx_refprofile.hip: the one definition of profile_row
#include "gemx_refprofile.hip"

#if !defined(GEMX_INST_SYS) || !defined(GEMX_INST_CONV)
#error "define GEMX_INST_SYS and GEMX_INST_CONV"
#endif

namespace gemx {
// Row k of the references, behind the row store of step k: restart where the episode ended, advance, store.  Everything is read from the
// handle's arrays and written back here (a lane touches the words of its own env only); nothing of it is live across the actor.
// Lanes behind N take no part -- but for the profile's wave vote, which all 64 lanes reach together.
// (Dev: PcWienerDev with GEN = PC_GEN_WIENER, PcProfileDev with PC_GEN_PROFILE)
template <int GEN, class Dev>
__device__ __forceinline__ void pc_references(const Dev &gen, float *__restrict__ refs_out, int64_t N, int n_ref, int k, int64_t env, bool valid, bool end) {
    if constexpr (GEN == PC_GEN_WIENER) {
        using namespace refgen_lane;
        // (the description is read from device memory, one column after the other in a rolled loop: as a kernel argument its columns'
        // ranges were computed in front of the K-step loop and carried through the actor in registers, and indexed by a runtime column
        // it went to scratch)
        const RefgenDev &G = *gen.G;
        if (!valid) return;
#pragma unroll 1
        for (int g = 0; g < n_ref; ++g) {
            const int64_t si = (int64_t)g * N + env, o = ((int64_t)k * N + env) * n_ref + g;
            double v = gen.value[si], sg = gen.sigma[si];
            int32_t lf = gen.left[si];
            if (end) {
                uint32_t nr = gen.n_reset[si], ns = 0u;
                reset_generator(G, env, g, nr, ns, lf, sg, v);
                gen.n_reset[si] = nr;
            }
            if (lf <= 0) {
                uint32_t ns = gen.n_sub[si];
                new_subepisode(G, env, g, ns, lf, sg);
                gen.n_sub[si] = ns;
                gen.sigma[si] = sg;
            }
            v = walk_step(G, g, v, sg, (double)refs_out[o]);  // (z: refgen_normals_kernel left it there)
            --lf;
            gen.value[si] = v;
            gen.left[si] = lf;
            refs_out[o] = (float)v;
        }
    } else {
        using namespace profile_lane;
        const ProfileDev &P = gen.P;
        ProfileLane s = {0, 0, 0u};
        float row[GEMX_MAX_REF];
        if (valid) {
            s = profile_load(gen.state, N, env);
            if (end) profile_restart(P, env, s);
        }
        profile_row<float>(P, gen.tab, env, valid, s, row);
        if (valid) {
            profile_save(gen.state, N, env, s);
#pragma unroll
            for (int g = 0; g < GEMX_MAX_REF; ++g)
                if (g < n_ref) refs_out[((int64_t)k * N + env) * n_ref + g] = row[g];
        }
    }
}

struct PcGen {  // launch_policy_t's V: the references and exactly one of the two generator views
    const PcRefs *refs;
    const PcWienerDev *wiener;
    const PcProfileDev *profile;
    static constexpr const char *WHAT = "complete policy rollout";
    static constexpr int PIPE = EP_LAUNCH_POLICY_COMPLETE;
    int kind() const { return wiener != nullptr ? PC_GEN_WIENER : PC_GEN_PROFILE; }
    template <int SYS, int CONV, int LOAD, int SOLVER, bool TAB> void launch(const PolicyLaunch &l) const {
        if (wiener != nullptr) launch_policy_kernel<SYS, CONV, LOAD, SOLVER, TAB, PC_GEN_WIENER>(l, *refs, *wiener);
        else launch_policy_kernel<SYS, CONV, LOAD, SOLVER, TAB, PC_GEN_PROFILE>(l, *refs, *profile);
    }
};
}  // namespace gemx

extern "C" {
__attribute__((visibility("default"))) int gemx_pc_unit_init(unsigned long long handle_bytes, int abi, void (*set_error)(const char *)) {
    return gemx::unit_init(handle_bytes, abi, set_error);
}
__attribute__((visibility("default"))) int gemx_pc_unit_launch(gemx_handle *h, const gemx::PolicyDev *pol, const gemx::PcRefs *refs, const gemx::PcWienerDev *wiener,
                                                               const gemx::PcProfileDev *profile, int K, const int32_t *length, int32_t max_steps, void *obs, uint8_t *terminated,
                                                               uint8_t *truncated, uint8_t *ended, hipStream_t st, int *linmap_built) {
    if (h->envp != nullptr && h->envp_fields != gemx::ep_fields(GEMX_INST_SYS)) return gemx::fail(GEMX_ERR_ARG, "internal: complete policy rollout unit launched with another system's table");
    if ((wiener != nullptr) == (profile != nullptr)) return gemx::fail(GEMX_ERR_ARG, "internal: complete policy rollout unit launched without exactly one generator view");
    const gemx::PolicyCall c = {pol, K, length, max_steps, obs, terminated, truncated, ended, linmap_built};
    return gemx::launch_policy_unit<GEMX_INST_SYS, GEMX_INST_CONV>(h, c, gemx::PcGen{refs, wiener, profile}, st);
}
}
