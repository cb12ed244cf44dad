// gemx_lookahead.hip -- ONE lookahead rollout unit: K control steps per launch, each on the BEST of the converter's switching actions one
// step ahead (one-step finite-control-set model predictive control), with the episode time limit, the env's reference generators and the
// scores inside the launch (gemx_rollout_lookahead_complete), for one (system, FINITE converter unit), fp32, built as its own shared object
//   hipcc -DGEMX_INST_SYS=<0..7> -DGEMX_INST_CONV=<1|3|5|7|9> -shared gemx_lookahead.hip -o libgemx_la<S>_<C>.so
// and loaded with dlopen by the first gemx_rollout_lookahead_complete of such a handle (gemx_capi.hip: load_la_unit).  Every other unit is
// untouched.
//
// Shape: episodic_rollout_kernel's -- one lane per env, no LDS, no barrier; state, angle, episode counter, the references shown and (TAB)
// the lane's table column in registers across the K steps.  Control step k:
//   for a = 0 .. NACTIONS-1, a ROLLED runtime loop (one copy of the step's code, whatever NACTIONS is):
//       (yt, angt) = (y, ang);  the episodic kernel's control step with action a -> row_a, done_a
//           (the one-step map decided ONCE per control step, on the state the step starts from, as the episodic kernel decides it)
//       score[a] = reward_row(row_a, the references shown in front of step k, done_a)      -- gemx_reward.hpp, THE definition
//       the running choice: a == 0, or score[a] + noise[k][env][a] > the best so far       -- the lowest index among the maxima
//       where chosen, (yt, angt, row_a, done_a) are kept in registers of their own
//   commit the kept trial: nothing is recomputed, so the stored row is the scored row
//   then episodic_rollout_kernel's tail, statement for statement: the pin of the stepped state, episode_row's rule, the row store in
//   front of the restart; then the generators (restart where the episode ended, advance, refs_out[k]) and the uint8 action.
// The reward description reaches the kernel as the reward pass passes it: RewardHot and RewardDev by value, i.e. scalar loads.
//
// The references: la_references steps the generators with the lane functions the generator units and the complete policy units call
// (gemx_refgen_lane.hpp, gemx_refprofile_lane.hpp), in pc_references' order, and hands the row back in registers: it is what step k + 1
// scores against.  The generator state itself is read from the handle's arrays behind the row store and written back at once, and the
// Wiener step's standard normals come from refgen_normals_kernel's launch in front, through refs_out -- both as in the complete policy
// rollout, so the state left behind is gemx_refgen_rollout_shell's / gemx_refprofile_rollout_shell's bit for bit.
// Tail lanes recompute env N - 1 (every load at its index, every store masked): the lanes of a wave run in lockstep, a lane's loads of a
// step have returned before the stores that depend on them are issued, so the tail lanes see what lane N - 1 sees and all 64 lanes arrive
// at the profile's wave vote.
#include "gemx_kernels.hpp"
#include "gemx_unit_host.hpp"
#include "gemx_envparams.hpp"
#include "gemx_envparams_dev.hpp"
#include "gemx_lookahead.hpp"
#define GEMX_REFPROFILE_ROW_ONLY  // the head section of gemx_refprofile.hip: the one definition of profile_row
#include "gemx_refprofile.hip"

#if !defined(GEMX_INST_SYS) || !defined(GEMX_INST_CONV)
#error "define GEMX_INST_SYS and GEMX_INST_CONV"
#endif

namespace gemx {
// (the tail lanes' reads of env N - 1's words, above, are ordered against lane N - 1's stores only inside ONE wave)
static_assert(BLOCK == 64, "a workgroup is one wave: the tail lanes and the lane of env N - 1 run in lockstep");

// column `col` of a row in registers (as AND / OR on the bit patterns: a dynamic index would put the row into scratch, and a chain of
// selects is folded back into one -- gemx_envparams.hip: ep_pick)
template <int NOUT> __device__ __forceinline__ float la_pick(const float (&obs)[NOUT], int col) {
    uint32_t v = 0u;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) v |= __builtin_bit_cast(uint32_t, obs[j]) & (col == j ? 0xFFFFFFFFu : 0u);
    return __builtin_bit_cast(float, v);
}

// Row k of the references, behind the row store of step k: restart where the episode ended, advance, store -- and the row back in rv.
// e: the env whose words are read (N - 1 in a tail lane); valid: the lane stores.  (Dev: PcWienerDev | PcProfileDev)
template <int GEN, class Dev>
__device__ __forceinline__ void la_references(const Dev &gen, float *refs_out, int64_t N, int n_ref, int k, int64_t e, bool valid, bool end, float (&rv)[GEMX_MAX_REF]) {
    if constexpr (GEN == PC_GEN_WIENER) {
        using namespace refgen_lane;
        const RefgenDev &G = *gen.G;  // (in device memory, one column after the other in a rolled loop: pc_references has the reason)
        uint32_t rb[GEMX_MAX_REF];
#pragma unroll
        for (int j = 0; j < GEMX_MAX_REF; ++j) rb[j] = 0u;
#pragma unroll 1
        for (int g = 0; g < n_ref; ++g) {
            const int64_t si = (int64_t)g * N + e, o = ((int64_t)k * N + e) * n_ref + g;
            double v = gen.value[si], sg = gen.sigma[si];
            int32_t lf = gen.left[si];
            const float z = refs_out[o];  // (refgen_normals_kernel left it there)
            if (end) {
                uint32_t nr = gen.n_reset[si], ns = 0u;
                reset_generator(G, e, g, nr, ns, lf, sg, v);
                if (valid) gen.n_reset[si] = nr;
            }
            if (lf <= 0) {
                uint32_t ns = gen.n_sub[si];
                new_subepisode(G, e, g, ns, lf, sg);
                if (valid) { gen.n_sub[si] = ns; gen.sigma[si] = sg; }
            }
            v = walk_step(G, g, v, sg, (double)z);
            --lf;
            const float shown = (float)v;
            if (valid) {
                gen.value[si] = v;
                gen.left[si] = lf;
                refs_out[o] = shown;
            }
#pragma unroll
            for (int j = 0; j < GEMX_MAX_REF; ++j) rb[j] |= __builtin_bit_cast(uint32_t, shown) & (j == g ? 0xFFFFFFFFu : 0u);  // (rv[g], without a dynamic index)
        }
#pragma unroll
        for (int j = 0; j < GEMX_MAX_REF; ++j) rv[j] = __builtin_bit_cast(float, rb[j]);
    } else {
        using namespace profile_lane;
        const ProfileDev &P = gen.P;
        ProfileLane s = profile_load(gen.state, N, e);
        if (end) profile_restart(P, e, s);
        float row[GEMX_MAX_REF];
#pragma unroll
        for (int g = 0; g < GEMX_MAX_REF; ++g) row[g] = 0.0f;
        profile_row<float>(P, gen.tab, e, true, s, row);
        if (valid) {
            profile_save(gen.state, N, e, s);
#pragma unroll
            for (int g = 0; g < GEMX_MAX_REF; ++g)
                if (g < n_ref) refs_out[((int64_t)k * N + e) * n_ref + g] = row[g];
        }
#pragma unroll
        for (int g = 0; g < GEMX_MAX_REF; ++g) rv[g] = g < n_ref ? row[g] : 0.0f;
    }
}

// what the lookahead adds to the episodic kernel's arguments
struct LaDev {
    const float *shown;    // [N][n_ref]: the references shown in front of step 0
    float *refs_out;       // [K][N][n_ref]
    uint8_t *actions_out;  // [K][N]
    float *scores;         // [K][N][NACTIONS] | nullptr
    const float *noise;    // [K][N][NACTIONS] | nullptr
    int32_t n_ref;
};

template <int SYS, int CONV, int LOAD, int SOLVER, bool TAB, int GEN, class Dev>
__global__ __launch_bounds__(BLOCK) void lookahead_rollout_kernel(const KArgs<float> a, const float *__restrict__ tab, const int32_t *__restrict__ length_in, const int32_t M,
                                                                  uint8_t *__restrict__ truncated, uint8_t *__restrict__ ended, const LaDev la, const RewardDev<float> W,
                                                                  const Dev gen) {
    using R = float;
    static_assert(ConvTraits<CONV>::DISCRETE, "the lookahead enumerates a finite action set");
    constexpr int ND = SysTraits<SYS>::ND, NOUT = SysTraits<SYS>::NOUT, NA = ConvTraits<CONV>::NACTIONS, HOT = GEMX_REWARD_HOT;
    constexpr bool LINABLE = !TAB && linable<SYS, LOAD, SOLVER, false, R>();
    using AngT = typename Angle<R>::T;
    using ST = Stepper<SYS, conv_base<CONV>(), LOAD, SOLVER, false, R>;
    const DevParams<R> &P = a.P;
    const RewardHot<R> &H = a.rh;
    const int64_t N = a.N;
    const int K = a.K;
    const int64_t env = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool valid = env < N;
    const int64_t e = valid ? env : N - 1;  // tail lanes recompute the last env; their stores are masked

    // ---- prologue: state, angle, the episode counter, the references shown, the lane's table column -- one batch of loads
    R y[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) y[j] = a.state[(int64_t)j * N + e];
    AngT ang = AngT(0);
    if (SysTraits<SYS>::HAS_ANGLE) ang = a.angle[e];
    int32_t length = length_in[e];
    R rv[GEMX_MAX_REF];
#pragma unroll
    for (int r = 0; r < GEMX_MAX_REF; ++r) rv[r] = r < la.n_ref ? la.shown[e * la.n_ref + r] : R(0);
    // per-lane view: the table's fields (TAB), else the handle's own values -- the kernel argument itself, not a copy of it
    // (policy_rollout_kernel has the reason)
    DevParams<R> PT;
    if constexpr (TAB) {
        PT = P;
        R col[ep_fields(SYS)];
        ep_load<SYS, R>(tab, N, e, col);
        ep_apply<SYS, R>(col, PT);
    }
    const DevParams<R> &PL = TAB ? PT : P;
    const AngT init_ang = Angle<R>::from_bits(P.init_angle_rep);

    for (int k = 0; k < K; ++k) {
        // ---- the trials.  (a compiler barrier, no instruction: the generator state is re-read from memory behind the row store, not
        // carried through the trials in registers)
        asm volatile("" ::: "memory");
        bool lin_ok = false;
        if constexpr (!TAB) lin_ok = lin_usable<SYS, LOAD, SOLVER, false, R>(P, y[0]);  // wave-uniform; ONE decision per control step
        const int64_t at_a = ((int64_t)k * N + e) * NA;
        R by[ND], obs[NOUT];  // the kept trial: its state and its row
#pragma unroll
        for (int j = 0; j < ND; ++j) by[j] = y[j];
#pragma unroll
        for (int c = 0; c < NOUT; ++c) obs[c] = R(0);
        AngT bang = ang;
        bool done = false;
        R best_score = R(0);
        uint32_t best = 0;
#pragma unroll 1
        for (uint32_t ai = 0; ai < (uint32_t)NA; ++ai) {
            R yt[ND], ot[NOUT], act[MAX_ACT];
#pragma unroll
            for (int j = 0; j < ND; ++j) yt[j] = y[j];
#pragma unroll
            for (int i = 0; i < MAX_ACT; ++i) act[i] = R(0);
            AngT angt = ang;
            bool dt;
            if constexpr (TAB) {
                uint32_t bad = 0;  // (ai < NACTIONS)
                dt = ep_control_step<SYS, CONV, LOAD, SOLVER, R>(P, PL, yt, angt, act, ai, bad, ot);
            } else {  // step_kernel's control step, as episodic_rollout_kernel takes it
                uint32_t sw = 0;
                R hcar = R(0);
                if (LINABLE && lin_ok) full_step<ST, ND, NOUT, R, LINABLE>(PL, yt, angt, sw, act, ai, ot);
                else full_step<ST, ND, NOUT, R, false>(PL, yt, angt, sw, act, ai, ot, nullptr, &hcar);
                dt = constraint_done<ST, NOUT, R>(P, ot);
            }
            // the stepped trial state pinned in registers of its own (episodic_rollout_kernel has the story of the coalescer): the trial
            // copy is merged into the kept one below, which is exactly where a merged register would hurt
#pragma unroll
            for (int j = 0; j < ND; ++j) asm volatile("" : "+v"(yt[j]));

            R oh[HOT];
#pragma unroll
            for (int t = 0; t < HOT; ++t) oh[t] = la_pick<NOUT>(ot, H.col[t]);
            const R score = reward_row<R>(H, &W, oh, [&](int c) { return la_pick<NOUT>(ot, c); }, rv, dt);
            if (valid && la.scores != nullptr) la.scores[at_a + ai] = score;
            const R noisy = score + (la.noise != nullptr ? la.noise[at_a + ai] : R(0));
            const bool take = ai == 0u || noisy > best_score;  // the lowest index among the maxima
            best_score = take ? noisy : best_score;
            best = take ? ai : best;
            done = take ? dt : done;
            bang = take ? angt : bang;
#pragma unroll
            for (int j = 0; j < ND; ++j) by[j] = take ? yt[j] : by[j];
#pragma unroll
            for (int c = 0; c < NOUT; ++c) obs[c] = take ? ot[c] : obs[c];
        }
        // ---- commit the kept trial
#pragma unroll
        for (int j = 0; j < ND; ++j) y[j] = by[j];
        ang = bang;

        // ---- from here on: episodic_rollout_kernel's step, statement for statement
#pragma unroll
        for (int j = 0; j < ND; ++j) asm volatile("" : "+v"(y[j]));

        // ---- episode_row's rule on the lane's own counter
        length += 1;
        const bool trunc = length >= M && !done;  // (done and limit at once: terminated)
        const bool end = done | trunc;
        if (end) {  // `env.reset()`: the initial state is one per handle; the switching state survives
            length = 0;
#pragma unroll
            for (int j = 0; j < ND; ++j) y[j] = P.init[j];
            ang = init_ang;
        }

        if (valid) {
            ep_store_row<NOUT, R>(P, a.obs + (int64_t)k * N * NOUT, N, env, obs);
            const int64_t at = (int64_t)k * N + env;
            if (a.done != nullptr) a.done[at] = done ? 1 : 0;
            if (truncated != nullptr) truncated[at] = trunc ? 1 : 0;
            if (ended != nullptr) ended[at] = end ? 1 : 0;
            la.actions_out[at] = (uint8_t)best;
        }
        // ---- the references: the generators of an env that ended restart, then every generator advances -> refs_out[k], and rv
        la_references<GEN>(gen, la.refs_out, N, la.n_ref, k, e, valid, end, rv);
    }

    if (valid) {
#pragma unroll
        for (int j = 0; j < ND; ++j) a.state[(int64_t)j * N + env] = y[j];
        if (SysTraits<SYS>::HAS_ANGLE) a.angle[env] = ang;
        if constexpr (GEN == PC_GEN_WIENER) {  // the index of the normal draws: K steps on (refgen_walk_kernel's last line)
#pragma unroll
            for (int r = 0; r < GEMX_MAX_REF; ++r)
                if (r < la.n_ref) gen.t[(int64_t)r * N + env] += (uint64_t)K;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host launcher
// ------------------------------------------------------------------------------------------------
template <int SYS, int CONV, int LOAD, int SOLVER, bool TAB>
static void launch_la_kernel(const KArgs<float> &a, const float *tab, const LaCall &c, const LaDev &la, const RewardDev<float> &W, unsigned blocks, hipStream_t st) {
    if (c.wiener != nullptr)
        hipLaunchKernelGGL((lookahead_rollout_kernel<SYS, CONV, LOAD, SOLVER, TAB, PC_GEN_WIENER, PcWienerDev>), dim3(blocks), dim3(BLOCK), 0, st, a, tab, c.length, c.max_steps,
                           c.truncated, c.ended, la, W, *c.wiener);
    else
        hipLaunchKernelGGL((lookahead_rollout_kernel<SYS, CONV, LOAD, SOLVER, TAB, PC_GEN_PROFILE, PcProfileDev>), dim3(blocks), dim3(BLOCK), 0, st, a, tab, c.length, c.max_steps,
                           c.truncated, c.ended, la, W, *c.profile);
}

template <int SYS, int CONV, int LOAD, int SOLVER>
static int launch_la_t(gemx_handle *h, const RolloutCall &call, const LaCall &c, hipStream_t st) {
    using R = float;
    const bool tab = h->envp != nullptr;
    if (const int rc = ensure_linmap<SYS, LOAD, SOLVER>(h, st, c.linmap_built)) return rc;
    KArgs<R> a;
    fill_unit_kargs<LOAD>(a, h, tab, call.K, call.obs, call.done);  // (tab: the episodic launcher's view of a handle with a table)
    a.rh = h->rh_f;
    const LaDev la = {(const float *)call.refs, c.refs_out, c.actions_out, c.scores_out, c.noise, c.n_ref};
    const int64_t blocks = (h->n + BLOCK - 1) / BLOCK;
    if (tab) launch_la_kernel<SYS, CONV, LOAD, SOLVER, true>(a, (const R *)h->envp, c, la, h->rw_f, (unsigned)blocks, st);
    else launch_la_kernel<SYS, CONV, LOAD, SOLVER, false>(a, nullptr, c, la, h->rw_f, (unsigned)blocks, st);
    GEMX_HIP_TRY(hipGetLastError());
    h->ll = {EP_LAUNCH_LOOKAHEAD, SYS, CONV, LOAD, SOLVER, c.wiener != nullptr ? PC_GEN_WIENER : PC_GEN_PROFILE, (int)sizeof(R), tab ? 1 : 0, BLOCK, call.K, c.max_steps,
             (long long)blocks, 0};
    return GEMX_OK;
}

template <int SYS, int CONV>
static int launch_la_unit(gemx_handle *h, const RolloutCall &call, const LaCall &c, hipStream_t st) {
    return dispatch_load_solver(h, "lookahead rollout", [&](auto ls) { return launch_la_t<SYS, CONV, decltype(ls)::LOAD, decltype(ls)::SOLVER>(h, call, c, st); });
}
}  // namespace gemx

extern "C" {
__attribute__((visibility("default"))) int gemx_la_unit_init(unsigned long long handle_bytes, int abi, void (*set_error)(const char *)) {
    return gemx::unit_init(handle_bytes, abi, set_error);
}
__attribute__((visibility("default"))) int gemx_la_unit_launch(gemx_handle *h, const gemx::RolloutCall *call, const gemx::LaCall *la, hipStream_t st) {
    if (h->envp != nullptr && h->envp_fields != gemx::ep_fields(GEMX_INST_SYS)) return gemx::fail(GEMX_ERR_ARG, "internal: lookahead rollout unit launched with another system's table");
    if ((la->wiener != nullptr) == (la->profile != nullptr)) return gemx::fail(GEMX_ERR_ARG, "internal: lookahead rollout unit launched without exactly one generator view");
    if (h->rw_n_ref < 0) return gemx::fail(GEMX_ERR_ARG, "internal: lookahead rollout unit launched without a reward");
    return gemx::launch_la_unit<GEMX_INST_SYS, GEMX_INST_CONV>(h, *call, *la, st);
}
}
