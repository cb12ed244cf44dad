// gemx_envparams.hip -- ONE per-env-parameter unit: the two kernels that step every env with ITS OWN motor, load and supply parameters
// (gemx_set_env_params), for one (system, converter unit), fp32, built as its own shared object
//   hipcc -DGEMX_INST_SYS=<0..7> -DGEMX_INST_CONV=<0..11> -shared gemx_envparams.hip -o libgemx_ep<S>_<C>.so
// and loaded with dlopen by the first gemx_set_env_params of such a handle (gemx_capi.hip: load_ep_unit).  The stepping units
// (gemx_inst.hip) and their kernels are untouched: a handle without a table launches what it always launched.
//
// Both kernels are step_kernel's shape -- one lane per env, no LDS, no barrier, rows stored from the lane's registers -- and call the device
// functions the other kernels call (dq_action_stage, full_step<Stepper>, constraint_done, the reward's reward_term) with a per-lane
// DevParams: `PL = P` with the table's fields (gemx_envparams.hpp) replaced by the lane's column, as step_kernel does for the RC supply's
// u_sup.  Same expressions on the same values, so lane e equals, bit for bit, a uniform handle built with lane e's parameters (tests).
// Always the stage-by-stage solver: the one-step map of the constant-speed loads (lin_usable) is built for one parameter set.
// Not served (refused by gemx_set_env_params): fp64, the Dormand-Prince solver, converter dead time, DeadTimeProcessor, RC supply, random
// initial states -- so there is no leg state, no FIFO, no supply state and no draw in here.
#include "gemx_kernels.hpp"
#include "gemx_unit_host.hpp"
#include "gemx_envparams.hpp"
#include "gemx_envparams_dev.hpp"

#if !defined(GEMX_INST_SYS) || !defined(GEMX_INST_CONV)
#error "define GEMX_INST_SYS and GEMX_INST_CONV"
#endif

namespace gemx {
// (ep_load, ep_apply, ep_store_row, ep_control_step: gemx_envparams_dev.hpp, shared with the episodic rollout units)

// ------------------------------------------------------------------------------------------------
// K = 1 (gemx_step): ONE batch of loads -- state, angle, action and the lane's table column, all issued before the first wait --, the
// control step, the row stored from registers, the done byte, auto-reset.
// ------------------------------------------------------------------------------------------------
template <int SYS, int CONV, int LOAD, int SOLVER, class R>
__global__ __launch_bounds__(BLOCK) void envparams_step_kernel(const KArgs<R> a, const R *__restrict__ tab) {
    constexpr int ND = SysTraits<SYS>::ND, NOUT = SysTraits<SYS>::NOUT, NACT = ConvTraits<CONV>::NACT;
    constexpr bool DISCRETE = ConvTraits<CONV>::DISCRETE;
    using AngT = typename Angle<R>::T;
    const DevParams<R> &P = a.P;
    const int64_t N = a.N;
    const int64_t env = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool valid = env < N;
    const int64_t e = valid ? env : N - 1;  // tail lanes recompute the last env; their stores are masked

    // ---- one batch of loads
    R y[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) y[j] = a.state[(int64_t)j * N + e];
    AngT ang = AngT(0);
    if (SysTraits<SYS>::HAS_ANGLE) ang = a.angle[e];
    R act[MAX_ACT];
#pragma unroll
    for (int i = 0; i < MAX_ACT; ++i) act[i] = R(0);
    uint32_t dact = 0;
    if (DISCRETE) dact = a.actions[e];
    else {
#pragma unroll
        for (int i = 0; i < NACT; ++i) act[i] = reinterpret_cast<const R *>(a.actions)[e * NACT + i];
    }
    R col[ep_fields(SYS)];
    ep_load<SYS, R>(tab, N, e, col);
    DevParams<R> PL = P;
    ep_apply<SYS, R>(col, PL);

    // ---- the control step
    uint32_t bad_action = 0;
    R obs[NOUT];
    const bool done = ep_control_step<SYS, CONV, LOAD, SOLVER, R>(P, PL, y, ang, act, dact, bad_action, obs);
    if (done && P.auto_reset) {  // `if terminated: env.reset()`: the initial state is one per handle
#pragma unroll
        for (int j = 0; j < ND; ++j) y[j] = P.init[j];
        ang = Angle<R>::from_bits(P.init_angle_rep);
    }

    // ---- stores
    if (valid) {
        ep_store_row<NOUT, R>(P, a.obs, N, env, obs);
        if (a.done != nullptr) a.done[env] = done ? 1 : 0;
#pragma unroll
        for (int j = 0; j < ND; ++j) a.state[(int64_t)j * N + env] = y[j];
        if (SysTraits<SYS>::HAS_ANGLE) a.angle[env] = ang;
        if (bad_action) atomicOr(a.err, 1u);
    }
}

// ------------------------------------------------------------------------------------------------
// K control steps per launch (gemx_rollout, gemx_rollout_reward): state and parameters stay in the lane's registers across the K steps, the
// action (and the fused reward's references) of step k + 1 is loaded before step k computes and stores -- loads and stores retire through
// one in-order counter, so a load issued BEHIND a step's stores would wait for them --, every step's row, done byte and reward are written
// in the layout gemx_rollout / gemx_rollout_reward write ([K][N][S_out] or [K][S_out][N], [K][N], [K][N]).
// The fused reward is reward_row's statements (gemx_reward.hpp, the definition of WeightedSumOfErrors) on the row in registers, kept in
// place because the call changed this kernel's code (profiles/reward_row_refactor.md): the hot terms by value from the kernel arguments,
// further terms and general powers through the description in memory; a column is picked without a dynamic index into the row, which
// would put it into scratch (ep_pick).
// ------------------------------------------------------------------------------------------------
// (as AND / OR on the bit patterns: a chain of selects on one index is folded back into an indexed array by the compiler -- the DFIM's
// 24-value rows went through scratch that way)
template <int NOUT> __device__ __forceinline__ float ep_pick(const float (&obs)[NOUT], int col) {
    uint32_t v = 0u;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) v |= __builtin_bit_cast(uint32_t, obs[j]) & (col == j ? 0xFFFFFFFFu : 0u);
    return __builtin_bit_cast(float, v);
}
template <int SYS, int CONV, int LOAD, int SOLVER, class R>
__global__ __launch_bounds__(BLOCK) void envparams_rollout_kernel(const KArgs<R> a, const R *__restrict__ tab) {
    constexpr int ND = SysTraits<SYS>::ND, NOUT = SysTraits<SYS>::NOUT, NACT = ConvTraits<CONV>::NACT;
    constexpr bool DISCRETE = ConvTraits<CONV>::DISCRETE;
    constexpr int ABYTES = DISCRETE ? 1 : NACT * (int)sizeof(R);
    constexpr int HOT = RewardRegs<R>::HOT;
    using AngT = typename Angle<R>::T;
    const DevParams<R> &P = a.P;
    const int64_t N = a.N;
    const int K = a.K;
    const int64_t env = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool valid = env < N;
    const int64_t e = valid ? env : N - 1;
    const bool rewarded = a.rw != nullptr;  // wave-uniform
    const int n_ref = a.rh.n_ref;

    auto read_action = [&](int k, R (&dst)[MAX_ACT], uint32_t &ddst) {
        const unsigned char *g = a.actions + ((int64_t)k * N + e) * ABYTES;
        if (DISCRETE) ddst = *g;
        else {
#pragma unroll
            for (int i = 0; i < NACT; ++i) dst[i] = reinterpret_cast<const R *>(g)[i];
        }
    };
    auto read_refs = [&](int k, R (&dst)[GEMX_MAX_REF]) {
#pragma unroll
        for (int j = 0; j < GEMX_MAX_REF; ++j) {
            dst[j] = R(0);
            if (rewarded && j < n_ref) dst[j] = a.refs[((int64_t)k * N + e) * n_ref + j];
        }
    };

    // ---- prologue: state, angle, the first action (and references), the lane's table column
    R y[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) y[j] = a.state[(int64_t)j * N + e];
    AngT ang = AngT(0);
    if (SysTraits<SYS>::HAS_ANGLE) ang = a.angle[e];
    R nact[MAX_ACT];
#pragma unroll
    for (int i = 0; i < MAX_ACT; ++i) nact[i] = R(0);
    uint32_t ndact = 0;
    read_action(0, nact, ndact);
    R nref[GEMX_MAX_REF];
    read_refs(0, nref);
    R col[ep_fields(SYS)];
    ep_load<SYS, R>(tab, N, e, col);
    DevParams<R> PL = P;
    ep_apply<SYS, R>(col, PL);
    RewardRegs<R> W;
    W.load(a.rh);
    const AngT init_ang = Angle<R>::from_bits(P.init_angle_rep);

    uint32_t bad_action = 0;
    for (int k = 0; k < K; ++k) {
        R act[MAX_ACT], ref[GEMX_MAX_REF];
#pragma unroll
        for (int i = 0; i < MAX_ACT; ++i) act[i] = nact[i];
#pragma unroll
        for (int j = 0; j < GEMX_MAX_REF; ++j) ref[j] = nref[j];
        const uint32_t dact = ndact;
        if (k + 1 < K) {  // the next step's inputs, ahead of this step's stores
            read_action(k + 1, nact, ndact);
            read_refs(k + 1, nref);
        }
        R obs[NOUT];
        const bool done = ep_control_step<SYS, CONV, LOAD, SOLVER, R>(P, PL, y, ang, act, dact, bad_action, obs);
        if (done && P.auto_reset) {
#pragma unroll
            for (int j = 0; j < ND; ++j) y[j] = P.init[j];
            ang = init_ang;
        }
        R rwd = R(0);
        if (rewarded) {  // reward_row (gemx_reward.hpp), its statements in place: through the call this kernel compiles to other code
            R acc = R(0);
            if (!W.general) {
#pragma unroll
                for (int t = 0; t < HOT; ++t)
                    acc += reward_term<false, R>(ep_pick<NOUT>(obs, W.col[t]), t < GEMX_MAX_REF ? ref[t] : R(0), W.inv_len[t], W.kind[t], W.power[t], W.coef[t]);
            }
#pragma nounroll
            for (int t = W.general ? 0 : HOT; t < W.n_term; ++t) {
                R rf = R(0);
#pragma unroll
                for (int j = 0; j < GEMX_MAX_REF; ++j) rf = (t == j) ? ref[j] : rf;
                acc += reward_term<true, R>(ep_pick<NOUT>(obs, a.rw->col[t]), rf, a.rw->inv_len[t], a.rw->kind[t], a.rw->power[t], a.rw->coef[t]);
            }
            const R wse = W.bias - acc;
            rwd = done ? W.violation_reward : wse;
        }
        if (valid) {
            ep_store_row<NOUT, R>(P, a.obs + (int64_t)k * N * NOUT, N, env, obs);
            if (a.done != nullptr) a.done[(int64_t)k * N + env] = done ? 1 : 0;
            if (rewarded) a.reward[(int64_t)k * N + env] = rwd;
        }
    }

    if (valid) {
#pragma unroll
        for (int j = 0; j < ND; ++j) a.state[(int64_t)j * N + env] = y[j];
        if (SysTraits<SYS>::HAS_ANGLE) a.angle[env] = ang;
        if (bad_action) atomicOr(a.err, 1u);
    }
}

// ------------------------------------------------------------------------------------------------
// host launcher
// ------------------------------------------------------------------------------------------------
template <int SYS, int CONV, int LOAD, int SOLVER>
static int launch_ep_t(gemx_handle *h, const float *tab, const RolloutCall &c, hipStream_t st) {
    using R = float;
    const int K = c.K;
    KArgs<R> a;
    fill_unit_kargs<LOAD>(a, h, true, K, c.obs, c.done);
    a.actions = (const unsigned char *)c.actions;
    a.rw = c.reward != nullptr ? (const RewardDev<R> *)h->rw_dev : nullptr;
    a.rh = h->rh_f;
    a.refs = (const R *)c.refs;
    a.reward = (R *)c.reward;
    const int64_t blocks = (h->n + BLOCK - 1) / BLOCK;
    const bool step = K == 1 && c.reward == nullptr;
    if (step) hipLaunchKernelGGL((envparams_step_kernel<SYS, CONV, LOAD, SOLVER, R>), dim3((unsigned)blocks), dim3(BLOCK), 0, st, a, tab);
    else hipLaunchKernelGGL((envparams_rollout_kernel<SYS, CONV, LOAD, SOLVER, R>), dim3((unsigned)blocks), dim3(BLOCK), 0, st, a, tab);
    GEMX_HIP_TRY(hipGetLastError());
    h->ll = {step ? EP_LAUNCH_STEP : EP_LAUNCH_ROLLOUT, SYS, CONV, LOAD, SOLVER, 0, (int)sizeof(R), 0, BLOCK, K, 1, (long long)blocks, 0};
    return GEMX_OK;
}

template <int SYS, int CONV>
static int launch_ep_unit(gemx_handle *h, const void *tab, const RolloutCall &c, hipStream_t st) {
    return dispatch_load_solver(h, "per-env parameters", [&](auto ls) {
        return launch_ep_t<SYS, CONV, decltype(ls)::LOAD, decltype(ls)::SOLVER>(h, (const float *)tab, c, st);
    });
}
}  // namespace gemx

extern "C" {
__attribute__((visibility("default"))) int gemx_ep_unit_init(unsigned long long handle_bytes, int abi, void (*set_error)(const char *)) {
    return gemx::unit_init(handle_bytes, abi, set_error);
}
__attribute__((visibility("default"))) int gemx_ep_unit_launch(gemx_handle *h, const gemx::RolloutCall &call, hipStream_t st) {
    if (h->envp == nullptr || h->envp_fields != gemx::ep_fields(GEMX_INST_SYS)) return gemx::fail(GEMX_ERR_ARG, "internal: per-env parameter unit launched without its table");
    return gemx::launch_ep_unit<GEMX_INST_SYS, GEMX_INST_CONV>(h, h->envp, call, st);
}
}
