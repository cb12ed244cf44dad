// gemx_episodic.hip -- ONE episodic rollout unit: K control steps per launch WITH the episode time limit inside the launch
// (gemx_rollout_episodic), for one (system, converter unit), fp32, built as its own shared object
//   hipcc -DGEMX_INST_SYS=<0..7> -DGEMX_INST_CONV=<0..11> -shared gemx_episodic.hip -o libgemx_tl<S>_<C>.so
// and loaded with dlopen by the first gemx_rollout_episodic of such a handle (gemx_capi.hip: load_tl_unit).  The stepping units
// (gemx_inst.hip) and the per-env units (gemx_envparams.hip) are untouched.
//
// A fused K-step launch cannot restart an env on a mask another launch decides -- but the time limit's mask is the lane's own: truncation
// is `length >= M && !done`, and `length` depends on nothing but the lane's own done history.  So the kernel keeps the episode counter in
// a register beside the state and applies episode_row's rule (gemx_episode.hip) behind every control step:
//     length += 1;  truncated = length >= M && !done;  ended = done | truncated;  if (ended) { length = 0; state = the reset state; }
// Every ended env restarts, whatever P.auto_reset says: with a time limit the stepped path resets all of them too (the terminated ones in
// the stepping kernel or by the masked reset, the truncated ones by the masked reset), and for constant initial states the masked reset
// writes what the in-kernel reset writes.  The kernel READS `length` and never stores it: the episode stage's rows pass
// (gemx_episode_rows) runs behind it on the same done rows with the same limit from the same starting value -- one owner of the counters.
//
// Shape: envparams_rollout_kernel's -- one lane per env, no LDS, no barrier, state / counter / table column in registers across the K
// steps, the action of step k + 1 loaded ahead of step k's stores.  Two forms per (load, solver):
//   TAB = false  a uniform handle: the lane takes step_kernel's code path -- the one-step map wherever step_kernel would use it
//                (linable && lin_usable, decided per step on the state the step starts from), kink_split as the handle has it
//   TAB = true   a handle with a parameter table: ep_load / ep_apply / ep_control_step, i.e. envparams_step_kernel's step
// so the rows are, bit for bit, what K gemx_step calls with the episode stage and the masked reset between them write (tests).
// Not served (refused by gemx_rollout_episodic): fp64, the Dormand-Prince solvers, converter dead time, DeadTimeProcessor, RC supply,
// random initial states -- no leg state, no FIFO, no supply state, no carried step size and no draw in here.
#include "gemx_kernels.hpp"
#include "gemx_unit_host.hpp"
#include "gemx_envparams.hpp"
#include "gemx_envparams_dev.hpp"

#if !defined(GEMX_INST_SYS) || !defined(GEMX_INST_CONV)
#error "define GEMX_INST_SYS and GEMX_INST_CONV"
#endif

namespace gemx {
template <int SYS, int CONV, int LOAD, int SOLVER, bool TAB, class R>
__global__ __launch_bounds__(BLOCK) void episodic_rollout_kernel(const KArgs<R> a, const R *__restrict__ tab, const int32_t *__restrict__ length_in, const int32_t M,
                                                                 uint8_t *__restrict__ truncated, uint8_t *__restrict__ ended) {
    constexpr int ND = SysTraits<SYS>::ND, NOUT = SysTraits<SYS>::NOUT, NACT = ConvTraits<CONV>::NACT;
    constexpr bool DISCRETE = ConvTraits<CONV>::DISCRETE;
    constexpr int ABYTES = DISCRETE ? 1 : NACT * (int)sizeof(R);
    constexpr bool LINABLE = !TAB && linable<SYS, LOAD, SOLVER, false, R>();
    using AngT = typename Angle<R>::T;
    using ST = Stepper<SYS, conv_base<CONV>(), LOAD, SOLVER, false, R>;
    const DevParams<R> &P = a.P;
    const int64_t N = a.N;
    const int K = a.K;
    const int64_t env = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool valid = env < N;
    const int64_t e = valid ? env : N - 1;  // tail lanes recompute the last env; their stores are masked

    auto read_action = [&](int k, R (&dst)[MAX_ACT], uint32_t &ddst) {
        const unsigned char *g = a.actions + ((int64_t)k * N + e) * ABYTES;
        if (DISCRETE) ddst = *g;
        else {
#pragma unroll
            for (int i = 0; i < NACT; ++i) dst[i] = reinterpret_cast<const R *>(g)[i];
        }
    };

    // ---- prologue: state, angle, the episode counter, the first action, the lane's table column -- one batch of loads
    R y[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) y[j] = a.state[(int64_t)j * N + e];
    AngT ang = AngT(0);
    if (SysTraits<SYS>::HAS_ANGLE) ang = a.angle[e];
    int32_t length = length_in[e];
    R nact[MAX_ACT];
#pragma unroll
    for (int i = 0; i < MAX_ACT; ++i) nact[i] = R(0);
    uint32_t ndact = 0;
    read_action(0, nact, ndact);
    DevParams<R> PL = P;  // per-lane view: the table's fields (TAB), else the handle's own values
    if constexpr (TAB) {
        R col[ep_fields(SYS)];
        ep_load<SYS, R>(tab, N, e, col);
        ep_apply<SYS, R>(col, PL);
    }
    const AngT init_ang = Angle<R>::from_bits(P.init_angle_rep);

    uint32_t bad_action = 0;
    for (int k = 0; k < K; ++k) {
        R act[MAX_ACT];
#pragma unroll
        for (int i = 0; i < MAX_ACT; ++i) act[i] = nact[i];
        uint32_t dact = ndact;
        if (k + 1 < K) read_action(k + 1, nact, ndact);  // the next step's action, ahead of this step's stores

        R obs[NOUT];
        bool done;
        if constexpr (TAB) {
            done = ep_control_step<SYS, CONV, LOAD, SOLVER, R>(P, PL, y, ang, act, dact, bad_action, obs);
        } else {  // step_kernel's control step (no dead time, no DeadTimeProcessor, no RC supply), the one-step map decided where it decides it
            const bool lin_ok = lin_usable<SYS, LOAD, SOLVER, false, R>(P, y[0]);  // wave-uniform
            if (DISCRETE) { bad_action |= dact >= (uint32_t)ConvTraits<CONV>::NACTIONS; dact &= (uint32_t)(ConvTraits<CONV>::NACTIONS - 1); }
            if (conv_dq<CONV>()) dq_action_stage<SYS, CONV, R>(P, y, ang, act);
            uint32_t sw = 0;
            R hcar = R(0);
            if (LINABLE && lin_ok) full_step<ST, ND, NOUT, R, LINABLE>(PL, y, ang, sw, act, dact, obs);
            else full_step<ST, ND, NOUT, R, false>(PL, y, ang, sw, act, dact, obs, nullptr, &hcar);
            done = constraint_done<ST, NOUT, R>(P, obs);
        }

        // The stepped state pinned in registers of its own here.  Without it the register coalescer (ROCm 7 clang, gfx950, synchronous
        // machine behind a ConstantSpeedLoad, RK4) merged y[1]'s loop-carried register with the one the packed multiply of the
        // observation row had just written omega and the normalised torque into ("kill: def $vgpr9 killed $vgpr16" in the assembly):
        // every step but the first started from i_sd = the torque column, 1.9e-2 off in the rows.  An empty asm with a read-write operand
        // generates no instruction; the values are unchanged.
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
struct TlCall {
    const void *actions;
    int K;
    const int32_t *length;
    int32_t max_steps;
    void *obs;
    uint8_t *terminated, *truncated, *ended;
    int *linmap_built;
};

template <int SYS, int CONV, int LOAD, int SOLVER>
static int launch_tl_t(gemx_handle *h, const TlCall &c, hipStream_t st) {
    using R = float;
    const bool tab = h->envp != nullptr;
    if (const int rc = ensure_linmap<SYS, LOAD, SOLVER>(h, st, c.linmap_built)) return rc;
    KArgs<R> a;
    fill_unit_kargs<LOAD>(a, h, tab, c.K, c.obs, c.terminated);  // (tab: launch_ep_t's view of the handle)
    a.actions = (const unsigned char *)c.actions;
    const int64_t blocks = (h->n + BLOCK - 1) / BLOCK;
    if (tab)
        hipLaunchKernelGGL((episodic_rollout_kernel<SYS, CONV, LOAD, SOLVER, true, R>), dim3((unsigned)blocks), dim3(BLOCK), 0, st, a, (const R *)h->envp, c.length,
                           c.max_steps, c.truncated, c.ended);
    else
        hipLaunchKernelGGL((episodic_rollout_kernel<SYS, CONV, LOAD, SOLVER, false, R>), dim3((unsigned)blocks), dim3(BLOCK), 0, st, a, (const R *)nullptr, c.length,
                           c.max_steps, c.truncated, c.ended);
    GEMX_HIP_TRY(hipGetLastError());
    h->ll = {EP_LAUNCH_EPISODIC, SYS, CONV, LOAD, SOLVER, 0, (int)sizeof(R), tab ? 1 : 0, BLOCK, c.K, c.max_steps, (long long)blocks, 0};
    return GEMX_OK;
}

template <int SYS, int CONV>
static int launch_tl_unit(gemx_handle *h, const TlCall &c, hipStream_t st) {
    return dispatch_load_solver(h, "episodic rollout", [&](auto ls) { return launch_tl_t<SYS, CONV, decltype(ls)::LOAD, decltype(ls)::SOLVER>(h, c, st); });
}
}  // namespace gemx

extern "C" {
__attribute__((visibility("default"))) int gemx_tl_unit_init(unsigned long long handle_bytes, int abi, void (*set_error)(const char *)) {
    return gemx::unit_init(handle_bytes, abi, set_error);
}
__attribute__((visibility("default"))) int gemx_tl_unit_launch(gemx_handle *h, const void *actions, int K, const int32_t *length, int32_t max_steps, void *obs,
                                                               uint8_t *terminated, uint8_t *truncated, uint8_t *ended, hipStream_t st, int *linmap_built) {
    if (h->envp != nullptr && h->envp_fields != gemx::ep_fields(GEMX_INST_SYS)) return gemx::fail(GEMX_ERR_ARG, "internal: episodic rollout unit launched with another system's table");
    const gemx::TlCall c = {actions, K, length, max_steps, obs, terminated, truncated, ended, linmap_built};
    return gemx::launch_tl_unit<GEMX_INST_SYS, GEMX_INST_CONV>(h, c, st);
}
}
