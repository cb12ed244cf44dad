// gemx_policy_complete.hip -- ONE complete policy rollout unit: policy_rollout_kernel (gemx_policy.hip) with the env's own reference
// generators stepped in the lane that steps the env (gemx_rollout_policy_complete), for one (system, converter unit), fp32, built as its
// own shared object
//   hipcc -DGEMX_INST_SYS=<0..7> -DGEMX_INST_CONV=<0..11> -shared gemx_policy_complete.hip -o libgemx_pc<S>_<C>.so
// and loaded with dlopen by the first gemx_rollout_policy_complete of such a handle (gemx_capi.hip: load_pc_unit).  The policy units
// (libgemx_pl<S>_<C>.so) are untouched.
//
// The kernel is policy_rollout_kernel, statement for statement, with two changes:
//   * the references the actor of step k reads are not row k of a given tensor but the row the env SHOWED in front of step k: `shown`
//     [N][n_ref] at k = 0, refs_out[k - 1] afterwards -- the fp32 words this lane stored, re-read;
//   * behind the row store of step k the lane restarts its generators if the step ended the episode, advances them and stores
//     refs_out[k] -- the shell's order (restart first, then advance), which gemx_refgen_rollout_shell and gemx_refprofile_rollout_shell
//     replay on the ENDED rows.  The lane functions are the generator units' own (gemx_refgen_lane.hpp, gemx_refprofile_lane.hpp), so the
//     rows and the state left behind are theirs bit for bit.
// GEN, a template parameter, is the generator kind: PC_GEN_WIENER (an all-Wiener gemx_refgen) or PC_GEN_PROFILE (a gemx_refprofile).
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
#include <cstdarg>
#include <cstdio>

#include "gemx_kernels.hpp"
#include "gemx_envparams.hpp"
#include "gemx_envparams_dev.hpp"
#include "gemx_policy_dev.hpp"
#include "gemx_policy_complete.hpp"
#define GEMX_REFPROFILE_ROW_ONLY  // the head section of gemx_refprofile.hip: the one definition of profile_row
#include "gemx_refprofile.hip"

#if !defined(GEMX_INST_SYS) || !defined(GEMX_INST_CONV)
#error "define GEMX_INST_SYS and GEMX_INST_CONV"
#endif

namespace gemx {
static void (*g_set_error)(const char *) = nullptr;
int fail(int code, const char *fmt, ...) {  // gemx_common.hpp declares it; in a unit it formats and hands the text to libgemx.so's gemx_last_error()
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (g_set_error != nullptr) g_set_error(buf);
    return code;
}

// (the activations as register vectors, pl_fma8 and the other helpers of the actor: gemx_policy_dev.hpp, shared with gemx_policy.hip)

template <int GEN> struct PcGenDev { using T = PcWienerDev; };
template <> struct PcGenDev<PC_GEN_PROFILE> { using T = PcProfileDev; };

// Row k of the references, behind the row store of step k: restart where the episode ended, advance, store.  Everything is read from the
// handle's arrays and written back here (a lane touches the words of its own env only); nothing of it is live across the actor.
// Lanes behind N take no part -- but for the profile's wave vote, which all 64 lanes reach together.
template <int GEN>
__device__ __forceinline__ void pc_references(const typename PcGenDev<GEN>::T &gen, float *__restrict__ refs_out, int64_t N, int n_ref, int k, int64_t env, bool valid, bool end) {
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

template <int SYS, int CONV, int LOAD, int SOLVER, bool TAB, int GEN, class R>
__global__ __launch_bounds__(PL_BLOCK_MAX) void policy_complete_rollout_kernel(const KArgs<R> a, const R *__restrict__ tab, const int32_t *__restrict__ length_in, const int32_t M,
                                                                               uint8_t *__restrict__ truncated, uint8_t *__restrict__ ended, const PolicyDev pol,
                                                                               const PcRefs refs, const typename PcGenDev<GEN>::T gen) {
    static_assert(sizeof(R) == 4, "the policy rollout is fp32");
    constexpr int ND = SysTraits<SYS>::ND, NOUT = SysTraits<SYS>::NOUT, NACT = ConvTraits<CONV>::NACT;
    constexpr bool DISCRETE = ConvTraits<CONV>::DISCRETE;
    constexpr int NLOGIT = DISCRETE ? ConvTraits<CONV>::NACTIONS : NACT;  // the last layer's width (checked by the launcher)
    constexpr bool LINABLE = !TAB && linable<SYS, LOAD, SOLVER, false, R>();
    using AngT = typename Angle<R>::T;
    using ST = Stepper<SYS, conv_base<CONV>(), LOAD, SOLVER, false, R>;
    extern __shared__ float lds[];  // the blob, then the reset observation [NOUT]
    const DevParams<R> &P = a.P;
    const int64_t N = a.N;
    const int K = a.K;
    const int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = env < N;
    const int64_t e = valid ? env : N - 1;  // tail lanes recompute the last env; their stores are masked

    // ---- the weights, once per workgroup
    for (int w = threadIdx.x; w < pol.blob_words; w += blockDim.x) lds[w] = pol.blob[w];
    if (threadIdx.x < NOUT) lds[pol.blob_words + threadIdx.x] = pol.reset_obs[threadIdx.x];
    const float *reset_row = lds + pol.blob_words;

    // ---- prologue: state, angle, the episode counter, the observation in front of step 0, the lane's table column
    R y[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) y[j] = a.state[(int64_t)j * N + e];
    AngT ang = AngT(0);
    if (SysTraits<SYS>::HAS_ANGLE) ang = a.angle[e];
    int32_t length = length_in[e];
    R op[NOUT];  // obs_prev
#pragma unroll
    for (int c = 0; c < NOUT; ++c) op[c] = P.obs_layout == GEMX_OBS_AOS ? pol.obs0[e * NOUT + c] : pol.obs0[(int64_t)c * N + e];
    // per-lane view: the table's fields (TAB), else the handle's own values -- the kernel argument itself, not a copy of it: the copy's
    // model constants went through 24 bytes of scratch in the induction machines' PolynomialStaticLoad instantiations
    DevParams<R> PT;
    if constexpr (TAB) {
        PT = P;
        R col[ep_fields(SYS)];
        ep_load<SYS, R>(tab, N, e, col);
        ep_apply<SYS, R>(col, PT);
    }
    const DevParams<R> &PL = TAB ? PT : P;
    const AngT init_ang = Angle<R>::from_bits(P.init_angle_rep);
    __syncthreads();

    uint32_t bad_action = 0;
    for (int k = 0; k < K; ++k) {
        // (a compiler barrier, no instruction: the generator state and the reference row of step k - 1 are re-read from memory, not
        // carried through the actor in registers)
        asm volatile("" ::: "memory");
        // ---- the actor.  Layer 0: x = [op[columns], the references shown in front of step k], the observation columns in ascending
        // column order; the references: `shown` at k = 0, then the row this lane stored behind step k - 1 (lanes behind N: zeros --
        // they have stored none)
        const pl_v8 zero8 = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        PlAct ha = {zero8, zero8, zero8, zero8, zero8, zero8, zero8, zero8}, hb = ha;  // (per step: nothing of them is live across the control step)
        float rf[GEMX_MAX_REF];
        const float *shown = k == 0 ? refs.shown + e * pol.n_ref : refs.out + ((int64_t)(k - 1) * N + e) * pol.n_ref;
#pragma unroll
        for (int r = 0; r < GEMX_MAX_REF; ++r) rf[r] = (valid && r < pol.n_ref) ? shown[r] : 0.0f;
        const float *lw = lds;
        {
            const int rows = pol.n_in, jb_n = (pol.width[0] + 7) >> 3;
            const float *bias = lw + jb_n * rows * 8;
            for (int jb = 0; jb < jb_n; ++jb) {
                const float *wb = lw + jb * rows * 8;
                pl_v8 acc = pl_load8(bias + 8 * jb);
#pragma unroll
                for (int c = 0; c < NOUT; ++c) {
                    const int i = pol.pos[c];
                    if (i >= 0) pl_fma8(wb + i * 8, op[c], acc);
                }
#pragma unroll
                for (int r = 0; r < GEMX_MAX_REF; ++r)
                    if (r < pol.n_ref) pl_fma8(wb + (pol.n_cols + r) * 8, rf[r], acc);
                if (pol.n_layers > 1) pl_activate(pol.activation, acc);
                pl_scatter(jb, acc, ha);
            }
            lw = bias + 8 * jb_n;
        }
        // later layers: ha -> hb -> ha, the inputs in order, skipped in blocks of 8 past the previous layer's (padded) width
#pragma unroll
        for (int l = 1; l < PL_MAX_LAYERS; ++l) {  // (unrolled: pol.width[] is read at constant indices, from SGPRs)
            if (l >= pol.n_layers) break;
            const int rows = (pol.width[l - 1] + 7) & ~7, jb_n = (pol.width[l] + 7) >> 3;
            const float *bias = lw + jb_n * rows * 8;
            // all (up to) 64 accumulators at once, from the biases; a runtime loop over the input blocks, whose member is picked on the
            // wave-uniform block index; inside, inputs and output blocks at constant indices.  Per output the order is still input 0, 1, ...
            hb.b0 = pl_load8(bias);
            if (jb_n > 1) hb.b1 = pl_load8(bias + 8);
            if (jb_n > 2) hb.b2 = pl_load8(bias + 16);
            if (jb_n > 3) hb.b3 = pl_load8(bias + 24);
            if (jb_n > 4) hb.b4 = pl_load8(bias + 32);
            if (jb_n > 5) hb.b5 = pl_load8(bias + 40);
            if (jb_n > 6) hb.b6 = pl_load8(bias + 48);
            if (jb_n > 7) hb.b7 = pl_load8(bias + 56);
            for (int ib = 0; 8 * ib < rows; ++ib) {
                const pl_v8 x = pl_pick(ha, ib);
                const float *wi = lw + 64 * ib;  // row 8 ib of output block 0
                const int jstride = rows * 8;
                pl_in_block(wi, x, hb.b0);
                if (jb_n > 1) pl_in_block(wi + jstride, x, hb.b1);
                if (jb_n > 2) pl_in_block(wi + 2 * jstride, x, hb.b2);
                if (jb_n > 3) pl_in_block(wi + 3 * jstride, x, hb.b3);
                if (jb_n > 4) pl_in_block(wi + 4 * jstride, x, hb.b4);
                if (jb_n > 5) pl_in_block(wi + 5 * jstride, x, hb.b5);
                if (jb_n > 6) pl_in_block(wi + 6 * jstride, x, hb.b6);
                if (jb_n > 7) pl_in_block(wi + 7 * jstride, x, hb.b7);
            }
            if (l + 1 < pol.n_layers) {
                pl_activate(pol.activation, hb.b0); pl_activate(pol.activation, hb.b1); pl_activate(pol.activation, hb.b2); pl_activate(pol.activation, hb.b3);
                pl_activate(pol.activation, hb.b4); pl_activate(pol.activation, hb.b5); pl_activate(pol.activation, hb.b6); pl_activate(pol.activation, hb.b7);
            }
            ha = hb;
            lw = bias + 8 * jb_n;
        }
        // ---- the action: out + noise[k], squashed (continuous) or its lowest-index maximum (finite)
        R act[MAX_ACT];
#pragma unroll
        for (int i = 0; i < MAX_ACT; ++i) act[i] = R(0);
        uint32_t dact = 0;
        {
            const float *nz = pol.noise != nullptr ? pol.noise + ((int64_t)k * N + e) * NLOGIT : nullptr;
            // (the logits leave the vectors at constant indices: member i / 8, element i % 8)
            auto logit = [&](int i) -> float {
                const pl_v8 &m = i < 8 ? ha.b0 : i < 16 ? ha.b1 : i < 24 ? ha.b2 : i < 32 ? ha.b3 : i < 40 ? ha.b4 : i < 48 ? ha.b5 : i < 56 ? ha.b6 : ha.b7;
                return m[i & 7] + (nz != nullptr ? nz[i] : 0.0f);
            };
            if constexpr (DISCRETE) {
                float best = logit(0);
#pragma unroll
                for (int i = 1; i < NLOGIT; ++i) {
                    const float v = logit(i);
                    if (v > best) { best = v; dact = (uint32_t)i; }
                }
                if (valid) reinterpret_cast<uint8_t *>(pol.actions_out)[(int64_t)k * N + env] = (uint8_t)dact;
            } else {
#pragma unroll
                for (int i = 0; i < NACT; ++i) {
                    const float v = logit(i);
                    act[i] = pol.squash == PL_SQUASH_TANH ? tanhf(v) : fminf(fmaxf(v, -1.0f), 1.0f);
                }
                if (valid) {
#pragma unroll
                    for (int i = 0; i < NACT; ++i) reinterpret_cast<float *>(pol.actions_out)[((int64_t)k * N + env) * NACT + i] = act[i];
                }
            }
        }

        // ---- from here on: episodic_rollout_kernel's step, statement for statement
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

        // The stepped state pinned in registers of its own, as in episodic_rollout_kernel (see the comment there: without it the register
        // coalescer merged y[1]'s loop-carried register with one the observation row's packed multiply had just written).  An empty asm
        // with a read-write operand generates no instruction; the values are unchanged.
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
        // ---- the references: the generators of an env that ended restart, then every generator advances -> refs_out[k]
        pc_references<GEN>(gen, refs.out, N, pol.n_ref, k, env, valid, end);
        // the next step's actor input: the row just stored, or the reset observation where the episode ended -- from registers and LDS
#pragma unroll
        for (int c = 0; c < NOUT; ++c) op[c] = end ? reset_row[c] : obs[c];
    }

    if (valid) {
#pragma unroll
        for (int j = 0; j < ND; ++j) a.state[(int64_t)j * N + env] = y[j];
        if (SysTraits<SYS>::HAS_ANGLE) a.angle[env] = ang;
        if (bad_action) atomicOr(a.err, 1u);
        if constexpr (GEN == PC_GEN_WIENER) {  // the index of the normal draws: K steps on (refgen_walk_kernel's last line)
#pragma unroll
            for (int g = 0; g < GEMX_MAX_REF; ++g)
                if (g < pol.n_ref) gen.t[(int64_t)g * N + env] += (uint64_t)K;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host launcher
// ------------------------------------------------------------------------------------------------
struct PcCall {
    const PolicyDev *pol;
    const PcRefs *refs;
    const PcWienerDev *wiener;    // exactly one of the two
    const PcProfileDev *profile;
    int K;
    const int32_t *length;
    int32_t max_steps;
    void *obs;
    uint8_t *terminated, *truncated, *ended;
    int *linmap_built;
};

template <int SYS, int CONV, int LOAD, int SOLVER, bool TAB, int GEN>
static void launch_pc_kernel(const KArgs<float> &a, const float *tab, const PcCall &c, const PolicyDev &pol, const typename PcGenDev<GEN>::T &gen, unsigned blocks, int threads,
                             size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((policy_complete_rollout_kernel<SYS, CONV, LOAD, SOLVER, TAB, GEN, float>), dim3(blocks), dim3(threads), lds, st, a, tab, c.length, c.max_steps,
                       c.truncated, c.ended, pol, *c.refs, gen);
}

template <int SYS, int CONV, int LOAD, int SOLVER>
static int launch_pc_t(gemx_handle *h, const PcCall &c, hipStream_t st) {
    using R = float;
    constexpr int NLOGIT = ConvTraits<CONV>::DISCRETE ? ConvTraits<CONV>::NACTIONS : ConvTraits<CONV>::NACT;
    PolicyDev pol = *c.pol;
    if (pol.width[pol.n_layers - 1] != NLOGIT)
        return fail(GEMX_ERR_ARG, "complete policy rollout: the policy's output width is %d, the converter takes %d (%s)", pol.width[pol.n_layers - 1], NLOGIT,
                    ConvTraits<CONV>::DISCRETE ? "one logit per discrete action" : "one output per action component");
    const bool tab = h->envp != nullptr;
    if (!tab && h->linmap_state == 0) {  // once per handle, exactly as the policy unit's launcher builds it: the electrical subsystem's one-step map
        if constexpr (linable<SYS, LOAD, SOLVER, false, R>()) {
            hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
            (void)hipStreamIsCapturing(st, &capturing);
            if ((h->cfg.solver_flags & GEMX_SOLVER_ADAPTIVE) || h->cfg.solver_nsteps != 1) {
                h->linmap_state = -1;
            } else if (capturing == hipStreamCaptureStatusNone) {  // (a first launch that is being captured goes without the map, as a stepped one does)
                hipLaunchKernelGGL((linmap_kernel<SYS, SOLVER, R>), dim3(1), dim3(64), 0, st, params_of<double>(h), (R *)h->linmap_dev);
                GEMX_HIP_TRY(hipGetLastError());
                GEMX_HIP_TRY(hipStreamSynchronize(st));
                h->linmap_state = 1;
                h->pf.lin_on = 1;
                if (c.linmap_built != nullptr) *c.linmap_built = 1;
            }
        } else {
            h->linmap_state = -1;
        }
    }
    KArgs<R> a;
    memset(&a, 0, sizeof(a));
    a.P = h->pf;
    if (tab) {  // the episodic launcher's view of a handle with a table
        a.P.lin_on = 0;
        a.P.kink_split = ((h->cfg.solver_flags & GEMX_SOLVER_SPLIT_KINKS) && LOAD == GEMX_LOAD_POLY_STATIC) ? 1 : 0;
    }
    a.P.errw = h->err;
    a.state = (R *)h->state;
    a.angle = (Angle<R>::T *)h->angle;
    a.sw = h->sw;
    a.obs = (R *)c.obs;
    a.done = c.terminated;
    a.err = h->err;
    a.N = h->n;
    a.K = c.K;
    a.obs_every = 1;
    a.S = 1;
    a.D = 1;
    pol.reset_obs = (const float *)h->reset_obs_dev;
    const int64_t waves = (h->n + 63) / 64;
    const int threads = waves > 4 * (int64_t)h->n_cu ? PL_BLOCK_MAX : 64;
    const int64_t blocks = (h->n + threads - 1) / threads;
    const size_t lds = sizeof(float) * ((size_t)pol.blob_words + SysTraits<SYS>::NOUT);
    const bool wiener = c.wiener != nullptr;
    if (tab && wiener) launch_pc_kernel<SYS, CONV, LOAD, SOLVER, true, PC_GEN_WIENER>(a, (const R *)h->envp, c, pol, *c.wiener, (unsigned)blocks, threads, lds, st);
    else if (tab) launch_pc_kernel<SYS, CONV, LOAD, SOLVER, true, PC_GEN_PROFILE>(a, (const R *)h->envp, c, pol, *c.profile, (unsigned)blocks, threads, lds, st);
    else if (wiener) launch_pc_kernel<SYS, CONV, LOAD, SOLVER, false, PC_GEN_WIENER>(a, nullptr, c, pol, *c.wiener, (unsigned)blocks, threads, lds, st);
    else launch_pc_kernel<SYS, CONV, LOAD, SOLVER, false, PC_GEN_PROFILE>(a, nullptr, c, pol, *c.profile, (unsigned)blocks, threads, lds, st);
    GEMX_HIP_TRY(hipGetLastError());
    h->ll = {EP_LAUNCH_POLICY_COMPLETE, SYS, CONV, LOAD, SOLVER, wiener ? PC_GEN_WIENER : PC_GEN_PROFILE, (int)sizeof(R), tab ? 1 : 0, threads, c.K, c.max_steps, (long long)blocks, lds};
    return GEMX_OK;
}

template <int SYS, int CONV>
static int launch_pc_unit(gemx_handle *h, const PcCall &c, hipStream_t st) {
    const int ld = h->cfg.load_kind, sv = h->cfg.solver_kind;
#define GEMX_PC_LS(LD, SV) \
    if (ld == LD && sv == SV) return launch_pc_t<SYS, CONV, LD, SV>(h, c, st);
    GEMX_PC_LS(GEMX_LOAD_CONST_SPEED, GEMX_SOLVER_EULER)
    GEMX_PC_LS(GEMX_LOAD_CONST_SPEED, GEMX_SOLVER_RK4)
    GEMX_PC_LS(GEMX_LOAD_POLY_STATIC, GEMX_SOLVER_EULER)
    GEMX_PC_LS(GEMX_LOAD_POLY_STATIC, GEMX_SOLVER_RK4)
#undef GEMX_PC_LS
    return fail(GEMX_ERR_ARG, "complete policy rollout: load/solver combination %d/%d is not built (EulerSolver and RK4Solver only)", ld, sv);
}
}  // namespace gemx

extern "C" {
// GEMX_OK if this unit was compiled against the caller's handle layout and ABI
__attribute__((visibility("default"))) int gemx_pc_unit_init(unsigned long long handle_bytes, int abi, void (*set_error)(const char *)) {
    if (handle_bytes != (unsigned long long)sizeof(gemx_handle) || abi != GEMX_ABI_VERSION) return GEMX_ERR_ARG;
    gemx::g_set_error = set_error;
    return GEMX_OK;
}
__attribute__((visibility("default"))) int gemx_pc_unit_launch(gemx_handle *h, const gemx::PolicyDev *pol, const gemx::PcRefs *refs, const gemx::PcWienerDev *wiener,
                                                               const gemx::PcProfileDev *profile, int K, const int32_t *length, int32_t max_steps, void *obs, uint8_t *terminated,
                                                               uint8_t *truncated, uint8_t *ended, hipStream_t st, int *linmap_built) {
    if (h->envp != nullptr && h->envp_fields != gemx::ep_fields(GEMX_INST_SYS)) return gemx::fail(GEMX_ERR_ARG, "internal: complete policy rollout unit launched with another system's table");
    if ((wiener != nullptr) == (profile != nullptr)) return gemx::fail(GEMX_ERR_ARG, "internal: complete policy rollout unit launched without exactly one generator view");
    const gemx::PcCall c = {pol, refs, wiener, profile, K, length, max_steps, obs, terminated, truncated, ended, linmap_built};
    return gemx::launch_pc_unit<GEMX_INST_SYS, GEMX_INST_CONV>(h, c, st);
}
}
