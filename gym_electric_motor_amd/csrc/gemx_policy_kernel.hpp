// gemx_policy_kernel.hpp -- THE policy rollout kernel and its host launcher, included by both kinds of policy unit: gemx_policy.hip
// (libgemx_pl<S>_<C>.so, gemx_rollout_policy) and gemx_policy_complete.hip (libgemx_pc<S>_<C>.so, gemx_rollout_policy_complete).  One
// template, policy_rollout_kernel<SYS, CONV, LOAD, SOLVER, TAB, GEN, R>; GEN is where the references the actor reads come from:
//   PC_GEN_NONE     row k of a given tensor, pol.refs[k]                                           (the policy units)
//   PC_GEN_WIENER   } the row the env SHOWED in front of step k, from the env's own generators stepped in the lane that steps the env
//   PC_GEN_PROFILE  } (gemx_policy_complete.hip: pc_references)                                    (the complete policy units)
// The four places where a generator differs stand under `if constexpr` on GEN; everything else is one body, so the two kinds of unit
// cannot drift apart.  (gemx_last_launch and the coverage keys go on calling the GEN != NONE instantiations policy_complete_rollout_kernel.)
//
// The kernel is episodic_rollout_kernel (gemx_episodic.hip) with one change: the action of step k is not read from a tensor, it is computed
// in front of the step by a small MLP from the row step k - 1 left in the lane's registers,
//     x = [obs_prev[columns], references[k]],   out = W_L act(... act(W_1 x + b_1) ...) + b_L,
//     continuous converters: action = squash(out + noise[k]);   finite converters: action = the lowest index among the maxima of out + noise[k]
// obs_prev is obs0 at k = 0 and the handle's reset observation behind a step that ended the episode (what the masked reset writes); it is
// never re-read from memory.  The action is stored to actions_out [K][N][A] | [K][N] uint8.  Everything behind the action -- the control
// step, the pin of the stepped state, episode_row's rule, the row store in front of the restart -- is the episodic kernel's code, statement
// for statement, so the physics rows are bit for bit what gemx_rollout_episodic writes when fed the stored actions (tests).  It is kept as
// inline statements of this one body, not as helpers shared with the episodic kernel: the kernel sits at one wave per SIMD with the
// register file full, and the pin, the episode rule and the row store behind a __forceinline__ call cost every instantiation 64 bytes of
// scratch per lane.
//
// THE ACTOR: per-lane FMAs, not the exact-f32 MFMA.  One lane is one env, and its observation, its hidden activations and its state live in
// that lane's registers; a dot product is a chain  acc = fmaf(w, x_i, acc)  over the inputs in ASCENDING order starting from the bias --
// layer 0: the selected observation columns in ascending COLUMN order, then the references; later layers: the previous layer's outputs in
// order.  v_mfma_f32_16x16x4_f32 has the same numerics and, on gfx950, the same peak rate as the f32 VALU (64 FLOP/clk/SIMD), so it buys no
// throughput here, and it wants the wave's 64 envs as the N index of four 16-wide tiles with the activations laid ACROSS lanes: every layer
// would transpose registers <-> lanes through LDS or DPP, in front of a control step that needs them per lane again.  The weights are staged
// once per workgroup into LDS (gemx_policy.hpp: the blob as it is) and read at wave-uniform addresses: one 16-byte LDS read (4 LDS cycles
// per wave) feeds 4 FMAs (16 VALU cycles per wave), which four SIMDs sharing one LDS would sustain exactly.  Activations stay in registers: every
// index into them is a compile-time constant (the loop over 8-output blocks is a runtime loop whose block lands in the array through a
// switch on the wave-uniform block index), so nothing goes to scratch.  Widths are runtime values: inputs are skipped in wave-uniform
// blocks of 8, outputs in blocks of 8 -- a (16,) plan costs a quarter of a (64,) plan.
//
// Workgroups are 64 lanes (one wave stages the blob for itself) while there are at most four waves per CU, 256 lanes above that: four
// waves then stage and share one copy of the blob instead of four.
//
// What this costs, as compiled: the two activation sets (2 x 64 registers), the accumulators, the weights in flight and the control step's
// own registers exceed the 256 architectural VGPRs, the allocator parks the rest in AGPRs (profiles/policy_rollout.md lists all 152
// instantiations without a generator: 254-256 VGPRs, up to 160 AGPRs, 120-240 SGPRs spilled to VGPR lanes, no scratch;
// profiles/policy_complete_rollout.md the 304 with one), so ONE wave is resident per SIMD and nothing hides a wave's LDS and memory
// latency but its own instruction-level parallelism.  The LDS-to-FMA balance above is arithmetic from the documented instruction rates and
// the MFMA comparison is from the documented peak rates; neither has been measured with this kernel, and no rate of it has been measured
// at all.  A form with one live activation set (outputs rolled through LDS, or a narrower maximal width) would lift the occupancy; it is
// not what this file does.
#pragma once
#include "gemx_kernels.hpp"
#include "gemx_unit_host.hpp"
#include "gemx_envparams.hpp"
#include "gemx_envparams_dev.hpp"
#include "gemx_policy_dev.hpp"

namespace gemx {

// (GEN's values, PC_GEN_WIENER, PC_GEN_PROFILE and PC_GEN_NONE: gemx_policy.hpp)
// What a generator kind adds to the kernel's arguments, the pack G: where the reference rows are shown and stored (PcRefs), then the
// kernel's view of the generator (PcWienerDev | PcProfileDev), both of gemx_policy_complete.hpp.  Without a generator the pack is empty
// and the kernel takes the arguments up to `pol` and nothing else -- an empty struct in their place would still be a kernel argument of
// one byte.  gemx_policy_complete.hip defines pc_references: row k of the references, behind the row store of step k.
template <int GEN, class Dev>
__device__ __forceinline__ void pc_references(const Dev &gen, float *__restrict__ refs_out, int64_t N, int n_ref, int k, int64_t env, bool valid, bool end);
template <class Refs, class Dev> __device__ __forceinline__ const Refs &pc_refs_of(const Refs &refs, const Dev &) { return refs; }
template <class Refs, class Dev> __device__ __forceinline__ const Dev &pc_gen_of(const Refs &, const Dev &gen) { return gen; }

// (the activations as register vectors, pl_fma8 and the other helpers of the actor: gemx_policy_dev.hpp)

template <int SYS, int CONV, int LOAD, int SOLVER, bool TAB, int GEN, class R, class... G>
__global__ __launch_bounds__(PL_BLOCK_MAX) void policy_rollout_kernel(const KArgs<R> a, const R *__restrict__ tab, const int32_t *__restrict__ length_in, const int32_t M,
                                                                      uint8_t *__restrict__ truncated, uint8_t *__restrict__ ended, const PolicyDev pol, const G... g) {
    static_assert(sizeof(R) == 4, "the policy rollout is fp32");
    static_assert(sizeof...(G) == (GEN == PC_GEN_NONE ? 0 : 2), "a generator kind comes with its two arguments, none with none");
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
        // (with a generator -- a compiler barrier, no instruction: the generator state and the reference row of step k - 1 are re-read
        // from memory, not carried through the actor in registers)
        if constexpr (GEN != PC_GEN_NONE) asm volatile("" ::: "memory");
        // ---- the actor.  Layer 0: x = [op[columns], the references of step k], the observation columns in ascending column order.  The
        // references: row k of pol.refs, or with a generator the row shown in front of step k -- `shown` at k = 0, then the row this
        // lane stored behind step k - 1, its fp32 words re-read (lanes behind N: zeros -- they have stored none)
        const pl_v8 zero8 = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        PlAct ha = {zero8, zero8, zero8, zero8, zero8, zero8, zero8, zero8}, hb = ha;  // (per step: nothing of them is live across the control step)
        float rf[GEMX_MAX_REF];
        if constexpr (GEN == PC_GEN_NONE) {
#pragma unroll
            for (int r = 0; r < GEMX_MAX_REF; ++r) rf[r] = r < pol.n_ref ? pol.refs[((int64_t)k * N + e) * pol.n_ref + r] : 0.0f;
        } else {
            const auto &refs = pc_refs_of(g...);
            const float *shown = k == 0 ? refs.shown + e * pol.n_ref : refs.out + ((int64_t)(k - 1) * N + e) * pol.n_ref;
#pragma unroll
            for (int r = 0; r < GEMX_MAX_REF; ++r) rf[r] = (valid && r < pol.n_ref) ? shown[r] : 0.0f;
        }
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
        // ---- the references: the generators of an env that ended restart, then every generator advances -> refs.out[k]
        if constexpr (GEN != PC_GEN_NONE) pc_references<GEN>(pc_gen_of(g...), pc_refs_of(g...).out, N, pol.n_ref, k, env, valid, end);
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
            const auto &gen = pc_gen_of(g...);
#pragma unroll
            for (int r = 0; r < GEMX_MAX_REF; ++r)
                if (r < pol.n_ref) gen.t[(int64_t)r * N + env] += (uint64_t)K;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host launcher
// ------------------------------------------------------------------------------------------------
struct PolicyCall {
    const PolicyDev *pol;
    int K;
    const int32_t *length;
    int32_t max_steps;
    void *obs;
    uint8_t *terminated, *truncated, *ended;
    int *linmap_built;
};

// one launch but for its generator kind: what launch_policy_t hands to the unit's generator view, and that on to launch_policy_kernel
struct PolicyLaunch {
    const KArgs<float> &a;
    const float *tab;
    const PolicyCall &c;
    const PolicyDev &pol;
    unsigned blocks;
    int threads;
    size_t lds;
    hipStream_t st;
};
template <int SYS, int CONV, int LOAD, int SOLVER, bool TAB, int GEN, class... G>
static void launch_policy_kernel(const PolicyLaunch &l, const G &...g) {
    hipLaunchKernelGGL((policy_rollout_kernel<SYS, CONV, LOAD, SOLVER, TAB, GEN, float, G...>), dim3(l.blocks), dim3(l.threads), l.lds, l.st, l.a, l.tab, l.c.length,
                       l.c.max_steps, l.c.truncated, l.c.ended, l.pol, g...);
}

// V is what differs between the two kinds of unit, the unit's view of the call's generator:
//   V::WHAT, V::PIPE                                the prefix of the error messages; gemx_handle::LastLaunch::pipe
//   v.kind()                                        LastLaunch::il
//   v.launch<SYS, CONV, LOAD, SOLVER, TAB>(l)       launch_policy_kernel with the call's GEN and its arguments (G)
template <int SYS, int CONV, int LOAD, int SOLVER, class V>
static int launch_policy_t(gemx_handle *h, const PolicyCall &c, const V &v, hipStream_t st) {
    using R = float;
    constexpr int NLOGIT = ConvTraits<CONV>::DISCRETE ? ConvTraits<CONV>::NACTIONS : ConvTraits<CONV>::NACT;
    PolicyDev pol = *c.pol;
    if (pol.width[pol.n_layers - 1] != NLOGIT)
        return fail(GEMX_ERR_ARG, "%s: the policy's output width is %d, the converter takes %d (%s)", V::WHAT, pol.width[pol.n_layers - 1], NLOGIT,
                    ConvTraits<CONV>::DISCRETE ? "one logit per discrete action" : "one output per action component");
    const bool tab = h->envp != nullptr;
    if (const int rc = ensure_linmap<SYS, LOAD, SOLVER>(h, st, c.linmap_built)) return rc;
    KArgs<R> a;
    fill_unit_kargs<LOAD>(a, h, tab, c.K, c.obs, c.terminated);  // (tab: the episodic launcher's view of a handle with a table)
    pol.reset_obs = (const float *)h->reset_obs_dev;
    const int64_t waves = (h->n + 63) / 64;
    const int threads = waves > 4 * (int64_t)h->n_cu ? PL_BLOCK_MAX : 64;
    const int64_t blocks = (h->n + threads - 1) / threads;
    const size_t lds = sizeof(float) * ((size_t)pol.blob_words + SysTraits<SYS>::NOUT);
    const PolicyLaunch l = {a, tab ? (const R *)h->envp : nullptr, c, pol, (unsigned)blocks, threads, lds, st};
    if (tab) v.template launch<SYS, CONV, LOAD, SOLVER, true>(l);
    else v.template launch<SYS, CONV, LOAD, SOLVER, false>(l);
    GEMX_HIP_TRY(hipGetLastError());
    h->ll = {V::PIPE, SYS, CONV, LOAD, SOLVER, v.kind(), (int)sizeof(R), tab ? 1 : 0, threads, c.K, c.max_steps, (long long)blocks, lds};
    return GEMX_OK;
}

template <int SYS, int CONV, class V>
static int launch_policy_unit(gemx_handle *h, const PolicyCall &c, const V &v, hipStream_t st) {
    return dispatch_load_solver(h, V::WHAT, [&](auto ls) { return launch_policy_t<SYS, CONV, decltype(ls)::LOAD, decltype(ls)::SOLVER>(h, c, v, st); });
}

}  // namespace gemx
