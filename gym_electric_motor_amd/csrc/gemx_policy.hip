// gemx_policy.hip -- ONE policy rollout unit: K control steps per launch with the episode time limit AND the actor inside the launch
// (gemx_rollout_policy), for one (system, converter unit), fp32, built as its own shared object
//   hipcc -DGEMX_INST_SYS=<0..7> -DGEMX_INST_CONV=<0..11> -shared gemx_policy.hip -o libgemx_pl<S>_<C>.so
// and loaded with dlopen by the first gemx_rollout_policy of such a handle (gemx_capi.hip: load_pl_unit).  The stepping units, the per-env
// units and the episodic units (gemx_episodic.hip) are untouched.
//
// The kernel is episodic_rollout_kernel (gemx_episodic.hip) with one change: the action of step k is not read from a tensor, it is computed
// in front of the step by a small MLP from the row step k - 1 left in the lane's registers,
//     x = [obs_prev[columns], references[k]],   out = W_L act(... act(W_1 x + b_1) ...) + b_L,
//     continuous converters: action = squash(out + noise[k]);   finite converters: action = the lowest index among the maxima of out + noise[k]
// obs_prev is obs0 at k = 0 and the handle's reset observation behind a step that ended the episode (what the masked reset writes); it is
// never re-read from memory.  The action is stored to actions_out [K][N][A] | [K][N] uint8.  Everything behind the action -- the control
// step, the pin of the stepped state, episode_row's rule, the row store in front of the restart -- is the episodic kernel's code, statement
// for statement, so the physics rows are bit for bit what gemx_rollout_episodic writes when fed the stored actions (tests).
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
// instantiations: 254-256 VGPRs, up to 160 AGPRs, 120-240 SGPRs spilled to VGPR lanes, no scratch), so ONE wave is resident per SIMD and
// nothing hides a wave's LDS and memory latency but its own instruction-level parallelism.  The LDS-to-FMA balance above is arithmetic from
// the documented instruction rates and the MFMA comparison is from the documented peak rates; neither has been measured with this kernel,
// and no rate of it has been measured at all.  A form with one live activation set (outputs rolled through LDS, or a narrower maximal
// width) would lift the occupancy; it is not what this file does.
#include <cstdarg>
#include <cstdio>

#include "gemx_kernels.hpp"
#include "gemx_envparams.hpp"
#include "gemx_envparams_dev.hpp"
#include "gemx_policy.hpp"

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

constexpr int PL_BLOCK_MAX = 256;

// The activations: eight 8-float vector VALUES per layer (struct members, never an array in memory), so that they are registers whatever
// the optimiser's passes make of the loops around them
typedef float pl_v8 __attribute__((ext_vector_type(8)));
struct PlAct { pl_v8 b0, b1, b2, b3, b4, b5, b6, b7; };
// one 8-output block's accumulators into its member, on the wave-uniform block index
__device__ __forceinline__ void pl_scatter(int jb, pl_v8 acc, PlAct &dst) {
    switch (jb) {
    case 0: dst.b0 = acc; break;
    case 1: dst.b1 = acc; break;
    case 2: dst.b2 = acc; break;
    case 3: dst.b3 = acc; break;
    case 4: dst.b4 = acc; break;
    case 5: dst.b5 = acc; break;
    case 6: dst.b6 = acc; break;
    default: dst.b7 = acc;
    }
}
// acc[q] = fmaf(w[q], x, acc[q]) for the 8 outputs of a block: w = 8 consecutive words of the blob in LDS, one address for the wave
__device__ __forceinline__ void pl_fma8(const float *w, float x, pl_v8 &acc) {
    const float4 w0 = *reinterpret_cast<const float4 *>(w), w1 = *reinterpret_cast<const float4 *>(w + 4);
    acc[0] = fmaf(w0.x, x, acc[0]); acc[1] = fmaf(w0.y, x, acc[1]); acc[2] = fmaf(w0.z, x, acc[2]); acc[3] = fmaf(w0.w, x, acc[3]);
    acc[4] = fmaf(w1.x, x, acc[4]); acc[5] = fmaf(w1.y, x, acc[5]); acc[6] = fmaf(w1.z, x, acc[6]); acc[7] = fmaf(w1.w, x, acc[7]);
}
// the 8 inputs of one input block of a later layer (x: that member of the previous layer's activations) into one output block's
// accumulators, in order; w: row 8 ib of that output block
__device__ __forceinline__ void pl_in_block(const float *w, pl_v8 x, pl_v8 &acc) {
#pragma unroll
    for (int q = 0; q < 8; ++q) pl_fma8(w + q * 8, x[q], acc);
}
__device__ __forceinline__ pl_v8 pl_pick(const PlAct &h, int ib) {
    switch (ib) {
    case 0: return h.b0;
    case 1: return h.b1;
    case 2: return h.b2;
    case 3: return h.b3;
    case 4: return h.b4;
    case 5: return h.b5;
    case 6: return h.b6;
    default: return h.b7;
    }
}
__device__ __forceinline__ pl_v8 pl_load8(const float *p) {
    const float4 v0 = *reinterpret_cast<const float4 *>(p), v1 = *reinterpret_cast<const float4 *>(p + 4);
    pl_v8 r = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    return r;
}
__device__ __forceinline__ void pl_activate(int activation, pl_v8 &acc) {
    if (activation == PL_ACT_TANH) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = tanhf(acc[q]);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = fmaxf(acc[q], 0.0f);
    }
}

template <int SYS, int CONV, int LOAD, int SOLVER, bool TAB, class R>
__global__ __launch_bounds__(PL_BLOCK_MAX) void policy_rollout_kernel(const KArgs<R> a, const R *__restrict__ tab, const int32_t *__restrict__ length_in, const int32_t M,
                                                                      uint8_t *__restrict__ truncated, uint8_t *__restrict__ ended, const PolicyDev pol) {
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
        // ---- the actor.  Layer 0: x = [op[columns], references[k]], the observation columns in ascending column order
        const pl_v8 zero8 = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        PlAct ha = {zero8, zero8, zero8, zero8, zero8, zero8, zero8, zero8}, hb = ha;  // (per step: nothing of them is live across the control step)
        float rf[GEMX_MAX_REF];
#pragma unroll
        for (int r = 0; r < GEMX_MAX_REF; ++r) rf[r] = r < pol.n_ref ? pol.refs[((int64_t)k * N + e) * pol.n_ref + r] : 0.0f;
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
        // the next step's actor input: the row just stored, or the reset observation where the episode ended -- from registers and LDS
#pragma unroll
        for (int c = 0; c < NOUT; ++c) op[c] = end ? reset_row[c] : obs[c];
    }

    if (valid) {
#pragma unroll
        for (int j = 0; j < ND; ++j) a.state[(int64_t)j * N + env] = y[j];
        if (SysTraits<SYS>::HAS_ANGLE) a.angle[env] = ang;
        if (bad_action) atomicOr(a.err, 1u);
    }
}

// the unit's tanhf over n values: the tests' epsilon_tanh is measured on what the actor calls
__global__ void pl_tanh_kernel(const float *__restrict__ x, float *__restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = tanhf(x[i]);
}

// ------------------------------------------------------------------------------------------------
// host launcher
// ------------------------------------------------------------------------------------------------
struct PlCall {
    const PolicyDev *pol;
    int K;
    const int32_t *length;
    int32_t max_steps;
    void *obs;
    uint8_t *terminated, *truncated, *ended;
    int *linmap_built;
};

template <int SYS, int CONV, int LOAD, int SOLVER>
static int launch_pl_t(gemx_handle *h, const PlCall &c, hipStream_t st) {
    using R = float;
    constexpr int NLOGIT = ConvTraits<CONV>::DISCRETE ? ConvTraits<CONV>::NACTIONS : ConvTraits<CONV>::NACT;
    PolicyDev pol = *c.pol;
    if (pol.width[pol.n_layers - 1] != NLOGIT)
        return fail(GEMX_ERR_ARG, "policy rollout: the policy's output width is %d, the converter takes %d (%s)", pol.width[pol.n_layers - 1], NLOGIT,
                    ConvTraits<CONV>::DISCRETE ? "one logit per discrete action" : "one output per action component");
    const bool tab = h->envp != nullptr;
    if (!tab && h->linmap_state == 0) {  // once per handle, exactly as the episodic unit's launcher builds it: the electrical subsystem's one-step map
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
    if (tab)
        hipLaunchKernelGGL((policy_rollout_kernel<SYS, CONV, LOAD, SOLVER, true, R>), dim3((unsigned)blocks), dim3(threads), lds, st, a, (const R *)h->envp, c.length,
                           c.max_steps, c.truncated, c.ended, pol);
    else
        hipLaunchKernelGGL((policy_rollout_kernel<SYS, CONV, LOAD, SOLVER, false, R>), dim3((unsigned)blocks), dim3(threads), lds, st, a, (const R *)nullptr, c.length,
                           c.max_steps, c.truncated, c.ended, pol);
    GEMX_HIP_TRY(hipGetLastError());
    h->ll = {EP_LAUNCH_POLICY, SYS, CONV, LOAD, SOLVER, 0, (int)sizeof(R), tab ? 1 : 0, threads, c.K, c.max_steps, (long long)blocks, lds};
    return GEMX_OK;
}

template <int SYS, int CONV>
static int launch_pl_unit(gemx_handle *h, const PlCall &c, hipStream_t st) {
    const int ld = h->cfg.load_kind, sv = h->cfg.solver_kind;
#define GEMX_PL_LS(LD, SV) \
    if (ld == LD && sv == SV) return launch_pl_t<SYS, CONV, LD, SV>(h, c, st);
    GEMX_PL_LS(GEMX_LOAD_CONST_SPEED, GEMX_SOLVER_EULER)
    GEMX_PL_LS(GEMX_LOAD_CONST_SPEED, GEMX_SOLVER_RK4)
    GEMX_PL_LS(GEMX_LOAD_POLY_STATIC, GEMX_SOLVER_EULER)
    GEMX_PL_LS(GEMX_LOAD_POLY_STATIC, GEMX_SOLVER_RK4)
#undef GEMX_PL_LS
    return fail(GEMX_ERR_ARG, "policy rollout: load/solver combination %d/%d is not built (EulerSolver and RK4Solver only)", ld, sv);
}
}  // namespace gemx

extern "C" {
// GEMX_OK if this unit was compiled against the caller's handle layout and ABI
__attribute__((visibility("default"))) int gemx_pl_unit_init(unsigned long long handle_bytes, int abi, void (*set_error)(const char *)) {
    if (handle_bytes != (unsigned long long)sizeof(gemx_handle) || abi != GEMX_ABI_VERSION) return GEMX_ERR_ARG;
    gemx::g_set_error = set_error;
    return GEMX_OK;
}
__attribute__((visibility("default"))) int gemx_pl_unit_launch(gemx_handle *h, const gemx::PolicyDev *pol, int K, const int32_t *length, int32_t max_steps, void *obs,
                                                               uint8_t *terminated, uint8_t *truncated, uint8_t *ended, hipStream_t st, int *linmap_built) {
    if (h->envp != nullptr && h->envp_fields != gemx::ep_fields(GEMX_INST_SYS)) return gemx::fail(GEMX_ERR_ARG, "internal: policy rollout unit launched with another system's table");
    const gemx::PlCall c = {pol, K, length, max_steps, obs, terminated, truncated, ended, linmap_built};
    return gemx::launch_pl_unit<GEMX_INST_SYS, GEMX_INST_CONV>(h, c, st);
}
__attribute__((visibility("default"))) int gemx_pl_unit_tanh(const float *x, float *y, long long n, hipStream_t st) {
    if (n <= 0) return GEMX_OK;
    hipLaunchKernelGGL(gemx::pl_tanh_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, n);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}
}
