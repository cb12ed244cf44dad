// gemx_policy_eval.hip -- an MLP of gemx_policy_create evaluated on every row of a stored policy rollout (include/gemx.h:
// gemx_policy_eval_rows): what a learner needs behind a rollout -- a critic's value, last_value and final_value for gemx_returns_rows, the
// actor's log-probability and entropy -- as ONE launch, with the rollout kernels' own arithmetic.  No physics, no env handle, no state
// that survives a call; the weights are the policy's device blob as it is (gemx_policy.hpp), no second copy.
//
// A lane owns one (k, env) row.  It gathers the actor input the rollout kernel builds (gemx_policy_kernel.hpp, with and without a generator),
//     SEEN: o = k == 0 ? obs0 : ended[k-1] ? reset observation : rows[k-1];   NEXT: o = rows[k]
//     x = [o[columns], r]            (r: the reference row the header names for the mode and the form)
// runs the MLP with gemx_policy_dev.hpp's helpers in the policy rollout kernel's order -- layer 0 per 8-output block over the selected
// columns in ascending COLUMN order and then the references, later layers per 8-output block over the input blocks in order, every
// dot product one fmaf chain from the bias -- and applies the head in the same lane.  The chains are explicit fmaf calls and the
// activations are the same tanhf / fmaxf, so `out` is bit for bit what the rollout kernel had in front of `+ noise[k]` (tests).  Per-lane
// FMAs, not MFMA: the exact-f32 MFMA has the same rate on gfx950 and another accumulation order.
//
// Workgroups of 256 lanes loop over tiles of 256 rows: the blob is staged into LDS once per workgroup, not once per tile, and read at
// wave-uniform addresses (pl_fma8 / pl_in_block).  Activations are PlAct register values, every index into them a compile-time
// constant.  Rows are [n_state] floats at a lane-private address (array of structures, as the policy rollouts write them); 64-bit row
// indices; the lanes of the partial last tile recompute the last row and store nothing.
//
// Heads (HEAD, the one template parameter): they read the fp32 out, compute in double with every operation rounded on its own
// (contraction off, as gemx_returns.hip's row function) and round once to the output dtype.  The operation order is the one
// include/gemx.h states; tests/policy_eval_restatement.py restates it in numpy.
#include "gemx_support.hpp"
#include "gemx_policy_dev.hpp"

namespace {

using gemx::PlAct;
using gemx::pl_v8;

constexpr int EVAL_BLOCK = 256;
constexpr double HALF_LOG_2PI = 0.9189385332046727, HALF_LOG_2PIE = 1.4189385332046727, LOG_2 = 0.6931471805599453;

// the kernel's view of one call (kernel argument, by value -> SGPRs)
struct EvalDev {
    const float *blob;
    int32_t blob_words, n_layers, n_in;
    int32_t width[gemx::PL_MAX_LAYERS];
    int32_t activation;
    int32_t n_cols, n_ref, n_state, n_out;
    int8_t pos[GEMX_MAX_OUT];  // row column c is input pos[c] of layer 0; -1: not selected
    int32_t next, squash_correction, f64, reset_per_env;
    const float *obs0, *rows, *reset_obs;
    const uint8_t *ended;
    const float *refs, *refs0, *last_refs;
    const uint8_t *actions;
    const float *pre_squash, *log_std;
    float *out, *out_last;
    void *value, *value_last, *log_prob, *entropy;
    uint32_t *err;
    int64_t N, total, tiles;  // total = (K + last) * N rows in tiles of EVAL_BLOCK
    int32_t K;
};

__device__ __forceinline__ void eval_store(void *dst, int64_t at, double v, int f64) {
    if (f64) reinterpret_cast<double *>(dst)[at] = v;
    else reinterpret_cast<float *>(dst)[at] = (float)v;
}

// The heads walk the outputs in blocks of 8 (a runtime loop over the members of the activation set, the 8 elements of a member at
// constant indices): unrolled over all 64 outputs they were the kernel's register peak.
//
// log_prob of action a and the entropy of softmax(z): max-shifted logsumexp, every sum in ascending index order from 0
__device__ __forceinline__ void head_categorical(const PlAct &h, int n, uint32_t a, double &log_prob, double &entropy) {
#pragma clang fp contract(off)
    float mf = h.b0[0];  // (the maximum of the floats: the conversion is exact and monotone)
#pragma nounroll
    for (int b = 0; 8 * b < n; ++b) {
        const pl_v8 v = gemx::pl_pick(h, b);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (8 * b + q < n) mf = fmaxf(mf, v[q]);
    }
    const double m = (double)mf;
    double s = 0.0;
#pragma nounroll
    for (int b = 0; 8 * b < n; ++b) {
        const pl_v8 v = gemx::pl_pick(h, b);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (8 * b + q < n) s = s + exp((double)v[q] - m);
    }
    const double lse = m + log(s);
    double e = 0.0, la = __longlong_as_double(0x7ff8000000000000ll);  // (an action outside [0, n): NaN)
#pragma nounroll
    for (int b = 0; 8 * b < n; ++b) {
        const pl_v8 v = gemx::pl_pick(h, b);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (8 * b + q < n) {
                const double l = (double)v[q] - lse;
                e = e + exp(l) * l;
                if (a == (uint32_t)(8 * b + q)) la = l;
            }
    }
    log_prob = la;
    entropy = -e;
}

// log_prob of the pre-squash sample u under N(z, exp(log_std)^2) per component, optionally with the tanh change of variables; the entropy
__device__ __forceinline__ void head_gaussian(const PlAct &h, int n, const float *__restrict__ u_row, const float *__restrict__ log_std, bool correction,
                                              double &log_prob, double &entropy) {
#pragma clang fp contract(off)
    double lp = 0.0, c = 0.0, e = 0.0;
#pragma nounroll
    for (int b = 0; 8 * b < n; ++b) {
        const pl_v8 v = gemx::pl_pick(h, b);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = 8 * b + q;
            if (j < n) {
                const double ls = (double)log_std[j], u = (double)u_row[j];
                const double sg = exp(ls), d = u - (double)v[q];
                const double t2 = (d * d) / (2.0 * (sg * sg));
                lp = lp + (((-t2) - ls) - HALF_LOG_2PI);
                e = e + (ls + HALF_LOG_2PIE);
                if (correction) {
                    const double t = -2.0 * u;
                    const double sp = fmax(t, 0.0) + log1p(exp(-fabs(t)));
                    c = c + 2.0 * ((LOG_2 - u) - sp);
                }
            }
        }
    }
    log_prob = correction ? lp - c : lp;
    entropy = e;
}

// Two waves per SIMD are asked for where the kernel fits them without scratch (none, value: 226-230 registers).  The categorical and the
// Gaussian kernel come out 6 to 8 registers above 256; held to 256 they spill 2 to 4 registers to scratch, so they are left at one wave
// per SIMD and no scratch (profiles/policy_eval.md).
constexpr int eval_waves(int head) { return head == GEMX_EVAL_HEAD_NONE || head == GEMX_EVAL_HEAD_VALUE ? 2 : 1; }

template <int HEAD>
__global__ __launch_bounds__(EVAL_BLOCK, eval_waves(HEAD)) void policy_eval_kernel(const EvalDev a) {
    using namespace gemx;
    extern __shared__ float lds[];  // the blob
    for (int w = threadIdx.x; w < a.blob_words; w += EVAL_BLOCK) lds[w] = a.blob[w];
    __syncthreads();
    const int64_t N = a.N;
    uint32_t bad_action = 0;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        // (the widths redefined per tile by an empty asm: the comparisons of the unrolled loops against them are then made where they are
        // used, not once in front of the tile loop and held in -- and spilled from -- some hundred scalar registers)
        int S = a.n_state, n_ref = a.n_ref, n_out = a.n_out;
        asm volatile("" : "+s"(S), "+s"(n_ref), "+s"(n_out));
        const int64_t row = tile * EVAL_BLOCK + threadIdx.x;
        const bool valid = row < a.total;
        const int64_t r = valid ? row : a.total - 1;  // tail lanes recompute the last row; their stores are masked
        const int64_t k = r / N, e = r - k * N;
        const bool last_row = k >= a.K;  // (the row behind the stored ones: GEMX_EVAL_LAST)
        // ---- the row gather: the previous row or the reset row, selected by the `ended` byte; the references of the mode and the form
        const float *src, *rsrc = nullptr;
        if (a.next) {
            src = a.rows + r * S;
            if (n_ref > 0) rsrc = a.refs + r * n_ref;
        } else {
            const int64_t prev = r - N;  // row k-1 of the same env
            if (k == 0) src = a.obs0 + e * S;
            else if (a.ended[prev] != 0) src = a.reset_obs + (a.reset_per_env ? e * S : (int64_t)0);
            else src = a.rows + prev * S;
            if (n_ref > 0) {
                if (a.refs0 != nullptr) rsrc = k == 0 ? a.refs0 + e * n_ref : a.refs + prev * n_ref;
                else rsrc = last_row ? a.last_refs + e * n_ref : a.refs + r * n_ref;
            }
        }
        float op[GEMX_MAX_OUT], rf[GEMX_MAX_REF];
#pragma unroll
        for (int c = 0; c < GEMX_MAX_OUT; ++c) op[c] = c < S ? src[c] : 0.0f;
#pragma unroll
        for (int q = 0; q < GEMX_MAX_REF; ++q) rf[q] = q < n_ref ? rsrc[q] : 0.0f;

        // ---- the MLP, policy_rollout_kernel's chains.  Layer 0: per 8-output block, the columns in ascending column order
        const pl_v8 zero8 = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        PlAct ha = {zero8, zero8, zero8, zero8, zero8, zero8, zero8, zero8};
        const float *lw = lds;
        {
            const int rows = a.n_in, jb_n = (a.width[0] + 7) >> 3;
            const float *bias = lw + jb_n * rows * 8;
#pragma nounroll
            for (int jb = 0; jb < jb_n; ++jb) {
                const float *wb = lw + jb * rows * 8;
                pl_v8 acc = pl_load8(bias + 8 * jb);
                // The inputs redefined per block by an empty asm (no instruction, the values unchanged): without it the packed-FMA operand
                // pairs {x, x} of all 28 inputs, one pair per use, were built in front of this loop and held across it -- 224 registers, spilled
#pragma unroll
                for (int c = 0; c < GEMX_MAX_OUT; ++c) asm volatile("" : "+v"(op[c]));
#pragma unroll
                for (int q = 0; q < GEMX_MAX_REF; ++q) asm volatile("" : "+v"(rf[q]));
#pragma unroll
                for (int c = 0; c < GEMX_MAX_OUT; ++c) {
                    int i = a.pos[c];
                    asm volatile("" : "+s"(i));  // (as S above: the 24 conditions and weight addresses are made here, not held in scalar registers)
                    if (c < S && i >= 0) pl_fma8(wb + i * 8, op[c], acc);
                }
#pragma unroll
                for (int q = 0; q < GEMX_MAX_REF; ++q)
                    if (q < n_ref) pl_fma8(wb + (a.n_cols + q) * 8, rf[q], acc);
                if (a.n_layers > 1) pl_activate(a.activation, acc);
                pl_scatter(jb, acc, ha);
            }
            lw = bias + 8 * jb_n;
        }
        // later layers: ha -> hb (-> ha), the inputs in order, skipped in blocks of 8 past the previous layer's (padded) width.  One 8-output
        // block at a time (8 independent chains; the other resident wave covers their latency): per output the order is input 0, 1, ... as
        // in the rollout kernel, which runs all blocks side by side -- the same chains, fewer live registers
        auto dense = [&](int l, const PlAct &in, PlAct &out) {
            const int rows = (a.width[l - 1] + 7) & ~7, jb_n = (a.width[l] + 7) >> 3;
            const float *bias = lw + jb_n * rows * 8;
#pragma nounroll
            for (int jb = 0; jb < jb_n; ++jb) {
                const float *wb = lw + jb * rows * 8;  // row 0 of output block jb
                pl_v8 acc = pl_load8(bias + 8 * jb);
#pragma nounroll
                for (int ib = 0; 8 * ib < rows; ++ib) pl_in_block(wb + 64 * ib, pl_pick(in, ib), acc);  // (a runtime loop: unrolled, the operand pairs {x, x} of the packed FMAs of all 64 inputs were held across the block loop)
                if (l + 1 < a.n_layers) pl_activate(a.activation, acc);
                pl_scatter(jb, acc, out);
            }
            lw = bias + 8 * jb_n;
        };
        if (a.n_layers > 1) {
            PlAct hb = {zero8, zero8, zero8, zero8, zero8, zero8, zero8, zero8};
            dense(1, ha, hb);
            if (a.n_layers > 2) dense(2, hb, ha);
            else ha = hb;
        }
        // ---- the head, in the same lane
        if constexpr (HEAD == GEMX_EVAL_HEAD_NONE) {
            if (valid) {
                float *dst = last_row ? a.out_last + e * n_out : a.out + r * n_out;
#pragma nounroll
                for (int b = 0; 8 * b < n_out; ++b) {
                    const pl_v8 v = pl_pick(ha, b);
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (8 * b + q < n_out) dst[8 * b + q] = v[q];
                }
            }
        } else if constexpr (HEAD == GEMX_EVAL_HEAD_VALUE) {
            if (valid) {
                if (last_row) eval_store(a.value_last, e, (double)ha.b0[0], a.f64);
                else eval_store(a.value, r, (double)ha.b0[0], a.f64);
            }
        } else if constexpr (HEAD == GEMX_EVAL_HEAD_CATEGORICAL) {
            const uint32_t act = a.actions[r];
            double lp, h;
            head_categorical(ha, n_out, act, lp, h);
            if (valid) {
                bad_action |= act >= (uint32_t)n_out;
                if (a.log_prob != nullptr) eval_store(a.log_prob, r, lp, a.f64);
                if (a.entropy != nullptr) eval_store(a.entropy, r, h, a.f64);
            }
        } else {
            double lp, h;
            head_gaussian(ha, n_out, a.pre_squash + r * n_out, a.log_std, a.squash_correction != 0, lp, h);
            if (valid) {
                if (a.log_prob != nullptr) eval_store(a.log_prob, r, lp, a.f64);
                if (a.entropy != nullptr) eval_store(a.entropy, r, h, a.f64);
            }
        }
    }
    if (bad_action && a.err != nullptr) atomicOr(a.err, GEMX_ERRFLAG_ACTION);
}

template <int HEAD>
void eval_launch(unsigned blocks, size_t lds, hipStream_t st, const EvalDev &a) {
    hipLaunchKernelGGL(policy_eval_kernel<HEAD>, dim3(blocks), dim3(EVAL_BLOCK), lds, st, a);
}

}  // namespace

extern "C" {

int gemx_policy_eval_rows(const gemx_policy *p, const gemx_policy_eval_call *call, int64_t n_envs, int32_t K, int device, void *stream) {
    static const char *const what = "policy evaluation";
    using gemx::fail;
    if (!p || !call) return fail(GEMX_ERR_ARG, "%s: the policy and the call must not be null", what);
    if (call->struct_size != (int32_t)sizeof(gemx_policy_eval_call)) return fail(GEMX_ERR_ARG, "gemx_policy_eval_call size mismatch");
    const gemx_policy_eval_call &c = *call;
    if (c.mode != GEMX_EVAL_SEEN && c.mode != GEMX_EVAL_NEXT) return fail(GEMX_ERR_ARG, "%s: unknown mode %d", what, c.mode);
    if (c.head < GEMX_EVAL_HEAD_NONE || c.head > GEMX_EVAL_HEAD_GAUSSIAN) return fail(GEMX_ERR_ARG, "%s: unknown head %d", what, c.head);
    if (c.flags & ~(GEMX_EVAL_LAST | GEMX_EVAL_SQUASH_CORRECTION)) return fail(GEMX_ERR_ARG, "%s: unknown flags %d", what, c.flags);
    if (c.out_dtype != GEMX_F32 && c.out_dtype != GEMX_F64) return fail(GEMX_ERR_ARG, "%s: unknown out_dtype %d", what, c.out_dtype);
    if (c.reserved != 0 || (c.reset_per_env != 0 && c.reset_per_env != 1)) return fail(GEMX_ERR_ARG, "%s: reserved must be 0 and reset_per_env 0 or 1", what);
    if (K < 1) return fail(GEMX_ERR_ARG, "%s: K must be >= 1", what);
    if (n_envs < 1) return fail(GEMX_ERR_ARG, "%s: n_envs must be >= 1", what);
    if (c.n_state < 1 || c.n_state > GEMX_MAX_OUT) return fail(GEMX_ERR_ARG, "%s: n_state = %d; 1 to %d", what, c.n_state, GEMX_MAX_OUT);
    if (c.n_ref < 0 || c.n_ref > GEMX_MAX_REF) return fail(GEMX_ERR_ARG, "%s: n_ref = %d; 0 to %d", what, c.n_ref, GEMX_MAX_REF);
    if (c.n_cols < 0 || c.n_cols > c.n_state) return fail(GEMX_ERR_ARG, "%s: n_cols = %d; 0 to %d", what, c.n_cols, c.n_state);
    if (c.n_cols + c.n_ref != p->n_in)
        return fail(GEMX_ERR_ARG, "%s: %d observation columns + %d references = %d inputs, the policy's first layer takes %d", what, c.n_cols, c.n_ref, c.n_cols + c.n_ref, p->n_in);
    EvalDev a;
    memset(&a, 0, sizeof(a));
    for (int j = 0; j < GEMX_MAX_OUT; ++j) a.pos[j] = -1;
    for (int i = 0; i < c.n_cols; ++i) {
        const int col = c.columns[i];
        if (col < 0 || col >= c.n_state) return fail(GEMX_ERR_ARG, "%s: columns[%d] = %d is outside the row of %d columns", what, i, col, c.n_state);
        if (a.pos[col] >= 0) return fail(GEMX_ERR_ARG, "%s: column %d is selected twice", what, col);
        a.pos[col] = (int8_t)i;
    }
    const bool last = (c.flags & GEMX_EVAL_LAST) != 0, next = c.mode == GEMX_EVAL_NEXT, complete = c.refs0_dev != nullptr;
    const int n_out = p->width[p->n_layers - 1];
    // the tensors of the mode
    if (!c.rows_dev && (next || K > 1 || last)) return fail(GEMX_ERR_ARG, "%s: rows_dev must not be null", what);
    if (next) {
        if (last) return fail(GEMX_ERR_ARG, "%s: GEMX_EVAL_LAST has no meaning with GEMX_EVAL_NEXT (there is no row behind the last one)", what);
        if (c.obs0_dev || c.ended_dev || c.reset_obs_dev || c.refs0_dev || c.last_refs_dev)
            return fail(GEMX_ERR_ARG, "%s: GEMX_EVAL_NEXT reads rows_dev and refs_dev only: obs0_dev, ended_dev, reset_obs_dev, refs0_dev and last_refs_dev must be null", what);
    } else {
        if (!c.obs0_dev) return fail(GEMX_ERR_ARG, "%s: obs0_dev must not be null", what);
        if ((K > 1 || last) && (!c.ended_dev || !c.reset_obs_dev)) return fail(GEMX_ERR_ARG, "%s: ended_dev and reset_obs_dev must not be null", what);
        if (c.n_ref > 0 && last && !complete && !c.last_refs_dev) return fail(GEMX_ERR_ARG, "%s: last_refs_dev must not be null with GEMX_EVAL_LAST in the physics-only form", what);
        if (c.last_refs_dev && (!last || complete)) return fail(GEMX_ERR_ARG, "%s: last_refs_dev is read with GEMX_EVAL_LAST in the physics-only form only", what);
    }
    if (c.n_ref > 0 && !c.refs_dev && (!complete || K > 1 || last)) return fail(GEMX_ERR_ARG, "%s: refs_dev must not be null with n_ref = %d", what, c.n_ref);
    if (c.n_ref == 0 && (c.refs_dev || c.refs0_dev || c.last_refs_dev)) return fail(GEMX_ERR_ARG, "%s: reference tensors given with n_ref = 0", what);
    // the tensors of the head
    const bool none = c.head == GEMX_EVAL_HEAD_NONE, value = c.head == GEMX_EVAL_HEAD_VALUE, cat = c.head == GEMX_EVAL_HEAD_CATEGORICAL, gauss = c.head == GEMX_EVAL_HEAD_GAUSSIAN;
    if (value && n_out != 1) return fail(GEMX_ERR_ARG, "%s: the value head needs a policy with one output, this one has %d", what, n_out);
    if ((cat || gauss) && last) return fail(GEMX_ERR_ARG, "%s: GEMX_EVAL_LAST with the categorical or the Gaussian head (no action was taken behind the last row)", what);
    if (none != (c.out_dev != nullptr) || (none && last) != (c.out_last_dev != nullptr)) return fail(GEMX_ERR_ARG, "%s: out_dev (and out_last_dev with GEMX_EVAL_LAST) belong to GEMX_EVAL_HEAD_NONE", what);
    if (value != (c.value_out_dev != nullptr) || (value && last) != (c.value_last_dev != nullptr))
        return fail(GEMX_ERR_ARG, "%s: value_out_dev (and value_last_dev with GEMX_EVAL_LAST) belong to GEMX_EVAL_HEAD_VALUE", what);
    if ((cat || gauss) ? (!c.log_prob_out_dev && !c.entropy_out_dev) : (c.log_prob_out_dev || c.entropy_out_dev))
        return fail(GEMX_ERR_ARG, "%s: log_prob_out_dev / entropy_out_dev: at least one with the categorical and the Gaussian head, none otherwise", what);
    if (cat != (c.actions_dev != nullptr)) return fail(GEMX_ERR_ARG, "%s: actions_dev belongs to GEMX_EVAL_HEAD_CATEGORICAL", what);
    if (gauss != (c.pre_squash_dev != nullptr) || gauss != (c.log_std_dev != nullptr)) return fail(GEMX_ERR_ARG, "%s: pre_squash_dev and log_std_dev belong to GEMX_EVAL_HEAD_GAUSSIAN", what);
    if ((c.flags & GEMX_EVAL_SQUASH_CORRECTION) && !gauss) return fail(GEMX_ERR_ARG, "%s: GEMX_EVAL_SQUASH_CORRECTION belongs to GEMX_EVAL_HEAD_GAUSSIAN", what);
    const bool f64 = c.out_dtype == GEMX_F64;
    if (!gemx::elem_aligned(false, c.obs0_dev, c.rows_dev, c.reset_obs_dev, c.refs_dev, c.refs0_dev, c.last_refs_dev, c.pre_squash_dev, c.log_std_dev, c.out_dev, c.out_last_dev) ||
        !gemx::elem_aligned(f64, c.value_out_dev, c.value_last_dev, c.log_prob_out_dev, c.entropy_out_dev))
        return gemx::fail_unaligned();
    if (int rc = gemx::check_device_dtype(device, c.out_dtype)) return rc;
    if (p->device != device) return fail(GEMX_ERR_ARG, "%s: the policy lives on device %d, the call names device %d", what, p->device, device);
    if (c.error_handle && c.error_handle->device != device) return fail(GEMX_ERR_ARG, "%s: error_handle lives on device %d, the call names device %d", what, c.error_handle->device, device);
    const int64_t rows_k = (int64_t)K + (last ? 1 : 0);
    if (n_envs > 0x7fffffffffffffffLL / (rows_k * 4 * GEMX_MAX_OUT * gemx::PL_MAX_WIDTH)) return fail(GEMX_ERR_ARG, "%s: (K + 1) * n_envs rows exceed the 64-bit byte offsets", what);

    a.blob = p->blob;
    a.blob_words = p->blob_words;
    a.n_layers = p->n_layers;
    a.n_in = p->n_in;
    for (int l = 0; l < gemx::PL_MAX_LAYERS; ++l) a.width[l] = p->width[l];
    a.activation = p->activation;
    a.n_cols = c.n_cols;
    a.n_ref = c.n_ref;
    a.n_state = c.n_state;
    a.n_out = n_out;
    a.next = next ? 1 : 0;
    a.squash_correction = (c.flags & GEMX_EVAL_SQUASH_CORRECTION) ? 1 : 0;
    a.f64 = f64 ? 1 : 0;
    a.reset_per_env = c.reset_per_env;
    a.obs0 = c.obs0_dev; a.rows = c.rows_dev; a.reset_obs = c.reset_obs_dev; a.ended = c.ended_dev;
    a.refs = c.refs_dev; a.refs0 = c.refs0_dev; a.last_refs = c.last_refs_dev;
    a.actions = c.actions_dev; a.pre_squash = c.pre_squash_dev; a.log_std = c.log_std_dev;
    a.out = c.out_dev; a.out_last = c.out_last_dev;
    a.value = c.value_out_dev; a.value_last = c.value_last_dev; a.log_prob = c.log_prob_out_dev; a.entropy = c.entropy_out_dev;
    a.err = c.error_handle ? c.error_handle->err : nullptr;
    a.N = n_envs;
    a.K = K;
    a.total = rows_k * n_envs;
    a.tiles = (a.total + EVAL_BLOCK - 1) / EVAL_BLOCK;

    gemx::DeviceGuard guard(device);
    static int n_cu[64] = {0};  // compute units per device, asked once
    if (device < 64 && n_cu[device] == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v < 1) v = 256;
        n_cu[device] = v;
    }
    const int64_t resident = eval_waves(c.head) * (int64_t)(device < 64 ? n_cu[device] : 256);  // workgroups of four waves, one per SIMD each
    const unsigned blocks = (unsigned)(a.tiles < resident ? a.tiles : resident);
    const size_t lds = sizeof(float) * (size_t)a.blob_words;
    hipStream_t st = (hipStream_t)stream;
    switch (c.head) {
    case GEMX_EVAL_HEAD_NONE: gemx_cov_note("policy_eval_kernel<0>"); eval_launch<GEMX_EVAL_HEAD_NONE>(blocks, lds, st, a); break;
    case GEMX_EVAL_HEAD_VALUE: gemx_cov_note("policy_eval_kernel<1>"); eval_launch<GEMX_EVAL_HEAD_VALUE>(blocks, lds, st, a); break;
    case GEMX_EVAL_HEAD_CATEGORICAL: gemx_cov_note("policy_eval_kernel<2>"); eval_launch<GEMX_EVAL_HEAD_CATEGORICAL>(blocks, lds, st, a); break;
    default: gemx_cov_note("policy_eval_kernel<3>"); eval_launch<GEMX_EVAL_HEAD_GAUSSIAN>(blocks, lds, st, a);
    }
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

}  // extern "C"
