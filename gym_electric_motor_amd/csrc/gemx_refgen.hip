// gemx_refgen.hip -- device-side reference generation (second half): N x n_ref independent
// WienerProcessReferenceGenerator streams, i.e. what `MultipleReferenceGenerator([WienerProcessReferenceGenerator(...)] * n_ref)`
// produces for N envs.  Reference (paths relative to src/gym_electric_motor/reference_generators/):
//   SubepisodedReferenceGenerator  subepisoded_reference_generator.py:66-119  (sub-episodes of int(U(len_lo, len_hi)) steps;
//                                  reset(): reference value := initial reference, a new sub-episode starts at once)
//   WienerProcessReferenceGenerator wiener_process_reference_generator.py:30-49 (per sub-episode sigma = 10 ** U(log10 sigma_range),
//                                  value += N(0, sigma) per step, clipped to the limit margin; reset(): initial value ~ U(initial_range))
//   MultipleReferenceGenerator      multiple_reference_generator.py:77-92       (independent sub-generators, concatenated)
// numpy's PCG64 streams cannot be reproduced on a device: parity is DISTRIBUTIONAL (tests/test_gpu_parity.py); the arithmetic of the
// clipped random walk is the reference's.  Randomness: counter-based Philox4x32-10 (gemx_common.hpp) indexed by
// (seed; env, generator, draw kind, draw index), so chunked == one-shot generation and no RNG state is stored.
//
// Two kernels per rollout: (1) all K*N*n_ref standard normals in parallel, written into the output tensor; (2) one lane per
// (env, generator) walks its K steps sequentially: scale by the sub-episode's sigma, accumulate, clip, restart on `done`.
// One kernel per env-shell step (gemx_refgen_step): one lane per env resets its generators on `done`, draws the step's normal inline and
// advances every generator by one step -- the same draws, the same double arithmetic, hence the same bits as a rollout.
// K such steps in one call (gemx_refgen_rollout_shell): the two rollout kernels with the reset of done[k] BEFORE row k, the env shell's order.
// The step index of the normal draws lives on the device, per (generator, env) like the other counters (every lane advances its own:
// no lane reads a counter another lane writes), so a replayed HIP graph of steps advances the streams.
//
// The reference's other kinds (gemx_refgen_create_kinds; second half of this file): Laplace walk, sinusoidal, step, triangular, sawtooth
// and constant columns, freely mixed with Wiener columns.  ONE kernel (refgen_kinds_kernel) serves reset, rollout and step: one lane per
// (env, column) keeps the sub-episode's drawn parameters in SoA arrays and evaluates its waveform in closed form at its step index --
// nothing is tabulated.  A Wiener column there makes the draws and the arithmetic of the kernels above: the same bits.
//
// SwitchedReferenceGenerator (gemx_refgen_create_switched; last part of the kernels): a column that runs one of several alternatives per
// super-episode.  A kernel of its own (refgen_switched_kernel) beside the kinds kernel, on the same helpers; handles without such a column
// launch what they launched before.
#include "gemx_support.hpp"

// the head of a checkpoint blob (gemx_refgen_get_blob): who may take the arrays behind it.  64 bytes; kept in the handle, so that the
// asynchronous copy into a blob reads memory that outlives the call
struct RefgenBlobHeader {
    uint32_t magic, owners;  // owners: the OWN_* bits of the arrays that follow (plain / kinds / switched handle)
    int64_t n_envs;
    int32_t n_ref, reserved;
    int64_t env_base, bytes;     // bytes: of the whole blob, gemx_refgen_state_bytes
    int32_t column[GEMX_MAX_REF];  // per column: its kind | the number of its alternatives << 8 (a plain handle: Wiener columns)
    int64_t pad;
};
static_assert(sizeof(RefgenBlobHeader) == GEMX_REFGEN_BLOB_HEADER_BYTES, "the blob header is 64 bytes");

struct gemx_refgen {
    gemx_refgen_config cfg;
    int64_t n;
    int device, f64;
    // per (generator, env): current reference value, steps left in the sub-episode, sigma, sub-episode / reset counters
    double *value = nullptr, *sigma = nullptr;
    int32_t *left = nullptr;
    uint32_t *n_sub = nullptr, *n_reset = nullptr;
    uint64_t *t = nullptr;  // steps generated so far (index of the per-step normal draws)
    // handles of gemx_refgen_create_kinds: a kind per column (`cfg` then holds the Wiener view of the columns; `mixed`: the handle runs
    // refgen_kinds_kernel, else its columns are all Wiener and it runs the kernels above) and, per (column, env), the sub-episode's
    // length, the waveform's parameters par[6][n_ref][N] (amplitude, frequency, offset, phase, width | ratio, roll)
    gemx_refgen_kinds_config kcfg;
    int has_kinds = 0, mixed = 0;
    int32_t *len = nullptr;
    double *par = nullptr;
    // handles of gemx_refgen_create_switched with a switched column (`switched`: the handle runs refgen_switched_kernel; `kcfg` then holds
    // alternative 0 of every column): per (column, env) the current alternative, the super-episode's step counter and length, the
    // super-episodes drawn so far; `sdev`: the kernel's description (RefgenSwitchedDev), derived once
    int switched = 0;
    int32_t *alt = nullptr, *sk = nullptr, *slen = nullptr;
    uint32_t *n_super = nullptr;
    void *sdev = nullptr;
    RefgenBlobHeader blob_head;  // written by every gemx_refgen_get_blob, read by its copy
    void *dev_desc = nullptr;    // RefgenDev of `cfg` in device memory, made by the first complete policy rollout (refgen_policy_view)
};

namespace {

// the draws, the sub-episode, the restart and the clipped walk of one (column, env): gemx_refgen_lane.hpp, through gemx_support.hpp (shared
// with the complete policy rollout units, which step the generators in the lane that steps the env)
using namespace gemx::refgen_lane;

// (1) standard normals for steps t .. t+K-1 of every (env, generator), t = the (generator, env)'s step counter
template <class R>
__global__ void refgen_normals_kernel(R *out, int64_t N, int n_ref, int K, uint64_t seed, const uint64_t *t, int64_t env_base) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)K * N * n_ref;
    if (idx >= total) return;
    const int g = (int)(idx % n_ref);
    const int64_t env = (idx / n_ref) % N;
    const int64_t k = idx / ((int64_t)n_ref * N);
    out[idx] = step_normal<R>(seed, env_base + env, g, t[(int64_t)g * N + env] + (uint64_t)k);
}

// (2) out[k][env][g] holds z on entry and the reference of step k on exit.  done[k][env] != 0: the env terminated in step k, its
// generators are reset before the reference of step k+1 is produced (env.reset() -> reference_generator.reset(), core.py:312-313).
// done_first (gemx_refgen_rollout_shell, the env shell's order): the reset of done[k][env] comes BEFORE row k instead -- row k is then what
// refgen_step_kernel produces with the mask done[k].
template <class R>
__global__ void refgen_walk_kernel(R *out, const uint8_t *done, int done_first, const uint8_t *reset_mask, int reset_all, int64_t N, int K, RefgenDev G,
                                   double *value, double *sigma, int32_t *left, uint32_t *n_sub, uint32_t *n_reset, uint64_t *t) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * G.n_ref) return;
    const int g = (int)(idx % G.n_ref);
    const int64_t env = idx / G.n_ref;
    const int64_t si = (int64_t)g * N + env;
    double v = value[si], sg = sigma[si];
    int32_t lf = left[si];
    uint32_t ns = n_sub[si], nr = n_reset[si];
    if (K == 0) {  // gemx_refgen_reset: the masked envs, or all of them (reset_all: no mask buffer at all)
        if (reset_all || (reset_mask != nullptr && reset_mask[env])) reset_generator(G, env, g, nr, ns, lf, sg, v);
    }
    for (int k = 0; k < K; ++k) {
        const int64_t o = ((int64_t)k * N + env) * G.n_ref + g;
        const bool dn = done != nullptr && done[(int64_t)k * N + env];
        if (dn && done_first) reset_generator(G, env, g, nr, ns, lf, sg, v);
        if (lf <= 0) new_subepisode(G, env, g, ns, lf, sg);
        v = walk_step(G, g, v, sg, (double)out[o]);
        --lf;
        out[o] = (R)v;
        if (dn && !done_first) reset_generator(G, env, g, nr, ns, lf, sg, v);
    }
    value[si] = v; sigma[si] = sg; left[si] = lf; n_sub[si] = ns; n_reset[si] = nr;
    if (K > 0) t[si] += (uint64_t)K;
}

// (3) one env-shell step, one lane per env: reset on done, then advance every generator by one step; row [n_ref] of `out` written at once
// (VEC: n_ref in {2, 4} and an aligned tensor -> one vector store per lane)
template <class R, int VEC>
__global__ void refgen_step_kernel(R *out, const uint8_t *done, int64_t N, RefgenDev G, double *value, double *sigma, int32_t *left,
                                   uint32_t *n_sub, uint32_t *n_reset, uint64_t *t) {
    const int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    const bool dn = done != nullptr && done[env];
    R row[GEMX_MAX_REF];
#pragma unroll
    for (int g = 0; g < GEMX_MAX_REF; ++g) {
        if (g >= G.n_ref) break;
        const int64_t si = (int64_t)g * N + env;
        double v = value[si], sg = sigma[si];
        int32_t lf = left[si];
        uint32_t ns = n_sub[si], nr = n_reset[si];
        const uint64_t ti = t[si];
        if (dn) reset_generator(G, env, g, nr, ns, lf, sg, v);
        if (lf <= 0) new_subepisode(G, env, g, ns, lf, sg);
        v = walk_step(G, g, v, sg, (double)step_normal<R>(G.seed, G.env_base + env, g, ti));
        --lf;
        value[si] = v; sigma[si] = sg; left[si] = lf; n_sub[si] = ns; n_reset[si] = nr; t[si] = ti + 1;
        row[g] = (R)v;
    }
    if constexpr (VEC == 2) {
        struct alignas(2 * sizeof(R)) V2 { R a, b; };
        reinterpret_cast<V2 *>(out)[env] = V2{row[0], row[1]};
    } else if constexpr (VEC == 4) {
        struct alignas(sizeof(R) == 4 ? 16 : 32) V4 { R a, b, c, d; };
        reinterpret_cast<V4 *>(out)[env] = V4{row[0], row[1], row[2], row[3]};
    } else {
#pragma unroll
        for (int g = 0; g < GEMX_MAX_REF; ++g)
            if (g < G.n_ref) out[env * G.n_ref + g] = row[g];
    }
}

RefgenDev make_dev(const gemx_refgen_config &c) {
    RefgenDev G;
    memset(&G, 0, sizeof(G));
    G.n_ref = c.n_ref; G.len_lo = c.episode_len_lo; G.len_hi = c.episode_len_hi; G.seed = c.seed; G.env_base = c.env_base;
    for (int g = 0; g < c.n_ref; ++g) {
        G.log_sig_lo[g] = log10(c.sigma_lo[g]); G.log_sig_hi[g] = log10(c.sigma_hi[g]);
        G.m_lo[g] = c.margin_lo[g]; G.m_hi[g] = c.margin_hi[g]; G.i_lo[g] = c.initial_lo[g]; G.i_hi[g] = c.initial_hi[g];
    }
    return G;
}

template <class R> int walk(gemx_refgen *r, void *out, const uint8_t *done, int done_first, const uint8_t *mask, int reset_all, int K, hipStream_t st) {
    const int64_t lanes = r->n * r->cfg.n_ref;
    gemx_cov_note(sizeof(R) == 4 ? "refgen_walk_kernel<float>" : "refgen_walk_kernel<double>");
    hipLaunchKernelGGL(refgen_walk_kernel<R>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, (R *)out, done, done_first, mask, reset_all, r->n, K, make_dev(r->cfg),
                       r->value, r->sigma, r->left, r->n_sub, r->n_reset, r->t);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

template <class R> int step(gemx_refgen *r, void *out, const uint8_t *done, hipStream_t st) {
    const int n_ref = r->cfg.n_ref;
    // one vector store per row where the rows are 2 or 4 wide and the tensor is aligned to them
    const int vec = ((n_ref == 2 || n_ref == 4) && (uintptr_t)out % (n_ref * sizeof(R)) == 0) ? n_ref : 1;
    gemx_cov_note(sizeof(R) == 4 ? "refgen_step_kernel<float>" : "refgen_step_kernel<double>");
    const dim3 grid((unsigned)((r->n + 255) / 256)), block(256);
    const RefgenDev G = make_dev(r->cfg);
#define GEMX_REFGEN_STEP(V) hipLaunchKernelGGL((refgen_step_kernel<R, V>), grid, block, 0, st, (R *)out, done, r->n, G, r->value, r->sigma, r->left, r->n_sub, r->n_reset, r->t)
    if (vec == 2) GEMX_REFGEN_STEP(2);
    else if (vec == 4) GEMX_REFGEN_STEP(4);
    else GEMX_REFGEN_STEP(1);
#undef GEMX_REFGEN_STEP
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

// ---- the other generator kinds (paths relative to reference_generators/) ----------------------------------------------------------------
// Draw layout of a column, all blocks keyed (seed; global env, column, draw kind, index):
//   DRAW_STEP  index t      word 0, 1: the step's normal (Wiener)          | word 0: the step's Laplace increment (Laplace)
//   DRAW_SUB   index n_sub  word 0: sub-episode length (every kind)        | word 1: sigma (Wiener, Laplace) or amplitude; word 2: frequency;
//                           word 3: offset
//   DRAW_SUB2  index n_sub  word 0: phase (sinus, triangular, sawtooth) or the high/low ratio (step); word 1: width (triangular) or the
//                           roll's phase (step)
//   DRAW_RESET index n_reset word 0: initial value (Wiener only; the other kinds restart from 0 and draw nothing)
enum { DRAW_SUB2 = 3 };
enum { PAR_AMP = 0, PAR_FREQ = 1, PAR_OFF = 2, PAR_PHASE = 3, PAR_WIDTH = 4, PAR_ROLL = 5, N_PAR = 6 };

// The description of a handle's columns, a kernel argument: S slots of one generator kind each.  A kinds handle has one slot per column
// (RefgenKindsDev); a switched handle has GEMX_MAX_ALT per column, alternative a of column g at slot g * GEMX_MAX_ALT + a, and -- only
// it -- the super-episodes' description (RefgenSwitchedDev, 2560 B).
constexpr int ALT_SLOTS = GEMX_MAX_REF * GEMX_MAX_ALT;
struct NoSuperDev {};
struct SuperDev {
    int32_t n_alt[GEMX_MAX_REF], sup_lo[GEMX_MAX_REF], sup_hi[GEMX_MAX_REF];  // n_alt = 0: a plain column
    double cdf[ALT_SLOTS];                                                    // running sums of p
};
struct DescriptionHead {
    int32_t n_ref;
    uint64_t seed;
    int64_t env_base;
    double tau;
};
template <int S> struct RefgenDescription : DescriptionHead, std::conditional_t<S == ALT_SLOTS, SuperDev, NoSuperDev> {
    int32_t kind[S], len_lo[S], len_hi[S];
    double log_sig_lo[S], log_sig_hi[S], m_lo[S], m_hi[S], i_lo[S], i_hi[S];
    double a_lo[S], a_hi[S], f_lo[S], f_hi[S], o_lo[S], o_hi[S], c[S];
};
using RefgenKindsDev = RefgenDescription<GEMX_MAX_REF>;
using RefgenSwitchedDev = RefgenDescription<ALT_SLOTS>;

struct KindLane {  // the state of one (column, env), in registers
    double v, sg, amp, freq, off, phase, width, roll;
    int32_t lf, len;
    uint32_t ns, nr;
    uint64_t t;
};

__device__ inline double clip(double x, double a, double b) { return fmin(fmax(x, a), b); }  // np.clip: min(max(x, a), b), also for a > b
__device__ inline double uniform(double lo, double hi, uint32_t w) { return (hi - lo) * gemx::Philox::u01(w) + lo; }  // _get_current_value, 112-119

// scipy.signal.sawtooth(x, w), restated: m = x mod 2 pi; rising from -1 to 1 on [0, 2 pi w), falling back on [2 pi w, 2 pi)
__device__ inline double sawtooth(double x, double w) {
    const double m = fmod(x, gemx::kTwoPi);  // (x >= 0: fmod is numpy's mod)
    return m < gemx::kTwoPi * w ? m / (gemx::kPi * w) - 1.0 : (gemx::kPi * (w + 1.0) - m) / (gemx::kPi * (1.0 - w));
}

// get_reference_observation, subepisoded_reference_generator.py:93-99, and the kinds' _reset_reference: length, then the parameters in the
// reference's order (amplitude, frequency, offset, extras)
template <class Dev> __device__ inline void kinds_new_subepisode(const Dev &G, int64_t env, int g, int c, KindLane &s) {
    uint32_t r[4], q[4];
    const int kind = G.kind[c];
    refgen_block(G.seed, G.env_base + env, g, DRAW_SUB, s.ns, r);
    s.len = (int32_t)((double)(G.len_hi[c] - G.len_lo[c]) * gemx::Philox::u01(r[0]) + (double)G.len_lo[c]);
    s.lf = s.len;
    if (kind == GEMX_REF_WIENER || kind == GEMX_REF_LAPLACE) {  // wiener ... :31, laplace ... :27
        s.sg = pow(10.0, (G.log_sig_hi[c] - G.log_sig_lo[c]) * gemx::Philox::u01(r[1]) + G.log_sig_lo[c]);
    } else {
        refgen_block(G.seed, G.env_base + env, g, DRAW_SUB2, s.ns, q);
        s.amp = uniform(G.a_lo[c], G.a_hi[c], r[1]);
        s.freq = uniform(G.f_lo[c], G.f_hi[c], r[2]);
        // sinusoidal ... :53-57 (triangle, sawtooth alike): [-m_hi + A, m_hi - A]; step_reference_generator.py:41-45: [m_lo + A, m_hi - A]
        const double lo = (kind == GEMX_REF_STEP ? G.m_lo[c] : -G.m_hi[c]) + s.amp, hi = G.m_hi[c] - s.amp;
        s.off = uniform(clip(G.o_lo[c], lo, hi), clip(G.o_hi[c], lo, hi), r[3]);
        const double u0 = gemx::Philox::u01(q[0]), u1 = gemx::Philox::u01(q[1]);
        s.phase = 0.0; s.width = 1.0; s.roll = 0.0;
        if (kind == GEMX_REF_STEP) {
            s.width = u0 < 0.5 ? sqrt(0.5 * u0) : 1.0 - sqrt(0.5 * (1.0 - u0));  // Triangular(0, 0.5, 1) by its inverse distribution function
            s.roll = floor(fmin(1.0 / s.freq / G.tau * u1, 2147483647.0));      // int(steps_per_period * phase), :56-58
        } else {
            s.phase = u0 * 2.0 * gemx::kPi;
            if (kind == GEMX_REF_TRIANGULAR) s.width = u1;
        }
    }
    ++s.ns;
}

// reset(): Wiener draws its initial value (wiener ... :43-49), every other sub-episoded kind restarts from 0 (subepisoded ... :80-86);
// a new sub-episode starts with the next step.  (Constant columns never get here: the kernels write their value and return.)
template <class Dev> __device__ inline void kinds_reset(const Dev &G, int64_t env, int g, int c, KindLane &s) {
    const int kind = G.kind[c];
    if (kind == GEMX_REF_WIENER) {
        uint32_t r[4];
        refgen_block(G.seed, G.env_base + env, g, DRAW_RESET, s.nr++, r);
        s.v = (G.i_hi[c] - G.i_lo[c]) * gemx::Philox::u01(r[0]) + G.i_lo[c];
    } else {
        s.v = 0.0;
    }
    s.lf = 0;
}

template <class R, class Dev> __device__ inline double kinds_advance(const Dev &G, int64_t env, int g, int c, KindLane &s) {
    const int kind = G.kind[c];
    if (s.lf <= 0) kinds_new_subepisode(G, env, g, c, s);
    const int32_t k = s.len - s.lf;  // index inside the sub-episode
    const double m_lo = G.m_lo[c], m_hi = G.m_hi[c];
    double v;
    if (kind == GEMX_REF_WIENER) {  // (walk_step's arithmetic on step_normal's draw: the bits of the all-Wiener kernels)
        v = s.v + s.sg * (double)step_normal<R>(G.seed, G.env_base + env, g, s.t);
        if (v > m_hi) v = m_hi;
        if (v < m_lo) v = m_lo;
    } else if (kind == GEMX_REF_LAPLACE) {  // laplace ... :28-37; numpy's laplace(0, b): b log(2U) below the median, -b log(2(1 - U)) above
        uint32_t r[4];
        refgen_block(G.seed, G.env_base + env, g, DRAW_STEP, s.t, r);
        const double u = gemx::Philox::u01(r[0]);
        v = s.v + s.sg * (u < 0.5 ? log(2.0 * u) : -log(2.0 * (1.0 - u)));
        if (v > m_hi) v = m_hi;
        if (v < m_lo) v = m_lo;
    } else if (kind == GEMX_REF_STEP) {  // step ... :47-61
        const int64_t L = s.len;
        int64_t j = ((int64_t)k - (int64_t)s.roll) % L;
        if (j < 0) j += L;
        const double x = s.freq * fmod((double)j * G.tau, 1.0 / s.freq) - s.width;
        v = clip(s.amp * (double)((x > 0.0) - (x < 0.0)) + s.off, m_lo, m_hi);
    } else {
        const double x = gemx::kTwoPi * s.freq * ((double)k * G.tau) + s.phase;
        const double w = kind == GEMX_REF_SINUS ? sin(x) : sawtooth(x, s.width);
        v = clip(s.amp * w + s.off, m_lo, m_hi);
    }
    s.v = v;
    --s.lf;
    ++s.t;
    return v;
}

// description slot `s` of G from column / alternative `j` of a config (gemx_refgen_kinds_config, gemx_refgen_switched_config: the same fields)
template <class Dev, class Cfg> void set_description(Dev &G, int s, const Cfg &c, int j) {
    G.kind[s] = c.kind[j]; G.len_lo[s] = c.episode_len_lo[j]; G.len_hi[s] = c.episode_len_hi[j];
    G.m_lo[s] = c.margin_lo[j]; G.m_hi[s] = c.margin_hi[j]; G.c[s] = c.reference_value[j];
    if (c.kind[j] == GEMX_REF_WIENER || c.kind[j] == GEMX_REF_LAPLACE) {
        G.log_sig_lo[s] = log10(c.sigma_lo[j]); G.log_sig_hi[s] = log10(c.sigma_hi[j]);
        G.i_lo[s] = c.initial_lo[j]; G.i_hi[s] = c.initial_hi[j];
    } else {  // the reference's set_modules (e.g. sinusoidal ... :42-48): amplitudes within half the margin's width, offsets within the margin
        const double half = (c.margin_hi[j] - c.margin_lo[j]) / 2;
        G.a_lo[s] = fmin(fmax(c.amplitude_lo[j], 0.0), half); G.a_hi[s] = fmin(fmax(c.amplitude_hi[j], 0.0), half);
        G.o_lo[s] = fmin(fmax(c.offset_lo[j], c.margin_lo[j]), c.margin_hi[j]); G.o_hi[s] = fmin(fmax(c.offset_hi[j], c.margin_lo[j]), c.margin_hi[j]);
        G.f_lo[s] = c.frequency_lo[j]; G.f_hi[s] = c.frequency_hi[j];
    }
}

template <class Dev, class Cfg> Dev make_description(const Cfg &c) {  // (the slots: set_description, by the caller)
    Dev G;
    memset(&G, 0, sizeof(G));
    G.n_ref = c.n_ref; G.seed = c.seed; G.env_base = c.env_base; G.tau = c.tau;
    return G;
}
RefgenKindsDev make_kinds_dev(const gemx_refgen_kinds_config &c) {
    RefgenKindsDev G = make_description<RefgenKindsDev>(c);
    for (int g = 0; g < c.n_ref; ++g) set_description(G, g, c, g);
    return G;
}

// small kernel of gemx_refgen_get_params: kind / step index / length per (column, env)
__global__ void refgen_kinds_index_kernel(int32_t *out, int64_t N, int n_ref, int mixed, RefgenKindsDev G, const int32_t *left, const int32_t *len) {
    const int64_t si = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = N * n_ref;
    if (si >= m) return;
    out[si] = G.kind[si / N];
    out[m + si] = mixed ? len[si] - left[si] : -1;
    out[2 * m + si] = mixed ? len[si] : -1;
}

// ---- SwitchedReferenceGenerator (switched_reference_generator.py:8-95; include/gemx.h) ---------------------------------------------------
// A switched column runs ONE of its alternatives per super-episode; which one is per-lane state, so the kernel reads the alternative's
// description at slot column * GEMX_MAX_ALT + alternative and hands it to the helpers of the kinds kernel above.  A plain column is
// slot column * GEMX_MAX_ALT with no super-episodes: the kinds kernel's draws and arithmetic.
//   DRAW_SUPER index n_super  word 0: super-episode length, integers(lo, hi); word 1: the alternative, inverse distribution function of p
enum { DRAW_SUPER = 4 };
__device__ inline bool is_wave(int kind) { return kind >= GEMX_REF_SINUS && kind <= GEMX_REF_SAWTOOTH; }

struct SuperLane {  // the super-episode state of one (column, env), in registers
    int32_t alt, sk, slen;
    uint32_t nsup;
};

// _reset_reference, switched ... :83-88: the length, then the alternative
__device__ inline void switched_new_superepisode(const RefgenSwitchedDev &G, int64_t env, int g, SuperLane &u) {
    uint32_t r[4];
    refgen_block(G.seed, G.env_base + env, g, DRAW_SUPER, u.nsup++, r);
    u.slen = (int32_t)((double)(G.sup_hi[g] - G.sup_lo[g]) * gemx::Philox::u01(r[0]) + (double)G.sup_lo[g]);
    const double x = gemx::Philox::u01(r[1]);
    int a = 0;
#pragma unroll
    for (int i = 0; i < GEMX_MAX_ALT - 1; ++i) a += (i + 1 < G.n_alt[g] && x >= G.cdf[g * GEMX_MAX_ALT + i]) ? 1 : 0;
    u.alt = a;
}
// reset(), :65-68: a new super-episode; the chosen alternative is reset without an initial reference.  Its own first value comes with the
// next step and is not counted: sk = -1 until then
__device__ inline void switched_reset(const RefgenSwitchedDev &G, int64_t env, int g, SuperLane &u, KindLane &s) {
    switched_new_superepisode(G, env, g, u);
    u.sk = -1;
    kinds_reset(G, env, g, g * GEMX_MAX_ALT + u.alt, s);
}
// get_reference_observation, :74-81: at the super-episode's end the newly chosen alternative restarts from the value shown last (kept in
// s.v) with a sub-episode of its own; a CONST alternative shows its value
template <class R> __device__ inline double switched_advance(const RefgenSwitchedDev &G, int64_t env, int g, SuperLane &u, KindLane &s) {
    if (u.sk >= u.slen) {
        switched_new_superepisode(G, env, g, u);
        u.sk = 0;
        s.lf = 0;
    }
    const int c = g * GEMX_MAX_ALT + u.alt;
    ++u.sk;
    if (G.kind[c] == GEMX_REF_CONST) return s.v = G.c[c];
    return kinds_advance<R>(G, env, g, c, s);
}

// reset (K = 0: the envs of reset_mask, or all), rollout (K steps, reset AFTER step k where done_post[k][env]), step (K = 1, reset
// BEFORE the step where done_pre[env]) and shell-order rollout (K steps, reset BEFORE step k where done_pre[k][env]): out[k][env][g],
// adjacent lanes write adjacent columns.  (This kernel and refgen_switched_kernel share the description template and the kinds_*
// helpers but not their skeleton: merged into one template, or over common load / write-back helpers, neither compiled to the
// instructions it had, and the kinds kernel's launches measured over their allowance: profiles/support_units_refactor.md.)
template <class R>
__global__ void refgen_kinds_kernel(R *out, const uint8_t *done_pre, const uint8_t *done_post, const uint8_t *reset_mask, int reset_all, int64_t N,
                                    int K, RefgenKindsDev G, double *value, double *sigma, int32_t *left, uint32_t *n_sub, uint32_t *n_reset,
                                    uint64_t *t, int32_t *len, double *par) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * G.n_ref) return;
    const int g = (int)(idx % G.n_ref);
    const int64_t env = idx / G.n_ref;
    const int64_t si = (int64_t)g * N + env, stride = (int64_t)G.n_ref * N;
    const int kind = G.kind[g];
    if (kind == GEMX_REF_CONST) {  // no state at all
        for (int k = 0; k < K; ++k) out[((int64_t)k * N + env) * G.n_ref + g] = (R)G.c[g];
        return;
    }
    const bool wave = kind != GEMX_REF_WIENER && kind != GEMX_REF_LAPLACE;
    KindLane s;
    s.v = value[si]; s.sg = sigma[si]; s.lf = left[si]; s.ns = n_sub[si]; s.nr = n_reset[si]; s.t = t[si]; s.len = len[si];
    s.amp = s.freq = s.off = s.phase = s.roll = 0.0; s.width = 1.0;
    if (wave) {
        s.amp = par[PAR_AMP * stride + si]; s.freq = par[PAR_FREQ * stride + si]; s.off = par[PAR_OFF * stride + si];
        s.phase = par[PAR_PHASE * stride + si]; s.width = par[PAR_WIDTH * stride + si]; s.roll = par[PAR_ROLL * stride + si];
    }
    const uint32_t ns0 = s.ns, nr0 = s.nr;
    if (K == 0) {
        if (reset_all || (reset_mask != nullptr && reset_mask[env])) kinds_reset(G, env, g, g, s);
    }
    for (int k = 0; k < K; ++k) {
        if (done_pre != nullptr && done_pre[(int64_t)k * N + env]) kinds_reset(G, env, g, g, s);
        out[((int64_t)k * N + env) * G.n_ref + g] = (R)kinds_advance<R>(G, env, g, g, s);
        if (done_post != nullptr && done_post[(int64_t)k * N + env]) kinds_reset(G, env, g, g, s);
    }
    value[si] = s.v; left[si] = s.lf; t[si] = s.t;
    if (s.nr != nr0) n_reset[si] = s.nr;
    if (s.ns != ns0) {
        n_sub[si] = s.ns; sigma[si] = s.sg; len[si] = s.len;
        if (wave) {
            par[PAR_AMP * stride + si] = s.amp; par[PAR_FREQ * stride + si] = s.freq; par[PAR_OFF * stride + si] = s.off;
            par[PAR_PHASE * stride + si] = s.phase; par[PAR_WIDTH * stride + si] = s.width; par[PAR_ROLL * stride + si] = s.roll;
        }
    }
}

// launched with 256 threads, and told so: without the bound the compiler keeps to 128 VGPRs and spills
template <class R>
__global__ void __launch_bounds__(256) refgen_switched_kernel(R *out, const uint8_t *done_pre, const uint8_t *done_post, const uint8_t *reset_mask, int reset_all, int64_t N,
                                       int K, RefgenSwitchedDev G, double *value, double *sigma, int32_t *left, uint32_t *n_sub, uint32_t *n_reset,
                                       uint64_t *t, int32_t *len, double *par, int32_t *alt, int32_t *sk, int32_t *slen, uint32_t *n_super) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * G.n_ref) return;
    const int g = (int)(idx % G.n_ref);
    const int64_t env = idx / G.n_ref;
    const int64_t si = (int64_t)g * N + env, stride = (int64_t)G.n_ref * N;
    const bool switched = G.n_alt[g] > 0;
    const int c0 = g * GEMX_MAX_ALT;
    if (!switched && G.kind[c0] == GEMX_REF_CONST) {  // a plain constant column: no state at all
        for (int k = 0; k < K; ++k) out[((int64_t)k * N + env) * G.n_ref + g] = (R)G.c[c0];
        return;
    }
    SuperLane u = {0, 0, 0, 0u};
    if (switched) { u.alt = alt[si]; u.sk = sk[si]; u.slen = slen[si]; u.nsup = n_super[si]; }
    const SuperLane u0 = u;
    // `wave`: the kind of the last sub-episode started in this launch is a waveform's.  A newly chosen alternative draws all its parameters
    // before it reads any; what is written back are the parameters of the LAST sub-episode, zeros where that was a walk's, so that the
    // stored state does not depend on how the steps were cut into launches
    const int kind0 = G.kind[c0 + u.alt];
    KindLane s;
    s.v = value[si]; s.sg = sigma[si]; s.lf = left[si]; s.ns = n_sub[si]; s.nr = n_reset[si]; s.t = t[si]; s.len = len[si];
    s.amp = s.freq = s.off = s.phase = s.roll = 0.0; s.width = 1.0;
    bool wave = is_wave(kind0);
    if (wave) {
        s.amp = par[PAR_AMP * stride + si]; s.freq = par[PAR_FREQ * stride + si]; s.off = par[PAR_OFF * stride + si];
        s.phase = par[PAR_PHASE * stride + si]; s.width = par[PAR_WIDTH * stride + si]; s.roll = par[PAR_ROLL * stride + si];
    }
    const uint32_t ns0 = s.ns, nr0 = s.nr;
    if (K == 0 && (reset_all || (reset_mask != nullptr && reset_mask[env]))) {
        if (switched) switched_reset(G, env, g, u, s);
        else kinds_reset(G, env, g, c0, s);
    }
    for (int k = 0; k < K; ++k) {
        if (done_pre != nullptr && done_pre[(int64_t)k * N + env]) {
            if (switched) switched_reset(G, env, g, u, s);
            else kinds_reset(G, env, g, c0, s);
        }
        const uint32_t ns1 = s.ns;
        out[((int64_t)k * N + env) * G.n_ref + g] = (R)(switched ? switched_advance<R>(G, env, g, u, s) : kinds_advance<R>(G, env, g, c0, s));
        if (s.ns != ns1) wave = is_wave(G.kind[c0 + u.alt]);
        if (done_post != nullptr && done_post[(int64_t)k * N + env]) {
            if (switched) switched_reset(G, env, g, u, s);
            else kinds_reset(G, env, g, c0, s);
        }
    }
    value[si] = s.v; left[si] = s.lf; t[si] = s.t;
    if (s.nr != nr0) n_reset[si] = s.nr;
    if (s.ns != ns0) {
        n_sub[si] = s.ns; sigma[si] = s.sg; len[si] = s.len;
        if (wave || switched) {
            par[PAR_AMP * stride + si] = wave ? s.amp : 0.0; par[PAR_FREQ * stride + si] = wave ? s.freq : 0.0; par[PAR_OFF * stride + si] = wave ? s.off : 0.0;
            par[PAR_PHASE * stride + si] = wave ? s.phase : 0.0; par[PAR_WIDTH * stride + si] = wave ? s.width : 0.0; par[PAR_ROLL * stride + si] = wave ? s.roll : 0.0;
        }
    }
    if (u.sk != u0.sk) sk[si] = u.sk;
    if (u.nsup != u0.nsup) { alt[si] = u.alt; slen[si] = u.slen; n_super[si] = u.nsup; }
}

RefgenSwitchedDev make_switched_dev(const gemx_refgen_switched_config &c) {
    RefgenSwitchedDev G = make_description<RefgenSwitchedDev>(c);
    for (int g = 0; g < c.n_ref; ++g) {
        G.n_alt[g] = c.n_alt[g]; G.sup_lo[g] = c.super_len_lo[g]; G.sup_hi[g] = c.super_len_hi[g];
        double sum = 0.0;
        for (int a = 0; a < (c.n_alt[g] > 0 ? c.n_alt[g] : 1); ++a) {
            const int s = g * GEMX_MAX_ALT + a;
            set_description(G, s, c, s);
            G.cdf[s] = (sum += c.p[s]);
        }
    }
    return G;
}

// every entry point's dispatch for the handles that run one kernel for all four uses: the switched kernel, else the kinds kernel
template <class R>
int kinds_launch(gemx_refgen *r, void *out, const uint8_t *done_pre, const uint8_t *done_post, const uint8_t *mask, int reset_all, int K, hipStream_t st) {
    const dim3 grid((unsigned)((r->n * r->cfg.n_ref + 255) / 256)), block(256);
    if (r->switched) {
        gemx_cov_note(sizeof(R) == 4 ? "refgen_switched_kernel<float>" : "refgen_switched_kernel<double>");
        hipLaunchKernelGGL(refgen_switched_kernel<R>, grid, block, 0, st, (R *)out, done_pre, done_post, mask, reset_all, r->n, K,
                           *(const RefgenSwitchedDev *)r->sdev, r->value, r->sigma, r->left, r->n_sub, r->n_reset, r->t, r->len, r->par, r->alt, r->sk,
                           r->slen, r->n_super);
    } else {
        gemx_cov_note(sizeof(R) == 4 ? "refgen_kinds_kernel<float>" : "refgen_kinds_kernel<double>");
        hipLaunchKernelGGL(refgen_kinds_kernel<R>, grid, block, 0, st, (R *)out, done_pre, done_post, mask, reset_all, r->n, K,
                           make_kinds_dev(r->kcfg), r->value, r->sigma, r->left, r->n_sub, r->n_reset, r->t, r->len, r->par);
    }
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}
int kinds(gemx_refgen *r, void *out, const uint8_t *done_pre, const uint8_t *done_post, const uint8_t *mask, int reset_all, int K, hipStream_t st) {
    return r->f64 ? kinds_launch<double>(r, out, done_pre, done_post, mask, reset_all, K, st)
                  : kinds_launch<float>(r, out, done_pre, done_post, mask, reset_all, K, st);
}

// gemx_refgen_get_params on a switched handle: the kind of the lane's current alternative
__global__ void refgen_switched_index_kernel(int32_t *out, int64_t N, int n_ref, RefgenSwitchedDev G, const int32_t *left, const int32_t *len, const int32_t *alt) {
    const int64_t si = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = N * n_ref;
    if (si >= m) return;
    const int g = (int)(si / N);
    const bool switched = G.n_alt[g] > 0;
    const int kind = G.kind[g * GEMX_MAX_ALT + (switched ? alt[si] : 0)];
    const bool none = switched && kind == GEMX_REF_CONST;  // (a constant alternative has no sub-episodes)
    out[si] = kind;
    out[m + si] = none ? -1 : len[si] - left[si];
    out[2 * m + si] = none ? -1 : len[si];
}

}  // namespace

// THE table of a handle's per-(column, env) arrays: pointer member, bytes per lane, which handles own it.  It drives allocation,
// zeroing and gemx_refgen_destroy.
enum { OWN_ALL = 1, OWN_KINDS = 2, OWN_SWITCHED = 4 };
struct LaneArrayRow { void **p; size_t bytes; int owner; };
template <class F> static void refgen_lane_arrays(gemx_refgen *r, F f) {
    const LaneArrayRow rows[] = {{(void **)&r->value, 8, OWN_ALL},      {(void **)&r->sigma, 8, OWN_ALL},    {(void **)&r->left, 4, OWN_ALL},
                                 {(void **)&r->n_sub, 4, OWN_ALL},      {(void **)&r->n_reset, 4, OWN_ALL},  {(void **)&r->t, 8, OWN_ALL},
                                 {(void **)&r->len, 4, OWN_KINDS},      {(void **)&r->par, 8 * N_PAR, OWN_KINDS},
                                 {(void **)&r->alt, 4, OWN_SWITCHED},   {(void **)&r->sk, 4, OWN_SWITCHED},  {(void **)&r->slen, 4, OWN_SWITCHED},
                                 {(void **)&r->n_super, 4, OWN_SWITCHED}};
    for (const LaneArrayRow &row : rows) f(row);
}
// allocate and zero the arrays of `owners`; false: a hipMalloc failed (the caller destroys the handle)
static bool refgen_alloc_arrays(gemx_refgen *r, int owners) {
    const size_t m = (size_t)r->n * r->cfg.n_ref;
    bool ok = true;
    refgen_lane_arrays(r, [&](const LaneArrayRow &a) {
        if (!ok || !(a.owner & owners)) return;
        ok = hipMalloc(a.p, m * a.bytes) == hipSuccess;
        if (ok) (void)hipMemset(*a.p, 0, m * a.bytes);
    });
    return ok;
}

// the handle and its zeroed per-(column, env) arrays; kcfg != NULL: a gemx_refgen_create_kinds handle (cfg: the Wiener view of its columns)
static int gemx_refgen_alloc(const gemx_refgen_config &cfg, const gemx_refgen_kinds_config *kcfg, int64_t n_envs, int device, int dtype, gemx_refgen **out) {
    gemx::DeviceGuard guard(device);
    gemx_refgen *r = new (std::nothrow) gemx_refgen();
    if (!r) return gemx::fail(GEMX_ERR_ALLOC, "out of host memory");
    r->cfg = cfg; r->n = n_envs; r->device = device; r->f64 = dtype == GEMX_F64;
    memset(&r->kcfg, 0, sizeof(r->kcfg));
    if (kcfg) { r->kcfg = *kcfg; r->has_kinds = 1; }
    if (!refgen_alloc_arrays(r, OWN_ALL | (kcfg ? OWN_KINDS : 0))) {
        gemx_refgen_destroy(r);
        return gemx::fail(GEMX_ERR_ALLOC, "hipMalloc(refgen) failed");
    }
    *out = r;
    return GEMX_OK;
}

// what every create function checks first; `name`: of its config struct, for the size message
template <class Cfg> static int refgen_check_create(const Cfg *cfg, const char *name, int64_t n_envs, gemx_refgen **out) {
    if (!cfg || !out) return gemx::fail(GEMX_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(Cfg)) return gemx::fail(GEMX_ERR_ARG, "%s size mismatch", name);
    if (cfg->env_base < 0) return gemx::fail(GEMX_ERR_ARG, "env_base must be >= 0");
    if (cfg->n_ref < 1 || cfg->n_ref > GEMX_MAX_REF) return gemx::fail(GEMX_ERR_ARG, "n_ref must be in [1, %d]", GEMX_MAX_REF);
    if (n_envs <= 0) return gemx::fail(GEMX_ERR_ARG, "n_envs must be positive");
    return GEMX_OK;
}

// the columns of a kinds config, checked; `w`: their Wiener view (what gemx_refgen_create would be given for these columns)
static int refgen_check_columns(const gemx_refgen_kinds_config &c, gemx_refgen_config &w, int &all_wiener) {
    const gemx_refgen_kinds_config *cfg = &c;
    memset(&w, 0, sizeof(w));
    w.struct_size = (int32_t)sizeof(w); w.n_ref = cfg->n_ref; w.seed = cfg->seed; w.env_base = cfg->env_base;
    w.episode_len_lo = cfg->episode_len_lo[0]; w.episode_len_hi = cfg->episode_len_hi[0];
    all_wiener = 1;
    for (int g = 0; g < cfg->n_ref; ++g) {
        const int kind = cfg->kind[g];
        if (kind < GEMX_REF_WIENER || kind > GEMX_REF_CONST) return gemx::fail(GEMX_ERR_ARG, "column %d: unknown generator kind %d", g, kind);
        w.margin_lo[g] = cfg->margin_lo[g]; w.margin_hi[g] = cfg->margin_hi[g]; w.sigma_lo[g] = cfg->sigma_lo[g]; w.sigma_hi[g] = cfg->sigma_hi[g];
        w.initial_lo[g] = cfg->initial_lo[g]; w.initial_hi[g] = cfg->initial_hi[g];
        if (kind != GEMX_REF_WIENER || cfg->episode_len_lo[g] != w.episode_len_lo || cfg->episode_len_hi[g] != w.episode_len_hi) all_wiener = 0;
        if (kind == GEMX_REF_CONST) continue;
        if (cfg->episode_len_lo[g] < 1 || cfg->episode_len_hi[g] < cfg->episode_len_lo[g]) return gemx::fail(GEMX_ERR_ARG, "episode lengths %d must satisfy 1 <= lo <= hi", g);
        if (cfg->margin_hi[g] < cfg->margin_lo[g]) return gemx::fail(GEMX_ERR_ARG, "empty margin %d", g);
        if (kind == GEMX_REF_WIENER || kind == GEMX_REF_LAPLACE) {
            if (!(cfg->sigma_lo[g] > 0) || cfg->sigma_hi[g] < cfg->sigma_lo[g]) return gemx::fail(GEMX_ERR_ARG, "sigma range %d must satisfy 0 < lo <= hi", g);
            if (kind == GEMX_REF_WIENER && cfg->initial_hi[g] < cfg->initial_lo[g]) return gemx::fail(GEMX_ERR_ARG, "empty initial range %d", g);
        } else {
            if (!(cfg->frequency_lo[g] >= 0) || cfg->frequency_hi[g] < cfg->frequency_lo[g] || !(cfg->frequency_hi[g] < HUGE_VAL))
                return gemx::fail(GEMX_ERR_ARG, "frequency range %d must satisfy 0 <= lo <= hi < inf", g);
            if (kind == GEMX_REF_STEP && !(cfg->frequency_lo[g] > 0)) return gemx::fail(GEMX_ERR_ARG, "frequency range %d of a step generator must be positive", g);
            if (cfg->amplitude_lo[g] != cfg->amplitude_lo[g] || cfg->amplitude_hi[g] != cfg->amplitude_hi[g] || cfg->offset_lo[g] != cfg->offset_lo[g] ||
                cfg->offset_hi[g] != cfg->offset_hi[g])
                return gemx::fail(GEMX_ERR_ARG, "amplitude / offset range %d is not a number", g);
        }
    }
    return GEMX_OK;
}
extern "C" {

int gemx_refgen_create(const gemx_refgen_config *cfg, int64_t n_envs, int device, int dtype, gemx_refgen **out) {
    if (int rc = refgen_check_create(cfg, "gemx_refgen_config", n_envs, out)) return rc;
    if (cfg->episode_len_lo < 1 || cfg->episode_len_hi < cfg->episode_len_lo) return gemx::fail(GEMX_ERR_ARG, "episode lengths must satisfy 1 <= lo <= hi");
    for (int g = 0; g < cfg->n_ref; ++g) {
        if (!(cfg->sigma_lo[g] > 0) || cfg->sigma_hi[g] < cfg->sigma_lo[g]) return gemx::fail(GEMX_ERR_ARG, "sigma range %d must satisfy 0 < lo <= hi", g);
        if (cfg->margin_hi[g] < cfg->margin_lo[g] || cfg->initial_hi[g] < cfg->initial_lo[g]) return gemx::fail(GEMX_ERR_ARG, "empty margin / initial range %d", g);
    }
    if (int rc = gemx::check_device_dtype(device, dtype)) return rc;
    return gemx_refgen_alloc(*cfg, nullptr, n_envs, device, dtype, out);
}

int gemx_refgen_create_kinds(const gemx_refgen_kinds_config *cfg, int64_t n_envs, int device, int dtype, gemx_refgen **out) {
    if (int rc = refgen_check_create(cfg, "gemx_refgen_kinds_config", n_envs, out)) return rc;
    if (!(cfg->tau > 0)) return gemx::fail(GEMX_ERR_ARG, "tau must be positive");
    gemx_refgen_config w;
    int all_wiener = 1;
    if (int rc = refgen_check_columns(*cfg, w, all_wiener)) return rc;
    if (int rc = gemx::check_device_dtype(device, dtype)) return rc;
    const int rc = gemx_refgen_alloc(w, cfg, n_envs, device, dtype, out);
    if (rc == GEMX_OK) (*out)->mixed = !all_wiener;  // all Wiener, one length range: the kernels (and bits) of a gemx_refgen_create handle
    return rc;
}

// column g of a kinds config := alternative a of column g of a switched config
static void refgen_alternative(const gemx_refgen_switched_config &c, int g, int a, gemx_refgen_kinds_config &k) {
    const int s = g * GEMX_MAX_ALT + a;
    k.kind[g] = c.kind[s]; k.episode_len_lo[g] = c.episode_len_lo[s]; k.episode_len_hi[g] = c.episode_len_hi[s];
    k.margin_lo[g] = c.margin_lo[s]; k.margin_hi[g] = c.margin_hi[s]; k.sigma_lo[g] = c.sigma_lo[s]; k.sigma_hi[g] = c.sigma_hi[s];
    k.initial_lo[g] = c.initial_lo[s]; k.initial_hi[g] = c.initial_hi[s]; k.amplitude_lo[g] = c.amplitude_lo[s]; k.amplitude_hi[g] = c.amplitude_hi[s];
    k.frequency_lo[g] = c.frequency_lo[s]; k.frequency_hi[g] = c.frequency_hi[s]; k.offset_lo[g] = c.offset_lo[s]; k.offset_hi[g] = c.offset_hi[s];
    k.reference_value[g] = c.reference_value[s];
}

int gemx_refgen_create_switched(const gemx_refgen_switched_config *cfg, int64_t n_envs, int device, int dtype, gemx_refgen **out) {
    if (int rc = refgen_check_create(cfg, "gemx_refgen_switched_config", n_envs, out)) return rc;
    if (!(cfg->tau > 0)) return gemx::fail(GEMX_ERR_ARG, "tau must be positive");
    int any = 0, most = 1;
    for (int g = 0; g < cfg->n_ref; ++g) {
        const int n = cfg->n_alt[g];
        if (n < 0 || n > GEMX_MAX_ALT) return gemx::fail(GEMX_ERR_ARG, "column %d: n_alt must be in [0, %d] (0: a plain column), not %d", g, GEMX_MAX_ALT, n);
        if (n == 0) continue;
        any = 1;
        if (n > most) most = n;
        double sum = 0.0;
        for (int a = 0; a < n; ++a) {
            const double p = cfg->p[g * GEMX_MAX_ALT + a];
            if (!(p >= 0.0)) return gemx::fail(GEMX_ERR_ARG, "column %d: probability %d must be >= 0", g, a);
            sum += p;
        }
        if (!(fabs(sum - 1.0) <= 1e-9)) return gemx::fail(GEMX_ERR_ARG, "column %d: the probabilities must sum to 1", g);
        if (cfg->super_len_lo[g] < 1 || cfg->super_len_hi[g] <= cfg->super_len_lo[g])
            return gemx::fail(GEMX_ERR_ARG, "column %d: super-episode lengths must satisfy 1 <= lo < hi", g);
    }
    // the alternatives, one kinds config per alternative index (a column with fewer alternatives repeats its last): checked as
    // gemx_refgen_create_kinds checks its columns
    gemx_refgen_kinds_config k0;
    gemx_refgen_config w0;
    for (int a = 0; a < most; ++a) {
        gemx_refgen_kinds_config k;
        memset(&k, 0, sizeof(k));
        k.struct_size = (int32_t)sizeof(k); k.n_ref = cfg->n_ref; k.seed = cfg->seed; k.env_base = cfg->env_base; k.tau = cfg->tau;
        for (int g = 0; g < cfg->n_ref; ++g) refgen_alternative(*cfg, g, a < cfg->n_alt[g] ? a : (cfg->n_alt[g] > 0 ? cfg->n_alt[g] - 1 : 0), k);
        gemx_refgen_config w;
        int all_wiener = 1;
        if (int rc = refgen_check_columns(k, w, all_wiener)) return rc;
        if (a == 0) { k0 = k; w0 = w; }
    }
    if (!any) return gemx_refgen_create_kinds(&k0, n_envs, device, dtype, out);  // no switched column: that handle, and its kernels
    if (int rc = gemx::check_device_dtype(device, dtype)) return rc;
    const int rc = gemx_refgen_alloc(w0, &k0, n_envs, device, dtype, out);
    if (rc != GEMX_OK) return rc;
    gemx_refgen *r = *out;
    gemx::DeviceGuard guard(device);
    RefgenSwitchedDev *G = new (std::nothrow) RefgenSwitchedDev(make_switched_dev(*cfg));
    r->sdev = G;
    if (!G || !refgen_alloc_arrays(r, OWN_SWITCHED)) {
        gemx_refgen_destroy(r);
        *out = nullptr;
        return gemx::fail(GEMX_ERR_ALLOC, "allocation (switched refgen) failed");
    }
    r->mixed = 1;
    r->switched = 1;
    return GEMX_OK;
}

int gemx_refgen_destroy(gemx_refgen *r) {
    if (!r) return GEMX_OK;
    gemx::DeviceGuard guard(r->device);
    refgen_lane_arrays(r, [](const LaneArrayRow &a) {
        if (*a.p) (void)hipFree(*a.p);
    });
    delete (RefgenSwitchedDev *)r->sdev;
    if (r->dev_desc) (void)hipFree(r->dev_desc);
    delete r;
    return GEMX_OK;
}

// reference_generator.reset() for the envs with mask != 0 (all if NULL): new initial reference value, a new sub-episode starts with
// the next generated step.
int gemx_refgen_reset(gemx_refgen *r, const uint8_t *mask_dev, void *stream) {
    if (!r) return gemx::fail(GEMX_ERR_ARG, "null handle");
    gemx::DeviceGuard guard(r->device);
    hipStream_t st = (hipStream_t)stream;
    const int all = mask_dev == nullptr;
    if (r->mixed) return kinds(r, nullptr, nullptr, nullptr, mask_dev, all, 0, st);
    return r->f64 ? walk<double>(r, nullptr, nullptr, 0, mask_dev, all, 0, st) : walk<float>(r, nullptr, nullptr, 0, mask_dev, all, 0, st);
}

// the all-Wiener pair: K * N * n_ref normals into the output tensor, then the sequential walk over them (which advances the step counters by K)
static int refgen_wiener_rollout(gemx_refgen *r, const uint8_t *done_dev, int done_first, int32_t K, void *refs_out_dev, hipStream_t st) {
    const int64_t total = (int64_t)K * r->n * r->cfg.n_ref;
    gemx_cov_note(r->f64 ? "refgen_normals_kernel<double>" : "refgen_normals_kernel<float>");
    if (r->f64)
        hipLaunchKernelGGL(refgen_normals_kernel<double>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (double *)refs_out_dev, r->n, r->cfg.n_ref, K,
                           r->cfg.seed, r->t, r->cfg.env_base);
    else
        hipLaunchKernelGGL(refgen_normals_kernel<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (float *)refs_out_dev, r->n, r->cfg.n_ref, K,
                           r->cfg.seed, r->t, r->cfg.env_base);
    GEMX_HIP_TRY(hipGetLastError());
    return r->f64 ? walk<double>(r, refs_out_dev, done_dev, done_first, nullptr, 0, K, st) : walk<float>(r, refs_out_dev, done_dev, done_first, nullptr, 0, K, st);
}

int gemx_refgen_rollout(gemx_refgen *r, const uint8_t *done_dev, int32_t K, void *refs_out_dev, void *stream) {
    if (!r || !refs_out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (K < 1) return gemx::fail(GEMX_ERR_ARG, "K must be >= 1");
    gemx::DeviceGuard guard(r->device);
    hipStream_t st = (hipStream_t)stream;
    if (r->mixed) return kinds(r, refs_out_dev, nullptr, done_dev, nullptr, 0, K, st);
    return refgen_wiener_rollout(r, done_dev, 0, K, refs_out_dev, st);
}

// K env-shell steps in the SHELL's order: row k = gemx_refgen_step(done[k]) -- restart where done[k][env], then advance (include/gemx.h)
int gemx_refgen_rollout_shell(gemx_refgen *r, const uint8_t *done_dev, int32_t K, void *refs_out_dev, void *stream) {
    if (!r || !refs_out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (K < 1) return gemx::fail(GEMX_ERR_ARG, "K must be >= 1");
    gemx::DeviceGuard guard(r->device);
    hipStream_t st = (hipStream_t)stream;
    if (r->mixed) return kinds(r, refs_out_dev, done_dev, nullptr, nullptr, 0, K, st);
    return refgen_wiener_rollout(r, done_dev, 1, K, refs_out_dev, st);
}

// One env-shell step in ONE launch: the generators of envs with done_dev[env] != 0 (NULL: none) are reset, then every generator advances
// by one step (core.py:351, get_reference_observation); refs_dev [N, n_ref] receives the new values.  K calls with the masks done[k-1]
// give the rows of one gemx_refgen_rollout(K, done), bit for bit.  Nothing is kept on the host: a captured launch replays correctly.
int gemx_refgen_step(gemx_refgen *r, const uint8_t *done_dev, void *refs_dev, void *stream) {
    if (!r || !refs_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(r->device);
    hipStream_t st = (hipStream_t)stream;
    if (r->mixed) return kinds(r, refs_dev, done_dev, nullptr, nullptr, 0, 1, st);
    return r->f64 ? step<double>(r, refs_dev, done_dev, st) : step<float>(r, refs_dev, done_dev, st);
}

// debug / test access: per (generator, env) arrays [n_ref][N]: value (double), sigma (double), steps left (int32)
int gemx_refgen_get_state(gemx_refgen *r, double *value_out_dev, double *sigma_out_dev, int32_t *left_out_dev, void *stream) {
    if (!r) return gemx::fail(GEMX_ERR_ARG, "null handle");
    gemx::DeviceGuard guard(r->device);
    const size_t m = (size_t)r->n * r->cfg.n_ref;
    hipStream_t st = (hipStream_t)stream;
    if (value_out_dev) GEMX_HIP_TRY(hipMemcpyAsync(value_out_dev, r->value, m * 8, hipMemcpyDeviceToDevice, st));
    if (sigma_out_dev) GEMX_HIP_TRY(hipMemcpyAsync(sigma_out_dev, r->sigma, m * 8, hipMemcpyDeviceToDevice, st));
    if (left_out_dev) GEMX_HIP_TRY(hipMemcpyAsync(left_out_dev, r->left, m * 4, hipMemcpyDeviceToDevice, st));
    return GEMX_OK;
}

int gemx_refgen_get_params(gemx_refgen *r, int32_t *kind_index_len_out_dev, double *params_out_dev, void *stream) {
    if (!r) return gemx::fail(GEMX_ERR_ARG, "null handle");
    if (!r->has_kinds) return gemx::fail(GEMX_ERR_ARG, "gemx_refgen_get_params needs a gemx_refgen_create_kinds handle");
    gemx::DeviceGuard guard(r->device);
    const int64_t m = r->n * r->kcfg.n_ref;
    hipStream_t st = (hipStream_t)stream;
    if (kind_index_len_out_dev && r->switched) {
        hipLaunchKernelGGL(refgen_switched_index_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, kind_index_len_out_dev, r->n, r->kcfg.n_ref,
                           *(const RefgenSwitchedDev *)r->sdev, r->left, r->len, r->alt);
        GEMX_HIP_TRY(hipGetLastError());
    } else if (kind_index_len_out_dev) {
        hipLaunchKernelGGL(refgen_kinds_index_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, kind_index_len_out_dev, r->n, r->kcfg.n_ref, r->mixed,
                           make_kinds_dev(r->kcfg), r->left, r->len);
        GEMX_HIP_TRY(hipGetLastError());
    }
    if (params_out_dev) GEMX_HIP_TRY(hipMemcpyAsync(params_out_dev, r->par, (size_t)m * 8 * N_PAR, hipMemcpyDeviceToDevice, st));
    return GEMX_OK;
}

int gemx_refgen_get_switch_state(gemx_refgen *r, int32_t *alt_sk_slen_nsuper_out_dev, void *stream) {
    if (!r || !alt_sk_slen_nsuper_out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (!r->switched) return gemx::fail(GEMX_ERR_ARG, "gemx_refgen_get_switch_state needs a gemx_refgen_create_switched handle with a switched column");
    gemx::DeviceGuard guard(r->device);
    const size_t m = (size_t)r->n * r->cfg.n_ref;
    hipStream_t st = (hipStream_t)stream;
    const void *src[4] = {r->alt, r->sk, r->slen, r->n_super};
    for (int i = 0; i < 4; ++i) GEMX_HIP_TRY(hipMemcpyAsync(alt_sk_slen_nsuper_out_dev + i * m, src[i], m * 4, hipMemcpyDeviceToDevice, st));
    return GEMX_OK;
}

// ---- checkpoint blob (include/gemx.h): the header, then EVERY array of refgen_lane_arrays the handle owns, in the table's order, each
// section padded to 8 bytes.  The three functions walk the table: an array added to it is carried without a change here.
static int refgen_owners(const gemx_refgen *r) { return OWN_ALL | (r->has_kinds ? OWN_KINDS : 0) | (r->switched ? OWN_SWITCHED : 0); }
static size_t refgen_section_bytes(const gemx_refgen *r, const LaneArrayRow &a) { return ((size_t)r->n * r->cfg.n_ref * a.bytes + 7) & ~(size_t)7; }
static RefgenBlobHeader refgen_blob_header(gemx_refgen *r) {
    RefgenBlobHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = 0x47525847u;  // "GXRG"
    h.owners = (uint32_t)refgen_owners(r);
    h.n_envs = r->n; h.n_ref = r->cfg.n_ref; h.env_base = r->cfg.env_base;
    h.bytes = gemx_refgen_state_bytes(r);
    for (int g = 0; g < r->cfg.n_ref; ++g) {
        h.column[g] = r->has_kinds ? r->kcfg.kind[g] : GEMX_REF_WIENER;
        if (r->switched) h.column[g] |= ((const RefgenSwitchedDev *)r->sdev)->n_alt[g] << 8;
    }
    return h;
}

int64_t gemx_refgen_state_bytes(gemx_refgen *r) {
    if (!r) return 0;
    size_t total = sizeof(RefgenBlobHeader);
    const int owners = refgen_owners(r);
    refgen_lane_arrays(r, [&](const LaneArrayRow &a) {
        if (a.owner & owners) total += refgen_section_bytes(r, a);
    });
    return (int64_t)total;
}

int gemx_refgen_get_blob(gemx_refgen *r, void *out_dev, void *stream) {
    if (!r || !out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(r->device);
    hipStream_t st = (hipStream_t)stream;
    // (equal states give equal blobs: the sections' padding is zeroed)
    GEMX_HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)gemx_refgen_state_bytes(r), st));
    r->blob_head = refgen_blob_header(r);  // (the same words on every call: a copy still in flight reads what this writes)
    GEMX_HIP_TRY(hipMemcpyAsync(out_dev, &r->blob_head, sizeof(RefgenBlobHeader), hipMemcpyHostToDevice, st));
    const int owners = refgen_owners(r);
    const size_t m = (size_t)r->n * r->cfg.n_ref;
    size_t at = sizeof(RefgenBlobHeader);
    hipError_t err = hipSuccess;
    refgen_lane_arrays(r, [&](const LaneArrayRow &a) {
        if (!(a.owner & owners)) return;
        if (err == hipSuccess) err = hipMemcpyAsync((char *)out_dev + at, *a.p, m * a.bytes, hipMemcpyDeviceToDevice, st);
        at += refgen_section_bytes(r, a);
    });
    GEMX_HIP_TRY(err);
    return GEMX_OK;
}

int gemx_refgen_set_blob(gemx_refgen *r, const void *in_dev, void *stream) {
    if (!r || !in_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(r->device);
    hipStream_t st = (hipStream_t)stream;
    // the header alone comes to the host first (synchronises `stream`); nothing is enqueued before it has been checked
    RefgenBlobHeader got;
    GEMX_HIP_TRY(hipMemcpyAsync(&got, in_dev, sizeof(got), hipMemcpyDeviceToHost, st));
    GEMX_HIP_TRY(hipStreamSynchronize(st));
    const RefgenBlobHeader want = refgen_blob_header(r);
    if (got.magic != want.magic) return gemx::fail(GEMX_ERR_ARG, "not a reference generator blob (magic %08x)", got.magic);
    if (got.n_envs != want.n_envs) return gemx::fail(GEMX_ERR_ARG, "the reference generator blob is for n_envs = %lld, this handle has %lld", (long long)got.n_envs, (long long)want.n_envs);
    if (got.n_ref != want.n_ref) return gemx::fail(GEMX_ERR_ARG, "the reference generator blob has %d reference columns, this handle has %d", got.n_ref, want.n_ref);
    if (got.owners != want.owners)
        return gemx::fail(GEMX_ERR_ARG, "the reference generator blob is of another generator kind (arrays %u: 1 Wiener, 3 kinds, 7 switched; this handle: %u)", got.owners, want.owners);
    for (int g = 0; g < want.n_ref; ++g)
        if (got.column[g] != want.column[g])
            return gemx::fail(GEMX_ERR_ARG, "the reference generator blob's column %d is of another generator kind (%d with %d alternatives; this handle: %d with %d)", g,
                              got.column[g] & 255, got.column[g] >> 8, want.column[g] & 255, want.column[g] >> 8);
    if (got.env_base != want.env_base)
        return gemx::fail(GEMX_ERR_ARG, "the reference generator blob belongs to the shard at env_base = %lld, this handle's is %lld", (long long)got.env_base, (long long)want.env_base);
    if (got.bytes != want.bytes) return gemx::fail(GEMX_ERR_ARG, "the reference generator blob has %lld bytes, this handle's has %lld", (long long)got.bytes, (long long)want.bytes);
    const int owners = refgen_owners(r);
    const size_t m = (size_t)r->n * r->cfg.n_ref;
    size_t at = sizeof(RefgenBlobHeader);
    hipError_t err = hipSuccess;
    refgen_lane_arrays(r, [&](const LaneArrayRow &a) {
        if (!(a.owner & owners)) return;
        if (err == hipSuccess) err = hipMemcpyAsync(*a.p, (const char *)in_dev + at, m * a.bytes, hipMemcpyDeviceToDevice, st);
        at += refgen_section_bytes(r, a);
    });
    GEMX_HIP_TRY(err);
    return GEMX_OK;
}

}  // extern "C"

// ---- the complete policy rollout (gemx_refgen_lane.hpp declares them): the kernel's view of an all-Wiener handle, and the normals in front of it
namespace gemx {
int refgen_policy_view(gemx_refgen *r, const char *what, int64_t n_envs, int device, int64_t env_base, PcWienerDev *out, int *n_ref) {
    if (r->switched || r->mixed || r->has_kinds)
        return fail(GEMX_ERR_ARG, "%s: a %s gemx_refgen is not served inside the launch (an all-Wiener gemx_refgen_create handle, or a gemx_refprofile)", what,
                    r->switched ? "switched" : r->mixed ? "mixed-kinds" : "kinds");
    if (r->n != n_envs) return fail(GEMX_ERR_ARG, "%s: the gemx_refgen serves n_envs = %lld, the handle %lld", what, (long long)r->n, (long long)n_envs);
    if (r->f64) return fail(GEMX_ERR_ARG, "%s: the gemx_refgen is fp64, the handle fp32", what);
    if (r->device != device) return fail(GEMX_ERR_ARG, "%s: the gemx_refgen lives on device %d, the handle on device %d", what, r->device, device);
    if (r->cfg.env_base != env_base) return fail(GEMX_ERR_ARG, "%s: the gemx_refgen's env_base is %lld, the handle's %lld", what, (long long)r->cfg.env_base, (long long)env_base);
    if (r->dev_desc == nullptr) {  // once per handle (synchronous: the first such call is not made inside a stream capture)
        DeviceGuard guard(r->device);
        const RefgenDev G = make_dev(r->cfg);
        if (hipMalloc(&r->dev_desc, sizeof(G)) != hipSuccess) { r->dev_desc = nullptr; return fail(GEMX_ERR_ALLOC, "%s: hipMalloc(generator description) failed", what); }
        if (hipMemcpy(r->dev_desc, &G, sizeof(G), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(r->dev_desc);
            r->dev_desc = nullptr;
            return fail(GEMX_ERR_DEVICE, "%s: hipMemcpy(generator description) failed", what);
        }
    }
    *out = {(const RefgenDev *)r->dev_desc, r->value, r->sigma, r->left, r->n_sub, r->n_reset, r->t};
    *n_ref = r->cfg.n_ref;
    return GEMX_OK;
}
int refgen_policy_normals(gemx_refgen *r, int32_t K, void *refs_out_dev, hipStream_t st) {
    const int64_t total = (int64_t)K * r->n * r->cfg.n_ref;
    gemx_cov_note("refgen_normals_kernel<float>");
    hipLaunchKernelGGL(refgen_normals_kernel<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (float *)refs_out_dev, r->n, r->cfg.n_ref, K, r->cfg.seed, r->t,
                       r->cfg.env_base);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}
}  // namespace gemx
