// gemx_statenoise.hip -- device-side StateNoiseProcessor (include/gemx.h: gemx_noise_*): the reference's measurement-noise wrapper
// (physical_system_wrappers/state_noise_processor.py:62-92) together with what the reference's env shell then does on the NOISY state
// (core.py:344-350): the constraint check and the reward.  The stepping kernels fuse both, and the auto-reset they trigger, into the
// physics; under a noise wrapper the physics runs with no constraint, no auto-reset and no reward, and this unit, ONE launch behind it,
//   1. adds the draw of (env, noisy column, stream position) to the noisy columns of the row,
//   2. decides `done` on the noisy row with constraint_done's expressions (gemx_kernels.hpp),
//   3. rewards the noisy row with reward_row (gemx_reward.hpp), the one definition gemx_reward_rows and the fused reward call too,
// and the env feeds the done mask back as the mask of the next step's gemx_reset.
//
// Shape: a streaming read-modify-write of N rows of n_in values, sizeof(R) * (2 n_in + n_ref + 1) + 1 bytes per row -- the observation
// stage's problem (gemx_obsproc.hip), solved the same way: a tile of 1 KiB * n_in contiguous bytes goes through LDS in 16-byte units, rows
// at an ODD dword stride, lane r works on row r with conflict-free LDS accesses at uniform columns, and the SAME tile is gathered back into
// 16-byte units.  A workgroup has read its whole tile before it writes any of it and tiles are disjoint, so state_in == state_out is legal.
// References, the done byte and the reward are one short contiguous piece per lane and go straight to / from global memory.
//
// Randomness: Philox4x32-10 (gemx_common.hpp), counter (global env | block << 48 | 7 << 60, position), key = seed; one block serves two
// noisy columns (slot j: block j / 2, words 2 (j % 2) and 2 (j % 2) + 1), so the draw of (env, slot, position) is a pure function of
// (seed, env_base + env, position, slot).  The draw is evaluated in double from the uniform words -- normal by Box-Muller, uniform and
// Laplace by the inverse distribution function -- and rounded to R before it is added.
// Stream position: in device memory, so that a replayed HIP graph advances it.  Every workgroup owns a copy (pos[blockIdx.x]): it reads
// its copy before the first barrier and lane 0 writes position + 1 behind the last one -- no workgroup reads a word another one writes.
#include "gemx_support.hpp"

#include <cmath>

namespace {

using namespace gemx;  // RewardDev, Philox; the row tile: gemx_support.hpp

template <class R> struct NoiseTile { static constexpr int rows = 1024 / (int)sizeof(R); };  // 256 fp32 rows | 128 fp64 rows: 1 KiB per column
static_assert(tile_fits(NoiseTile<double>::rows, 2 * GEMX_MAX_OUT) && tile_fits(NoiseTile<float>::rows, GEMX_MAX_OUT), "the longest row is within tile_row's exactness bound");

struct NoiseDev {
    int32_t n_in, n_noisy, pair_form, pair_a, pair_b;  // pair_form: the constraint is a system's default squared pair (+ limits): default_done's expression
    uint32_t limit_mask, squared_mask;
    uint64_t seed;
    int64_t env_base;
    uint8_t index[GEMX_MAX_OUT], dist[GEMX_MAX_OUT];
    double p0[GEMX_MAX_OUT], p1[GEMX_MAX_OUT];  // loc, scale | low, high
};

__device__ inline void noise_block(uint64_t seed, int64_t env, uint32_t blk, uint64_t pos, uint32_t (&r)[4]) {
    const uint64_t env_word = (uint64_t)env | ((uint64_t)blk << 48) | (7ull << 60);  // (7: no draw kind of the reference generators, which share the seed)
    uint32_t c[4] = {(uint32_t)env_word, (uint32_t)(env_word >> 32), (uint32_t)pos, (uint32_t)(pos >> 32)};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int i = 0; i < 10; ++i) {
        Philox::round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    for (int i = 0; i < 4; ++i) r[i] = c[i];
}

// the draw of one noisy slot from its two words, in double
__device__ inline double noise_draw(int dist, double p0, double p1, uint32_t w0, uint32_t w1) {
    const double u = Philox::u01(w0);
    if (dist == GEMX_NOISE_UNIFORM) return p0 + (p1 - p0) * u;
    if (dist == GEMX_NOISE_LAPLACE) {  // loc - scale sign(u - 1/2) ln(1 - 2 |u - 1/2|); the argument is >= 2^-32
        const double t = u - 0.5;
        const double m = -log(1.0 - 2.0 * fabs(t));
        return p0 + p1 * (t < 0.0 ? -m : m);
    }
    return p0 + p1 * (sqrt(-2.0 * log(u)) * cos(kTwoPi * Philox::u01(w1)));
}

template <class R> __device__ inline R noise_value(const NoiseDev &D, int64_t env, uint64_t pos, int j) {
    uint32_t r[4];
    noise_block(D.seed, D.env_base + env, (uint32_t)j >> 1, pos, r);
    const int o = (j & 1) * 2;
    return (R)noise_draw(D.dist[j], D.p0[j], D.p1[j], r[o], r[o + 1]);
}

template <class R>
__global__ __launch_bounds__(NoiseTile<R>::rows) void state_noise_kernel(const R *state_in, const R *__restrict__ refs, R *state_out, uint8_t *__restrict__ done,
                                                                        R *__restrict__ reward, uint64_t *__restrict__ pos, int64_t rows, uint32_t magic, int vec_in,
                                                                        int vec_out, NoiseDev D, RewardHot<R> H, RewardDev<R> W) {
    constexpr int T = NoiseTile<R>::rows, DW = (int)sizeof(R) / 4, HOT = gemx::GEMX_REWARD_HOT;
    extern __shared__ __attribute__((aligned(16))) uint32_t noise_smem[];
    const uint32_t L = (uint32_t)D.n_in * DW, S = L | 1u;  // odd row stride: lanes r and r' != r (mod 32) touch distinct banks
    const int64_t tile0 = (int64_t)blockIdx.x * T;
    const uint32_t rows_t = (uint32_t)(rows - tile0 < (int64_t)T ? rows - tile0 : (int64_t)T);
    const uint64_t position = pos[blockIdx.x];  // this workgroup's copy

    tile_stage_in<T>(noise_smem, S, L, magic, reinterpret_cast<const uint32_t *>(state_in + tile0 * D.n_in), rows_t * L, vec_in);
    const bool valid = threadIdx.x < rows_t;
    const int64_t g = tile0 + threadIdx.x;
    R rv[GEMX_MAX_REF];
#pragma unroll
    for (int j = 0; j < GEMX_MAX_REF; ++j) rv[j] = R(0);
    if (valid && reward != nullptr) {  // this lane's references, in flight across the barrier
        const R *rp = refs + g * H.n_ref;
#pragma unroll
        for (int j = 0; j < GEMX_MAX_REF; ++j)
            if (j < H.n_ref) rv[j] = rp[j];
    }
    __syncthreads();
    if (valid) {
        uint32_t *mine = noise_smem + threadIdx.x * S;
        // 1. the noise
        uint32_t r[4];
        for (int j = 0; j < D.n_noisy; ++j) {  // (uniform: the description sits in SGPRs)
            if ((j & 1) == 0) noise_block(D.seed, D.env_base + g, (uint32_t)j >> 1, position, r);
            const int o = (j & 1) * 2;
            const R draw = (R)noise_draw(D.dist[j], D.p0[j], D.p1[j], r[o], r[o + 1]);
            uint32_t *p = mine + (uint32_t)D.index[j] * DW;
            tile_put(p, tile_get(p, R(0)) + draw);
        }
        // 2. ConstraintMonitor on the noisy row: constraint_done's two forms
        bool dn;
        if (D.pair_form) {
            const R a = tile_get(mine + (uint32_t)D.pair_a * DW, R(0)), b = tile_get(mine + (uint32_t)D.pair_b * DW, R(0));
            dn = a * a + b * b > R(1);
            for (uint32_t m = D.limit_mask; m; m &= m - 1u) dn |= fabs(tile_get(mine + (uint32_t)(__ffs(m) - 1) * DW, R(0))) > R(1);
        } else {
            R lim = R(0), sq = R(0);
            for (int i = 0; i < D.n_in; ++i) {
                const R x = tile_get(mine + (uint32_t)i * DW, R(0));
                const R cl = (D.limit_mask >> i & 1u) ? R(1) : R(0), cs = (D.squared_mask >> i & 1u) ? R(1) : R(0);
                lim = fmax(lim, cl * fabs(x));
                sq += (cs * x) * x;
            }
            dn = (lim > R(1)) | (sq > R(1));
        }
        done[g] = dn ? 1 : 0;
        // 3. the reward of the noisy row
        if (reward != nullptr) {
            auto at = [&](int col) { return tile_get(mine + (uint32_t)col * DW, R(0)); };
            R oh[HOT];
#pragma unroll
            for (int t = 0; t < HOT; ++t) oh[t] = at(H.col[t]);
            reward[g] = reward_row<R>(H, &W, oh, at, rv, dn);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) pos[blockIdx.x] = position + 1u;
    tile_stage_out<T>(noise_smem, S, L, magic, reinterpret_cast<uint32_t *>(state_out + tile0 * D.n_in), rows_t * L, vec_out);
}

// gemx_noise_draws: out[k][env][j] = the draw of (env, slot j, step0 + k)
template <class R> __global__ void noise_draws_kernel(R *__restrict__ out, int64_t N, int K, uint64_t step0, NoiseDev D) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)K * N * D.n_noisy) return;
    const int j = (int)(idx % D.n_noisy);
    const int64_t env = (idx / D.n_noisy) % N;
    out[idx] = noise_value<R>(D, env, step0 + (uint64_t)(idx / ((int64_t)D.n_noisy * N)), j);
}

__global__ void noise_fill_kernel(uint64_t *pos, int n, uint64_t value) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pos[i] = value;
}

}  // namespace

struct gemx_noise {
    gemx_noise_config cfg;
    NoiseDev dev;
    RewardDev<float> wf;  // the reward description and its hot terms, both dtypes (zero without a reward)
    RewardDev<double> wd;
    RewardHot<float> hf;
    RewardHot<double> hd;
    int64_t n;
    int device, f64, tiles;
    uint64_t *pos;  // [tiles]
};

template <class R>
static int noise_launch(gemx_noise *h, const RewardHot<R> &H, const RewardDev<R> &W, const void *in, const void *refs, void *out, uint8_t *done, void *reward, hipStream_t st) {
    constexpr int T = NoiseTile<R>::rows, DW = (int)sizeof(R) / 4;
    const uint32_t L = (uint32_t)h->dev.n_in * DW;
    const size_t lds = (size_t)T * (L | 1u) * 4u;
    gemx_cov_note(sizeof(R) == 4 ? "state_noise_kernel<float>" : "state_noise_kernel<double>");
    hipLaunchKernelGGL(state_noise_kernel<R>, dim3((unsigned)h->tiles), dim3(T), lds, st, (const R *)in, (const R *)refs, (R *)out, done, (R *)reward, h->pos, h->n,
                       tile_magic(L), (int)(((uintptr_t)in & 15u) == 0), (int)(((uintptr_t)out & 15u) == 0), h->dev, H, W);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

extern "C" {

int gemx_noise_create(const gemx_noise_config *cfg, int64_t n_envs, int dtype, int device, gemx_noise **out) {
    if (!cfg || !out) return gemx::fail(GEMX_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(gemx_noise_config)) return gemx::fail(GEMX_ERR_ARG, "gemx_noise_config size mismatch");
    if (cfg->n_in < 1 || cfg->n_in > GEMX_MAX_OUT) return gemx::fail(GEMX_ERR_ARG, "n_in must be in [1, %d]", GEMX_MAX_OUT);
    if (cfg->n_noisy < 0 || cfg->n_noisy > cfg->n_in) return gemx::fail(GEMX_ERR_ARG, "n_noisy must be in [0, n_in = %d]", cfg->n_in);
    if (n_envs < 1) return gemx::fail(GEMX_ERR_ARG, "n_envs must be >= 1");
    if (cfg->env_base < 0 || cfg->env_base + n_envs > (1ll << 48)) return gemx::fail(GEMX_ERR_ARG, "env_base + n_envs must be in [0, 2^48]");
    const uint32_t valid = cfg->n_in >= 32 ? 0xffffffffu : (1u << cfg->n_in) - 1u;
    if ((cfg->limit_mask | cfg->squared_mask) & ~valid) return gemx::fail(GEMX_ERR_ARG, "a constraint mask names a column >= n_in = %d", cfg->n_in);
    uint32_t seen = 0;
    for (int j = 0; j < cfg->n_noisy; ++j) {
        const int i = cfg->index[j];
        if (i < 0 || i >= cfg->n_in) return gemx::fail(GEMX_ERR_ARG, "index[%d] = %d outside [0, %d)", j, i, cfg->n_in);
        if (seen >> i & 1u) return gemx::fail(GEMX_ERR_ARG, "index[%d] = %d is listed twice", j, i);
        seen |= 1u << i;
        if (cfg->dist[j] < GEMX_NOISE_NORMAL || cfg->dist[j] > GEMX_NOISE_LAPLACE) return gemx::fail(GEMX_ERR_ARG, "dist[%d]: unknown distribution %d", j, cfg->dist[j]);
        if (!std::isfinite(cfg->param0[j]) || !std::isfinite(cfg->param1[j])) return gemx::fail(GEMX_ERR_ARG, "slot %d: parameters must be finite", j);
        if (cfg->dist[j] == GEMX_NOISE_UNIFORM ? cfg->param1[j] < cfg->param0[j] : cfg->param1[j] < 0.0)
            return gemx::fail(GEMX_ERR_ARG, "slot %d: scale must be >= 0 (uniform: high >= low)", j);
    }
    if (cfg->has_reward != 0 && cfg->has_reward != 1) return gemx::fail(GEMX_ERR_ARG, "has_reward must be 0 or 1");
    if (cfg->has_reward)
        if (int rc = gemx::reward_check(&cfg->reward, cfg->n_in)) return rc;
    if (int rc = gemx::check_device_dtype(device, dtype)) return rc;
    gemx_noise *h = new (std::nothrow) gemx_noise();
    if (!h) return gemx::fail(GEMX_ERR_ALLOC, "out of host memory");
    h->cfg = *cfg; h->n = n_envs; h->device = device; h->f64 = dtype == GEMX_F64; h->pos = nullptr;
    const int T = h->f64 ? NoiseTile<double>::rows : NoiseTile<float>::rows;
    const int64_t tiles = (n_envs + T - 1) / T;
    if (tiles > 0x7fffffffLL) { delete h; return gemx::fail(GEMX_ERR_ARG, "n_envs = %lld exceeds %d tiles of %d rows", (long long)n_envs, 0x7fffffff, T); }
    h->tiles = (int)tiles;
    NoiseDev &D = h->dev;
    memset(&D, 0, sizeof(D));
    D.n_in = cfg->n_in; D.n_noisy = cfg->n_noisy; D.limit_mask = cfg->limit_mask; D.squared_mask = cfg->squared_mask; D.seed = cfg->seed; D.env_base = cfg->env_base;
    for (int j = 0; j < cfg->n_noisy; ++j) { D.index[j] = (uint8_t)cfg->index[j]; D.dist[j] = (uint8_t)cfg->dist[j]; D.p0[j] = cfg->param0[j]; D.p1[j] = cfg->param1[j]; }
    // the default constraint of the systems with an angle (gemx_capi.hip: constr_kind 1) is evaluated by default_done's expression: the squared
    // pair (i_sd, i_sq) = columns 5, 6 of a row of 14 (SYNC, SCIM), 16 (EESM, with the limit on i_e = column 7) or 24 (DFIM) values
    const bool pair_rows = cfg->n_in == 14 || cfg->n_in == 16 || cfg->n_in == 24;
    D.pair_form = pair_rows && cfg->squared_mask == 0x60u && cfg->limit_mask == (cfg->n_in == 16 ? 0x80u : 0u);
    D.pair_a = 5; D.pair_b = 6;
    if (cfg->has_reward) {
        reward_build(cfg->n_in, &cfg->reward, h->wf);
        reward_build(cfg->n_in, &cfg->reward, h->wd);
    } else {
        memset(&h->wf, 0, sizeof(h->wf));
        memset(&h->wd, 0, sizeof(h->wd));
    }
    reward_hot_from(h->wf, h->hf);
    reward_hot_from(h->wd, h->hd);
    gemx::DeviceGuard guard(device);
    if (hipMalloc(&h->pos, (size_t)tiles * sizeof(uint64_t)) != hipSuccess) { delete h; return gemx::fail(GEMX_ERR_ALLOC, "hipMalloc(noise position) failed"); }
    if (hipMemset(h->pos, 0, (size_t)tiles * sizeof(uint64_t)) != hipSuccess) { (void)hipFree(h->pos); delete h; return gemx::fail(GEMX_ERR_DEVICE, "hipMemset(noise position) failed"); }
    *out = h;
    return GEMX_OK;
}

int gemx_noise_destroy(gemx_noise *h) {
    if (!h) return GEMX_OK;
    {
        gemx::DeviceGuard guard(h->device);
        if (h->pos) (void)hipFree(h->pos);
    }
    delete h;
    return GEMX_OK;
}

int gemx_noise_step(gemx_noise *h, const void *state_in_dev, const void *refs_dev, void *state_out_dev, uint8_t *done_out_dev, void *reward_out_dev, void *stream) {
    if (!h || !state_in_dev || !state_out_dev || !done_out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (reward_out_dev && !h->cfg.has_reward) return gemx::fail(GEMX_ERR_ARG, "reward_out_dev given, but the handle has no reward description");
    const bool refs = reward_out_dev && h->cfg.reward.n_ref > 0;
    if (refs && !refs_dev) return gemx::fail(GEMX_ERR_ARG, "a reward with n_ref = %d needs refs_dev", h->cfg.reward.n_ref);
    if (!gemx::elem_aligned(h->f64 != 0, state_in_dev, state_out_dev, reward_out_dev, refs ? refs_dev : nullptr)) return gemx::fail_unaligned();
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    return h->f64 ? noise_launch<double>(h, h->hd, h->wd, state_in_dev, refs_dev, state_out_dev, done_out_dev, reward_out_dev, st)
                  : noise_launch<float>(h, h->hf, h->wf, state_in_dev, refs_dev, state_out_dev, done_out_dev, reward_out_dev, st);
}

int gemx_noise_draws(gemx_noise *h, uint64_t step0, int32_t K, void *out_dev, void *stream) {
    if (!h || !out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (K < 1) return gemx::fail(GEMX_ERR_ARG, "K must be >= 1");
    if (!gemx::elem_aligned(h->f64 != 0, out_dev)) return gemx::fail_unaligned();
    if (h->dev.n_noisy == 0) return GEMX_OK;
    const int64_t total = (int64_t)K * h->n * h->dev.n_noisy, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return gemx::fail(GEMX_ERR_ARG, "K * N * n_noisy = %lld exceeds %d blocks of 256", (long long)total, 0x7fffffff);
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    gemx_cov_note(h->f64 ? "noise_draws_kernel<double>" : "noise_draws_kernel<float>");
    if (h->f64) hipLaunchKernelGGL(noise_draws_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, st, (double *)out_dev, h->n, K, step0, h->dev);
    else hipLaunchKernelGGL(noise_draws_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (float *)out_dev, h->n, K, step0, h->dev);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

int gemx_noise_get_position(gemx_noise *h, uint64_t *position_host, void *stream) {
    if (!h || !position_host) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    GEMX_HIP_TRY(hipMemcpyAsync(position_host, h->pos, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    GEMX_HIP_TRY(hipStreamSynchronize(st));
    return GEMX_OK;
}

int gemx_noise_set_position(gemx_noise *h, uint64_t position, void *stream) {
    if (!h) return gemx::fail(GEMX_ERR_ARG, "null handle");
    gemx::DeviceGuard guard(h->device);
    gemx_cov_note("noise_fill_kernel");
    hipLaunchKernelGGL(noise_fill_kernel, dim3((unsigned)((h->tiles + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->pos, h->tiles, position);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

}  // extern "C"
