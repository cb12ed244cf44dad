// gemx_episode.hip -- device-side episode time limit and episode statistics (include/gemx.h: gemx_episode_*): what a user of the reference
// gets from gymnasium's TimeLimit and RecordEpisodeStatistics around `gem.make(...)`, as ONE launch behind the launch that wrote a step's
// `done` byte and reward.  Per env the handle keeps, as SoA [field][N],
//     length (i32)  ret (f64)      the running episode: its steps so far and the sum of its rewards
//     last_length   last_ret       the totals of the episode that ended last
//     n_finished (u32)             how many episodes have ended
// and a step is, per lane (episode_row below -- THE row function, which the step kernel and the rows pass both call, so that K calls of
// gemx_episode_step and one gemx_episode_rows over K stored rows agree bit for bit: flux_row's rule, gemx_fluxobs.hip):
//     length += 1, ret += (double)reward
//     truncated = max_steps > 0 && length >= max_steps && !done        (a step that terminates AND reaches the limit counts as terminated)
//     ended = done | truncated;   where ended: last_* = the totals, n_finished += 1, length = 0, ret = 0
// The return accumulates in fp64 whatever the row dtype: the accumulator is 8 bytes beside the row and the sum runs for a whole episode
// (the flux observer's Psi).  The only arithmetic is that one fp64 add: no contraction can change it.
//
// Shape: N independent lanes, 1 + sizeof(R) bytes read and 3 bytes written per env and step beside the 28 bytes of state -- no LDS, no
// atomics, no host state, no memset: a launch can be captured in a HIP graph and replayed.  Every lane reads all of its inputs before it
// writes any output, and no lane touches another lane's bytes: `done` and `reset_mask` may be the same buffer.
// Rows pass: a lane owns one env and scans its K rows in order (adjacent lanes read adjacent addresses of row k); the loads of the next
// ROWS_AHEAD rows are issued before the dependent adds of the first of them.
#include "gemx_support.hpp"

namespace {

struct EpisodeDev {  // the handle's state: one allocation of 28 N bytes, the 8-byte fields first
    double *ret, *last_ret;
    int32_t *length, *last_length;
    uint32_t *n_finished;
};

struct EpisodeRow {
    int32_t length, last_length;
    double ret, last_ret;
    uint32_t n_finished;
};

__device__ __forceinline__ EpisodeRow episode_load(const EpisodeDev &E, int64_t i) { return {E.length[i], E.last_length[i], E.ret[i], E.last_ret[i], E.n_finished[i]}; }
__device__ __forceinline__ void episode_store(const EpisodeDev &E, int64_t i, const EpisodeRow &s) {
    E.length[i] = s.length; E.last_length[i] = s.last_length; E.ret[i] = s.ret; E.last_ret[i] = s.last_ret; E.n_finished[i] = s.n_finished;
}

// one step of one env -> bit 0: truncated, bit 1: ended
__device__ __forceinline__ uint32_t episode_row(EpisodeRow &s, int32_t max_steps, bool done, double reward) {
    s.length += 1;
    s.ret += reward;
    const bool truncated = max_steps > 0 && s.length >= max_steps && !done;
    const bool ended = done | truncated;
    if (ended) {
        s.last_length = s.length; s.last_ret = s.ret;
        s.n_finished += 1u;
        s.length = 0; s.ret = 0.0;
    }
    return (truncated ? 1u : 0u) | (ended ? 2u : 0u);
}

// done and reset_mask may alias: no __restrict__ on either
template <class R>
__global__ __launch_bounds__(256) void episode_step_kernel(EpisodeDev E, const uint8_t *done, const R *__restrict__ reward, uint8_t *__restrict__ truncated,
                                                           uint8_t *__restrict__ ended, uint8_t *reset_mask, int64_t N, int32_t max_steps, int32_t in_kernel) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const bool dn = done[i] != 0;
    const double rw = reward != nullptr ? (double)reward[i] : 0.0;
    EpisodeRow s = episode_load(E, i);
    const uint32_t f = episode_row(s, max_steps, dn, rw);
    episode_store(E, i, s);
    truncated[i] = (uint8_t)(f & 1u);
    ended[i] = (uint8_t)(f >> 1);
    if (reset_mask != nullptr) reset_mask[i] = (uint8_t)(in_kernel ? (f & 1u) : (f >> 1));
}

constexpr int ROWS_AHEAD = 8;

template <class R>
__global__ __launch_bounds__(256) void episode_rows_kernel(EpisodeDev E, const uint8_t *__restrict__ done, const R *__restrict__ reward, uint8_t *__restrict__ ended,
                                                           double *__restrict__ fin_ret, int32_t *__restrict__ fin_len, int64_t N, int32_t K, int32_t max_steps) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    EpisodeRow s = episode_load(E, i);
    for (int32_t k0 = 0; k0 < K; k0 += ROWS_AHEAD) {
        uint8_t dn[ROWS_AHEAD];
        R rw[ROWS_AHEAD];
#pragma unroll
        for (int j = 0; j < ROWS_AHEAD; ++j) {  // the loads of the next rows, all in flight before the first add
            const bool in = k0 + j < K;
            const int64_t a = (int64_t)(k0 + j) * N + i;
            dn[j] = in ? done[a] : (uint8_t)0;
            rw[j] = in && reward != nullptr ? reward[a] : R(0);
        }
#pragma unroll
        for (int j = 0; j < ROWS_AHEAD; ++j) {
            if (k0 + j < K) {
                const int64_t a = (int64_t)(k0 + j) * N + i;
                const uint32_t f = episode_row(s, max_steps, dn[j] != 0, (double)rw[j]);
                const bool e = (f >> 1) != 0;
                ended[a] = (uint8_t)(f >> 1);
                if (fin_ret != nullptr) fin_ret[a] = e ? s.last_ret : 0.0;
                if (fin_len != nullptr) fin_len[a] = e ? s.last_length : 0;
            }
        }
    }
    episode_store(E, i, s);
}

}  // namespace

struct gemx_episode {
    gemx_episode_config cfg;
    EpisodeDev dev;
    void *base;  // the 28 N bytes behind `dev`
    int64_t n;
    int device, f64, owns;
    unsigned blocks;
};

extern "C" {

int gemx_episode_create(const gemx_episode_config *cfg, int64_t n_envs, int dtype, int device, void *state_dev, gemx_episode **out) {
    if (!cfg || !out) return gemx::fail(GEMX_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(gemx_episode_config)) return gemx::fail(GEMX_ERR_ARG, "gemx_episode_config size mismatch");
    if (cfg->max_steps < 0) return gemx::fail(GEMX_ERR_ARG, "max_steps must be >= 0 (0: no time limit)");
    if (cfg->auto_reset_in_kernel != 0 && cfg->auto_reset_in_kernel != 1) return gemx::fail(GEMX_ERR_ARG, "auto_reset_in_kernel must be 0 or 1");
    if (cfg->has_reward != 0 && cfg->has_reward != 1) return gemx::fail(GEMX_ERR_ARG, "has_reward must be 0 or 1");
    if (n_envs < 1) return gemx::fail(GEMX_ERR_ARG, "n_envs must be >= 1");
    const int64_t blocks = (n_envs + 255) / 256;
    if (blocks > 0x7fffffffLL) return gemx::fail(GEMX_ERR_ARG, "n_envs = %lld exceeds %d blocks of 256 lanes", (long long)n_envs, 0x7fffffff);
    if (((uintptr_t)state_dev & 7u) != 0) return gemx::fail(GEMX_ERR_ARG, "state_dev must be 8-byte aligned");
    if (int rc = gemx::check_device_dtype(device, dtype)) return rc;
    gemx_episode *h = new (std::nothrow) gemx_episode();
    if (!h) return gemx::fail(GEMX_ERR_ALLOC, "out of host memory");
    h->cfg = *cfg; h->n = n_envs; h->device = device; h->f64 = dtype == GEMX_F64; h->blocks = (unsigned)blocks; h->base = state_dev; h->owns = state_dev == nullptr;
    gemx::DeviceGuard guard(device);
    const size_t bytes = (size_t)n_envs * GEMX_EPISODE_STATE_BYTES;
    if (h->owns) {
        if (hipMalloc(&h->base, bytes) != hipSuccess) { delete h; return gemx::fail(GEMX_ERR_ALLOC, "hipMalloc(episode state) failed"); }
        if (hipMemset(h->base, 0, bytes) != hipSuccess) { (void)hipFree(h->base); delete h; return gemx::fail(GEMX_ERR_DEVICE, "hipMemset(episode state) failed"); }
    }
    char *p = (char *)h->base;
    h->dev.ret = (double *)p;
    h->dev.last_ret = (double *)(p + 8 * n_envs);
    h->dev.length = (int32_t *)(p + 16 * n_envs);
    h->dev.last_length = (int32_t *)(p + 20 * n_envs);
    h->dev.n_finished = (uint32_t *)(p + 24 * n_envs);
    *out = h;
    return GEMX_OK;
}

int gemx_episode_destroy(gemx_episode *h) {
    if (!h) return GEMX_OK;
    if (h->owns && h->base) {
        gemx::DeviceGuard guard(h->device);
        (void)hipFree(h->base);
    }
    delete h;
    return GEMX_OK;
}

int gemx_episode_step(gemx_episode *h, const uint8_t *done_dev, const void *reward_dev, uint8_t *truncated_out_dev, uint8_t *ended_out_dev, uint8_t *reset_mask_out_dev,
                      void *stream) {
    if (!h || !done_dev || !truncated_out_dev || !ended_out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if ((reward_dev != nullptr) != (h->cfg.has_reward != 0)) return gemx::fail(GEMX_ERR_ARG, "reward_dev must be given exactly when the handle has_reward");
    if (!gemx::elem_aligned(h->f64 != 0, reward_dev)) return gemx::fail_unaligned();
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    gemx_cov_note(h->f64 ? "episode_step_kernel<double>" : "episode_step_kernel<float>");
    if (h->f64)
        hipLaunchKernelGGL(episode_step_kernel<double>, dim3(h->blocks), dim3(256), 0, st, h->dev, done_dev, (const double *)reward_dev, truncated_out_dev, ended_out_dev,
                           reset_mask_out_dev, h->n, h->cfg.max_steps, h->cfg.auto_reset_in_kernel);
    else
        hipLaunchKernelGGL(episode_step_kernel<float>, dim3(h->blocks), dim3(256), 0, st, h->dev, done_dev, (const float *)reward_dev, truncated_out_dev, ended_out_dev,
                           reset_mask_out_dev, h->n, h->cfg.max_steps, h->cfg.auto_reset_in_kernel);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

int gemx_episode_rows(gemx_episode *h, const uint8_t *done_dev, const void *reward_dev, int32_t K, uint8_t *ended_out_dev, double *finished_return_out_dev,
                      int32_t *finished_length_out_dev, void *stream) {
    if (!h || !done_dev || !ended_out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (K < 1) return gemx::fail(GEMX_ERR_ARG, "K must be >= 1");
    if ((reward_dev != nullptr) != (h->cfg.has_reward != 0)) return gemx::fail(GEMX_ERR_ARG, "reward_dev must be given exactly when the handle has_reward");
    if (!gemx::elem_aligned(h->f64 != 0, reward_dev) || !gemx::elem_aligned(true, finished_return_out_dev) || !gemx::elem_aligned(false, finished_length_out_dev))
        return gemx::fail_unaligned();
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    gemx_cov_note(h->f64 ? "episode_rows_kernel<double>" : "episode_rows_kernel<float>");
    if (h->f64)
        hipLaunchKernelGGL(episode_rows_kernel<double>, dim3(h->blocks), dim3(256), 0, st, h->dev, done_dev, (const double *)reward_dev, ended_out_dev,
                           finished_return_out_dev, finished_length_out_dev, h->n, K, h->cfg.max_steps);
    else
        hipLaunchKernelGGL(episode_rows_kernel<float>, dim3(h->blocks), dim3(256), 0, st, h->dev, done_dev, (const float *)reward_dev, ended_out_dev,
                           finished_return_out_dev, finished_length_out_dev, h->n, K, h->cfg.max_steps);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

int gemx_episode_get_state(gemx_episode *h, void *out_dev, void *stream) {
    if (!h || !out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    GEMX_HIP_TRY(hipMemcpyAsync(out_dev, h->base, (size_t)h->n * GEMX_EPISODE_STATE_BYTES, hipMemcpyDeviceToDevice, st));
    GEMX_HIP_TRY(hipStreamSynchronize(st));
    return GEMX_OK;
}

int gemx_episode_set_state(gemx_episode *h, const void *in_dev, void *stream) {
    if (!h || !in_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    GEMX_HIP_TRY(hipMemcpyAsync(h->base, in_dev, (size_t)h->n * GEMX_EPISODE_STATE_BYTES, hipMemcpyDeviceToDevice, st));
    GEMX_HIP_TRY(hipStreamSynchronize(st));
    return GEMX_OK;
}

}  // extern "C"
