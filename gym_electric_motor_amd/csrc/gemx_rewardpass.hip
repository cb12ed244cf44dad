// gemx_rewardpass.hip -- the reward of a STORED trajectory (include/gemx.h: gemx_reward_rows): WeightedSumOfErrors.reward
// (reward_functions/weighted_sum_of_errors.py:125-129 of the reference) over the K * N observation rows a physics rollout wrote, against
// the references the env shell showed before each step.  It is the third launch of a complete K-step rollout
//   gemx_rollout (obs, done)  ->  gemx_refgen_rollout_shell (done -> references)  ->  gemx_reward_rows (obs, references, done -> reward)
// which exists because the generators' restarts depend on the physics' done mask while the fused reward (gemx_rollout_reward) needs the
// references BEFORE the physics runs; the physics never reads the references, so the chain streams in one direction.
//
// Arithmetic: reward_row (gemx_reward.hpp), the one definition the fused reward of the stepping kernels calls too, so the result is the
// same bits.
//
// Traffic: sizeof(R) * (S_out + n_ref + 1) + 1 bytes per row, nearly all of it read.  A row of 4..24 values read by "its" lane would be a
// strided 4-byte access, so -- as in the observation stage (gemx_obsproc.hip), whose shape problem this is -- a tile of TILE rows goes
// through LDS: the workgroup loads 1 KiB * S_out contiguous bytes in 16-byte units, consecutive lanes consecutive units, scatters them
// into rows at an ODD dword stride, and lane r evaluates row r with one conflict-free LDS read per operand.  References (<= 4 values), the
// done byte and the reward are one short contiguous piece per lane: adjacent lanes touch adjacent bytes, so they go straight to / from
// global memory, the loads issued before the barrier.  A tensor that is only element-aligned (a view at an odd offset) takes the dword
// loop; the last, partial tile moves its whole 16-byte units and then single dwords: nothing beyond K * N rows is read or written.
// The whole reward description (all GEMX_MAX_OUT terms) and its hot terms, padded by the host (reward_hot_from), are kernel arguments
// BY VALUE: kernel arguments are read with scalar loads, so no uniform-address vector load of the description waits behind the stores
// (gemx_reward.hpp, RewardHot, has the measurement).
#include "gemx_support.hpp"

namespace {

using namespace gemx;  // RewardDev; the row tile: gemx_support.hpp

template <class R> struct RewTile { static constexpr int rows = 1024 / (int)sizeof(R); };  // 256 fp32 rows | 128 fp64 rows: 1 KiB per column
static_assert(tile_fits(RewTile<double>::rows, 2 * GEMX_MAX_OUT) && tile_fits(RewTile<float>::rows, GEMX_MAX_OUT), "the longest row is within tile_row's exactness bound");

// rows: K * N flat rows of n_out columns.  Row g is rewarded against refs_first[g] (g < N: the first control step) or refs_rows[g - N]
// (the references shown after step k - 1), both [.][n_ref].
template <class R>
__global__ __launch_bounds__(RewTile<R>::rows) void reward_rows_kernel(const R *__restrict__ obs, const R *__restrict__ refs_first, const R *__restrict__ refs_rows,
                                                                      const uint8_t *__restrict__ done, R *__restrict__ reward, int64_t rows, int64_t N,
                                                                      int n_out, uint32_t magic, int vec, RewardHot<R> H, RewardDev<R> W) {
    constexpr int T = RewTile<R>::rows, DW = (int)sizeof(R) / 4, HOT = gemx::GEMX_REWARD_HOT;
    extern __shared__ __attribute__((aligned(16))) uint32_t rew_smem[];
    const uint32_t L = (uint32_t)n_out * DW, S = L | 1u;  // odd row stride: lanes r and r' != r (mod 32) read distinct banks
    const int64_t tile0 = (int64_t)blockIdx.x * T;        // (64-bit: rows * n_out may exceed 2^31)
    const uint32_t rows_t = (uint32_t)(rows - tile0 < (int64_t)T ? rows - tile0 : (int64_t)T);

    tile_stage_in<T>(rew_smem, S, L, magic, reinterpret_cast<const uint32_t *>(obs + tile0 * n_out), rows_t * L, vec);
    // this lane's references and done byte, in flight across the barrier
    const bool valid = threadIdx.x < rows_t;
    const int64_t g = tile0 + threadIdx.x;
    R rv[GEMX_MAX_REF];
    unsigned char dn = 0;
#pragma unroll
    for (int j = 0; j < GEMX_MAX_REF; ++j) rv[j] = R(0);
    if (valid) {
        const R *rp = g < N ? refs_first + g * H.n_ref : refs_rows + (g - N) * H.n_ref;
#pragma unroll
        for (int j = 0; j < GEMX_MAX_REF; ++j)
            if (j < H.n_ref) rv[j] = rp[j];
        dn = done[g];
    }
    __syncthreads();
    if (!valid) return;
    const uint32_t *mine = rew_smem + threadIdx.x * S;
    auto at = [&](int col) { return tile_get(mine + (uint32_t)col * DW, R(0)); };
    R oh[HOT];
#pragma unroll
    for (int t = 0; t < HOT; ++t) oh[t] = at(H.col[t]);
    reward[g] = reward_row<R>(H, &W, oh, at, rv, dn != 0);
}

template <class R>
int rew_launch(const gemx_handle *h, const RewardHot<R> &H, const RewardDev<R> &W, const void *obs, const void *refs_first, const void *refs_rows, const uint8_t *done, int64_t rows,
               void *reward, hipStream_t st) {
    constexpr int T = RewTile<R>::rows, DW = (int)sizeof(R) / 4;
    const int64_t tiles = (rows + T - 1) / T;
    if (tiles > 0x7fffffffLL) return gemx::fail(GEMX_ERR_ARG, "K * N = %lld rows exceed %d tiles of %d rows", (long long)rows, 0x7fffffff, T);
    const uint32_t L = (uint32_t)h->nout * DW;
    const size_t lds = (size_t)T * (L | 1u) * 4u;
    gemx_cov_note(sizeof(R) == 4 ? "reward_rows_kernel<float>" : "reward_rows_kernel<double>");
    hipLaunchKernelGGL(reward_rows_kernel<R>, dim3((unsigned)tiles), dim3(T), lds, st, (const R *)obs, (const R *)refs_first, (const R *)refs_rows, done, (R *)reward,
                       rows, h->n, h->nout, tile_magic(L), (int)(((uintptr_t)obs & 15u) == 0), H, W);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

}  // namespace

extern "C" int gemx_reward_rows(gemx_handle *h, const void *obs_dev, const void *refs_first_dev, const void *refs_rows_dev, const uint8_t *done_dev, int32_t K,
                                void *reward_out_dev, void *stream) {
    if (!h) return gemx::fail(GEMX_ERR_ARG, "null handle");
    if (h->rw_n_ref < 0) return gemx::fail(GEMX_ERR_ARG, "no reward function installed (gemx_set_reward)");
    if (h->cfg.obs_layout != GEMX_OBS_AOS) return gemx::fail(GEMX_ERR_ARG, "gemx_reward_rows reads observation rows: it needs GEMX_OBS_AOS");
    if (K < 1) return gemx::fail(GEMX_ERR_ARG, "K must be >= 1");
    if (!obs_dev || !done_dev || !reward_out_dev) return gemx::fail(GEMX_ERR_ARG, "obs_dev, done_dev and reward_out_dev must not be null");
    if (h->rw_n_ref > 0 && (!refs_first_dev || (K > 1 && !refs_rows_dev)))
        return gemx::fail(GEMX_ERR_ARG, "a reward with n_ref = %d needs refs_first_dev (and refs_rows_dev when K > 1)", h->rw_n_ref);
    const bool f64 = h->cfg.dtype == GEMX_F64;
    const bool refs = h->rw_n_ref > 0;
    if (!gemx::elem_aligned(f64, obs_dev, reward_out_dev, refs ? refs_first_dev : nullptr, refs ? refs_rows_dev : nullptr)) return gemx::fail_unaligned();
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)K * h->n;
    return f64 ? rew_launch<double>(h, h->rh_d, h->rw_d, obs_dev, refs_first_dev, refs_rows_dev, done_dev, rows, reward_out_dev, st)
               : rew_launch<float>(h, h->rh_f, h->rw_f, obs_dev, refs_first_dev, refs_rows_dev, done_dev, rows, reward_out_dev, st);
}
