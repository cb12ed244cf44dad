// gemx_rewardpass.hip -- the reward of a STORED trajectory (include/gemx.h: gemx_reward_rows): WeightedSumOfErrors.reward
// (reward_functions/weighted_sum_of_errors.py:125-129 of the reference) over the K * N observation rows a physics rollout wrote, against
// the references the env shell showed before each step.  It is the third launch of a complete K-step rollout
//   gemx_rollout (obs, done)  ->  gemx_refgen_rollout_shell (done -> references)  ->  gemx_reward_rows (obs, references, done -> reward)
// which exists because the generators' restarts depend on the physics' done mask while the fused reward (gemx_rollout_reward) needs the
// references BEFORE the physics runs; the physics never reads the references, so the chain streams in one direction.
//
// Arithmetic: the fused reward's (gemx_kernels.hpp, reward_term / reward_apply), restated here operation for operation so that the result
// is the same bits: the first GEMX_REWARD_HOT terms with the select for powers 1 and 2 (unused hot terms padded with column 0, weight 0),
// the remaining terms in order -- or, as soon as one power is neither 1 nor 2, every term in order through the one pow() site --, each
// term rounded as a product before it is added (the term is a function's return value: -ffp-contract=on forms no fused multiply-add across
// it, there as here), bias - sum, and violation_reward where the row's done byte is set.
//
// Traffic: sizeof(R) * (S_out + n_ref + 1) + 1 bytes per row, nearly all of it read.  A row of 4..24 values read by "its" lane would be a
// strided 4-byte access, so -- as in the observation stage (gemx_obsproc.hip), whose shape problem this is -- a tile of TILE rows goes
// through LDS: the workgroup loads 1 KiB * S_out contiguous bytes in 16-byte units, consecutive lanes consecutive units, scatters them
// into rows at an ODD dword stride, and lane r evaluates row r with one conflict-free LDS read per operand.  References (<= 4 values), the
// done byte and the reward are one short contiguous piece per lane: adjacent lanes touch adjacent bytes, so they go straight to / from
// global memory, the loads issued before the barrier.  A tensor that is only element-aligned (a view at an odd offset) takes the dword
// loop; the last, partial tile moves its whole 16-byte units and then single dwords: nothing beyond K * N rows is read or written.
// The whole reward description (all GEMX_MAX_OUT terms) is a kernel argument BY VALUE: kernel arguments are read with scalar loads, so
// no uniform-address vector load of the description waits behind the stores (gemx_common.hpp, RewardHot, has the measurement).
#include "gemx_support.hpp"

#include <mutex>
#include <unordered_map>

namespace {

using namespace gemx;  // RewardDev; the row tile: gemx_support.hpp

template <class R> struct RewTile { static constexpr int rows = 1024 / (int)sizeof(R); };  // 256 fp32 rows | 128 fp64 rows: 1 KiB per column
static_assert(tile_fits(RewTile<double>::rows, 2 * GEMX_MAX_OUT) && tile_fits(RewTile<float>::rows, GEMX_MAX_OUT), "the longest row is within tile_row's exactness bound");

// reward_term of gemx_kernels.hpp, restated.  GENERAL: reward_power other than 1 or 2 allowed (pow())
template <bool GENERAL, class R> __device__ __forceinline__ R rew_term(R o, R ref, R inv_len, int kind, R power, R coef) {
    const R dlt = fabs(o - ref) * inv_len;
    R p = dlt * (kind == 2 ? dlt : R(1));  // (a select, not a branch: dlt * 1 == dlt exactly)
    if (GENERAL && kind == 3) p = pow(dlt, power);
    return coef * p;
}

// rows: K * N flat rows of n_out columns.  Row g is rewarded against refs_first[g] (g < N: the first control step) or refs_rows[g - N]
// (the references shown after step k - 1), both [.][n_ref].
template <class R>
__global__ __launch_bounds__(RewTile<R>::rows) void reward_rows_kernel(const R *__restrict__ obs, const R *__restrict__ refs_first, const R *__restrict__ refs_rows,
                                                                      const uint8_t *__restrict__ done, R *__restrict__ reward, int64_t rows, int64_t N,
                                                                      int n_out, uint32_t magic, int vec, int general, RewardDev<R> W) {
    constexpr int T = RewTile<R>::rows, DW = (int)sizeof(R) / 4, HOT = gemx::GEMX_REWARD_HOT;
    static_assert(HOT >= GEMX_MAX_REF, "referenced states must be hot terms");
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
        const R *rp = g < N ? refs_first + g * W.n_ref : refs_rows + (g - N) * W.n_ref;
#pragma unroll
        for (int j = 0; j < GEMX_MAX_REF; ++j)
            if (j < W.n_ref) rv[j] = rp[j];
        dn = done[g];
    }
    __syncthreads();
    if (!valid) return;
    const uint32_t *mine = rew_smem + threadIdx.x * S;
    R acc = R(0);
    if (!general) {
#pragma unroll
        for (int t = 0; t < HOT; ++t) {  // terms < n_ref are the referenced states (reference column t), the others compare with 0
            const bool used = t < W.n_term;  // unused hot terms: column 0, kind 1, weight 0 (reward_hot_from)
            const int col = used ? W.col[t] : 0, kind = used ? W.kind[t] : 1;
            const R coef = used ? W.coef[t] : R(0), inv_len = used ? W.inv_len[t] : R(0), power = used ? W.power[t] : R(1);
            acc += rew_term<false, R>(tile_get(mine + (uint32_t)col * DW, R(0)), rv[t], inv_len, kind, power, coef);
        }
    }
    // terms beyond the hot ones, and EVERY term when some reward_power is not 1 or 2 (one pow() site)
#pragma nounroll
    for (int t = general ? 0 : HOT; t < W.n_term; ++t) {
        R ref = R(0);
#pragma unroll
        for (int j = 0; j < GEMX_MAX_REF; ++j) ref = (t == j) ? rv[j] : ref;
        acc += rew_term<true, R>(tile_get(mine + (uint32_t)W.col[t] * DW, R(0)), ref, W.inv_len[t], W.kind[t], W.power[t], W.coef[t]);
    }
    const R wse = W.bias - acc;
    reward[g] = dn ? W.violation_reward : wse;  // (1 - v) * wse + v * violation_reward, v in {0, 1}
}

// The reward descriptions as gemx_set_reward built them, by handle, on the HOST: the handle itself keeps the full description in device
// memory only (the fused reward reads it there), and a kernel argument has to come from the host without a copy back per call.
struct RewDesc {
    RewardDev<float> f;
    RewardDev<double> d;
};
std::mutex g_rew_mutex;
std::unordered_map<const gemx_handle *, RewDesc> &rew_table() {
    static std::unordered_map<const gemx_handle *, RewDesc> t;
    return t;
}

template <class R>
int rew_launch(const gemx_handle *h, const RewardDev<R> &W, const void *obs, const void *refs_first, const void *refs_rows, const uint8_t *done, int64_t rows,
               void *reward, hipStream_t st) {
    constexpr int T = RewTile<R>::rows, DW = (int)sizeof(R) / 4;
    const int64_t tiles = (rows + T - 1) / T;
    if (tiles > 0x7fffffffLL) return gemx::fail(GEMX_ERR_ARG, "K * N = %lld rows exceed %d tiles of %d rows", (long long)rows, 0x7fffffff, T);
    const uint32_t L = (uint32_t)h->nout * DW;
    const size_t lds = (size_t)T * (L | 1u) * 4u;
    int general = 0;
    for (int t = 0; t < W.n_term; ++t) general |= W.kind[t] == 3;
    gemx_cov_note(sizeof(R) == 4 ? "reward_rows_kernel<float>" : "reward_rows_kernel<double>");
    hipLaunchKernelGGL(reward_rows_kernel<R>, dim3((unsigned)tiles), dim3(T), lds, st, (const R *)obs, (const R *)refs_first, (const R *)refs_rows, done, (R *)reward,
                       rows, h->n, h->nout, tile_magic(L), (int)(((uintptr_t)obs & 15u) == 0), general, W);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

}  // namespace

// called by gemx_set_reward (desc: the RewardDev<R> of the handle's dtype it has just built; nullptr: the reward was removed) and by
// gemx_destroy (nullptr)
void gemx_rewardpass_note(const gemx_handle *h, const void *desc) {
    std::lock_guard<std::mutex> lock(g_rew_mutex);
    if (!desc) {
        rew_table().erase(h);
        return;
    }
    RewDesc &e = rew_table()[h];
    if (h->cfg.dtype == GEMX_F64) memcpy(&e.d, desc, sizeof(e.d));
    else memcpy(&e.f, desc, sizeof(e.f));
}

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
    RewDesc desc;
    {
        std::lock_guard<std::mutex> lock(g_rew_mutex);
        auto it = rew_table().find(h);
        if (it == rew_table().end()) return gemx::fail(GEMX_ERR_ARG, "no reward function installed (gemx_set_reward)");
        desc = it->second;
    }
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)K * h->n;
    return f64 ? rew_launch<double>(h, desc.d, obs_dev, refs_first_dev, refs_rows_dev, done_dev, rows, reward_out_dev, st)
               : rew_launch<float>(h, desc.f, obs_dev, refs_first_dev, refs_rows_dev, done_dev, rows, reward_out_dev, st);
}
