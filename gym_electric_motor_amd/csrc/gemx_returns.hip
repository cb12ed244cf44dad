// gemx_returns.hip -- discounted returns and generalised advantage estimates, GAE(lambda), over the stored rows of a rollout
// (include/gemx.h: gemx_returns_rows): the first learner-side consumer of what the env hands out, as ONE launch -- the reversed loop of
// torch ops it replaces is four to six launches per row.  No per-env state survives a call: there is no handle.
//
// Per env the pass walks k = K-1 ... 0 with ONE fp64 accumulator A (returns_row below -- THE row function, the only arithmetic of this unit;
// everything is converted to double first):
//     term = terminated[k] != 0;  end = ended[k] != 0 (no `ended`: end = term);  trunc = end && !term
//     v      = value[k]
//     v_next = k == K-1 ? last_value : value[k+1]                              (no `last_value`: 0)
//     if (end)  v_next = trunc && final_value ? final_value[k] : 0             (final_value is read at rows with end && !term ONLY)
//     t1 = gamma * v_next;  delta = (reward[k] + t1) - v
//     t2 = gamma * lam;     t3 = t2 * A;   A = end ? delta : delta + t3
//     advantage[k] = (R)A;  return[k] = (R)(A + v)
// A starts as carry_in (no `carry_in`: 0) and carry_out receives it after row 0: rows [K/2, K) and then rows [0, K/2) with
// carry_out -> carry_in and last_value = value[K/2] are one scan, bit for bit.  A TRUNCATED ROW WITHOUT final_value IS TREATED AS
// TERMINATED: its successor's value is not the value of the state the episode ended in, so nothing is bootstrapped from it.
// Every product and sum above is rounded on its own (__dmul_rn / __dadd_rn / __dsub_rn, contraction off in the row function): no FMA
// is formed across them, so a float64 host restatement of the same operations gives the same bits.  A is fp64 whatever the row dtype:
// 8 bytes beside the row, and the recursion runs for a whole episode.
//
// Without `value` the pass is the plain discounted return-to-go, the same row function with
//     v = 0 and v_next = 0 in every row, lam taken as 1 (cfg->lam is ignored),
//     A starts as carry_in if given, else as (double)last_value if given, else as 0      (both given: GEMX_ERR_ARG)
// so return[k] = reward[k] + gamma * return[k+1], cut where an episode ended; return_out is the only output allowed and final_value is
// refused (a truncated row is treated as terminated).
//
// Shape: a lane owns one env, lanes adjacent in N: row k is a coalesced access.  The lane walks k downwards in groups of GROUP_ROWS rows;
// the loads of a whole group -- the two bytes, reward, value, then final_value where a row is truncated -- are issued before the first
// dependent operation, and value[k+1] comes from the registers of the row above, never from a second load.  256 lanes per workgroup,
// 64-bit indices, the partial last workgroup masked.  No LDS, no atomics, no scratch, no host state, no memset, no synchronisation: the
// launch can be captured in a HIP graph.  One env per lane is kept (byte loads of one byte per lane, as gemx_episode.hip's rows pass): a
// lane owning four adjacent envs would need N % 4 == 0 and 16-byte aligned rows or a second path for the rest.
#include "gemx_support.hpp"

namespace {

constexpr int GROUP_ROWS = 16;  // rows in flight per lane: 16 x (2 sizeof(R) + 2) bytes x 64 lanes per wave

struct ReturnsOut {
    double advantage, ret;
};

// one row of one env, k descending; A is the accumulator entering from row k+1 and leaving to row k-1
__device__ __forceinline__ ReturnsOut returns_row(double &A, double gamma, double lam, double reward, double v, double v_next, bool term, bool end, bool has_final,
                                                  double final_v) {
#pragma clang fp contract(off)
    const bool trunc = end && !term;
    if (end) v_next = trunc && has_final ? final_v : 0.0;
    const double t1 = __dmul_rn(gamma, v_next);
    const double delta = __dsub_rn(__dadd_rn(reward, t1), v);
    const double t2 = __dmul_rn(gamma, lam);
    const double t3 = __dmul_rn(t2, A);
    A = end ? delta : __dadd_rn(delta, t3);
    return {A, __dadd_rn(A, v)};
}

template <class R>
__global__ __launch_bounds__(256) void returns_rows_kernel(const R *__restrict__ reward, const R *__restrict__ value, const R *__restrict__ last_value,
                                                           const uint8_t *__restrict__ terminated, const uint8_t *__restrict__ ended,
                                                           const R *__restrict__ final_value, const double *__restrict__ carry_in, double *__restrict__ carry_out,
                                                           R *__restrict__ advantage_out, R *__restrict__ return_out, int64_t N, int32_t K, double gamma, double lam) {
    const int64_t base = (int64_t)blockIdx.x * 256;  // wave-uniform: a row's address is a scalar base plus the lane's 32-bit offset
    const uint32_t lane = threadIdx.x;
    const int64_t i = base + lane;
    if (i >= N) return;
    double A = carry_in != nullptr ? carry_in[i] : 0.0;
    double v_above = last_value != nullptr ? (double)last_value[i] : 0.0;  // the value of the row above: v_next of the next row down
    if (value == nullptr) {  // return-to-go: last_value seeds the accumulator (the entry point refuses carry_in AND last_value)
        if (carry_in == nullptr) A = v_above;
        v_above = 0.0;
    }
    // rows hi-1 ... hi-GROUP_ROWS, slot j is row hi-1-j; FULL: all of them exist (the last group of a K that is no multiple is partial)
    auto group = [&](int32_t hi, auto full) {
        constexpr bool FULL = decltype(full)::value;
        uint8_t tm[GROUP_ROWS], en[GROUP_ROWS];
        R rw[GROUP_ROWS], vl[GROUP_ROWS], fv[GROUP_ROWS];
#pragma unroll
        for (int j = 0; j < GROUP_ROWS; ++j) {  // the loads of the group, all in flight before the first dependent operation: the bytes first
            const int32_t k = hi - 1 - j;
            const bool in = FULL || k >= 0;
            const int64_t a = (int64_t)(in ? k : 0) * N + base;
            tm[j] = in ? (terminated + a)[lane] : (uint8_t)0;
            en[j] = in && ended != nullptr ? (ended + a)[lane] : (uint8_t)0;
        }
#pragma unroll
        for (int j = 0; j < GROUP_ROWS; ++j) {
            const int32_t k = hi - 1 - j;
            const bool in = FULL || k >= 0;
            const int64_t a = (int64_t)(in ? k : 0) * N + base;
            rw[j] = in ? (reward + a)[lane] : R(0);
            vl[j] = in && value != nullptr ? (value + a)[lane] : R(0);
        }
#pragma unroll
        for (int j = 0; j < GROUP_ROWS; ++j) {  // final_value: read where a row is truncated and nowhere else
            const int32_t k = hi - 1 - j;
            const bool in = FULL || k >= 0;
            const int64_t a = (int64_t)(in ? k : 0) * N + base;
            if (ended == nullptr) en[j] = tm[j];
            fv[j] = in && final_value != nullptr && en[j] != 0 && tm[j] == 0 ? (final_value + a)[lane] : R(0);
        }
#pragma unroll
        for (int j = 0; j < GROUP_ROWS; ++j) {
            const int32_t k = hi - 1 - j;
            if (FULL || k >= 0) {
                const int64_t a = (int64_t)k * N + base;
                const double v = (double)vl[j];
                const ReturnsOut o = returns_row(A, gamma, lam, (double)rw[j], v, v_above, tm[j] != 0, en[j] != 0, final_value != nullptr, (double)fv[j]);
                if (advantage_out != nullptr) (advantage_out + a)[lane] = (R)o.advantage;
                if (return_out != nullptr) (return_out + a)[lane] = (R)o.ret;
                v_above = v;
            }
        }
    };
    int32_t hi = K;
    for (; hi >= GROUP_ROWS; hi -= GROUP_ROWS) group(hi, std::true_type());
    if (hi > 0) group(hi, std::false_type());
    if (carry_out != nullptr) carry_out[i] = A;
}

template <class R>
void returns_launch(unsigned blocks, hipStream_t st, const void *reward, const void *value, const void *last_value, const uint8_t *terminated, const uint8_t *ended,
                    const void *final_value, const double *carry_in, double *carry_out, void *advantage_out, void *return_out, int64_t N, int32_t K, double gamma,
                    double lam) {
    hipLaunchKernelGGL(returns_rows_kernel<R>, dim3(blocks), dim3(256), 0, st, (const R *)reward, (const R *)value, (const R *)last_value, terminated, ended,
                       (const R *)final_value, carry_in, carry_out, (R *)advantage_out, (R *)return_out, N, K, gamma, lam);
}

}  // namespace

extern "C" {

int gemx_returns_rows(const gemx_returns_config *cfg, int64_t n_envs, int32_t K, int dtype, int device, const void *reward_dev, const void *value_dev,
                      const void *last_value_dev, const uint8_t *terminated_dev, const uint8_t *ended_dev, const void *final_value_dev, const double *carry_in_dev,
                      double *carry_out_dev, void *advantage_out_dev, void *return_out_dev, void *stream) {
    if (!cfg) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (cfg->struct_size != (int32_t)sizeof(gemx_returns_config)) return gemx::fail(GEMX_ERR_ARG, "gemx_returns_config size mismatch");
    if (cfg->flags != 0) return gemx::fail(GEMX_ERR_ARG, "gemx_returns_config.flags must be 0");
    if (!(cfg->gamma >= 0.0 && cfg->gamma <= 1.0)) return gemx::fail(GEMX_ERR_ARG, "gamma must be in [0, 1]");
    if (!reward_dev || !terminated_dev) return gemx::fail(GEMX_ERR_ARG, "reward_dev and terminated_dev must be given");
    if (!advantage_out_dev && !return_out_dev) return gemx::fail(GEMX_ERR_ARG, "at least one of advantage_out_dev and return_out_dev must be given");
    if (value_dev) {
        if (!(cfg->lam >= 0.0 && cfg->lam <= 1.0)) return gemx::fail(GEMX_ERR_ARG, "lam must be in [0, 1]");
    } else {
        if (advantage_out_dev) return gemx::fail(GEMX_ERR_ARG, "without value_dev the pass is the discounted return-to-go: return_out_dev is the only output");
        if (!return_out_dev) return gemx::fail(GEMX_ERR_ARG, "without value_dev return_out_dev must be given");
        if (final_value_dev) return gemx::fail(GEMX_ERR_ARG, "without value_dev there is no final_value_dev: a truncated row is treated as terminated");
        if (last_value_dev && carry_in_dev) return gemx::fail(GEMX_ERR_ARG, "without value_dev last_value_dev seeds the accumulator: give it or carry_in_dev, not both");
    }
    if (K < 1) return gemx::fail(GEMX_ERR_ARG, "K must be >= 1");
    if (n_envs < 1) return gemx::fail(GEMX_ERR_ARG, "n_envs must be >= 1");
    const int64_t blocks = (n_envs + 255) / 256;
    if (blocks > 0x7fffffffLL) return gemx::fail(GEMX_ERR_ARG, "n_envs = %lld exceeds %d blocks of 256 lanes", (long long)n_envs, 0x7fffffff);
    const bool f64 = dtype == GEMX_F64;
    if (!gemx::elem_aligned(f64, reward_dev, value_dev, last_value_dev, final_value_dev, advantage_out_dev, return_out_dev) ||
        !gemx::elem_aligned(true, carry_in_dev, carry_out_dev))
        return gemx::fail_unaligned();
    if (int rc = gemx::check_device_dtype(device, dtype)) return rc;
    gemx::DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    const double lam = value_dev ? cfg->lam : 1.0;
    gemx_cov_note(f64 ? "returns_rows_kernel<double>" : "returns_rows_kernel<float>");
    if (f64)
        returns_launch<double>((unsigned)blocks, st, reward_dev, value_dev, last_value_dev, terminated_dev, ended_dev, final_value_dev, carry_in_dev, carry_out_dev,
                               advantage_out_dev, return_out_dev, n_envs, K, cfg->gamma, lam);
    else
        returns_launch<float>((unsigned)blocks, st, reward_dev, value_dev, last_value_dev, terminated_dev, ended_dev, final_value_dev, carry_in_dev, carry_out_dev,
                              advantage_out_dev, return_out_dev, n_envs, K, cfg->gamma, lam);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

}  // extern "C"
