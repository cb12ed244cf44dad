// gemx_reward.hpp -- THE definition of the WeightedSumOfErrors reward (reward_functions/weighted_sum_of_errors.py:125-129 of the
// reference), included by gemx_common.hpp: the description and its hot terms, the checks and the builder of a gemx_reward_config, and
// the reward of one row, reward_row.  reward_rows_kernel (gemx_rewardpass.hip) and state_noise_kernel (gemx_statenoise.hip) call it;
// reward_apply (gemx_kernels.hpp, the fused reward of the stepping kernels) and envparams_rollout_kernel (gemx_envparams.hip) carry its
// statements in place, because through the call those kernels compile to other instructions (profiles/reward_row_refactor.md) -- a
// change to reward_row is a change to those two blocks.
#pragma once

namespace gemx {

int fail(int code, const char *fmt, ...);  // sets gemx_last_error() (gemx_common.hpp)

// ------------------------------------------------------------------------------------------------
// fused reward (WeightedSumOfErrors): device-resident description, read through scalar loads when a reward is requested
// ------------------------------------------------------------------------------------------------
template <class R> struct RewardDev {
    // terms 0 .. n_ref-1 compare state column col[t] with reference column t; terms n_ref .. n_term-1 compare with 0
    int32_t n_ref, n_term;
    int32_t col[GEMX_MAX_OUT];
    int32_t kind[GEMX_MAX_OUT];   // 1: power 1, 2: power 2, 3: general power (pow)
    R coef[GEMX_MAX_OUT];         // weight (applied after the power)
    R inv_len[GEMX_MAX_OUT];      // 1 / state_length
    R power[GEMX_MAX_OUT];
    R bias, violation_reward;
};

// The first GEMX_REWARD_HOT terms by value, inside the kernel arguments: kernel arguments are read with SCALAR loads (lgkmcnt).  Read
// through the device pointer (KArgs::rw) the same words are VECTOR loads with a uniform address -- the compiler cannot prove that the
// kernel's own stores do not alias them -- and their `s_waitcnt vmcnt(0)` waits, vmcnt retiring in order, for every observation store
// the wave has in flight: ~5000 cycles per block in the pipelined kernel's output waves (s_memtime probe).
constexpr int GEMX_REWARD_HOT = 4;
static_assert(GEMX_REWARD_HOT >= GEMX_MAX_REF, "referenced states must be hot terms");
template <class R> struct RewardHot {
    int32_t n_ref, n_term, general;  // general: some term has a power other than 1 or 2 (pow() path through the full description)
    int32_t col[GEMX_REWARD_HOT], kind[GEMX_REWARD_HOT];  // unused terms: column 0, kind 1, weight 0
    R coef[GEMX_REWARD_HOT], inv_len[GEMX_REWARD_HOT], power[GEMX_REWARD_HOT];
    R bias, violation_reward;
};
template <class R> inline void reward_hot_from(const RewardDev<R> &W, RewardHot<R> &H) {
    H.n_ref = W.n_ref;
    H.n_term = W.n_term;
    H.general = 0;
    for (int t = 0; t < W.n_term; ++t) H.general |= W.kind[t] == 3;
    for (int t = 0; t < GEMX_REWARD_HOT; ++t) {
        const bool used = t < W.n_term;
        H.col[t] = used ? W.col[t] : 0;
        H.kind[t] = used ? W.kind[t] : 1;
        H.coef[t] = used ? W.coef[t] : R(0);
        H.inv_len[t] = used ? W.inv_len[t] : R(0);
        H.power[t] = used ? W.power[t] : R(1);
    }
    H.bias = W.bias;
    H.violation_reward = W.violation_reward;
}

// ------------------------------------------------------------------------------------------------
// host: a gemx_reward_config for rows of n_cols columns -- its checks, and the description built from it
// ------------------------------------------------------------------------------------------------
inline int reward_check(const gemx_reward_config *rc, int n_cols) {
    if (rc->struct_size != (int32_t)sizeof(gemx_reward_config)) return fail(GEMX_ERR_ARG, "gemx_reward_config size mismatch");
    if (rc->n_ref < 0 || rc->n_ref > GEMX_MAX_REF) return fail(GEMX_ERR_ARG, "n_ref must be in [0, %d]", GEMX_MAX_REF);
    for (int j = 0; j < rc->n_ref; ++j) {
        if (rc->ref_index[j] < 0 || rc->ref_index[j] >= n_cols) return fail(GEMX_ERR_ARG, "ref_index[%d] out of range", j);
        for (int k = 0; k < j; ++k)
            if (rc->ref_index[k] == rc->ref_index[j]) return fail(GEMX_ERR_ARG, "ref_index has duplicates");
    }
    for (int i = 0; i < n_cols; ++i)
        if (rc->weight[i] != 0.0 && !(rc->state_length[i] > 0)) return fail(GEMX_ERR_ARG, "state_length[%d] must be positive", i);
    return GEMX_OK;
}
template <class R> inline void reward_build(int n_cols, const gemx_reward_config *rc, RewardDev<R> &W) {
    memset(&W, 0, sizeof(W));
    int t = 0;
    bool referenced[GEMX_MAX_OUT] = {};
    auto add = [&](int col) {
        W.col[t] = col;
        const double pw = rc->power[col];
        W.kind[t] = pw == 1.0 ? 1 : (pw == 2.0 ? 2 : 3);
        W.coef[t] = (R)rc->weight[col];
        W.inv_len[t] = (R)(1.0 / rc->state_length[col]);
        W.power[t] = (R)pw;
        ++t;
    };
    for (int j = 0; j < rc->n_ref; ++j) { add(rc->ref_index[j]); referenced[rc->ref_index[j]] = true; }
    W.n_ref = rc->n_ref;
    for (int i = 0; i < n_cols; ++i)
        if (!referenced[i] && rc->weight[i] != 0.0) add(i);  // weighted but un-referenced states are compared with 0 (core.py:346)
    W.n_term = t;
    W.bias = (R)rc->bias;
    W.violation_reward = (R)rc->violation_reward;
}

// ------------------------------------------------------------------------------------------------
// device: one term, one row
// ------------------------------------------------------------------------------------------------
// GENERAL: reward_power other than 1 or 2 allowed (pow(): a ~300-instruction expansion, so it must not be unrolled per term)
template <bool GENERAL, class R> __device__ __forceinline__ R reward_term(R o, R ref, R inv_len, int kind, R power, R coef) {
    const R dlt = fabs(o - ref) * inv_len;
    R p = dlt * (kind == 2 ? dlt : R(1));  // (a select, not a branch: dlt * 1 == dlt exactly)
    if (GENERAL && kind == 3) p = pow(dlt, power);
    return coef * p;
}
// The reward of one row.  H: the hot terms BY VALUE (a RewardHot from the kernel arguments, or registers loaded from one); D: the full
// description for the slow path (in memory behind KArgs::rw, or a kernel argument by value); oh[t]: the row's value in column H.col[t],
// fetched by the caller (who may have many rows' fetches in flight at once); obs(col): the row's value in any column; rv: the row's
// references, 0 beyond n_ref.  The first GEMX_REWARD_HOT terms with the select for powers 1 and 2 (the unused ones carry weight 0:
// reward_hot_from), the remaining terms in order -- or, as soon as one power is neither 1 nor 2, EVERY term in order through the one
// pow() site --, each term rounded as a product before it is added (it is a function's return value: -ffp-contract=on forms no fused
// multiply-add across it), bias - sum, and violation_reward where the row is done.
template <class R, class Hot, class Obs>
__device__ __forceinline__ R reward_row(const Hot &H, const RewardDev<R> *D, const R (&oh)[GEMX_REWARD_HOT], Obs &&obs, const R (&rv)[GEMX_MAX_REF], bool done) {
    constexpr int HOT = GEMX_REWARD_HOT;
    R acc = R(0);
    if (!H.general) {
#pragma unroll
        for (int t = 0; t < HOT; ++t)  // terms < n_ref are the referenced states (reference column t), the others compare with 0
            acc += reward_term<false, R>(oh[t], t < GEMX_MAX_REF ? rv[t] : R(0), H.inv_len[t], H.kind[t], H.power[t], H.coef[t]);
    }
    // slow path through the description: terms beyond the hot ones, and EVERY term when some reward_power is not 1 or 2
#pragma nounroll
    for (int t = H.general ? 0 : HOT; t < H.n_term; ++t) {
        R ref = R(0);
#pragma unroll
        for (int j = 0; j < GEMX_MAX_REF; ++j) ref = (t == j) ? rv[j] : ref;
        acc += reward_term<true, R>(obs(D->col[t]), ref, D->inv_len[t], D->kind[t], D->power[t], D->coef[t]);
    }
    const R wse = H.bias - acc;
    return done ? H.violation_reward : wse;  // (1 - v) * wse + v * violation_reward, v in {0, 1}
}

}  // namespace gemx
