// gemx_policy.hip -- ONE policy rollout unit: K control steps per launch with the episode time limit AND the actor inside the launch
// (gemx_rollout_policy), for one (system, converter unit), fp32, built as its own shared object
//   hipcc -DGEMX_INST_SYS=<0..7> -DGEMX_INST_CONV=<0..11> -shared gemx_policy.hip -o libgemx_pl<S>_<C>.so
// and loaded with dlopen by the first gemx_rollout_policy of such a handle (gemx_capi.hip: load_pl_unit).  The stepping units, the per-env
// units and the episodic units (gemx_episodic.hip) are untouched.
//
// The kernel and its launcher are gemx_policy_kernel.hpp's, shared with the complete policy units (gemx_policy_complete.hip); this unit
// instantiates policy_rollout_kernel without a generator (GEN = PC_GEN_NONE): the references the actor reads are row k of the call's
// tensor.  The actor's design and what it costs are described there.
#include "gemx_policy_kernel.hpp"

#if !defined(GEMX_INST_SYS) || !defined(GEMX_INST_CONV)
#error "define GEMX_INST_SYS and GEMX_INST_CONV"
#endif

namespace gemx {
// the unit's tanhf over n values: the tests' epsilon_tanh is measured on what the actor calls
__global__ void pl_tanh_kernel(const float *__restrict__ x, float *__restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = tanhf(x[i]);
}

struct PlGen {  // launch_policy_t's V: no generator
    static constexpr const char *WHAT = "policy rollout";
    static constexpr int PIPE = EP_LAUNCH_POLICY;
    int kind() const { return 0; }
    template <int SYS, int CONV, int LOAD, int SOLVER, bool TAB> void launch(const PolicyLaunch &l) const {
        launch_policy_kernel<SYS, CONV, LOAD, SOLVER, TAB, PC_GEN_NONE>(l);
    }
};
}  // namespace gemx

extern "C" {
__attribute__((visibility("default"))) int gemx_pl_unit_init(unsigned long long handle_bytes, int abi, void (*set_error)(const char *)) {
    return gemx::unit_init(handle_bytes, abi, set_error);
}
__attribute__((visibility("default"))) int gemx_pl_unit_launch(gemx_handle *h, const gemx::PolicyDev *pol, int K, const int32_t *length, int32_t max_steps, void *obs,
                                                               uint8_t *terminated, uint8_t *truncated, uint8_t *ended, hipStream_t st, int *linmap_built) {
    if (h->envp != nullptr && h->envp_fields != gemx::ep_fields(GEMX_INST_SYS)) return gemx::fail(GEMX_ERR_ARG, "internal: policy rollout unit launched with another system's table");
    const gemx::PolicyCall c = {pol, K, length, max_steps, obs, terminated, truncated, ended, linmap_built};
    return gemx::launch_policy_unit<GEMX_INST_SYS, GEMX_INST_CONV>(h, c, gemx::PlGen{}, st);
}
__attribute__((visibility("default"))) int gemx_pl_unit_tanh(const float *x, float *y, long long n, hipStream_t st) {
    if (n <= 0) return GEMX_OK;
    hipLaunchKernelGGL(gemx::pl_tanh_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, n);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}
}
