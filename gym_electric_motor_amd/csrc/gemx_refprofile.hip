// gemx_refprofile.hip -- device-side profile references (include/gemx.h: gemx_refprofile_*): given reference trajectories (drive cycles,
// recorded set-point profiles) shown per env from a table in device memory.  Per env the handle keeps, as SoA [field][N],
//     k (i32)  steps shown since the episode began      s (i32)  the episode's start row      e (u32)  episodes begun so far
// and a step is, per lane (profile_row below -- THE row function, which the step kernel and the rows kernel both call, so that K calls of
// gemx_refprofile_step and one gemx_refprofile_rollout_shell over K done rows agree bit for bit: episode_row's rule, gemx_episode.hip):
//     p = s + k * ratio in double from the integers (product and sum rounded separately: no contraction, the host restates it in numpy)
//     i = floor(p), w = p - i; the end rule gives the rows (ia, ib); value = w == 0 or zero-order hold ? tab[ia] : fma((R)w, b - a, a)
//     k += 1
// A restart (reset mask, done byte) sets k = 0, e += 1 and redraws s where the start row is random: one Philox block keyed by the global
// env index and e, nothing else -- no stream position to carry.
//
// Shape: N independent lanes, one per env; 12 bytes of state per env, no LDS, no atomics, no host state: every launch can be captured in a
// HIP graph and replayed.  Table reads: a SHARED table [T][n_ref] is read with a wave-uniform address where every lane of the wave stands on
// the same rows (start row zero and no done byte has desynchronised the wave: the usual case) -- the address then comes from
// readfirstlane, so the load can take the scalar path and one fetch serves 64 lanes -- and per lane otherwise (a gather inside a table
// that is small and cache-resident).  A PER-ENV table [T][N][n_ref] is read with the lane's own row: lanes on one row read adjacent
// addresses (coalesced), lanes on different rows gather.  Rows [N][n_ref] are written by adjacent lanes to adjacent addresses, as one
// vector store per lane where n_ref is 2 or 4 and the tensor is aligned to the row.  No lane leaves before the last wave vote: lanes
// behind N are predicated, not returned.
#include "gemx_support.hpp"

// ---- THE row function (declared in gemx_refprofile_lane.hpp).  This section alone is what a complete policy rollout unit compiles of this
// file: gemx_policy_complete.hip defines GEMX_REFPROFILE_ROW_ONLY and includes it, so that its kernel calls this definition, not a copy
namespace gemx {
namespace profile_lane {
// one step of one env: the n_ref values at the lane's position into row[], then k += 1.  `active`: the lane has an env (all 64 lanes of a
// wave come here together: the vote below needs them)
template <class R>
__device__ __forceinline__ void profile_row(const ProfileDev &P, const R *__restrict__ tab, int64_t env, bool active, ProfileLane &s, R (&row)[GEMX_MAX_REF]) {
    int32_t ia = 0, ib = 0;
    double w = 0.0;
    if (active) profile_rows_of(P, s, ia, ib, w);
    const bool lerp = P.interp != 0 && w != 0.0;
    const R wr = (R)w;
    bool uniform = false;
    int32_t ua = 0, ub = 0;
    if (!P.per_env) {
        ua = __builtin_amdgcn_readfirstlane(ia);
        ub = __builtin_amdgcn_readfirstlane(ib);
        uniform = __all((!active || (ia == ua && ib == ub)) ? 1 : 0) != 0;
    }
    if (active) {
#pragma unroll
        for (int g = 0; g < GEMX_MAX_REF; ++g) {
            if (g >= P.n_ref) break;
            R a, b;
            if (P.per_env) {
                a = tab[((int64_t)ia * P.N + env) * P.n_ref + g];
                b = lerp ? tab[((int64_t)ib * P.N + env) * P.n_ref + g] : a;
            } else if (uniform) {  // the wave's one row: a uniform address
                a = tab[(int64_t)ua * P.n_ref + g];
                b = tab[(int64_t)ub * P.n_ref + g];
            } else {
                a = tab[(int64_t)ia * P.n_ref + g];
                b = lerp ? tab[(int64_t)ib * P.n_ref + g] : a;
            }
            row[g] = lerp ? fma(wr, b - a, a) : a;
        }
        s.k += 1;
    }
}
}  // namespace profile_lane
}  // namespace gemx

#ifndef GEMX_REFPROFILE_ROW_ONLY
namespace {

// the uniform parameters, the 12 bytes of state and the restart of one env: gemx_refprofile_lane.hpp, through gemx_support.hpp (shared with the
// complete policy rollout units, which show the profile in the lane that steps the env)
using namespace gemx::profile_lane;

// row [n_ref] of env `at` (an index into rows of n_ref values): one vector store where the launch found the tensor aligned to the row
template <class R> __device__ __forceinline__ void profile_store(R *__restrict__ out, int64_t at, const R (&row)[GEMX_MAX_REF], int32_t n_ref, int vec) {
    if (vec == 2) {
        struct alignas(2 * sizeof(R)) V2 { R a, b; };
        reinterpret_cast<V2 *>(out)[at] = V2{row[0], row[1]};
    } else if (vec == 4) {
        struct alignas(sizeof(R) == 4 ? 16 : 32) V4 { R a, b, c, d; };
        reinterpret_cast<V4 *>(out)[at] = V4{row[0], row[1], row[2], row[3]};
    } else {
#pragma unroll
        for (int g = 0; g < GEMX_MAX_REF; ++g)
            if (g < n_ref) out[at * n_ref + g] = row[g];
    }
}

__global__ __launch_bounds__(256) void refprofile_reset_kernel(ProfileDev P, int32_t *__restrict__ st, const uint8_t *__restrict__ mask) {
    const int64_t env = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (env >= P.N) return;
    if (mask != nullptr && mask[env] == 0) return;
    ProfileLane s = profile_load(st, P.N, env);
    profile_restart(P, env, s);
    profile_save(st, P.N, env, s);
}

template <class R>
__global__ __launch_bounds__(256) void refprofile_step_kernel(ProfileDev P, const R *__restrict__ tab, int32_t *__restrict__ st, const uint8_t *__restrict__ done,
                                                              R *__restrict__ out, int vec) {
    const int64_t env = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = env < P.N;
    ProfileLane s = {0, 0, 0u};
    R row[GEMX_MAX_REF];
    if (active) {
        s = profile_load(st, P.N, env);
        if (done != nullptr && done[env] != 0) profile_restart(P, env, s);
    }
    profile_row<R>(P, tab, env, active, s, row);
    if (active) {
        profile_save(st, P.N, env, s);
        profile_store<R>(out, env, row, P.n_ref, vec);
    }
}

// K rows per lane; done_first: the restart of done[k][env] comes BEFORE row k (the env shell's order), else AFTER it
template <class R>
__global__ __launch_bounds__(256) void refprofile_rows_kernel(ProfileDev P, const R *__restrict__ tab, int32_t *__restrict__ st, const uint8_t *__restrict__ done,
                                                              int32_t K, int done_first, R *__restrict__ out, int vec) {
    const int64_t env = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = env < P.N;
    ProfileLane s = {0, 0, 0u};
    R row[GEMX_MAX_REF];
    if (active) s = profile_load(st, P.N, env);
    for (int32_t k = 0; k < K; ++k) {
        const int64_t at = (int64_t)k * P.N + env;
        const bool dn = active && done != nullptr && done[at] != 0;
        if (dn && done_first) profile_restart(P, env, s);
        profile_row<R>(P, tab, env, active, s, row);
        if (active) profile_store<R>(out, at, row, P.n_ref, vec);
        if (dn && !done_first) profile_restart(P, env, s);
    }
    if (active) profile_save(st, P.N, env, s);
}

struct ProfileBlobHeader {
    uint32_t magic;
    int32_t n_ref;
    int64_t n_envs;
    int32_t n_rows, per_env;
    int64_t env_base, bytes;
    int64_t pad[3];
};
static_assert(sizeof(ProfileBlobHeader) == GEMX_REFPROFILE_BLOB_HEADER_BYTES, "the blob header is 64 bytes");

}  // namespace

struct gemx_refprofile {
    gemx_refprofile_config cfg;
    ProfileDev dev;
    const void *table;  // borrowed
    int32_t *state;     // [3][N]: k, s, e
    int64_t n;
    int device, f64;
    unsigned blocks;
    ProfileBlobHeader blob_head;  // written by every get_blob, read by its asynchronous copy
};

namespace {

ProfileBlobHeader profile_blob_header(const gemx_refprofile *h) {
    ProfileBlobHeader b;
    memset(&b, 0, sizeof(b));
    b.magic = 0x46505847u;  // "GXPF"
    b.n_ref = h->cfg.n_ref; b.n_envs = h->n; b.n_rows = h->cfg.n_rows; b.per_env = h->cfg.per_env; b.env_base = h->cfg.env_base;
    b.bytes = (int64_t)sizeof(ProfileBlobHeader) + 12 * h->n;
    return b;
}

// one vector store per row where the rows are 2 or 4 wide and the tensor is aligned to them
int profile_vec(const gemx_refprofile *h, const void *out) {
    const int n_ref = h->cfg.n_ref;
    return ((n_ref == 2 || n_ref == 4) && (uintptr_t)out % (n_ref * (h->f64 ? 8u : 4u)) == 0) ? n_ref : 1;
}

int profile_rows(gemx_refprofile *h, const uint8_t *done_dev, int32_t K, int done_first, void *refs_out_dev, void *stream) {
    if (!h || !refs_out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (K < 1) return gemx::fail(GEMX_ERR_ARG, "K must be >= 1");
    if (!gemx::elem_aligned(h->f64 != 0, refs_out_dev)) return gemx::fail_unaligned();
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int vec = profile_vec(h, refs_out_dev);
    gemx_cov_note(h->f64 ? "refprofile_rows_kernel<double>" : "refprofile_rows_kernel<float>");
    if (h->f64)
        hipLaunchKernelGGL(refprofile_rows_kernel<double>, dim3(h->blocks), dim3(256), 0, st, h->dev, (const double *)h->table, h->state, done_dev, K, done_first,
                           (double *)refs_out_dev, vec);
    else
        hipLaunchKernelGGL(refprofile_rows_kernel<float>, dim3(h->blocks), dim3(256), 0, st, h->dev, (const float *)h->table, h->state, done_dev, K, done_first,
                           (float *)refs_out_dev, vec);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

}  // namespace

extern "C" {

int gemx_refprofile_create(const gemx_refprofile_config *cfg, const void *table_dev, int64_t n_envs, int device, int dtype, gemx_refprofile **out) {
    if (!cfg || !out || !table_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(gemx_refprofile_config)) return gemx::fail(GEMX_ERR_ARG, "gemx_refprofile_config size mismatch");
    if (cfg->n_ref < 1 || cfg->n_ref > GEMX_MAX_REF) return gemx::fail(GEMX_ERR_ARG, "n_ref must be in [1, %d]", GEMX_MAX_REF);
    if (cfg->n_rows < 1) return gemx::fail(GEMX_ERR_ARG, "n_rows must be >= 1");
    if (cfg->per_env != 0 && cfg->per_env != 1) return gemx::fail(GEMX_ERR_ARG, "per_env must be 0 or 1");
    if (cfg->interpolation != GEMX_PROFILE_INTERP_HOLD && cfg->interpolation != GEMX_PROFILE_INTERP_LINEAR) return gemx::fail(GEMX_ERR_ARG, "unknown interpolation");
    if (cfg->end != GEMX_PROFILE_END_HOLD && cfg->end != GEMX_PROFILE_END_WRAP) return gemx::fail(GEMX_ERR_ARG, "unknown end rule");
    if (cfg->start != GEMX_PROFILE_START_ZERO && cfg->start != GEMX_PROFILE_START_RANDOM) return gemx::fail(GEMX_ERR_ARG, "unknown start rule");
    if (!(cfg->tau > 0.0) || !(cfg->profile_tau > 0.0) || !std::isfinite(cfg->tau) || !std::isfinite(cfg->profile_tau))
        return gemx::fail(GEMX_ERR_ARG, "tau and profile_tau must be positive and finite");
    const double ratio = cfg->tau / cfg->profile_tau;
    if (!(ratio > 0.0) || !(ratio <= 1048576.0)) return gemx::fail(GEMX_ERR_ARG, "tau / profile_tau = %g must be in (0, 2^20]", ratio);
    if (n_envs < 1) return gemx::fail(GEMX_ERR_ARG, "n_envs must be >= 1");
    const int64_t blocks = (n_envs + 255) / 256;
    if (blocks > 0x7fffffffLL) return gemx::fail(GEMX_ERR_ARG, "n_envs = %lld exceeds %d blocks of 256 lanes", (long long)n_envs, 0x7fffffff);
    if (int rc = gemx::check_device_dtype(device, dtype)) return rc;
    if (!gemx::elem_aligned(dtype == GEMX_F64, table_dev)) return gemx::fail_unaligned();
    gemx_refprofile *h = new (std::nothrow) gemx_refprofile();
    if (!h) return gemx::fail(GEMX_ERR_ALLOC, "out of host memory");
    h->cfg = *cfg; h->table = table_dev; h->n = n_envs; h->device = device; h->f64 = dtype == GEMX_F64; h->blocks = (unsigned)blocks; h->state = nullptr;
    ProfileDev &P = h->dev;
    memset(&P, 0, sizeof(P));
    P.n_ref = cfg->n_ref; P.T = cfg->n_rows; P.per_env = cfg->per_env; P.interp = cfg->interpolation == GEMX_PROFILE_INTERP_LINEAR;
    P.wrap = cfg->end == GEMX_PROFILE_END_WRAP; P.random = cfg->start == GEMX_PROFILE_START_RANDOM;
    P.seed = cfg->seed; P.env_base = cfg->env_base; P.N = n_envs; P.ratio = ratio;
    gemx::DeviceGuard guard(device);
    const size_t bytes = (size_t)n_envs * 12;
    if (hipMalloc((void **)&h->state, bytes) != hipSuccess) { delete h; return gemx::fail(GEMX_ERR_ALLOC, "hipMalloc(profile state) failed"); }
    if (hipMemset(h->state, 0, bytes) != hipSuccess) { (void)hipFree(h->state); delete h; return gemx::fail(GEMX_ERR_DEVICE, "hipMemset(profile state) failed"); }
    *out = h;
    return GEMX_OK;
}

int gemx_refprofile_destroy(gemx_refprofile *h) {
    if (!h) return GEMX_OK;
    if (h->state) {
        gemx::DeviceGuard guard(h->device);
        (void)hipFree(h->state);
    }
    delete h;
    return GEMX_OK;
}

int gemx_refprofile_reset(gemx_refprofile *h, const uint8_t *mask_dev, void *stream) {
    if (!h) return gemx::fail(GEMX_ERR_ARG, "null handle");
    gemx::DeviceGuard guard(h->device);
    gemx_cov_note("refprofile_reset_kernel");
    hipLaunchKernelGGL(refprofile_reset_kernel, dim3(h->blocks), dim3(256), 0, (hipStream_t)stream, h->dev, h->state, mask_dev);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

int gemx_refprofile_step(gemx_refprofile *h, const uint8_t *done_dev, void *refs_dev, void *stream) {
    if (!h || !refs_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (!gemx::elem_aligned(h->f64 != 0, refs_dev)) return gemx::fail_unaligned();
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int vec = profile_vec(h, refs_dev);
    gemx_cov_note(h->f64 ? "refprofile_step_kernel<double>" : "refprofile_step_kernel<float>");
    if (h->f64)
        hipLaunchKernelGGL(refprofile_step_kernel<double>, dim3(h->blocks), dim3(256), 0, st, h->dev, (const double *)h->table, h->state, done_dev, (double *)refs_dev, vec);
    else
        hipLaunchKernelGGL(refprofile_step_kernel<float>, dim3(h->blocks), dim3(256), 0, st, h->dev, (const float *)h->table, h->state, done_dev, (float *)refs_dev, vec);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

int gemx_refprofile_rollout(gemx_refprofile *h, const uint8_t *done_dev, int32_t K, void *refs_out_dev, void *stream) {
    return profile_rows(h, done_dev, K, 0, refs_out_dev, stream);
}

int gemx_refprofile_rollout_shell(gemx_refprofile *h, const uint8_t *done_dev, int32_t K, void *refs_out_dev, void *stream) {
    return profile_rows(h, done_dev, K, 1, refs_out_dev, stream);
}

int gemx_refprofile_get_state(gemx_refprofile *h, int32_t *k_s_e_out_dev, void *stream) {
    if (!h || !k_s_e_out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(h->device);
    GEMX_HIP_TRY(hipMemcpyAsync(k_s_e_out_dev, h->state, (size_t)h->n * 12, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return GEMX_OK;
}

int64_t gemx_refprofile_state_bytes(gemx_refprofile *h) { return h ? (int64_t)sizeof(ProfileBlobHeader) + 12 * h->n : 0; }

int gemx_refprofile_get_blob(gemx_refprofile *h, void *out_dev, void *stream) {
    if (!h || !out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    h->blob_head = profile_blob_header(h);  // (the same words on every call: a copy still in flight reads what this writes)
    GEMX_HIP_TRY(hipMemcpyAsync(out_dev, &h->blob_head, sizeof(ProfileBlobHeader), hipMemcpyHostToDevice, st));
    GEMX_HIP_TRY(hipMemcpyAsync((char *)out_dev + sizeof(ProfileBlobHeader), h->state, (size_t)h->n * 12, hipMemcpyDeviceToDevice, st));
    return GEMX_OK;
}

int gemx_refprofile_set_blob(gemx_refprofile *h, const void *in_dev, void *stream) {
    if (!h || !in_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    // the header alone comes to the host first (synchronises `stream`); nothing is enqueued before it has been checked
    ProfileBlobHeader got;
    GEMX_HIP_TRY(hipMemcpyAsync(&got, in_dev, sizeof(got), hipMemcpyDeviceToHost, st));
    GEMX_HIP_TRY(hipStreamSynchronize(st));
    const ProfileBlobHeader want = profile_blob_header(h);
    if (got.magic != want.magic) return gemx::fail(GEMX_ERR_ARG, "not a profile reference blob (magic %08x)", got.magic);
    if (got.n_envs != want.n_envs) return gemx::fail(GEMX_ERR_ARG, "the profile reference blob is for n_envs = %lld, this handle has %lld", (long long)got.n_envs, (long long)want.n_envs);
    if (got.n_ref != want.n_ref) return gemx::fail(GEMX_ERR_ARG, "the profile reference blob has %d reference columns, this handle has %d", got.n_ref, want.n_ref);
    if (got.n_rows != want.n_rows) return gemx::fail(GEMX_ERR_ARG, "the profile reference blob is for profiles of T = %d rows, this handle's have %d", got.n_rows, want.n_rows);
    if (got.per_env != want.per_env) return gemx::fail(GEMX_ERR_ARG, "the profile reference blob is for a %s table, this handle has a %s one", got.per_env ? "per-env" : "shared", want.per_env ? "per-env" : "shared");
    if (got.env_base != want.env_base)
        return gemx::fail(GEMX_ERR_ARG, "the profile reference blob belongs to the shard at env_base = %lld, this handle's is %lld", (long long)got.env_base, (long long)want.env_base);
    if (got.bytes != want.bytes) return gemx::fail(GEMX_ERR_ARG, "the profile reference blob has %lld bytes, this handle's has %lld", (long long)got.bytes, (long long)want.bytes);
    GEMX_HIP_TRY(hipMemcpyAsync(h->state, (const char *)in_dev + sizeof(ProfileBlobHeader), (size_t)h->n * 12, hipMemcpyDeviceToDevice, st));
    return GEMX_OK;
}

}  // extern "C"

// ---- the complete policy rollout (gemx_refprofile_lane.hpp declares it): the kernel's view of a profile handle
namespace gemx {
int refprofile_policy_view(gemx_refprofile *p, const char *what, int64_t n_envs, int device, int64_t env_base, PcProfileDev *out) {
    if (p->n != n_envs) return fail(GEMX_ERR_ARG, "%s: the gemx_refprofile serves n_envs = %lld, the handle %lld", what, (long long)p->n, (long long)n_envs);
    if (p->f64) return fail(GEMX_ERR_ARG, "%s: the gemx_refprofile is fp64, the handle fp32", what);
    if (p->device != device) return fail(GEMX_ERR_ARG, "%s: the gemx_refprofile lives on device %d, the handle on device %d", what, p->device, device);
    if (p->cfg.env_base != env_base) return fail(GEMX_ERR_ARG, "%s: the gemx_refprofile's env_base is %lld, the handle's %lld", what, (long long)p->cfg.env_base, (long long)env_base);
    *out = {p->dev, (const float *)p->table, p->state};
    return GEMX_OK;
}
}  // namespace gemx
#endif  // GEMX_REFPROFILE_ROW_ONLY
