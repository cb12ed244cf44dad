// gemx_fluxobs.hip -- device-side FluxObserver and flux-oriented dq actions (include/gemx.h: gemx_fluxobs_*): the reference's
//   FluxObserver              physical_system_wrappers/flux_observer.py:80-102              state || psi_abs, psi_angle
//   DqToAbcActionProcessor    physical_system_wrappers/dq_to_abc_action_processor.py:57-148 'SCIM' and 'DFIM': Park angle from psi_angle
// as a stage of its own behind the stepping kernels.  Per env the handle keeps the rotor-flux estimate Psi (re, im) -- ALWAYS fp64: the
// explicit Euler recursion  Psi += tau [(i_alpha + j i_beta) r_r l_m / l_r - Psi (r_r / l_r - j omega p)]  runs for the whole episode, and
// its accumulator is 16 bytes beside a row of 56 bytes or more -- and the frame(s) the next action will be rotated by.  The two new
// columns and the frames are evaluated from Psi in the row's own precision R.
//
// One kernel template serves gemx_fluxobs_step (one row per lane, ring depth 1) and gemx_fluxobs_rows (a lane walks its K rows in
// order, ring depth FLUX_DEPTH); the arithmetic of a row is ONE __device__ function, flux_row, so K steps and one K-row pass agree bit
// for bit.  A workgroup is ONE wave of 64 lanes = 64 envs (16384 envs: one wave per CU), and step k's tile -- rows [64][n_in] of
// state[k], contiguous -- goes through LDS the way gemx_obsproc.hip moves its tiles:
//   1. the wave loads the tile in 16-byte units, consecutive lanes consecutive units, into REGISTERS (a ring of FLUX_DEPTH tiles is in
//      flight ahead of the recursion: the row loads do not depend on Psi, and a dependent HBM round trip per row is what the pass would
//      cost otherwise), and scatters the oldest ring slot into the LDS tile -- laid out as the OUTPUT rows, n_in + 2 columns at an odd
//      dword stride, so the copied columns are placed once and never touched again;
//   2. lane r reads the four or five operands of row r, advances Psi, writes the two new columns of row r;
//   3. the wave gathers the tile back into 16-byte units and stores them.
// A tile starts at dword (k N + 64 b) L of its tensor, which is 16-byte aligned for some k and not for others (N L need not be a
// multiple of four dwords) and for no k at all in a view at an odd element offset: EVERY tile is moved as up to three single dwords
// up to the first 16-byte boundary, whole 16-byte units, and up to three single dwords behind the last one.  Nothing outside the tile
// is read or written; a lane with no unit of its own loads from the handle's own state array instead of branching around the load.
#include "gemx_support.hpp"

namespace {

using namespace gemx;  // the row tile: gemx_support.hpp

constexpr int FLUX_LANES = 64;  // one wave per workgroup
constexpr int FLUX_DEPTH = 4;   // tiles in flight ahead of the recursion in gemx_fluxobs_rows

struct FluxParams {
    int32_t n_in, omega, cur[3], eps, mode, auto_reset;
    uint32_t magic_in, magic_out;  // tile_magic of the row lengths in dwords
    double lim_omega, lim_cur[3], lim_eps, psi_limit;
    double p, tau, k_i, k_psi, adv_tau_p;  // adv_tau_p = (0.5 + dead time) tau p
    double reset_f0, reset_f1;             // the frames right after a reset
};

static_assert(tile_fits(FLUX_LANES, 2 * (GEMX_MAX_OUT + 2)), "the longest output row (fp64) is within tile_row's exactness bound");

__device__ inline float flux_hypot(float a, float b) { return hypotf(a, b); }
__device__ inline double flux_hypot(double a, double b) { return hypot(a, b); }
__device__ inline float flux_atan2(float a, float b) { return atan2f(a, b); }
__device__ inline double flux_atan2(double a, double b) { return atan2(a, b); }
__device__ inline void flux_sincos(float x, float *s, float *c) { sincosf(x, s, c); }
__device__ inline void flux_sincos(double x, double *s, double *c) { sincos(x, s, c); }

template <class R> struct FluxLane {
    double re, im;  // Psi
    R f0, f1;       // SCIM: f0 = action frame; DFIM: f0 = stator frame, f1 = rotor frame
};

// ONE control step of one env: the normalised operands of its row -> the two new columns; Psi and the frames advance.
// (flux_observer.py:87-102; dq_to_abc_action_processor.py:86-88, 135-139.)  The reset of a terminated lane comes LAST: the terminating
// step still shows the updated flux, as the reference's does before its reset().
template <class R>
__device__ inline void flux_row(const FluxParams &P, FluxLane<R> &s, R w, R ia, R ib, R ic, R eps, bool done, R &psi_abs, R &psi_angle) {
    const double a = (double)ia * P.lim_cur[0], b = (double)ib * P.lim_cur[1], c = (double)ic * P.lim_cur[2];
    const double t0 = 2.0 / 3.0, t1 = 2.0 / 3.0 * -0.5, t2 = 2.0 / 3.0 * (0.5 * 1.7320508075688772);
    const double i_al = t0 * a + t1 * b + t1 * c, i_be = t2 * b - t2 * c;
    const double w_el = (double)w * P.lim_omega * P.p;
    const double d_re = i_al * P.k_i - (s.re * P.k_psi + s.im * w_el);
    const double d_im = i_be * P.k_i - (s.im * P.k_psi - s.re * w_el);
    s.re += d_re * P.tau;
    s.im += d_im * P.tau;
    const R re = (R)s.re, im = (R)s.im;
    const R ang = flux_atan2(im, re);
    psi_abs = flux_hypot(re, im) / (R)P.psi_limit;
    psi_angle = ang / (R)3.14159265358979323846;
    const R adv = (R)P.adv_tau_p * (w * (R)P.lim_omega);
    if (P.mode == GEMX_FLUX_ACT_DFIM) {
        s.f0 = eps * (R)P.lim_eps + adv;
        s.f1 = ang - s.f0;
    } else {
        s.f0 = ang + adv;
        s.f1 = R(0);
    }
    if (done && P.auto_reset) {
        s.re = 0.0; s.im = 0.0;
        s.f0 = (R)P.reset_f0; s.f1 = (R)P.reset_f1;
    }
}

// how a tile of cnt dwords at g splits into head dwords, 16-byte units and tail dwords
struct FluxSplit { uint32_t head, nvec, tail; };
__device__ inline FluxSplit flux_split(const uint32_t *g, uint32_t cnt) {
    FluxSplit s;
    s.head = (4u - ((uint32_t)((uintptr_t)g >> 2) & 3u)) & 3u;
    if (s.head > cnt) s.head = cnt;
    s.nvec = (cnt - s.head) >> 2;
    s.tail = (cnt - s.head) & 3u;
    return s;
}

template <int NV> struct FluxTile {
    uint4 v[NV];    // this lane's 16-byte units: unit threadIdx.x + 64 i
    uint32_t e;     // this lane's head or tail dword, if it has one
    uint32_t done;  // this lane's done byte
};

// issue the loads of one tile (no branch around a load: a lane without a unit reads the 16-byte aligned `safe`)
template <int NV>
__device__ inline void flux_tile_load(FluxTile<NV> &t, const uint32_t *g, uint32_t cnt, const uint8_t *done, uint32_t lanes_t, const uint32_t *safe) {
    const FluxSplit s = flux_split(g, cnt);
    const uint4 *gv = reinterpret_cast<const uint4 *>(g + s.head);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const uint32_t v = threadIdx.x + (uint32_t)i * FLUX_LANES;
        const uint4 *p = v < s.nvec ? gv + v : reinterpret_cast<const uint4 *>(safe);
        t.v[i] = *p;
    }
    const uint32_t l = threadIdx.x;
    const uint32_t idx = l < s.head ? l : s.head + s.nvec * 4u + (l - s.head);
    const uint32_t *pe = l < s.head + s.tail ? g + idx : safe;
    t.e = *pe;
    const uint8_t *pd = (done && l < lanes_t) ? done + l : reinterpret_cast<const uint8_t *>(safe);
    t.done = done ? (uint32_t)*pd : 0u;
}

// registers -> LDS tile with rows of L dwords at `stride`.  (This loop and flux_tile_store's are the unit loops of gemx_support.hpp's
// stagers once more: calling shared unit helpers here, gemx_fluxobs_rows measured 1 - 2 % slower, profiles/support_units_refactor.md.)
template <int NV>
__device__ inline void flux_tile_scatter(const FluxTile<NV> &t, uint32_t *tile, uint32_t stride, uint32_t L, uint32_t magic, const uint32_t *g, uint32_t cnt) {
    const FluxSplit s = flux_split(g, cnt);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const uint32_t v = threadIdx.x + (uint32_t)i * FLUX_LANES;
        if (v < s.nvec) {
            const uint32_t w[4] = {t.v[i].x, t.v[i].y, t.v[i].z, t.v[i].w};
            const uint32_t d = s.head + v * 4u, row = tile_row(d, magic);
            uint32_t col = d - row * L, a = row * stride + col;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                tile[a] = w[j];
                ++col; ++a;
                if (col == L) { col = 0; a += stride - L; }
            }
        }
    }
    const uint32_t l = threadIdx.x;
    if (l < s.head + s.tail) {
        const uint32_t d = l < s.head ? l : s.head + s.nvec * 4u + (l - s.head), row = tile_row(d, magic);
        tile[row * stride + (d - row * L)] = t.e;
    }
}

// LDS tile -> global (cnt dwords at g)
__device__ inline void flux_tile_store(const uint32_t *tile, uint32_t stride, uint32_t L, uint32_t magic, uint32_t *g, uint32_t cnt) {
    const FluxSplit s = flux_split(g, cnt);
    uint4 *gv = reinterpret_cast<uint4 *>(g + s.head);
    for (uint32_t v = threadIdx.x; v < s.nvec; v += FLUX_LANES) {
        const uint32_t d = s.head + v * 4u, row = tile_row(d, magic);
        uint32_t col = d - row * L, a = row * stride + col;
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[j] = tile[a];
            ++col; ++a;
            if (col == L) { col = 0; a += stride - L; }
        }
        gv[v] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    const uint32_t l = threadIdx.x;
    if (l < s.head + s.tail) {
        const uint32_t d = l < s.head ? l : s.head + s.nvec * 4u + (l - s.head), row = tile_row(d, magic);
        g[d] = tile[row * stride + (d - row * L)];
    }
}

// lane state: hs = double [4][N]: Psi re, Psi im, frame 0, frame 1
template <class R, int NV, int D>
__global__ __launch_bounds__(FLUX_LANES) void flux_rows_kernel(const R *__restrict__ state, const uint8_t *__restrict__ done, R *__restrict__ out, double *__restrict__ hs,
                                                               int64_t N, int32_t K, FluxParams P) {
    constexpr uint32_t DW = (uint32_t)sizeof(R) / 4u;
    extern __shared__ __attribute__((aligned(16))) uint32_t flux_smem[];
    const uint32_t Li = (uint32_t)P.n_in * DW, Lo = Li + 2u * DW, SO = Lo | 1u;  // odd row stride: lanes read / write distinct banks
    const int64_t lane0 = (int64_t)blockIdx.x * FLUX_LANES;
    const uint32_t lanes_t = (uint32_t)(N - lane0 < (int64_t)FLUX_LANES ? N - lane0 : (int64_t)FLUX_LANES);
    const uint32_t cnt_in = lanes_t * Li, cnt_out = lanes_t * Lo;
    const bool mine = threadIdx.x < lanes_t;
    const int64_t env = lane0 + (mine ? threadIdx.x : 0u);
    const uint32_t *safe = reinterpret_cast<const uint32_t *>(hs);  // 16-byte aligned, at least 32 bytes
    const uint32_t *gin = reinterpret_cast<const uint32_t *>(state) + lane0 * Li;  // + k * N * Li
    uint32_t *gout = reinterpret_cast<uint32_t *>(out) + lane0 * Lo;
    const int64_t pitch_in = N * (int64_t)Li, pitch_out = N * (int64_t)Lo;
    const uint8_t *gdone = done ? done + lane0 : nullptr;

    FluxLane<R> s;
    s.re = hs[env]; s.im = hs[N + env]; s.f0 = (R)hs[2 * N + env]; s.f1 = (R)hs[3 * N + env];

    FluxTile<NV> ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const int32_t k = d < K ? d : K - 1;  // (a ring deeper than the trajectory re-reads its last tile: in bounds, never used)
        flux_tile_load<NV>(ring[d], gin + k * pitch_in, cnt_in, gdone ? gdone + (int64_t)k * N : nullptr, lanes_t, safe);
    }
    for (int32_t k0 = 0; k0 < K; k0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int32_t k = k0 + d;
            if (k >= K) break;  // (uniform)
            flux_tile_scatter<NV>(ring[d], flux_smem, SO, Li, P.magic_in, gin + k * pitch_in, cnt_in);
            const uint32_t dn = ring[d].done;
            if (D > 1) {  // refill the slot: the tile D steps ahead (clamped like the prologue)
                const int32_t kn = k + D < K ? k + D : K - 1;
                flux_tile_load<NV>(ring[d], gin + kn * pitch_in, cnt_in, gdone ? gdone + (int64_t)kn * N : nullptr, lanes_t, safe);
            }
            __syncthreads();
            if (mine) {
                uint32_t *row = flux_smem + threadIdx.x * SO;
                const R w = tile_get(row + (uint32_t)P.omega * DW, R(0));
                const R ia = tile_get(row + (uint32_t)P.cur[0] * DW, R(0)), ib = tile_get(row + (uint32_t)P.cur[1] * DW, R(0)), ic = tile_get(row + (uint32_t)P.cur[2] * DW, R(0));
                const R eps = P.eps >= 0 ? tile_get(row + (uint32_t)P.eps * DW, R(0)) : R(0);
                R pa, pg;
                flux_row<R>(P, s, w, ia, ib, ic, eps, dn != 0u, pa, pg);
                tile_put(row + Li, pa);
                tile_put(row + Li + DW, pg);
            }
            __syncthreads();
            flux_tile_store(flux_smem, SO, Lo, P.magic_out, gout + k * pitch_out, cnt_out);
            __syncthreads();  // (the next scatter overwrites the tile)
        }
    }
    if (mine) {
        hs[env] = s.re; hs[N + env] = s.im; hs[2 * N + env] = (double)s.f0; hs[3 * N + env] = (double)s.f1;
    }
}

__global__ void flux_reset_kernel(double *__restrict__ hs, const uint8_t *__restrict__ mask, int64_t N, double f0, double f1) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || (mask && !mask[i])) return;
    hs[i] = 0.0; hs[N + i] = 0.0; hs[2 * N + i] = f0; hs[3 * N + i] = f1;
}

// abc = t_32(q(dq, frame)) per env (three_phase_motor.py:24-28, 58-71); DFIM: the rotor pair by the rotor frame.  No clipping here: the
// inner converter clips, as in the reference.
template <class R>
__global__ void flux_actions_kernel(const double *__restrict__ hs, const R *__restrict__ dq, R *__restrict__ abc, int64_t N, int32_t pairs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    for (int32_t j = 0; j < pairs; ++j) {
        const R f = (R)hs[(2 + j) * N + i];
        R sn, cs;
        flux_sincos(f, &sn, &cs);
        const R d = dq[i * (2 * pairs) + 2 * j], q = dq[i * (2 * pairs) + 2 * j + 1];
        const R al = cs * d - sn * q, be = sn * d + cs * q;
        const R h = (R)(0.5 * 1.7320508075688772);
        R *o = abc + i * (3 * pairs) + 3 * j;
        o[0] = al;
        o[1] = R(-0.5) * al + h * be;
        o[2] = R(-0.5) * al - h * be;
    }
}

}  // namespace

struct gemx_fluxobs {
    gemx_fluxobs_config cfg;
    FluxParams prm;
    int64_t n;
    int device, f64;
    double *hs;  // [4][N]
};

template <class R, int NV>
static int flux_launch_nv(gemx_fluxobs *h, const void *state, const uint8_t *done, int32_t K, void *out, hipStream_t st, bool rows) {
    constexpr uint32_t DW = (uint32_t)sizeof(R) / 4u;
    const int64_t blocks = (h->n + FLUX_LANES - 1) / FLUX_LANES;
    const size_t lds = (size_t)FLUX_LANES * ((((size_t)h->prm.n_in + 2u) * DW) | 1u) * 4u;
    if (rows) {
        gemx_cov_note(sizeof(R) == 4 ? "flux_rows_kernel<float,rows>" : "flux_rows_kernel<double,rows>");
        hipLaunchKernelGGL((flux_rows_kernel<R, NV, FLUX_DEPTH>), dim3((unsigned)blocks), dim3(FLUX_LANES), lds, st, (const R *)state, done, (R *)out, h->hs, h->n, K, h->prm);
    } else {
        gemx_cov_note(sizeof(R) == 4 ? "flux_rows_kernel<float,step>" : "flux_rows_kernel<double,step>");
        hipLaunchKernelGGL((flux_rows_kernel<R, NV, 1>), dim3((unsigned)blocks), dim3(FLUX_LANES), lds, st, (const R *)state, done, (R *)out, h->hs, h->n, K, h->prm);
    }
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

template <class R>
static int flux_launch(gemx_fluxobs *h, const void *state, const uint8_t *done, int32_t K, void *out, hipStream_t st, bool rows) {
    const uint32_t nv = ((uint32_t)h->prm.n_in * ((uint32_t)sizeof(R) / 4u) + 3u) / 4u;  // 16-byte units per lane and tile
    if (nv <= 4) return flux_launch_nv<R, 4>(h, state, done, K, out, st, rows);
    if (nv <= 7) return flux_launch_nv<R, 7>(h, state, done, K, out, st, rows);
    return flux_launch_nv<R, 12>(h, state, done, K, out, st, rows);
}

static int flux_run(gemx_fluxobs *h, const void *state, const uint8_t *done, int32_t K, void *out, void *stream, bool rows) {
    if (!h || !state || !out) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (K < 1) return gemx::fail(GEMX_ERR_ARG, "K must be >= 1");
    if (!gemx::elem_aligned(h->f64, state, out)) return gemx::fail_unaligned();
    gemx::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    return h->f64 ? flux_launch<double>(h, state, done, K, out, st, rows) : flux_launch<float>(h, state, done, K, out, st, rows);
}

extern "C" {

int gemx_fluxobs_create(const gemx_fluxobs_config *cfg, int64_t n_envs, int dtype, int device, gemx_fluxobs **out) {
    if (!cfg || !out) return gemx::fail(GEMX_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(gemx_fluxobs_config)) return gemx::fail(GEMX_ERR_ARG, "gemx_fluxobs_config size mismatch");
    if (cfg->n_in < 4 || cfg->n_in > GEMX_MAX_OUT) return gemx::fail(GEMX_ERR_ARG, "n_in must be in [4, %d]", GEMX_MAX_OUT);
    if (n_envs < 1 || (n_envs + FLUX_LANES - 1) / FLUX_LANES > 0x7fffffffLL) return gemx::fail(GEMX_ERR_ARG, "n_envs = %lld out of range", (long long)n_envs);
    if (cfg->action_mode < GEMX_FLUX_ACT_NONE || cfg->action_mode > GEMX_FLUX_ACT_DFIM) return gemx::fail(GEMX_ERR_ARG, "unknown action_mode %d", cfg->action_mode);
    if (cfg->auto_reset != 0 && cfg->auto_reset != 1) return gemx::fail(GEMX_ERR_ARG, "auto_reset must be 0 or 1");
    const int32_t idx[4] = {cfg->omega_index, cfg->current_index[0], cfg->current_index[1], cfg->current_index[2]};
    for (int i = 0; i < 4; ++i)
        if (idx[i] < 0 || idx[i] >= cfg->n_in) return gemx::fail(GEMX_ERR_ARG, "column index %d outside [0, %d)", idx[i], cfg->n_in);
    if (cfg->action_mode == GEMX_FLUX_ACT_DFIM && (cfg->epsilon_index < 0 || cfg->epsilon_index >= cfg->n_in))
        return gemx::fail(GEMX_ERR_ARG, "the DFIM action mode needs epsilon_index in [0, %d)", cfg->n_in);
    if (!(cfg->psi_limit > 0.0) || !(cfg->tau > 0.0)) return gemx::fail(GEMX_ERR_ARG, "psi_limit and tau must be positive");
    if (int rc = gemx::check_device_dtype(device, dtype)) return rc;
    gemx_fluxobs *h = new (std::nothrow) gemx_fluxobs();
    if (!h) return gemx::fail(GEMX_ERR_ALLOC, "out of host memory");
    h->cfg = *cfg; h->n = n_envs; h->device = device; h->f64 = dtype == GEMX_F64; h->hs = nullptr;
    FluxParams &P = h->prm;
    memset(&P, 0, sizeof(P));
    const uint32_t dw = h->f64 ? 2u : 1u;
    P.n_in = cfg->n_in; P.omega = cfg->omega_index; P.mode = cfg->action_mode; P.auto_reset = cfg->auto_reset;
    P.eps = cfg->action_mode == GEMX_FLUX_ACT_DFIM ? cfg->epsilon_index : -1;
    for (int i = 0; i < 3; ++i) { P.cur[i] = cfg->current_index[i]; P.lim_cur[i] = cfg->current_limit[i]; }
    P.magic_in = tile_magic((uint32_t)P.n_in * dw); P.magic_out = tile_magic(((uint32_t)P.n_in + 2u) * dw);
    P.lim_omega = cfg->omega_limit; P.lim_eps = cfg->epsilon_limit; P.psi_limit = cfg->psi_limit;
    P.p = cfg->p; P.tau = cfg->tau; P.k_i = cfg->k_current; P.k_psi = cfg->k_flux;
    P.adv_tau_p = cfg->angle_advance * cfg->tau * cfg->p;
    // the frames after a reset: psi_angle = 0 and the reset observation's omega (and epsilon), as the reference's processor reads them
    const double adv = cfg->angle_advance * cfg->tau * (cfg->reset_omega * cfg->omega_limit) * cfg->p;
    if (cfg->action_mode == GEMX_FLUX_ACT_DFIM) {
        P.reset_f0 = cfg->reset_epsilon * cfg->epsilon_limit + adv;
        P.reset_f1 = 0.0 - P.reset_f0;
    } else {
        P.reset_f0 = adv;
        P.reset_f1 = 0.0;
    }
    gemx::DeviceGuard guard(device);
    const size_t bytes = (size_t)(n_envs < 4 ? 4 : n_envs) * 4u * sizeof(double);
    if (hipMalloc((void **)&h->hs, bytes) != hipSuccess) {
        delete h;
        return gemx::fail(GEMX_ERR_ALLOC, "out of device memory (%zu bytes of observer state)", bytes);
    }
    *out = h;
    const int rc = gemx_fluxobs_reset(h, nullptr, nullptr);
    if (rc != GEMX_OK || hipStreamSynchronize(nullptr) != hipSuccess) {
        *out = nullptr;
        (void)hipFree(h->hs);
        delete h;
        return rc != GEMX_OK ? rc : gemx::fail(GEMX_ERR_DEVICE, "the first reset of the observer state failed");
    }
    return GEMX_OK;
}

int gemx_fluxobs_destroy(gemx_fluxobs *h) {
    if (h) {
        gemx::DeviceGuard guard(h->device);
        (void)hipFree(h->hs);
        delete h;
    }
    return GEMX_OK;
}

int gemx_fluxobs_reset(gemx_fluxobs *h, const uint8_t *mask_dev, void *stream) {
    if (!h) return gemx::fail(GEMX_ERR_ARG, "null handle");
    gemx::DeviceGuard guard(h->device);
    gemx_cov_note("flux_reset_kernel");
    const int64_t blocks = (h->n + 255) / 256;
    hipLaunchKernelGGL(flux_reset_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, h->hs, mask_dev, h->n,
                       h->f64 ? h->prm.reset_f0 : (double)(float)h->prm.reset_f0, h->f64 ? h->prm.reset_f1 : (double)(float)h->prm.reset_f1);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

int gemx_fluxobs_step(gemx_fluxobs *h, const void *state_dev, const uint8_t *done_dev, void *ext_out_dev, void *stream) {
    return flux_run(h, state_dev, done_dev, 1, ext_out_dev, stream, false);
}

int gemx_fluxobs_rows(gemx_fluxobs *h, const void *state_dev, const uint8_t *done_dev, int32_t K, void *ext_out_dev, void *stream) {
    return flux_run(h, state_dev, done_dev, K, ext_out_dev, stream, true);
}

int gemx_fluxobs_actions(gemx_fluxobs *h, const void *dq_dev, void *abc_out_dev, void *stream) {
    if (!h || !dq_dev || !abc_out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (h->prm.mode == GEMX_FLUX_ACT_NONE) return gemx::fail(GEMX_ERR_ARG, "the handle was created with action_mode = GEMX_FLUX_ACT_NONE");
    if (!gemx::elem_aligned(h->f64, dq_dev, abc_out_dev)) return gemx::fail_unaligned();
    gemx::DeviceGuard guard(h->device);
    const int32_t pairs = h->prm.mode == GEMX_FLUX_ACT_DFIM ? 2 : 1;
    const int64_t blocks = (h->n + 255) / 256;
    if (h->f64) {
        gemx_cov_note("flux_actions_kernel<double>");
        hipLaunchKernelGGL(flux_actions_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, h->hs, (const double *)dq_dev, (double *)abc_out_dev, h->n, pairs);
    } else {
        gemx_cov_note("flux_actions_kernel<float>");
        hipLaunchKernelGGL(flux_actions_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, h->hs, (const float *)dq_dev, (float *)abc_out_dev, h->n, pairs);
    }
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

int gemx_fluxobs_get_state(gemx_fluxobs *h, double *out_dev, void *stream) {
    if (!h || !out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(h->device);
    GEMX_HIP_TRY(hipMemcpyAsync(out_dev, h->hs, (size_t)h->n * 4u * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return GEMX_OK;
}

int gemx_fluxobs_set_state(gemx_fluxobs *h, const double *in_dev, void *stream) {
    if (!h || !in_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    gemx::DeviceGuard guard(h->device);
    GEMX_HIP_TRY(hipMemcpyAsync(h->hs, in_dev, (size_t)h->n * 4u * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return GEMX_OK;
}

}  // extern "C"
