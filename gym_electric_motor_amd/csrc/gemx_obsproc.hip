// gemx_obsproc.hip -- device-side observation stage (include/gemx.h: gemx_obsproc_*): the observation-side physical-system wrappers of
// the reference (paths relative to src/gym_electric_motor/),
//   CurrentSumProcessor  physical_system_wrappers/current_sum_processor.py:40-57   state || sum of the named currents
//   CosSinProcessor      physical_system_wrappers/cos_sin_processor.py:52-66       state [without the angle] || cos(pi eps), sin(pi eps)
//   state_filter         core.py:273-276, 317, 366                                 a column selection, applied last
//   FlattenObservation   of the shell's Tuple(state, reference)                    processed state || references
// resolved on the host (observation.py) into a COLUMN PROGRAM over the base system's columns and evaluated in ONE pass over the rows
// the stepping kernels wrote: one launch per call, nothing kept between calls.
//
// The pass is pure memory traffic: sizeof(R) * (n_in + n_ref + n_out) bytes per row and about one VALU instruction per output column.  A row
// of n_in = 5..24 values read by "its" lane would be a strided 4-byte access, so a tile of TILE rows -- 1 KiB * n_in contiguous bytes of
// the input, 1 KiB * n_out of the output, whatever n_in and n_out are -- goes through LDS:
//   1. the workgroup loads the tile in 16-byte units, consecutive lanes consecutive units, and writes it into LDS with the rows at an ODD
//      dword stride (the references of a flat observation go straight into the output tile's last columns);
//   2. lane r evaluates row r: every operand is ONE LDS read at r * stride + (uniform column), which the odd stride spreads over distinct
//      banks; the result goes into a second tile with an odd stride of its own;
//   3. the workgroup gathers that tile back into 16-byte units and stores them.
// A 16-byte unit straddles rows whenever the row length is no multiple of four dwords, so the units are scattered into / gathered from
// the padded tiles dword by dword (ds_write_b32 / ds_read_b32 at a lane stride of four dwords: a 4-way bank conflict, twice the issue
// cost of the instruction; per tile that is ~1.4k LDS cycles beside the ~3.5k cycles its HBM traffic takes at the chip's copy rate).
// The dword index -> (row, column) split is a multiply-high by a reciprocal the host computes; both are wave-uniform kernel arguments,
// as is the whole program (SGPRs: no table in global memory).
// Alignment: a tile is a multiple of 16 bytes, so a 16-byte aligned tensor has 16-byte aligned tiles; a tensor that is only
// element-aligned (a view at an odd offset) takes the dword loop for the whole call, per tensor.  The last, partial tile moves its
// whole 16-byte units and then single dwords: nothing beyond rows * n_in is read, nothing beyond rows * n_out is written.
// fp64 rows are moved as pairs of dwords (TILE = 128 rows keeps the two tiles within 64 KiB of LDS for every program).
#include "gemx_support.hpp"

namespace {

using namespace gemx;  // the row tile: gemx_support.hpp

struct ObsProg {
    int32_t n_in, n_post, n_ref, n_out;      // n_ref: reference columns the kernel appends (0 unless flat); n_out = n_post + n_ref
    uint32_t magic_in, magic_ref, magic_out; // floor(2^32 / L) + 1 for the row length L in dwords (0: L == 1)
    uint32_t ent[GEMX_OBS_MAX_POST];         // op | src << 8
    uint32_t mask[GEMX_OBS_MAX_POST];
};

template <class R> struct ObsTile { static constexpr int rows = 1024 / (int)sizeof(R); };
static_assert(tile_fits(ObsTile<double>::rows, 2 * (GEMX_OBS_MAX_POST + GEMX_MAX_REF)) && tile_fits(ObsTile<float>::rows, GEMX_OBS_MAX_POST + GEMX_MAX_REF) &&
                  GEMX_MAX_OUT <= GEMX_OBS_MAX_POST,
              "the longest row of either tile is within tile_row's exactness bound");

// cos / sin of pi x, evaluated in half-turns (no product with a rounded pi)
__device__ inline float obs_cospi(float x) { return cospif(x); }
__device__ inline double obs_cospi(double x) { return cospi(x); }
__device__ inline float obs_sinpi(float x) { return sinpif(x); }
__device__ inline double obs_sinpi(double x) { return sinpi(x); }

template <class R>
__global__ __launch_bounds__(ObsTile<R>::rows) void obs_post_kernel(const R *__restrict__ state, const R *__restrict__ refs, R *__restrict__ out, int64_t rows,
                                                                   ObsProg P, int vec_in, int vec_ref, int vec_out) {
    constexpr int T = ObsTile<R>::rows, DW = (int)sizeof(R) / 4;
    extern __shared__ __attribute__((aligned(16))) uint32_t obs_smem[];
    const uint32_t Li = (uint32_t)P.n_in * DW, Lr = (uint32_t)P.n_ref * DW, Lo = (uint32_t)P.n_out * DW;
    const uint32_t SI = Li | 1u, SO = Lo | 1u;  // odd row strides: lanes r and r' != r (mod 32) read / write distinct banks
    uint32_t *tin = obs_smem, *tout = obs_smem + (uint32_t)T * SI;
    const int64_t tile0 = (int64_t)blockIdx.x * T;  // (64-bit: rows * n_in may exceed 2^31)
    const uint32_t rows_t = (uint32_t)(rows - tile0 < (int64_t)T ? rows - tile0 : (int64_t)T);

    tile_stage_in<T>(tin, SI, Li, P.magic_in, reinterpret_cast<const uint32_t *>(state + tile0 * P.n_in), rows_t * Li, vec_in);
    if (Lr) tile_stage_in<T>(tout + (uint32_t)P.n_post * DW, SO, Lr, P.magic_ref, reinterpret_cast<const uint32_t *>(refs + tile0 * P.n_ref), rows_t * Lr, vec_ref);
    __syncthreads();
    if (threadIdx.x < rows_t) {
        const uint32_t *mine = tin + threadIdx.x * SI;
        uint32_t *res = tout + threadIdx.x * SO;
        for (int c = 0; c < P.n_post; ++c) {  // (uniform: the program sits in SGPRs)
            const uint32_t e = P.ent[c], op = e & 0xffu, src = e >> 8;
            R v;
            if (op == GEMX_OBS_SUM) {
                uint32_t m = P.mask[c];
                v = tile_get(mine + (uint32_t)(__ffs(m) - 1) * DW, R(0));
                for (m &= m - 1u; m; m &= m - 1u) v = v + tile_get(mine + (uint32_t)(__ffs(m) - 1) * DW, R(0));  // ascending j, plain adds
            } else {
                v = tile_get(mine + src * DW, R(0));
                if (op == GEMX_OBS_COSPI) v = obs_cospi(v);
                else if (op == GEMX_OBS_SINPI) v = obs_sinpi(v);
            }
            tile_put(res + (uint32_t)c * DW, v);
        }
    }
    __syncthreads();
    tile_stage_out<T>(tout, SO, Lo, P.magic_out, reinterpret_cast<uint32_t *>(out + tile0 * P.n_out), rows_t * Lo, vec_out);
}

}  // namespace

struct gemx_obsproc {
    gemx_obsproc_config cfg;
    ObsProg prog;
    int device, f64;
};

template <class R>
static int obs_launch(gemx_obsproc *p, const void *state, const void *refs, int64_t rows, void *out, hipStream_t st) {
    constexpr int T = ObsTile<R>::rows, DW = (int)sizeof(R) / 4;
    const ObsProg &P = p->prog;
    const int64_t tiles = (rows + T - 1) / T;
    if (tiles > 0x7fffffffLL) return gemx::fail(GEMX_ERR_ARG, "rows = %lld exceeds %d tiles of %d rows", (long long)rows, 0x7fffffff, T);
    const size_t lds = (size_t)T * (((size_t)P.n_in * DW | 1u) + ((size_t)P.n_out * DW | 1u)) * 4u;
    const int vec_in = ((uintptr_t)state & 15u) == 0, vec_ref = ((uintptr_t)refs & 15u) == 0, vec_out = ((uintptr_t)out & 15u) == 0;
    gemx_cov_note(sizeof(R) == 4 ? "obs_post_kernel<float>" : "obs_post_kernel<double>");
    hipLaunchKernelGGL(obs_post_kernel<R>, dim3((unsigned)tiles), dim3(T), lds, st, (const R *)state, (const R *)refs, (R *)out, rows, P, vec_in, vec_ref, vec_out);
    GEMX_HIP_TRY(hipGetLastError());
    return GEMX_OK;
}

extern "C" {

int gemx_obsproc_create(const gemx_obsproc_config *cfg, int dtype, int device, gemx_obsproc **out) {
    if (!cfg || !out) return gemx::fail(GEMX_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(gemx_obsproc_config)) return gemx::fail(GEMX_ERR_ARG, "gemx_obsproc_config size mismatch");
    if (cfg->n_in < 1 || cfg->n_in > GEMX_MAX_OUT) return gemx::fail(GEMX_ERR_ARG, "n_in must be in [1, %d]", GEMX_MAX_OUT);
    if (cfg->n_post < 1 || cfg->n_post > GEMX_OBS_MAX_POST) return gemx::fail(GEMX_ERR_ARG, "n_post must be in [1, %d]", GEMX_OBS_MAX_POST);
    if (cfg->n_ref < 0 || cfg->n_ref > GEMX_MAX_REF) return gemx::fail(GEMX_ERR_ARG, "n_ref must be in [0, %d]", GEMX_MAX_REF);
    if (cfg->flat != 0 && cfg->flat != 1) return gemx::fail(GEMX_ERR_ARG, "flat must be 0 or 1");
    const uint32_t valid = cfg->n_in >= 32 ? 0xffffffffu : (1u << cfg->n_in) - 1u;
    for (int c = 0; c < cfg->n_post; ++c) {
        const gemx_obsproc_entry &e = cfg->entries[c];
        if (e.op < GEMX_OBS_COPY || e.op > GEMX_OBS_SINPI) return gemx::fail(GEMX_ERR_ARG, "column %d: unknown op %d", c, e.op);
        if (e.op == GEMX_OBS_SUM) {
            if (e.mask == 0) return gemx::fail(GEMX_ERR_ARG, "column %d: SUM over no column", c);
            if (e.mask & ~valid) return gemx::fail(GEMX_ERR_ARG, "column %d: SUM mask 0x%x names a column >= n_in = %d", c, e.mask, cfg->n_in);
        } else if (e.src < 0 || e.src >= cfg->n_in) {
            return gemx::fail(GEMX_ERR_ARG, "column %d: src %d outside [0, %d)", c, e.src, cfg->n_in);
        }
    }
    if (int rc = gemx::check_device_dtype(device, dtype)) return rc;
    gemx_obsproc *p = new (std::nothrow) gemx_obsproc();
    if (!p) return gemx::fail(GEMX_ERR_ALLOC, "out of host memory");
    p->cfg = *cfg; p->device = device; p->f64 = dtype == GEMX_F64;
    ObsProg &P = p->prog;
    memset(&P, 0, sizeof(P));
    const uint32_t dw = p->f64 ? 2u : 1u;
    P.n_in = cfg->n_in; P.n_post = cfg->n_post; P.n_ref = cfg->flat ? cfg->n_ref : 0; P.n_out = P.n_post + P.n_ref;
    P.magic_in = tile_magic((uint32_t)P.n_in * dw); P.magic_ref = tile_magic((uint32_t)P.n_ref * dw); P.magic_out = tile_magic((uint32_t)P.n_out * dw);
    for (int c = 0; c < cfg->n_post; ++c) {
        const gemx_obsproc_entry &e = cfg->entries[c];
        P.ent[c] = (uint32_t)e.op | (e.op == GEMX_OBS_SUM ? 0u : (uint32_t)e.src << 8);
        P.mask[c] = e.op == GEMX_OBS_SUM ? e.mask : 0u;
    }
    *out = p;
    return GEMX_OK;
}

int gemx_obsproc_apply(gemx_obsproc *p, const void *state_dev, const void *refs_dev, int64_t rows, void *out_dev, void *stream) {
    if (!p || !state_dev || !out_dev) return gemx::fail(GEMX_ERR_ARG, "null argument");
    if (p->prog.n_ref > 0 && !refs_dev) return gemx::fail(GEMX_ERR_ARG, "a flat observation with n_ref = %d needs refs_dev", p->prog.n_ref);
    if (rows < 0) return gemx::fail(GEMX_ERR_ARG, "rows must be >= 0");
    if (!gemx::elem_aligned(p->f64, state_dev, out_dev, p->prog.n_ref > 0 ? refs_dev : nullptr)) return gemx::fail_unaligned();
    if (rows == 0) return GEMX_OK;
    gemx::DeviceGuard guard(p->device);
    hipStream_t st = (hipStream_t)stream;
    return p->f64 ? obs_launch<double>(p, state_dev, refs_dev, rows, out_dev, st) : obs_launch<float>(p, state_dev, refs_dev, rows, out_dev, st);
}

int gemx_obsproc_destroy(gemx_obsproc *p) {
    delete p;
    return GEMX_OK;
}

}  // extern "C"
