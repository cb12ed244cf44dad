// gemx_support.hpp -- what the small units of libgemx.so behind the stepping kernels share (gemx_obsproc.hip, gemx_rewardpass.hip,
// gemx_fluxobs.hip, gemx_refgen.hip, gemx_statenoise.hip, gemx_episode.hip, gemx_refprofile.hip, gemx_returns.hip; nothing else includes it): the row tile in LDS and the checks of their entry points.
//
// Row tile: rows of L dwords, contiguous in global memory, sit in LDS at an ODD dword stride so that lane r reads row r without bank
// conflicts.  Global memory is moved in 16-byte units, consecutive lanes consecutive units; a unit straddles rows whenever L is no
// multiple of four, so it is scattered into / gathered from the tile dword by dword.  An fp64 value is a pair of dwords.
// The per-lane functions of the two generator units that the complete policy rollout units call too come in through this header
// (gemx_refgen_lane.hpp, gemx_refprofile_lane.hpp): the generator units include nothing else.
#pragma once
#include "gemx_common.hpp"
#include "gemx_refgen_lane.hpp"
#include "gemx_refprofile_lane.hpp"

void gemx_cov_note(const char *key);  // gemx_capi.hip: instantiation coverage (GEMX_COVERAGE_FILE)

namespace gemx {

// tile-local dword index d of a row-major [rows][L] tile -> row, by a multiply-high with the reciprocal the host computes (tile_magic;
// 0: L == 1).  THE exactness bound, stated here once: d * (magic * L - 2^32) < 2^32 holds for d < TILE_MAX_DWORDS and
// L <= TILE_MAX_ROW; every unit asserts tile_fits(rows, longest row) for its own tile.
constexpr uint32_t TILE_MAX_ROW = 72, TILE_MAX_DWORDS = 1u << 14;
constexpr bool tile_fits(uint32_t rows, uint32_t L) { return L <= TILE_MAX_ROW && rows * L <= TILE_MAX_DWORDS; }
__device__ inline uint32_t tile_row(uint32_t d, uint32_t magic) { return magic ? __umulhi(d, magic) : d; }
inline uint32_t tile_magic(uint32_t L) { return L <= 1u ? 0u : (uint32_t)((1ull << 32) / L) + 1u; }  // floor(2^32 / L) + 1

// one value of a row (the tiles hold dwords: a double sits at an odd dword offset in every other row)
__device__ inline float tile_get(const uint32_t *p, float) { return __uint_as_float(p[0]); }
__device__ inline double tile_get(const uint32_t *p, double) { return __hiloint2double((int)p[1], (int)p[0]); }
__device__ inline void tile_put(uint32_t *p, float v) { p[0] = __float_as_uint(v); }
__device__ inline void tile_put(uint32_t *p, double v) { p[0] = (uint32_t)__double2loint(v); p[1] = (uint32_t)__double2hiint(v); }

// global (contiguous, `cnt` dwords) <-> LDS tile with rows of L dwords at `stride`, by NT threads.  vec: g is 16-byte aligned (a tensor
// that is only element-aligned takes the dword loop); the whole units first, then the single dwords behind them: nothing beyond cnt.
// (The four dwords of a unit, wrapping at the row end, are written out in both: behind helpers of their own the kernels no longer
// compiled to the instructions they had, profiles/support_units_refactor.md.)
template <int NT> __device__ inline void tile_stage_in(uint32_t *tile, uint32_t stride, uint32_t L, uint32_t magic, const uint32_t *g, uint32_t cnt, int vec) {
    const uint32_t nvec = vec ? cnt >> 2 : 0u;
    for (uint32_t v = threadIdx.x; v < nvec; v += NT) {
        const uint4 q = reinterpret_cast<const uint4 *>(g)[v];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        const uint32_t d = v * 4u, row = tile_row(d, magic);
        uint32_t col = d - row * L, a = row * stride + col;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            tile[a] = w[i];
            ++col; ++a;
            if (col == L) { col = 0; a += stride - L; }
        }
    }
    for (uint32_t d = nvec * 4u + threadIdx.x; d < cnt; d += NT) {
        const uint32_t row = tile_row(d, magic);
        tile[row * stride + (d - row * L)] = g[d];
    }
}
template <int NT> __device__ inline void tile_stage_out(const uint32_t *tile, uint32_t stride, uint32_t L, uint32_t magic, uint32_t *g, uint32_t cnt, int vec) {
    const uint32_t nvec = vec ? cnt >> 2 : 0u;
    for (uint32_t v = threadIdx.x; v < nvec; v += NT) {
        const uint32_t d = v * 4u, row = tile_row(d, magic);
        uint32_t col = d - row * L, a = row * stride + col;
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = tile[a];
            ++col; ++a;
            if (col == L) { col = 0; a += stride - L; }
        }
        reinterpret_cast<uint4 *>(g)[v] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (uint32_t d = nvec * 4u + threadIdx.x; d < cnt; d += NT) {
        const uint32_t row = tile_row(d, magic);
        g[d] = tile[row * stride + (d - row * L)];
    }
}

// ---- host side: what every create function checks last, and what every entry point that takes tensors checks of them
inline int check_device_dtype(int device, int dtype) {
    if (dtype != GEMX_F32 && dtype != GEMX_F64) return fail(GEMX_ERR_ARG, "unknown dtype");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(GEMX_ERR_DEVICE, "no HIP device visible: there is no CPU fallback");
    if (device < 0 || device >= ndev) return fail(GEMX_ERR_ARG, "device %d out of range", device);
    return GEMX_OK;
}
// every pointer is aligned to the element size (null pointers are)
template <class... P> inline bool elem_aligned(bool f64, P... p) { return ((((uintptr_t)p | ...) & (f64 ? 7u : 3u)) == 0); }
inline int fail_unaligned() { return fail(GEMX_ERR_ARG, "tensors must be aligned to their element size"); }

}  // namespace gemx
