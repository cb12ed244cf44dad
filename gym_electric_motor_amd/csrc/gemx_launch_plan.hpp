// gemx_launch_plan.hpp -- how a fused rollout of the pipelined kernel is launched: which shape, how much LDS, and the rate limiter's intervals.
// Host code only: no kernel and no device function.  Two layers:
//   the PURE layer (namespace gemx::plan, first half of this file) takes numbers and returns numbers.  It includes no HIP header, a plain
//     host compiler builds it, and tests/test_launch_plan_cpu.py replays recorded launches through it without a GPU;
//   the RESOLVE layer (second half, under __HIPCC__) asks the runtime for what the pure layer is given -- registers and occupancy per
//     shape, the dynamic-LDS attribute, the calibration's event pairs -- and keeps each answer in the handle's cache.
// launch_advance_t (gemx_kernels.hpp) fills a Facts with the compile-time numbers of its instantiation, calls plan_rollout() and launches
// the shape it returns; nothing here depends on a template parameter, so a unit compiles it once.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gemx {
namespace plan {

// ---- the pipelined kernel's shapes, as gemx_common.hpp names them (the resolve layer asserts the two agree) -------------------------------
constexpr int ENVS = 64;       // envs per workgroup (BLOCK)
constexpr int REAL_BYTES = 4;  // the pipelined kernel is fp32 only
constexpr int NSHAPE = 8;      // pipe_kernel_of's index: 0 <12, 3>, 1 <4, 2>, 2 <2, 2>, 3 <12, 6>, 4 <4, 2> FULL, (5 not built,) 6 FULL SLOW, 7 FULL RINIT
constexpr int D_DEEP = 12, D_MID = 4, D_SHALLOW = 2;
constexpr int SHAPE_D[NSHAPE] = {D_DEEP, D_MID, D_SHALLOW, D_DEEP, D_MID, D_MID, D_MID, D_MID};
constexpr int SHAPE_OW[NSHAPE] = {3, 2, 2, 6, 2, 2, 2, 2};
constexpr int LOADER_WAVES = 1;
#ifndef GEMX_PIPE_AHEAD2
#define GEMX_PIPE_AHEAD2 0
#endif
constexpr int act_bufs(int D) { return ((D <= 4 && GEMX_PIPE_AHEAD2) ? 2 : 1) + 1; }
constexpr int ref_bufs(int D) { return ((D <= 4 && GEMX_PIPE_AHEAD2) ? 2 : 1) + 2; }
constexpr int queue_rows(int D, int delay, bool dq_processor, bool full) { return (D == D_DEEP && !full && dq_processor && delay > 0) ? D + delay : delay; }
constexpr int waves_per_wg(int shape) { return 1 + SHAPE_OW[shape] + LOADER_WAVES; }

// ---- what launch_advance_t knows at compile time ----------------------------------------------------------------------------------------
struct Facts {
    int abytes;           // action bytes per env and step (one for a discrete converter)
    int nht;              // values of a hand-off row without the FULL column
    int nact_c;           // conv_nact_c: width of the converter-side action (the DeadTimeProcessor queue's rows)
    int vt_bytes;         // per-action voltage table in LDS (0: none)
    int prep_q;           // prepared draws per lane (random initialisers)
    int init_desc_bytes;  // ... and the description beside them, padded to 16
    bool dq;              // conv_dq: a dq action frame
    bool compact_l;       // COMPACT hand-off rows exist for this instantiation (synchronous machine, finite converter, one-step map)
    bool sync;            // SYS == GEMX_SYS_SYNC
    bool deep_built, d3_built;    // pipe_deep_built, pipe_d3_built
    const void *kernel[NSHAPE];   // pipe_kernel_of(shape); nullptr: not built
};
// ---- ... and what one launch adds ---------------------------------------------------------------------------------------------------------
struct Launch {
    int64_t blocks;  // workgroups: ceil(n_envs / 64)
    int K, n_cu, nout, delay, rw_n_ref;
    int forced_shape;  // GEMX_PIPE_SHAPE (tests), -1: none
    size_t lds_max;
    bool dq_processor, need_full, fast_step, rinit, lin_on, reward, half, synth;
    bool pace_default_on;  // GEMX_PACE_DEFAULT_ON
    double pace_gbps;      // < 0: the built-in target, 0: off, > 0: an explicit target
    int regs[NSHAPE];      // VGPRs per shape (0: not built)
    int occ[NSHAPE];       // workgroups per CU the occupancy API reports for the shape at this launch's LDS bytes
};

// LDS footprint of one workgroup at hand-off depth D (steps per barrier): ring + done ring + double-buffered hand-off rows + ...
inline size_t lds_bytes(const Facts &f, const Launch &l, int D) {
    const int NHT = f.nht + (l.need_full ? 1 : 0);
    size_t b = (size_t)D * ENVS * l.nout * REAL_BYTES + (size_t)D * ENVS + 2 * (size_t)D * ENVS * NHT * REAL_BYTES;
    b += (size_t)queue_rows(D, l.delay, f.dq && l.dq_processor, l.need_full) * ENVS * f.nact_c * REAL_BYTES;  // DeadTimeProcessor queue
    b += act_bufs(D) * (size_t)((D + 3) / 4 * 4) * ENVS * f.abytes;  // action staging (global -> LDS direct, one or two blocks ahead)
    if (l.reward) b += ref_bufs(D) * (size_t)D * ENVS * l.rw_n_ref * REAL_BYTES;  // reference staging for the fused reward
    b += (size_t)f.vt_bytes;  // per-action voltage table
    if (l.rinit) b += (size_t)(f.prep_q * 8 + 1) * ENVS * sizeof(uint32_t) + (size_t)f.init_desc_bytes;  // prepared draws (random initialisers) + the description
    return (b + 15) & ~(size_t)15;
}
// workgroups of a shape one CU holds: LDS, wave slots -- and REGISTERS (round 4: the arithmetic used to stop at the first two and
// took four resident workgroups of a shallow shape for granted; a kernel at 129-136 VGPRs holds three, and a "one round" rule that
// does not know runs a round plus a tail)
inline int64_t regs_limit(int regs, int waves_per_wg_) {
    if (regs == 0) return 0;  // (a shape that is not built holds no workgroup)
    int waves_per_simd = 512 / ((regs + 7) & ~7);  // gfx950: 512 VGPRs per SIMD lane, allocation granule 8
    if (waves_per_simd < 1) waves_per_simd = 1;
    if (waves_per_simd > 8) waves_per_simd = 8;
    return (int64_t)(4 * waves_per_simd) / waves_per_wg_;
}
// ... and what the runtime itself says a CU holds (Launch::occ): the rate limiter below prices every workgroup's interval with the number
// of workgroups that are RUNNING, and the PermExDc <4, 2> kernel, eight per CU by LDS, wave slots and registers, runs five (r04m: 98304
// envs paced for 1536 concurrent workgroups with ~1280 resident ran 0.54 of the roofline against 0.90 at 65536)
inline int64_t resident(const Facts &f, const Launch &l, int shape) {
    const size_t smem = lds_bytes(f, l, SHAPE_D[shape]);
    int64_t w = (int64_t)(l.lds_max / smem);
    const int64_t wmax = 32 / waves_per_wg(shape);
    const int64_t wreg = regs_limit(l.regs[shape], waves_per_wg(shape));
    w = w > wmax ? wmax : w;
    w = w > wreg ? wreg : w;
    if (smem <= l.lds_max) {
        const int64_t wocc = (int64_t)l.occ[shape];
        w = w > wocc ? wocc : w;
    }
    if (wreg == 0) return (int64_t)0;  // not built (pipe_deep_built)
    return (w < 1 ? 1 : w) * (int64_t)l.n_cu;
}

inline bool pacing_on(const Launch &l) { return (l.pace_gbps < 0.0 ? l.pace_default_on : l.pace_gbps > 0.0) && l.K >= 64; }

struct Choice {
    int shape, D, OW;  // D == 0: no pipelined shape serves this launch (the single-wave kernel does)
    bool long_one;     // a long launch at one workgroup per CU that takes <12, 3> for the limiter's clock
};
inline Choice choose_shape(const Facts &f, const Launch &l) {
    const int64_t blocks = l.blocks;
    const size_t lds_max = l.lds_max;
    // one resident round of the 4-wave shape if N is that small, else the 3-wave shape at ANY N: measured at 131072 and 1048576
    // envs over all motor families (profiles/r01d_matrix.md) it is on par with or ahead of the single-wave kernel (PMSM
    // 1M envs: 100 vs 86 G env-steps/s) -- the split keeps stores fire-and-forget and the integrator free of vmcnt waits
    int D = 0, OW = 0, shape = 0;
    // six output waves (eight waves in all: still one workgroup per CU) where the output side carries more than three waves keep up
    // with: the fused reward, and the COMPACT hand-off rows of the synchronous machines behind a finite converter (advance_pipe_kernel,
    // COMPACT_K: the integrator is 8 % faster per block there, 3555 against 3875 cycles, and the output waves look the phase voltages
    // up themselves -- three of them need 4100 cycles per block, six 2500; PMSM headline 147.6 -> 140 us per launch)
    const bool compact_l = f.compact_l && l.lin_on && !l.need_full;
    // ... and with those rows the deep shape is ahead of <4, 2> at ANY N whose workgroups fill its rounds of one workgroup per CU: same box,
    // PMSM finite, of the roofline at 28672 / 32768 / 49152 / 65536 / 131072 envs: 0.71 / 0.72 / 0.70 / 0.77 / 0.79 against 0.68 / 0.68 / 0.67 /
    // 0.65 / 0.70 (profiles/r03s_shapes_compact.md); a last round less than ~85 % full loses instead (24576 envs: 0.59 against 0.65)
    // -- and a launch too short to amortise a workgroup's ~10 us outside its block loop, which <4, 2>'s four co-resident workgroups overlap
    // (1M envs x 100 steps: 0.53 against 0.68): K >= 400
    bool deep_rounds = false;
    // (not behind a DeadTimeProcessor: its delayed-read blocks are slower in the deep shape than <4, 2>'s queue: 131072 envs 0.57 against 0.69)
    // (nor with the fused reward, whose output waves are the bound at large N either way: 131072 envs 0.56 against 0.60)
    // (round 4: only while the rate limiter is OFF.  With it the shallow shapes hold 0.79 at every size from 32768 envs on, the deep shape in
    // rounds 0.64-0.77: profiles/r04m_pace_shapes.txt)
    const bool paced = pacing_on(l);
    if (f.deep_built && compact_l && !paced && l.K >= 400 && l.delay == 0 && !l.reward && lds_bytes(f, l, D_DEEP) <= lds_max) {
        const int64_t res0 = resident(f, l, 3), rounds = (blocks + res0 - 1) / res0;
        deep_rounds = blocks > res0 && 100 * blocks >= 85 * rounds * res0;
    }
    // (limiter on: the deep shape up to TWO workgroups per CU -- at three, 49152 envs, the DC machines it fits run 0.76 / 0.59 / 0.33 (PermExDc /
    // ShuntDc / SeriesDc SC) against 0.86 / 0.85 / 0.60 through <4, 2> under the limiter: profiles/r04p_shape_32768.txt)
    // LONG launches at one workgroup per CU lose their rate as well: the headline holds 0.80-0.83 of the roofline up to 1000 steps per launch,
    // 0.75 at 2000, 0.70 at 3000, 0.68 at 6000 -- workgroups that start in the same phase drift apart, and the stores of a CU's neighbours
    // stop landing in the same DRAM rows.  The limiter is also a clock that keeps them together: the same launches through <12, 3> at
    // the 32768-env target run 0.83 / 0.84 at 3000 / 6000 steps (PMSM cont 0.69 / 0.70 -> 0.77 / 0.79; profiles/r04r_probe5.txt).  Only the
    // rows whose integrator is faster than the target gain (the synchronous machines on the one-step map); an integrator-bound
    // row pays 3-6 % for the clock reads (SCIM finite 0.66 -> 0.62, ShuntDc 0.54 -> 0.52) and keeps its unpaced launch.  From 1200 steps on: at
    // 1000 the unpaced <12, 6> is ahead (0.84 against 0.81), at 1400 behind (0.77 against 0.81-0.83: profiles/r04q_probe3.txt A, r04r_probe5.txt).
    const bool long_one = paced && l.pace_gbps < 0.0 && l.K >= 1200 && f.sync && l.lin_on && !l.need_full && !l.reward && blocks <= (int64_t)l.n_cu;
    const int64_t deep_max = paced && resident(f, l, 0) > 2 * (int64_t)l.n_cu ? 2 * (int64_t)l.n_cu : resident(f, l, 0);
    if (f.deep_built && lds_bytes(f, l, D_DEEP) <= lds_max && (blocks <= deep_max || deep_rounds)) {
        shape = 0;
        // (long launches of the synchronous machines' one-step-map rows: <12, 3>, which carries the rate limiter -- see `long_one` above)
        if (l.reward || (compact_l && !long_one)) shape = 3;
        D = SHAPE_D[shape]; OW = SHAPE_OW[shape];
    }
    else if (f.d3_built && lds_bytes(f, l, D_SHALLOW) <= lds_max && blocks <= resident(f, l, 2) &&
             blocks > resident(f, l, 1) && 2 * blocks <= 3 * resident(f, l, 1)) {
        // (round 4: EVERY system.  Rounds 2-3 kept this to the induction machines on one sample -- ExtExDc at 131072 envs, which is not
        // this case at all (two full rounds of <4, 2>) -- but where <4, 2> runs a round plus a tail of at most half a round and <2, 2>
        // fits everything into one, the interleaved same-box A/B (tools/ab_matrix_shapes.py, profiles/r04c_shapes_ab.md, 65536 envs,
        // of the roofline) has it ahead almost everywhere: PMSM cont 0.57 -> 0.71, PMSM cont SC 0.50 -> 0.69, ShuntDc 0.61 -> 0.73,
        // EESM 0.57 -> 0.64 / 0.56 -> 0.61, DqToAbc + DeadTime 0.59 -> 0.75, PermExDc 0.78 -> 0.85, fused reward 0.56 -> 0.62;
        // level: SeriesDc SC, ExtExDc.)
        // (induction machines only: lighter steppers lose with the shallow shape -- ExtExDc 131072 envs 133 -> 104 G; PMSM finite at
        // 98304 envs, where this rule used to apply: 75.8 G against 84.2 G through <4, 2>, profiles/r03k_shapes_pmsm.md)
        // one resident round with the shallow shape where <4, 2> would run one round plus a tail of at most half a round: SCIM,
        // 65536 envs (BASELINE config 4) 49 -> 67 G env-steps/s.  Everywhere else <4, 2> is 5-20 % ahead of <2, 2> (fewer barriers,
        // fewer waves per SIMD): PMSM finite at 131072 envs = two FULL rounds of <4, 2>: 89-92 G against 79 G in one round of <2, 2>
        shape = 2; D = SHAPE_D[2]; OW = SHAPE_OW[2];
    } else if (lds_bytes(f, l, D_MID) <= lds_max) { shape = 1; D = SHAPE_D[1]; OW = SHAPE_OW[1]; }
    if (l.forced_shape >= 0 && l.forced_shape <= 3) {  // forced shape (tests)
        const int fs = l.forced_shape;
        if (lds_bytes(f, l, SHAPE_D[fs]) <= lds_max && f.kernel[fs] != nullptr) { shape = fs; D = SHAPE_D[fs]; OW = SHAPE_OW[fs]; }
    }
    if (l.need_full) {  // one instantiation serves these handles
        // ~180 VGPRs = two resident workgroups per CU.  RC supply: ahead of the single-wave kernel at every size (PMSM finite, same box:
        // 52 vs 14 G env-steps/s at 16384 envs, 89 vs 26 at 32768, 89 vs 47 at 65536).  Random initialisers (the fp64 draw sits in the
        // integrator's reset path): ahead up to 32768 envs (28 vs 16), level at 65536, behind beyond (28 vs 43 at 131072) --
        // tools/ab_full_variant.py
        // Round 5: random initialisers have their own instantiation (RINIT) whose loader wave prepares the draws; same box, PMSM finite:
        // 21 -> 54-57 G env-steps/s at 32768 / 65536 envs, and 57 against the single-wave kernel's 32 at 131072 -- the size rule
        // ("at most four workgroups per CU") is gone (profiles/r05r_ab_prep.txt).
        if (lds_bytes(f, l, D_MID) <= lds_max) { shape = l.rinit ? 7 : 4; D = SHAPE_D[shape]; OW = SHAPE_OW[shape]; }
        else D = 0;
    }
    if (!l.fast_step && D != 0) {  // solver sub-steps / a custom constraint set: the SLOW instantiations of <4, 2> (no limiter: integrator-bound)
        if (lds_bytes(f, l, D_MID) <= lds_max && !l.rinit) { shape = 6; D = SHAPE_D[6]; OW = SHAPE_OW[6]; }
        else D = 0;  // (together with random initialisers: the single-wave kernel)
    }
    return Choice{shape, D, OW, long_one};
}

// ---- the rate limiter (advance_pipe_kernel): only where the batch oversubscribes the write path -- more workgroups than CUs; at one
// workgroup per CU in one round the integrator's instruction stream is the pacing, and an s_memrealtime per block would only cost
// it time.  interval per row and workgroup = algorithmic bytes of a 64-env step x workgroups resident on the chip / target rate. ------------
inline int abytes_eff(const Facts &f, const Launch &l) { return l.half ? f.abytes / 2 : f.abytes; }  // (gemx_rollout_half: two bytes per value)
// Target: a few per cent under the knee the sweeps over the real kernels found (profiles/r04l_pace_sweep.txt, r04n_pace_sweep2.txt;
// same box, of the 8 TB/s).  Under the limiter a launch runs at ~0.98 x target / 8000 up to the knee and collapses beyond it:
// rows of 14-24 values (3.5-6 KB per workgroup and step) at 32768 / 65536 / 131072 envs peak at 7000-7200 / 6800-7000 / 6400-6600
// GB/s (PMSM finite 0.65 / 0.66 / 0.65 unpaced -> 0.85 / 0.84 / 0.80 at the knee, 0.66 / 0.79 / 0.76 one step beyond it; SCIM,
// EESM, DFIM finite alike), the DC machines' 5-7 values (1.3-1.8 KB) at 7200-7600 / 7200 / 7000 (ShuntDc 0.62 / 0.61 / 0.65 ->
// 0.85 / 0.87 / 0.80).  The knee moves down with the number of workgroups in flight.  Kernels whose integrators offer less
// than the target (the speed-control rows, 16384 envs) never wait and are unchanged.
inline double builtin_target(const Facts &f, const Launch &l) {
    const bool few = l.blocks <= 2 * (int64_t)l.n_cu, some = l.blocks <= 4 * (int64_t)l.n_cu;
    // Launches that also READ eight bytes or more per env-step (continuous duty cycles through the loader wave) have the knee lower and
    // a softer landing beyond it (back to the unpaced level, not below): 65536 / 131072 envs PMSM cont 0.66 / 0.63 unpaced -> 0.68 / 0.63
    // at 6000 / 5600, EESM cont 0.62 / 0.59 -> 0.73 / 0.66, DFIM cont 0.60 / 0.70 -> 0.72 / 0.69, control_space='dq' 0.62 / 0.62 -> 0.68 /
    // 0.65, ExtExDc cont 0.72 / 0.64 -> 0.77 / 0.64 at 6400 (profiles/r04p_pace_sweep3.txt).
    const bool reads = abytes_eff(f, l) >= 8 && !l.synth;  // (synthetic actions are generated in the launch: nothing is read)
    return l.nout <= 8 ? (reads ? (few ? 7000.0 : 6400.0) : (some ? 7000.0 : 6600.0))
           : reads     ? (few ? 6400.0 : (some ? 6000.0 : 5800.0))
                       : (few ? 6800.0 : (some ? 6600.0 : 6400.0));
}
// the target before the calibration's factor: the built-in one, or the caller's
inline double open_loop_target(const Facts &f, const Launch &l) { return l.pace_gbps < 0.0 ? (l.pace_default_on ? builtin_target(f, l) : 0.0) : l.pace_gbps; }
// (<12, 6> carries no limiter: see the kernel; nor do the SLOW ones)
inline bool shape_paces(const Launch &l, int shape) { return l.K >= 64 && shape != 3 && shape < 5; }

struct Pace {
    uint32_t block_ticks, tail_ticks, tail_from;  // KArgs::pace_*: 0 / 0 / 0xFFFFFFFF = no limiter
    int64_t res;                                  // resident workgroups the intervals were priced for
};
inline uint32_t ticks_for(double wg_step_bytes, double active, double target, int D) {
    const double t = wg_step_bytes * active / target * D / 10.0;  // bytes / (GB/s) = ns; 10 ns per tick; D rows per block
    return t < 1.0 ? 1u : (t > 4.0e9 ? 0u : (uint32_t)(t + 0.5));
}
// target: open_loop_target() times the calibration's factor
inline Pace pace_for(const Facts &f, const Launch &l, const Choice &c, double target) {
    Pace p{0u, 0u, 0xFFFFFFFFu, 0};
    const int64_t blocks = l.blocks, n_cu = (int64_t)l.n_cu;
    // (round 5: the FULL instantiations are priced with their own registers and occupancy too -- without the draw code the RC-supply
    // kernel went from 207 to 118 VGPRs, four workgroups per CU instead of the two that used to be written here)
    int64_t res = resident(f, l, c.shape);
    // More than four workgroups per CU (the DC machines' small rows) and a launch that needs the LAST slot of every CU to be one round:
    // count one slot less.  Registers, LDS, wave slots and the occupancy API said seven of the ShuntDc <4, 2> kernel; 114688 envs = 1792
    // workgroups were priced as one round of 1792 -- and ran 0.41 of the roofline against 0.63 unpaced: whichever workgroups do not
    // find their slot at once run alone afterwards at an interval meant for 1792.  Priced for six per CU they are a tail round,
    // 0.64.  (Only in that band: at 131072 envs, one round of 1792 and a tail of 256, the seven slots price right -- 0.79 against 0.65
    // with six; profiles/r04final_odd_sizes.txt, r04final_dc_residency.txt.)
    if (res > 4 * n_cu && blocks <= res && blocks > res - n_cu) res -= n_cu;
    p.res = res;
    if (target > 0.0 && (blocks > n_cu || l.pace_gbps > 0.0 || c.long_one) && shape_paces(l, c.shape)) {
        const double wg_step_bytes = (double)ENVS * ((l.synth ? 0 : abytes_eff(f, l)) + l.nout * REAL_BYTES + 1 + (l.reward ? (l.rw_n_ref + 1) * REAL_BYTES : 0));
        const int64_t full = blocks / res, tail = blocks - full * res;
        p.block_ticks = ticks_for(wg_step_bytes, (double)(blocks < res ? blocks : res), target, c.D);
        if (full >= 1 && tail > 0) {  // the last round: `tail` workgroups on the chip
            p.tail_from = (uint32_t)(full * res);
            p.tail_ticks = ticks_for(wg_step_bytes, (double)(tail < n_cu ? n_cu : tail), target, c.D);
        }
    }
    return p;
}

// ---- closed loop: which candidate a launch runs (gemx_handle::PaceCal) --------------------------------------------------------------------
// Cal: a struct with PaceCal's members (NC, SAMPLES, RING, MAX_RECENTER; sig, center, recenters, next, chosen, best, count, issued, ev_cand,
// ev_init).  The event pairs themselves are the resolve layer's.
constexpr double CAL_SCALE[5] = {1.0, 0.93, 1.07, 0.86, 0.0};  // (0: unpaced)
inline bool cal_eligible(const Launch &l, const Choice &c, bool cal_on, double target) {
    return cal_on && l.pace_gbps < 0.0 && target > 0.0 && (l.blocks > (int64_t)l.n_cu || c.long_one) && shape_paces(l, c.shape);
}
// (the interval per hand-off block does not depend on the launch's length: K enters only through its class -- short launches,
// whose fixed costs weigh on the timings, and the long launches at one workgroup per CU, which pace a different shape.  A
// training loop that varies K within a class keeps its calibration; round 5 keyed it by K itself and re-calibrated, up to 240
// launches, at every change.)
inline long long cal_signature(const Launch &l, const Choice &c) {
    const int k_class = c.long_one ? 2 : (l.K < 256 ? 0 : 1);
    return ((long long)k_class << 40) ^ ((long long)l.blocks << 8) ^ (long long)c.shape ^ (l.reward ? 0x80 : 0) ^ (l.synth ? 0x40 : 0) ^ (l.half ? 0x20 : 0);
}
template <class Cal> inline void cal_clear(Cal &pc) {
    for (int c = 0; c < Cal::NC; ++c) { pc.best[c] = 1e30f; pc.count[c] = 0; pc.issued[c] = 0; }
}
// a new kind of launch: start over (events are kept)
template <class Cal> inline void cal_start(Cal &pc, long long sig) {
    if (pc.sig == sig) return;
    pc.sig = sig; pc.next = 0; pc.chosen = -1; pc.center = 1.0f; pc.recenters = 0;
    cal_clear(pc);
    if (pc.ev_init) for (int i = 0; i < Cal::RING; ++i) pc.ev_cand[i] = -1;
}
// pair `slot` has finished after `ms` (<= 0: no valid time): its candidate's sample, and the pair is free again
template <class Cal> inline void cal_harvest(Cal &pc, int slot, float ms) {
    if (ms > 0.0f) {
        const int c = pc.ev_cand[slot];
        pc.best[c] = ms < pc.best[c] ? ms : pc.best[c];
        pc.count[c]++;
    }
    pc.ev_cand[slot] = -1;
}
struct CalTurn { int slot, cand; };  // slot < 0: this launch is not timed
// One launch's turn, after the finished pairs were harvested: either the calibration ends (or moves its bracket), or a free pair and the
// candidate it times are handed out.
template <class Cal> inline CalTurn cal_turn(Cal &pc) {
    CalTurn t{-1, 0};
    bool done_cal = true;
    for (int c = 0; c < Cal::NC; ++c) done_cal &= pc.count[c] >= Cal::SAMPLES;
    if (done_cal) {
        int bi = 0;
        for (int c = 1; c < Cal::NC; ++c) if (pc.best[c] < pc.best[bi]) bi = c;
        // (a candidate must beat the starting point by more than 1 % to replace it: timing noise)
        const int win = pc.best[bi] < 0.99f * pc.best[0] ? bi : 0;
        // the winner at an EDGE of the bracket (x 1.07 or x 0.86): the optimum may lie beyond -- move the bracket there
        // and calibrate again (the built-in targets are one box's knees; a launch that reads nothing, e.g. with
        // synthetic actions, peaks well above them)
        if ((win == 2 || win == 3) && pc.recenters < Cal::MAX_RECENTER) {
            pc.center *= (float)CAL_SCALE[win];
            pc.recenters++;
            cal_clear(pc);
            // (pairs still in flight were timed at the OLD centre: they must not be harvested into the new bracket --
            // best[] keeps the minimum, one stale fast sample could pick the wrong candidate for good; advisor, round 5)
            for (int i = 0; i < Cal::RING; ++i) pc.ev_cand[i] = -1;
        } else {
            pc.chosen = win;
        }
    } else {
        for (int i = 0; i < Cal::RING; ++i)
            if (pc.ev_cand[i] < 0) { t.slot = i; break; }
        if (t.slot >= 0) {  // (no free pair: this launch runs the starting point, untimed)
            // the candidate handed out least often so far goes next (round robin, starting with the built-in target)
            int c = 0;
            for (int q = 1; q < Cal::NC; ++q) if (pc.issued[q] < pc.issued[c]) c = q;
            pc.issued[c]++;
            pc.next++;
            pc.ev_cand[t.slot] = c;
            t.cand = c;
        }
    }
    return t;
}
// the factor on the open-loop target this launch runs at
template <class Cal> inline double cal_scale(const Cal &pc, CalTurn t) {
    const int use = pc.chosen >= 0 ? pc.chosen : (t.slot >= 0 ? t.cand : 0);
    return CAL_SCALE[use] * pc.center;
}

}  // namespace plan
}  // namespace gemx

// ==============================================================================================================================================
// resolve layer
// ==============================================================================================================================================
#ifdef __HIPCC__
#include <cstdio>
#include <cstdlib>

#include "gemx_common.hpp"

// the large-batch rate limiter is on unless a launch says otherwise; its target: chip-wide algorithmic GB/s (tools/microbench_rowpitch.hip,
// profiles/r04k_*; GEMX_PACE_GBPS overrides)
#ifndef GEMX_PACE_DEFAULT_ON
#define GEMX_PACE_DEFAULT_ON 1
#endif

namespace gemx {
namespace plan {
static_assert(ENVS == BLOCK && D_DEEP == PIPE_D && D_MID == PIPE_D2 && D_SHALLOW == PIPE_D3 && SHAPE_OW[0] == PIPE_OUT_WAVES && SHAPE_OW[1] == PIPE_OUT_WAVES2 &&
              SHAPE_OW[2] == PIPE_OUT_WAVES3 && SHAPE_OW[3] == PIPE_OUT_WAVES_RW && LOADER_WAVES == pipe_loader_waves(0), "the pure layer's shapes are gemx_common.hpp's");
constexpr bool geometry_agrees() {
    const int depths[3] = {PIPE_D, PIPE_D2, PIPE_D3};
    for (int D : depths) {
        if (act_bufs(D) != pipe_act_bufs(D) || ref_bufs(D) != pipe_ref_bufs(D)) return false;
        for (int delay = 0; delay <= 8; ++delay)
            for (int m = 0; m < 4; ++m)
                if (queue_rows(D, delay, (m & 1) != 0, (m & 2) != 0) != pipe_queue_rows(D, delay, (m & 1) != 0, (m & 2) != 0)) return false;
    }
    return true;
}
static_assert(geometry_agrees(), "the pure layer's LDS arithmetic is gemx_common.hpp's");

// registers and occupancy of one shape, once per handle (the occupancy again when the LDS bytes move: the fused reward, the queue depth)
inline void resolve_shape(gemx_handle *h, const Facts &f, Launch &l, int shape) {
    const void *kp = f.kernel[shape];
    l.regs[shape] = 0;
    l.occ[shape] = 0;
    if (kp == nullptr) return;
    if (h->pipe_regs[shape] == 0) {
        hipFuncAttributes fa;
        h->pipe_regs[shape] = (hipFuncGetAttributes(&fa, kp) == hipSuccess && fa.numRegs > 0) ? fa.numRegs : 128;
    }
    l.regs[shape] = h->pipe_regs[shape];
    const size_t smem_b = lds_bytes(f, l, SHAPE_D[shape]);
    if (smem_b > l.lds_max) return;  // (never launched at this footprint: nothing to ask)
    if (h->pipe_occ[shape] == 0 || h->pipe_occ_smem[shape] != smem_b) {
        int nb_ = 0;
        h->pipe_occ_smem[shape] = smem_b;
        if (!(h->pipe_attr_set & (1u << shape))) {  // (the bit only on success: the launch path then repeats the call, checked, and reports the error)
            if (hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_max) == hipSuccess) h->pipe_attr_set |= 1u << shape;
            else (void)hipGetLastError();
        }
        h->pipe_occ[shape] = (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb_, kp, waves_per_wg(shape) * BLOCK, smem_b) == hipSuccess && nb_ > 0) ? nb_ : 64;
        (void)hipGetLastError();
    }
    l.occ[shape] = h->pipe_occ[shape];
}

// the calibration's event pairs: created on demand, harvested without ever blocking; returns this launch's turn
inline CalTurn cal_resolve(gemx_handle *h) {
    using PC = gemx_handle::PaceCal;
    auto &pc = h->pcal;
    if (!pc.ev_init) {
        bool ok = true;
        for (int i = 0; i < PC::RING && ok; ++i) {
            ok = hipEventCreate((hipEvent_t *)&pc.ev0[i]) == hipSuccess && hipEventCreate((hipEvent_t *)&pc.ev1[i]) == hipSuccess;
            pc.ev_cand[i] = -1;
        }
        pc.ev_init = ok;
        if (!ok) { (void)hipGetLastError(); h->pace_cal_on = 0; }
    }
    if (!pc.ev_init) return CalTurn{-1, 0};
    // harvest the pairs whose launches have finished (never blocks)
    for (int i = 0; i < PC::RING; ++i) {
        if (pc.ev_cand[i] < 0 || hipEventQuery((hipEvent_t)pc.ev1[i]) != hipSuccess) continue;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, (hipEvent_t)pc.ev0[i], (hipEvent_t)pc.ev1[i]) != hipSuccess) ms = 0.0f;
        cal_harvest(pc, i, ms);
    }
    (void)hipGetLastError();
    return cal_turn(pc);
}

// GEMX_PLAN_RECORD=<file>: every planned launch appends the pure layer's inputs and outputs as one line (tools/record_launch_plans.py;
// tests/golden/launch_plans.txt is such a file, replayed by tests/test_launch_plan_cpu.py)
inline void record_plan(const Facts &f, const Launch &l, const Choice &c, const Pace &p, size_t lds, double scale) {
    static const char *path = getenv("GEMX_PLAN_RECORD");
    if (path == nullptr || path[0] == 0) return;
    FILE *fh = fopen(path, "a");
    if (fh == nullptr) return;
    fprintf(fh, "%d %d %d %d %d %d %d %d %d %d %d", f.abytes, f.nht, f.nact_c, f.vt_bytes, f.prep_q, f.init_desc_bytes, (int)f.dq, (int)f.compact_l, (int)f.sync, (int)f.deep_built, (int)f.d3_built);
    for (int s = 0; s < NSHAPE; ++s) fprintf(fh, " %d %d %d", f.kernel[s] != nullptr ? 1 : 0, l.regs[s], l.occ[s]);
    fprintf(fh, " %lld %d %d %d %d %d %d %zu %d %d %d %d %d %d %d %d %d %.17g %.17g", (long long)l.blocks, l.K, l.n_cu, l.nout, l.delay, l.rw_n_ref, l.forced_shape, l.lds_max, (int)l.dq_processor,
            (int)l.need_full, (int)l.fast_step, (int)l.rinit, (int)l.lin_on, (int)l.reward, (int)l.half, (int)l.synth, (int)l.pace_default_on, l.pace_gbps, scale);
    fprintf(fh, " -> %d %d %d %zu %u %u %u %lld\n", c.shape, c.D, c.OW, lds, p.block_ticks, p.tail_ticks, p.tail_from, (long long)p.res);
    fclose(fh);
}

struct Plan {
    int shape, D, OW, threads;  // D == 0: no pipelined shape serves this launch
    size_t lds;
    Pace pace;
    const void *kernel;
    int cal_slot;      // >= 0: the event pair that times this launch (cal_begin / cal_end)
    int cal_state;     // gemx_handle::pace_cal_state of this launch
    double cal_scale;  // gemx_handle::pace_scale_last
};

// One fused rollout of K >= 2 steps through the pipelined kernel: the shape, its LDS bytes and the limiter's intervals.  The kernel's
// dynamic-LDS attribute is set when this returns GEMX_OK with out.D != 0.
inline int plan_rollout(gemx_handle *h, const Facts &f, const RolloutCall &call, bool need_full, bool fast_step, hipStream_t st, Plan &out) {
    Launch l = {};
    l.blocks = (h->n + BLOCK - 1) / BLOCK;
    l.K = call.K; l.n_cu = h->n_cu; l.nout = h->nout; l.delay = h->cfg.action_delay; l.rw_n_ref = h->rw_n_ref;
    l.forced_shape = h->pipe_shape;
    l.lds_max = h->lds_max;
    l.dq_processor = h->pf.dq_processor != 0; l.need_full = need_full; l.fast_step = fast_step; l.rinit = h->cfg.init_kind != GEMX_INIT_CONST;
    l.lin_on = h->pf.lin_on != 0; l.reward = call.reward != nullptr; l.half = call.half; l.synth = call.synth;
    l.pace_default_on = GEMX_PACE_DEFAULT_ON != 0;
    l.pace_gbps = h->pace_gbps;
    for (int s = 0; s <= 3; ++s) resolve_shape(h, f, l, s);
    const Choice c = choose_shape(f, l);
    out = Plan{c.shape, c.D, c.OW, waves_per_wg(c.shape) * BLOCK, 0, Pace{0u, 0u, 0xFFFFFFFFu, 0}, nullptr, -1, 0, 1.0};
    if (c.D == 0) return GEMX_OK;
    if (c.shape > 3) resolve_shape(h, f, l, c.shape);
    double target = open_loop_target(f, l);
    if (cal_eligible(l, c, h->pace_cal_on != 0, target)) {
        cal_start(h->pcal, cal_signature(l, c));
        CalTurn turn{-1, 0};
        if (h->pcal.chosen < 0 && !stream_capturing(st)) turn = cal_resolve(h);
        out.cal_slot = turn.slot;
        out.cal_scale = cal_scale(h->pcal, turn);
        out.cal_state = h->pcal.chosen >= 0 ? 2 : (turn.slot >= 0 ? 1 : 0);
        target *= out.cal_scale;
    }
    out.pace = pace_for(f, l, c, target);
    out.lds = lds_bytes(f, l, c.D);
    out.kernel = f.kernel[c.shape];
    record_plan(f, l, c, out.pace, out.lds, out.cal_scale);
    if (out.kernel == nullptr) return fail(GEMX_ERR_ARG, "internal: pipelined shape %d is not built for this solver", c.shape);
    if (!(h->pipe_attr_set & (1u << c.shape))) {
        GEMX_HIP_TRY(hipFuncSetAttribute(out.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_max));
        h->pipe_attr_set |= 1u << c.shape;
    }
    return GEMX_OK;
}
// the event pair around a calibration launch
inline void cal_begin(gemx_handle *h, const Plan &p, hipStream_t st) {
    if (p.cal_slot >= 0) (void)hipEventRecord((hipEvent_t)h->pcal.ev0[p.cal_slot], st);
}
inline void cal_end(gemx_handle *h, const Plan &p, hipStream_t st) {
    if (p.cal_slot >= 0 && hipEventRecord((hipEvent_t)h->pcal.ev1[p.cal_slot], st) != hipSuccess) { h->pcal.ev_cand[p.cal_slot] = -1; (void)hipGetLastError(); }
}
}  // namespace plan
}  // namespace gemx
#endif  // __HIPCC__
