// gemx_unit_host.hpp -- the host code every unit repeats.  A unit is a shared object built once per (system, converter unit) and loaded
// with dlopen (gemx_inst.hip, gemx_envparams.hip, gemx_episodic.hip, gemx_policy.hip, gemx_policy_complete.hip); a unit links nothing of
// libgemx.so, so each one carries its own copy of what stands here.  Host code only: no kernel and no device function.
//   fail(), unit_init            the error sink and the body of every gemx_*_unit_init
//   dispatch_load_solver         a side unit's four (load, solver) pairs -> its launcher template
//   ensure_linmap                the once-per-handle build of the one-step map: the stepping units' launch_advance_t and the
//                                episodic-family launchers all call this one
//   fill_unit_kargs              the KArgs of a single-wave side-unit launch
// (How a fused rollout of the stepping units is launched -- shape, LDS, rate limiter -- is gemx_launch_plan.hpp's.)
#pragma once
#include <cstdarg>
#include <cstdio>

#include "gemx_kernels.hpp"

namespace gemx {
static void (*g_set_error)(const char *) = nullptr;
int fail(int code, const char *fmt, ...) {  // gemx_common.hpp declares it; in a unit it formats and hands the text to libgemx.so's gemx_last_error()
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (g_set_error != nullptr) g_set_error(buf);
    return code;
}
// GEMX_OK if this unit was compiled against the caller's handle layout and ABI
inline int unit_init(unsigned long long handle_bytes, int abi, void (*set_error)(const char *)) {
    if (handle_bytes != (unsigned long long)sizeof(gemx_handle) || abi != GEMX_ABI_VERSION) return GEMX_ERR_ARG;
    g_set_error = set_error;
    return GEMX_OK;
}

// The (load, solver) pairs the side units are built for.  `launch` is called with a LoadSolver<LD, SV> value whose type carries the pair:
//     dispatch_load_solver(h, "episodic rollout", [&](auto ls) { return launch_tl_t<SYS, CONV, decltype(ls)::LOAD, decltype(ls)::SOLVER>(h, c, st); });
template <int LD, int SV> struct LoadSolver { static constexpr int LOAD = LD, SOLVER = SV; };
template <class F> static int dispatch_load_solver(const gemx_handle *h, const char *what, F &&launch) {
    const int ld = h->cfg.load_kind, sv = h->cfg.solver_kind;
    if (ld == GEMX_LOAD_CONST_SPEED && sv == GEMX_SOLVER_EULER) return launch(LoadSolver<GEMX_LOAD_CONST_SPEED, GEMX_SOLVER_EULER>{});
    if (ld == GEMX_LOAD_CONST_SPEED && sv == GEMX_SOLVER_RK4) return launch(LoadSolver<GEMX_LOAD_CONST_SPEED, GEMX_SOLVER_RK4>{});
    if (ld == GEMX_LOAD_POLY_STATIC && sv == GEMX_SOLVER_EULER) return launch(LoadSolver<GEMX_LOAD_POLY_STATIC, GEMX_SOLVER_EULER>{});
    if (ld == GEMX_LOAD_POLY_STATIC && sv == GEMX_SOLVER_RK4) return launch(LoadSolver<GEMX_LOAD_POLY_STATIC, GEMX_SOLVER_RK4>{});
    return fail(GEMX_ERR_ARG, "%s: load/solver combination %d/%d is not built (EulerSolver and RK4Solver only)", what, ld, sv);
}

// Once per handle: the electrical subsystem's one-step map (constant-speed loads), for a handle WITHOUT a parameter table (the map is
// built for one parameter set).  THE one place that builds it: launch_advance_t and the episodic-family launchers all come here (the side
// units are fp32 without dead time, the defaults).
// (random initialisers that draw OMEGA per episode keep the stage-by-stage solver.  Round 5: only those -- a random MOTOR initialiser
// beside a constant-speed load leaves omega at init[0], the map stays valid, and the kernels check every lane's omega at launch
// anyway (lin_usable); until then every random-initialiser handle ran the full Runge-Kutta stages, 2.2 x the integrator time)
template <int SYS, int LOAD, int SOLVER, bool IL = false, class R = float> static int ensure_linmap(gemx_handle *h, hipStream_t st, int *linmap_built) {
    if (h->envp != nullptr || h->linmap_state != 0) return GEMX_OK;
    if constexpr (linable<SYS, LOAD, SOLVER, IL, R>()) {
        const bool capturing = stream_capturing(st);
        const bool omega_drawn = h->cfg.init_kind != GEMX_INIT_CONST && h->cfg.init_lo[0] < h->cfg.init_hi[0];
        if (omega_drawn || (h->cfg.solver_flags & GEMX_SOLVER_ADAPTIVE) || h->cfg.solver_nsteps != 1) {  // (error control, sub-steps: stage by stage)
            h->linmap_state = -1;
        } else if (!capturing) {
            // built and COMPLETED here, so that later launches on any stream (or from a captured graph) find it; a first launch
            // that is itself being captured into a graph goes without the map and leaves the attempt to the next eager launch
            hipLaunchKernelGGL((linmap_kernel<SYS, SOLVER, R>), dim3(1), dim3(64), 0, st, params_of<double>(h), (R *)h->linmap_dev);
            GEMX_HIP_TRY(hipGetLastError());
            GEMX_HIP_TRY(hipStreamSynchronize(st));
            h->linmap_state = 1;
            h->pf.lin_on = 1;
            if (linmap_built != nullptr) *linmap_built = 1;
        }
    } else {
        h->linmap_state = -1;
    }
    return GEMX_OK;
}

// The KArgs of a single-wave side-unit launch: the handle's state, K control steps, every step's row to `obs` and its done byte to `done`.
// tab: the view of a handle with a parameter table.  The actions and the fused reward's fields are the caller's.
template <int LOAD> static void fill_unit_kargs(KArgs<float> &a, const gemx_handle *h, bool tab, int K, void *obs, uint8_t *done) {
    using R = float;
    memset(&a, 0, sizeof(a));
    a.P = h->pf;
    if (tab) {
        a.P.lin_on = 0;  // (never the one-step map: it is built for one parameter set)
        a.P.kink_split = ((h->cfg.solver_flags & GEMX_SOLVER_SPLIT_KINKS) && LOAD == GEMX_LOAD_POLY_STATIC) ? 1 : 0;  // the FLAG: ep_apply decides per lane
    }
    a.P.errw = h->err;
    a.state = (R *)h->state;
    a.angle = (Angle<R>::T *)h->angle;
    a.sw = h->sw;
    a.obs = (R *)obs;
    a.done = done;
    a.err = h->err;
    a.N = h->n;
    a.K = K;
    a.obs_every = 1;
    a.S = 1;
    a.D = 1;
}
}  // namespace gemx
