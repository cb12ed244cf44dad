/*
 * gemx.h -- C ABI of the MI355X-native batched physical-system stepper for gym-electric-motor (GEM).
 *
 * The reference (upb-lea/gym-electric-motor 3.0.2) is pure Python and has no FFI: its replaceable seam is
 * the plugin base class gym_electric_motor.core.PhysicalSystem (core.py:589-705) whose two hot methods are
 *     simulate(action) -> state / limits        (core.py:687-698; SCMLSystem.simulate physical_systems.py:171-203,
 *                                                SynchronousMotorSystem.simulate 487-525,
 *                                                SquirrelCageInductionMotorSystem.simulate 771-814)
 *     reset()          -> state / limits        (core.py:678-685; physical_systems.py:256-287, 527-561, 816-847)
 * This library is what a GEM maintainer binds with ctypes behind that seam (INTEGRATION.md shows the stub):
 * one handle = N independent SCML systems (supply -> converter -> motor ODE + load ODE -> normalised state,
 * constraint-violation done flag) advanced in lockstep by hand-written gfx950 kernels.
 *
 * Conventions
 *  - plain pointers and sizes only; all `*_dev` pointers are DEVICE pointers owned by the caller
 *    (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - every call returns GEMX_OK (0) or a negative gemx_status; the message is in gemx_last_error().
 *    Nothing throws across the boundary.  Calls on one handle are not thread-safe; launches are asynchronous.
 *  - real type R = float (dtype GEMX_F32, default; the product path) or double (GEMX_F64, diagnostic).
 *  - there is NO CPU fallback: without a HIP device gemx_create() fails with GEMX_ERR_DEVICE.
 */
#ifndef GEMX_H
#define GEMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEMX_ABI_VERSION 9 /* 2: GEMX_MAX_OUT 16 -> 24 (DFIM system, 24 states); 3: gemx_config.solver_flags; 4: solver_rtol / solver_atol; 5: init_flux_mode / init_flux;
                            * 6: gemx_get_aux_state / gemx_set_aux_state / gemx_aux_state_bytes, gemx_reset_again; reset counters stay at 1 after gemx_create;
                            *    + gemx_rollout_synthetic / gemx_synthetic_actions, gemx_set_rate_limiter (new entry points only);
                            * 7: gemx_config.env_base / gemx_refgen_config.env_base: every device random stream is keyed by the GLOBAL env index
                            *    env_base + i (shards of one job draw what the unsharded job draws); gemx_rollout_half; gemx_config.solver_atol_omega; GEMX_SOLVER_ADAPTIVE
                            *    honours GEMX_SOLVER_SPLIT_KINKS; the initial-state streams are Threefry-4x32-12 (were Philox4x32-10: other draws from
                            *    the same seed, same distributions); one unit library per (system, converter, dtype), loaded by gemx_create;
                            * 8: gemx_refgen_step (new entry point: one fused generator step per launch); the generators' step index moved from the host
                            *    into device memory (gemx_refgen_rollout: same bits);
                            * 9: gemx_refgen_kinds_config / gemx_refgen_create_kinds / gemx_refgen_get_params (new struct and entry points only: a kind per
                            *    generator column -- Wiener, Laplace, sinusoidal, step, triangular, sawtooth, constant; gemx_refgen_config handles: same bits);
                            *    + gemx_episode_config / gemx_episode_* (new struct and entry points only: episode time limit and statistics)
                            *    + gemx_returns_config / gemx_returns_rows (new struct and entry point only: discounted returns and GAE over stored rows) */
#define GEMX_MAX_ODE 8  /* ODE state length incl. omega and the angle      */
#define GEMX_MAX_OUT 24 /* system-state (observation) length               */
#define GEMX_MODEL_ROWS 5
#define GEMX_MODEL_COLS 11

typedef enum gemx_status {
    GEMX_OK = 0,
    GEMX_ERR_ARG = -1,     /* invalid argument / unsupported configuration (cf. reference asserts, converters.py:204-206) */
    GEMX_ERR_DEVICE = -2,  /* no HIP device / HIP runtime error                                                        */
    GEMX_ERR_ALLOC = -3
} gemx_status;

/* SCML system class: DcMotorSystem / SynchronousMotorSystem / SquirrelCageInductionMotorSystem */
typedef enum {
    GEMX_SYS_DC_PERMEX = 0, /* DcMotorSystem + DcPermanentlyExcitedMotor                                   */
    GEMX_SYS_SYNC = 1,      /* SynchronousMotorSystem (PMSM, SynRM)                                         */
    GEMX_SYS_SCIM = 2,      /* SquirrelCageInductionMotorSystem                                             */
    GEMX_SYS_DC_SERIES = 3, /* DcMotorSystem + DcSeriesMotor (electric_motors/dc_series_motor.py)           */
    GEMX_SYS_DC_SHUNT = 4,  /* DcMotorSystem + DcShuntMotor  (electric_motors/dc_shunt_motor.py)            */
    GEMX_SYS_DC_EXTEX = 5,  /* DcMotorSystem + DcExternallyExcitedMotor (dc_externally_excited_motor.py)     */
    GEMX_SYS_EESM = 6,      /* ExternallyExcitedSynchronousMotorSystem (physical_systems.py:564-691)         */
    GEMX_SYS_DFIM = 7       /* DoublyFedInductionMotorSystem (physical_systems.py:850-1113)                  */
} gemx_system_kind;
/* ContFourQuadrantConverter (converters.py:438-495), FiniteB6BridgeConverter (743-839), ContB6BridgeConverter (842-911),
 * FiniteFourQuadrantConverter (313-368; DC systems, actions 0..3).
 * Kinds 4..9 are Cont/FiniteMultiConverter (converters.py:498-740) holding exactly the two sub-converters of the
 * reference's ExtExDc envs (2 x 4QC: armature, excitation), EESM envs (B6 stator + 4QC excitation) and DFIM envs
 * (2 x B6: stator, rotor).
 *   continuous actions: the sub-converters' actions concatenated, A = 2 | 4 | 6;
 *   discrete actions:   ONE uint8 = a_0 + n_0 * a_1, the flat index of the reference's MultiDiscrete([n_0, n_1])
 *                       action [a_0, a_1] (n_0 = 4 | 8), i.e. 0..15 | 0..31 | 0..63.
 * The two sub-converters share interlocking_time; EESM handles refuse interlocking_time > 0 (the reference's
 * dead-time branch for this system cannot execute, physical_systems.py:634). */
typedef enum {
    GEMX_CONV_CONT_4QC = 0, GEMX_CONV_FINITE_B6 = 1, GEMX_CONV_CONT_B6 = 2, GEMX_CONV_FINITE_4QC = 3,
    GEMX_CONV_CONT_2X4QC = 4, GEMX_CONV_FINITE_2X4QC = 5, GEMX_CONV_CONT_B6_4QC = 6, GEMX_CONV_FINITE_B6_4QC = 7,
    GEMX_CONV_CONT_2XB6 = 8, GEMX_CONV_FINITE_2XB6 = 9
} gemx_converter_kind;
/* ConstantSpeedLoad (constant_speed_load.py), PolynomialStaticLoad (polynomial_static_load.py) */
typedef enum { GEMX_LOAD_CONST_SPEED = 0, GEMX_LOAD_POLY_STATIC = 1 } gemx_load_kind;
/* EulerSolver(nsteps) (solvers.py:79-136); classical RK4 (not in the reference); one fixed Dormand-Prince-5
 * step per segment (what the reference's default scipy dopri5 does whenever its trial step is accepted) */
typedef enum { GEMX_SOLVER_EULER = 0, GEMX_SOLVER_RK4 = 1, GEMX_SOLVER_DP5 = 2 } gemx_solver_kind;
/* gemx_config.solver_flags.  GEMX_SOLVER_SPLIT_KINKS: with a PolynomialStaticLoad every (sub-)step is corrected for the kinks of the
 * load torque at |omega| = a * tau_decay / J (polynomial_static_load.py:87-92), where a fixed step loses its order and the reference's
 * default solver (scipy dopri5, solvers.py:139-184) rejects and splits its steps.  ABI >= 5 libraries do it in ONE pass of the scheme: the
 * saturation term is replaced by the affine piece of the region the mid-step omega is predicted in (a smooth system: the scheme keeps
 * its order), and the defect -- the time integral of (true - modelled) saturation along the step's own omega path, a cubic through both
 * ends with the first and last stage's slopes -- is added to omega in closed form.  (Earlier libraries cut the step at the predicted
 * crossings, up to three passes; the flag kept its name.)  Worst observed error against the reference's dopri5 trajectories over every
 * recorded PolynomialStaticLoad run (fp32): 7.9e-5 without, 6.3e-6 with.  Ignored for a ConstantSpeedLoad. */
#define GEMX_SOLVER_SPLIT_KINKS 1
/* GEMX_SOLVER_ADAPTIVE (with GEMX_SOLVER_DP5 only): error-controlled sub-stepping -- what the reference's default solver does
 * (ScipyOdeSolver('dopri5'), solvers.py:139-184: scipy's DOPRI5 with rtol 1e-6, atol 1e-12).  Every integration segment is tried as one
 * Dormand-Prince 5(4) step; where the embedded error estimate, in scipy's norm sqrt(mean((err_i / (solver_atol + solver_rtol
 * max(|y_i|, |y_i new|)))^2)), exceeds 1 the lane cuts its step (h <- h clamp(0.9 err^-1/5, 0.2, 1)) and goes on with steps chosen the same
 * way until the segment is through; the other lanes of its wave wait.  The step size a lane ends a control step with is CARRIED to its next
 * one (a state row, like DOPRI5's WORK(7); cleared by a reset, part of the checkpoint blob).  Still not scipy's step sequence (no PI term,
 * fp32 error estimates), so not its bits -- the same tolerance.  Floor: a step of 1/1024 of the segment is taken whatever its estimate and
 * raises GEMX_ERRFLAG_TOLERANCE.  Takes precedence over solver_nsteps; the one-step map and the small-batch DC kernel are not used.
 * Together with GEMX_SOLVER_SPLIT_KINKS (ABI 7; PolynomialStaticLoad): every attempt integrates the smooth model system of the kink
 * correction above and an accepted sub-step adds the kink's defect to omega in closed form, so that the error estimate never sees the
 * kink.  Without it a lane that crosses |omega| = a tau_decay / J cuts its step five to eight times, and under random actions some lane of
 * a 64-lane wave does in most control steps: 4.7 attempts per control step and wave against 1.8 (profiles/r06_wave_step_statistics.md). */
#define GEMX_SOLVER_ADAPTIVE 2
typedef enum { GEMX_F32 = 0, GEMX_F64 = 1 } gemx_dtype;
/* observation layout: [N, S_out] rows per env (the reference contract) or [S_out, N] */
typedef enum { GEMX_OBS_AOS = 0, GEMX_OBS_SOA = 1 } gemx_obs_layout;
typedef enum { GEMX_INIT_CONST = 0, GEMX_INIT_UNIFORM = 1, GEMX_INIT_GAUSSIAN = 2 } gemx_init_kind;
typedef enum { GEMX_SUPPLY_IDEAL = 0, GEMX_SUPPLY_RC = 1 } gemx_supply_kind;
typedef enum { GEMX_ACT_ABC = 0, GEMX_ACT_DQ_SPACE = 1, GEMX_ACT_DQ_PROCESSOR = 2 } gemx_action_frame;
#define GEMX_MAX_DELAY 8

/* Flat description of ONE SCML system shared by all N envs of a handle (parameters are uniform across envs:
 * they travel as kernel arguments -> SGPRs, 0 bytes of HBM traffic per env). */
typedef struct gemx_config {
    int32_t struct_size; /* = sizeof(gemx_config), ABI check */
    int32_t abi_version; /* = GEMX_ABI_VERSION */
    int32_t system_kind, converter_kind, load_kind;
    int32_t solver_kind, solver_nsteps; /* nsteps: sub-steps per integration segment (EulerSolver(nsteps)); >= 1 */
    int32_t solver_flags;               /* GEMX_SOLVER_* bits, 0 = plain fixed steps */
    int32_t dtype, obs_layout;
    int32_t auto_reset;    /* 1: an env whose step ended `done` restarts from init_state on its next step */
    uint32_t limit_mask;   /* LimitConstraint:   done if any |obs[i]| > 1      over set bits (constraints.py:55-58) */
    uint32_t squared_mask; /* SquaredConstraint: done if sum obs[i]^2 > 1      over set bits (constraints.py:96-98) */
    /* Action path in front of simulate() (continuous B6 converters of SYNC / SCIM / EESM systems only for the dq frames):
     *   GEMX_ACT_ABC          actions are the converter's own (default);
     *   GEMX_ACT_DQ_SPACE     system built with control_space='dq' (physical_systems.py:423-435, 491-492, 777-778):
     *                         A = 2, abc = T32(Q(a_dq, eps)) with the step-start (field) angle; SYNC and SCIM;
     *   GEMX_ACT_DQ_PROCESSOR DqToAbcActionProcessor around the system (physical_system_wrappers/
     *                         dq_to_abc_action_processor.py:100-114; EESM 158-175): A = 2 (SYNC) | 3 (EESM: u_d, u_q, u_e),
     *                         abc = T32(Q(a_dq, eps + (0.5 + action_delay) * tau * omega * p)).
     * action_delay = DeadTimeProcessor(steps) INSIDE the dq processor (dead_time_processor.py:63-85): the converter
     * receives the action submitted action_delay steps earlier; the per-env FIFO is refilled by every reset with
     * action_delay_reset below -- zeros, the reference's default reset_actions, or the ONE action a custom
     * `reset_action` callable returns action_delay copies of (dead_time_processor.py:27-50).  Any system / converter;
     * 0 = none, max GEMX_MAX_DELAY. */
    int32_t action_frame;
    int32_t action_delay;
    /* Supply: GEMX_SUPPLY_IDEAL (IdealVoltageSupply, voltage_supplies.py:60-72: u_sup = u_nominal) or GEMX_SUPPLY_RC
     * (RCVoltageSupply, 75-123): one extra state per env, advanced at the start of every control step by one explicit Euler
     * step of du/dt = (u_nominal - u - supply_r * i_sup) / (supply_r * supply_c) over the time since the previous step, with
     * i_sup = converter.i_sup(i_in) (converters.py:289-298, 429-435, 366-368, 493-495, 837-839, 909-911) evaluated, as the
     * reference does, on the NEW duty cycles of a continuous converter / the PREVIOUS step's final switching state of a
     * finite one.  reset() reloads the capacitor (u = u_nominal).  Not available for the finite EESM converter. */
    int32_t supply_kind;
    /* Initial ODE state (electric_motor.py:150-257, mechanical_load.py:100-160).  GEMX_INIT_CONST: init_state below.
     * GEMX_INIT_UNIFORM / GEMX_INIT_GAUSSIAN: every reset (gemx_reset and the in-kernel auto-reset) draws each ODE state j with
     * init_lo[j] < init_hi[j] anew -- uniformly in [lo, hi], or from a normal(init_mu[j], init_sigma[j]) truncated to [lo, hi]
     * (scipy.stats.truncnorm in the reference) -- from a counter-based stream (Threefry-4x32 with 12 rounds since ABI 7, Philox4x32-10
     * before: Salmon et al., SC'11) keyed by `seed` and indexed by (env_base + env, number of resets of that env, j); states with lo == hi
     * keep init_state[j].  numpy's PCG64 streams of the reference
     * cannot be reproduced on a device: parity is distributional (tests/test_gpu_parity.py), and exact for the state -> reset
     * observation map.  Every system; the load's omega for any system with a PolynomialStaticLoad.
     * Induction machines (SCIM, DFIM; ABI 5): init_flux_mode = 1 re-derives the bounds of the two flux states at EVERY reset as the
     * reference does (induction_motor.py:174-185, 250-285; squirrel_cage_induction_motor.py:146-157; doubly_fed_induction_motor.py:
     * 154-165): a field angle eps_mag ~ U(-pi, pi) is drawn, psi_d_max = init_flux[0] (= l_m * nominal i_sd) if this reset's omega
     * is 0, else 0.9 * clip((p omega sigma l_s i_d + (r_s + r_r l_mr^2) i_q + u_q_max + l_mr u_rq_max) / (-p omega l_mr), 0,
     * |l_m i_d|) with (i_d, i_q) = Q^-1(i_s alpha/beta OF THE PREVIOUS RESET'S DRAW -- the configured constants at the first reset --,
     * eps_mag) (the reference reads the motor's stale `_initial_states` there), and the flux states are drawn from
     * +-psi_d_max * (|cos eps_mag|, |sin eps_mag|) clipped to [init_lo, init_hi] of their slots (the user's `interval`;
     * +-HUGE_VAL = none).  init_flux = [l_m * i_sd_nominal, p, sigma * l_s, r_s + r_r * l_mr^2, u_q_max + l_mr * u_rq_max, l_mr, l_m, 0]. */
    int32_t init_kind;
    int32_t init_flux_mode;
    double init_flux[8];
    uint64_t seed;
    /* GLOBAL index of this handle's env 0 (ABI 7).  Every device-side random stream -- the initialisers above, the synthetic actions of
     * gemx_rollout_synthetic / gemx_synthetic_actions -- is a pure function of (seed, env_base + i, ...): a job sharded over W handles
     * (ranks / GPUs) with env_base = the shard's first env draws, env by env, exactly what ONE handle over all envs draws, as every env
     * object of the reference owns its own branch of the seed sequence (core.py:373-385, physical_systems.py:164-169,
     * random_component.py:60-87).  0 for a lone handle; >= 0. */
    int64_t env_base;
    double init_lo[GEMX_MAX_ODE], init_hi[GEMX_MAX_ODE], init_mu[GEMX_MAX_ODE], init_sigma[GEMX_MAX_ODE];
    double supply_r, supply_c;
    /* DeadTimeProcessor reset action, in the action space of the system the processor wraps: continuous converter actions
     * [0 .. A_conv - 1] (A_conv = 2 for control_space='dq'), or [0] = the flat index of a discrete action */
    double action_delay_reset[6];
    double solver_rtol, solver_atol; /* GEMX_SOLVER_ADAPTIVE: relative / absolute (state units) tolerance; 0 = 1e-6 / 1e-9 */
    /* GEMX_SOLVER_ADAPTIVE, systems whose omega is a state (PolynomialStaticLoad): the absolute tolerance of OMEGA in rad/s (ABI 7).
     * 0 = solver_atol x limits[omega], i.e. solver_atol in NORMALISED units -- 1e-9 of the speed range (4e-7 rad/s), not 1e-9 rad/s: a
     * speed-control episode starts at omega = 0, where the relative term vanishes and an absolute tolerance of 1e-9 rad/s (2e-12 of the
     * range, below anything an observation can show) makes lanes cut steps that no result depends on -- with 64 lock-stepped lanes some lane
     * does so in most control steps (BASELINE config 4: 1.7 attempts per control step and wave instead of 1.0; against scipy's dopri5 runs
     * 4e-6 either way: profiles/r06_wave_step_statistics.md).  solver_atol itself restores the behaviour of ABI <= 6. */
    double solver_atol_omega;
    double tau;               /* control step, PhysicalSystem.tau */
    double interlocking_time; /* converter dead time, converters.py:35-41; must be < tau */
    double u_nominal;         /* IdealVoltageSupply.u_nominal, voltage_supplies.py:60-72 */
    /* motor._model_constants zero-padded to 5x11, row-major; feature order as in the reference:
     * DC    (1x3) [omega, i, u]                                  dc_permanently_excited_motor.py:71-84
     * SERIES(1x3) [i, omega*i, u]                                dc_series_motor.py:68-83
     * SHUNT (2x5) [i_a, i_e, omega*i_e, u_a, u_e] (u_a = u_e = u) dc_motor.py:96-127, dc_shunt_motor.py:72-74
     * EXTEX (2x5) [i_a, i_e, omega*i_e, u_a, u_e]                 dc_motor.py:96-127
     * SYNC  (3x7) [omega, i_d, i_q, u_d, u_q, omega*i_d, omega*i_q]  synchronous_motor.py:143-168
     * EESM  (4x10)[omega, i_d, i_q, i_e, u_d, u_q, u_e, omega*i_d, omega*i_q, omega*i_e]
     *                                                            externally_excited_synchronous_motor.py:69-113
     * SCIM  (5x11)[omega, i_a, i_b, psi_a, psi_b, omega*psi_a, omega*psi_b, u_sa, u_sb, u_ra, u_rb] induction_motor.py:187-217
     *             (SCIM: the u_r columns are ignored -- zero rotor voltage; DFIM: same matrix, u_r columns live) */
    double model[GEMX_MODEL_ROWS * GEMX_MODEL_COLS];
    /* torque: DC T = tc[0]*i ; SYNC T = (tc[0] + tc[1]*i_d)*i_q ; SCIM T = tc[0]*(psi_a*i_b - psi_b*i_a) ;
     * SERIES T = tc[0]*i*i ; SHUNT / EXTEX T = tc[0]*i_a*i_e ; EESM T = (tc[0]*i_e + tc[1]*i_d)*i_q ;
     * DFIM: T as SCIM, plus the rotor-current reconstruction i_r = tc[2]*psi_r - tc[3]*i_s
     *       (tc[2] = 1/l_r, tc[3] = l_m/l_r; calculate_rotor_current, physical_systems.py:931-946) */
    double torque_coef[4];
    double j_total;                    /* load.j_total (j_load + j_rotor), mechanical_load.py:35-41 */
    double load_a, load_b, load_c;     /* PolynomialStaticLoad parameters */
    double tau_decay;                  /* PolynomialStaticLoad.tau_decay (1e-3) */
    double limits[GEMX_MAX_OUT];       /* PhysicalSystem.limits, physical_systems.py:105-113 */
    double init_state[GEMX_MAX_ODE];   /* ODE state after reset: [omega, motor states..., epsilon] */
} gemx_config;

typedef struct gemx_handle gemx_handle;

int gemx_abi_version(void);
int gemx_sizeof_config(void);
const char *gemx_last_error(void);
/* Diagnostics: per-wave cycle counts of the pipelined kernel's last launch (integrator / output / loader waves of workgroups 0 and
 * 37), filled only by a library compiled with -DGEMX_TIMING (all zeros otherwise); read by tools/pipe_timing_probe.py. */
int gemx_debug_read(gemx_handle *h, unsigned long long *out, int n);
/* number of visible HIP devices (0 => the library cannot run; callers must fail loudly) */
int gemx_device_count(void);

/* Create N envs on `device`, all at the reset state.  Replaces SCMLSystem.__init__ (physical_systems.py:54-103). */
int gemx_create(const gemx_config *cfg, int64_t n_envs, int device, gemx_handle **out);
int gemx_destroy(gemx_handle *h);

int gemx_n_envs(const gemx_handle *h, int64_t *n);
int gemx_n_ode(const gemx_handle *h);    /* S_ode: 2 | 3 | 4 | 5 | 6  */
int gemx_n_out(const gemx_handle *h);    /* S_out: 5 | 6 | 7 | 14 | 16 | 24 */
int gemx_n_action(const gemx_handle *h); /* A: 1 | 2 | 3 | 4 | 6 (1 for every discrete converter; dq frames: 2 | 3) */
int gemx_action_itemsize(const gemx_handle *h); /* 1 (uint8 discrete) | sizeof(R) */
/* normalised state returned by reset() for the configured constant initialiser, host doubles [S_out] */
int gemx_reset_observation(const gemx_handle *h, double *obs_host);

/* PhysicalSystem.reset(): envs with mask[i] != 0 (all if mask_dev == NULL) go back to init_state, their step
 * counter to 0; the converter switching state survives, as in the reference (converters.py:45-54).
 * obs_out_dev (optional, layout per config) receives the reset observation for the reset envs. */
int gemx_reset(gemx_handle *h, const uint8_t *mask_dev, void *obs_out_dev, void *stream);
/* The same reset WITHOUT drawing anew: with random initialisers (init_kind != GEMX_INIT_CONST) the masked envs go back to the state
 * their current episode started from (reset counters untouched); with constant initialisers identical to gemx_reset.  gemx_create leaves
 * every env in draw #1 with its counter at 1, so a binding obtains the construction-time observation rows with this call and the first
 * in-kernel auto-reset (or gemx_reset) of an env is draw #2 -- never draw #1 twice. */
int gemx_reset_again(gemx_handle *h, const uint8_t *mask_dev, void *obs_out_dev, void *stream);

/* PhysicalSystem.simulate() for all N envs: one control step.
 *   actions_dev : [N, A] R for continuous converters, [N] uint8 for finite ones (0..7 Finite-B6C, 0..3 Finite-4QC)
 *   obs_out_dev : [N, S_out] R (AoS) or [S_out, N] R (SoA); 16-byte aligned
 *   done_out_dev: [N] uint8 (may be NULL when no constraint is configured)                                    */
int gemx_step(gemx_handle *h, const void *actions_dev, void *obs_out_dev, uint8_t *done_out_dev, void *stream);

/* K fused control steps in ONE launch (ODE state stays in registers between steps).
 *   actions_dev [K, N, A]; obs_out_dev [K, N, S_out] (or [K, S_out, N]); done_out_dev [K, N].
 *   obs_every: 1 = write every step; 0 = write only the last step (obs_out_dev [N,S_out], done_out_dev [N] =
 *   OR over the K steps).                                                                                     */
int gemx_rollout(gemx_handle *h, const void *actions_dev, int32_t K, void *obs_out_dev, uint8_t *done_out_dev,
                 int32_t obs_every, void *stream);

/* Reward fused into the rollout: WeightedSumOfErrors.reward (reward_functions/
 * weighted_sum_of_errors.py:125-129) with the caller's reference tensor,
 *   r = (1 - v) * (bias - sum_i weight[i] * (|s_i - ref_i| / state_length[i]) ** power[i]) + v * violation_reward,
 * v = this step's done flag (ConstraintMonitor violation degree 0 | 1, core.py:348-350); ref_i = refs[.., j] for the n_ref
 * referenced states ref_index[j] (the generator's referenced_states, in ascending state order), 0 for all others.
 * weight / power / state_length are full-length state arrays exactly as the reference's reward function holds them
 * (_reward_weights, _n, _state_length = state_space.high - low). */
#define GEMX_MAX_REF 4
typedef struct gemx_reward_config {
    int32_t struct_size; /* = sizeof(gemx_reward_config) */
    int32_t n_ref;       /* 0..GEMX_MAX_REF columns of the reference tensor */
    int32_t ref_index[GEMX_MAX_REF];
    double weight[GEMX_MAX_OUT], power[GEMX_MAX_OUT], state_length[GEMX_MAX_OUT];
    double bias, violation_reward;
} gemx_reward_config;
/* Install (rc != NULL) or remove (NULL) the reward function of a handle. */
int gemx_set_reward(gemx_handle *h, const gemx_reward_config *rc);
/* SYNTHETIC random-action rollouts without an action tensor ("actions ... can be generated on-device"): the action of env e at
 * stream position t = step0 + k is a pure function of (seed, e, t, component) -- continuous entries uniform on (-1, 1), discrete indices
 * uniform over the converter's action set (the flat index for MultiDiscrete) -- generated inside the launch (fp32, K >= 2, the conditions
 * of the pipelined kernel; GEMX_ERR_ARG otherwise).  gemx_synthetic_actions writes the SAME stream into a tensor ([K, N, A] R | [K, N] uint8),
 * for policies / tests / the paths gemx_rollout_synthetic does not serve: gemx_rollout on that tensor gives the same bits. */
int gemx_rollout_synthetic(gemx_handle *h, uint64_t seed, uint32_t step0, int32_t K, void *obs_out_dev, uint8_t *done_out_dev, void *stream);
int gemx_synthetic_actions(gemx_handle *h, uint64_t seed, uint32_t step0, int32_t K, void *actions_out_dev, void *stream);

/* gemx_rollout with a NARROW action tensor (ABI 7): actions_half_dev [K, N, A] IEEE half (continuous converters, fp32 handles, K >= 2;
 * observations of every step).  A policy's duty cycles need no more than eleven bits; from 32768 envs on the launches of the continuous
 * converters are bound by the write path's tolerance for the action stream read between the row stores, and half the read
 * bytes is the one lever a tensor-fed rollout has.  The values are widened to fp32 while they are staged: the results are, bit for bit, those
 * of gemx_rollout on the same values as fp32 (the reference clips and uses float64 duty cycles: converters.py:144-158, 888-903; the
 * quantisation of a half, 2^-11 relative, is the caller's to accept). */
int gemx_rollout_half(gemx_handle *h, const void *actions_half_dev, int32_t K, void *obs_out_dev, uint8_t *done_out_dev, void *stream);

/* The large-batch RATE LIMITER of the fused rollout (more workgroups than CUs: every workgroup is held to one block of rows per interval,
 * because this chip's write path delivers more when it is offered slightly less than it can take -- DESIGN.md 4.1).  Results never depend
 * on it, only the rate.  mode 0: off; 1: open loop at the built-in target of the launch's family and size; 2: closed loop (the default on a
 * whole gfx950: each handle times its own launches with HIP events and keeps the best of a bracket around that target, or none).
 * target_gbps > 0 replaces the built-in target (algorithmic GB/s, chip-wide; then open loop); <= 0 keeps it.  The environment variables
 * GEMX_PACE_GBPS / GEMX_PACE_CAL set the same two things for every handle at gemx_create; this call overrides them for one handle
 * (e.g. several handles sharing the chip, a partitioned device: mode 0).  Forgets the handle's calibration. */
int gemx_set_rate_limiter(gemx_handle *h, int32_t mode, double target_gbps);

/* gemx_rollout (obs_every = 1) that additionally reads refs_dev [K, N, n_ref] (R) and writes reward_out_dev [K, N] (R). */
int gemx_rollout_reward(gemx_handle *h, const void *actions_dev, int32_t K, const void *refs_dev, void *obs_out_dev,
                        uint8_t *done_out_dev, void *reward_out_dev, void *stream);

/* Device-side reference generation: N x n_ref independent WienerProcessReferenceGenerator streams
 * (reference_generators/wiener_process_reference_generator.py:30-49 over subepisoded_reference_generator.py:66-119, combined as
 * multiple_reference_generator.py:77-92 does): sub-episodes of int(U(episode_len_lo, episode_len_hi)) steps, per sub-episode
 * sigma = 10 ** U(log10 sigma_lo, log10 sigma_hi), value += N(0, sigma) per step clipped to [margin_lo, margin_hi]; a reset draws the
 * initial value from U(initial_lo, initial_hi) and starts a new sub-episode.  Counter-based Philox4x32-10 streams keyed by `seed`:
 * chunked generation == one-shot generation; parity with the reference's numpy streams is distributional.
 *   gemx_refgen_rollout(r, done, K, refs): refs[k, env, j] = reference the reward of control step k is computed against (what the agent
 *   saw as "next reference" before acting); done[k, env] != 0 (optional, the physics rollout's done tensor) resets that env's generators
 *   after step k, as `if terminated: env.reset()` does.  The tensor feeds gemx_rollout_reward directly.
 *   gemx_refgen_step(r, done, refs) (ABI 8): one env-shell step of the generators in ONE launch -- the generators of envs with
 *   done[env] != 0 (NULL: none) are reset, then every generator advances by one step; refs [N, n_ref] (R) receives the new values.  K calls
 *   with the masks done[k-1] (none for the first) produce, row for row and bit for bit, what one gemx_refgen_rollout(K, done) of an
 *   identically configured and seeded handle produces, and the two may be mixed on one handle in any order.  All generator state, the step
 *   index of the draws included, lives in device memory: the call allocates nothing, never synchronises and can be captured in a HIP graph
 *   whose replays advance the streams.  gemx_refgen_reset(NULL) + one gemx_refgen_step(NULL) is the env shell's reset() (core.py:485-505). */
typedef struct gemx_refgen_config {
    int32_t struct_size; /* = sizeof(gemx_refgen_config) */
    int32_t n_ref;       /* 1..GEMX_MAX_REF sub-generators */
    uint64_t seed;
    int64_t env_base;    /* global index of env 0 (ABI 7; see gemx_config.env_base): streams are keyed by (seed, env_base + i, generator, ...) */
    int32_t episode_len_lo, episode_len_hi; /* episode_lengths, default (500, 2000) */
    double sigma_lo[GEMX_MAX_REF], sigma_hi[GEMX_MAX_REF];     /* sigma_range, default (1e-3, 1e-1) */
    double margin_lo[GEMX_MAX_REF], margin_hi[GEMX_MAX_REF];   /* limit_margin in normalised units */
    double initial_lo[GEMX_MAX_REF], initial_hi[GEMX_MAX_REF]; /* initial_range (default: the limit margin) */
} gemx_refgen_config;
typedef struct gemx_refgen gemx_refgen;
int gemx_refgen_create(const gemx_refgen_config *cfg, int64_t n_envs, int device, int dtype, gemx_refgen **out);
int gemx_refgen_destroy(gemx_refgen *r);
int gemx_refgen_reset(gemx_refgen *r, const uint8_t *mask_dev, void *stream);
int gemx_refgen_rollout(gemx_refgen *r, const uint8_t *done_dev, int32_t K, void *refs_out_dev, void *stream);
int gemx_refgen_step(gemx_refgen *r, const uint8_t *done_dev, void *refs_dev, void *stream);
int gemx_refgen_get_state(gemx_refgen *r, double *value_out_dev, double *sigma_out_dev, int32_t *left_out_dev, void *stream);
/* K env-shell steps of the generators in the SHELL's order (new entry point, ABI number unchanged): row k of refs_out_dev [K, N, n_ref] (R)
 * comes out as gemx_refgen_step(done[k]) would produce it -- the generators of envs with done_dev[k][env] != 0 restart FIRST, then every
 * generator advances once.  One call == K x gemx_refgen_step(done[k]), row for row and bit for bit.  (gemx_refgen_rollout resets AFTER
 * row k: its row k is what the reward of step k is computed against; here row k is what the env shell shows after step k.)  done_dev
 * [K, N] uint8 may be NULL (no restarts).  Serves both kernel families, may be mixed freely with step / rollout / reset on one handle,
 * keeps nothing on the host, allocates nothing and can be captured in a HIP graph. */
int gemx_refgen_rollout_shell(gemx_refgen *r, const uint8_t *done_dev, int32_t K, void *refs_out_dev, void *stream);

/* REWARD PASS over a stored trajectory (new entry point, ABI number unchanged): the reward installed with gemx_set_reward, evaluated for
 * the K * N rows of obs_dev [K, N, S_out] (R, AoS: what gemx_rollout wrote) with the arithmetic of the fused reward of
 * gemx_rollout_reward -- same term order, same select for powers 1 and 2, pow() for every other power, bias - sum, violation_reward where
 * done_dev[k][env] != 0 -- so reward_out_dev [K, N] (R) holds, bit for bit, what gemx_rollout_reward writes for the same rows and
 * references.  Row k is rewarded against the reference the agent saw BEFORE step k: refs_first_dev [N, n_ref] for k = 0,
 * refs_rows_dev[k - 1] after that (refs_rows_dev [K, N, n_ref] is the output of gemx_refgen_rollout_shell: its last row is not read).
 * Both may be NULL when the reward has n_ref = 0; refs_rows_dev may be NULL when K = 1.  The tensors need the alignment of R only.  One
 * kernel launch: no host state, no allocation, no synchronisation, capturable.  GEMX_ERR_ARG without an installed reward, for an SoA
 * handle, K < 1 or a null / misaligned tensor.
 * With gemx_rollout (physics -> obs, done) and gemx_refgen_rollout_shell (done -> references) this makes a complete K-step rollout of
 * three launches on one stream: the physics never reads the references, so nothing has to run twice. */
int gemx_reward_rows(gemx_handle *h, const void *obs_dev, const void *refs_first_dev, const void *refs_rows_dev, const uint8_t *done_dev,
                     int32_t K, void *reward_out_dev, void *stream);

/* The reference's other generator kinds behind the same handle (ABI 9): every column of a gemx_refgen_create_kinds handle has a kind of
 * its own, freely mixed as MultipleReferenceGenerator mixes its sub-generators (files under reference_generators/):
 *   WIENER     wiener_process_reference_generator.py    as above; the column draws what column j of a gemx_refgen_create handle draws
 *   LAPLACE    laplace_process_reference_generator.py   the clipped walk with Laplace(0, b) increments, b = 10 ** U(log10 sigma range)
 *   SINUS      sinusoidal_reference_generator.py        A sin(2 pi f t_k + phi) + o,       phi = 2 pi U
 *   STEP       step_reference_generator.py              A sign(f (t_j mod 1/f) - r) + o,   r ~ Triangular(0, 0.5, 1), j = (k - roll) mod L,
 *                                                       roll = int(U / (f tau)): numpy's roll over the sub-episode of L steps
 *   TRIANGULAR triangle_reference_generator.py          A saw(2 pi f t_k + phi, w) + o,    w = U   (saw: scipy.signal.sawtooth)
 *   SAWTOOTH   sawtooth_reference_generator.py          A saw(2 pi f t_k + phi, 1) + o
 *   CONST      const_reference_generator.py             reference_value, always; reset and done do nothing
 * with t_k = k * tau, k the step index inside the sub-episode (subepisoded_reference_generator.py:93-119; sub-episode lengths are per
 * column here).  Per sub-episode the waveform kinds draw amplitude, frequency, offset (in this order) and their extra parameters; the
 * offset range is clipped per sub-episode to [-margin_hi + A, margin_hi - A] (STEP: [margin_lo + A, margin_hi - A]) with numpy's clip
 * order min(max(x, a), b); every value is clipped to the margin.  Nothing is tabulated: each (column, env) keeps the parameters of its
 * sub-episode in device memory and evaluates the waveform in closed form, in double, rounded to R on store.  reset() sets the carried
 * value of every kind but WIENER to 0 (a Laplace walk restarts from 0).  Every call that takes a gemx_refgen takes these handles, with
 * the same invariants (step x K == rollout(K), chunked == one-shot, shards by env_base, graph capture).  A handle whose columns are
 * all WIENER with one common sub-episode length range runs the kernels of a gemx_refgen_create handle. */
enum { GEMX_REF_WIENER = 0, GEMX_REF_LAPLACE = 1, GEMX_REF_SINUS = 2, GEMX_REF_STEP = 3, GEMX_REF_TRIANGULAR = 4, GEMX_REF_SAWTOOTH = 5, GEMX_REF_CONST = 6 };
typedef struct gemx_refgen_kinds_config {
    int32_t struct_size; /* = sizeof(gemx_refgen_kinds_config) */
    int32_t n_ref;       /* 1..GEMX_MAX_REF columns */
    uint64_t seed;
    int64_t env_base;
    double tau;          /* control period of the physical system: the waveforms are functions of k * tau */
    int32_t kind[GEMX_MAX_REF]; /* GEMX_REF_* */
    int32_t episode_len_lo[GEMX_MAX_REF], episode_len_hi[GEMX_MAX_REF]; /* episode_lengths, per column */
    double margin_lo[GEMX_MAX_REF], margin_hi[GEMX_MAX_REF];       /* limit_margin in normalised units */
    double sigma_lo[GEMX_MAX_REF], sigma_hi[GEMX_MAX_REF];         /* WIENER, LAPLACE: sigma_range */
    double initial_lo[GEMX_MAX_REF], initial_hi[GEMX_MAX_REF];     /* WIENER: initial_range */
    double amplitude_lo[GEMX_MAX_REF], amplitude_hi[GEMX_MAX_REF]; /* waveform kinds: amplitude_range; clipped to [0, (margin_hi - margin_lo) / 2] */
    double frequency_lo[GEMX_MAX_REF], frequency_hi[GEMX_MAX_REF]; /* waveform kinds: frequency_range, Hz (STEP: > 0) */
    double offset_lo[GEMX_MAX_REF], offset_hi[GEMX_MAX_REF];       /* waveform kinds: offset_range; clipped to the margin */
    double reference_value[GEMX_MAX_REF];                          /* CONST */
} gemx_refgen_kinds_config;
int gemx_refgen_create_kinds(const gemx_refgen_kinds_config *cfg, int64_t n_envs, int device, int dtype, gemx_refgen **out);
/* debug / test access, per (column, env) arrays [n_ref][N] (any pointer may be NULL): kind_index_len int32 [3][n_ref][N] = the kind, the
 * step index inside the sub-episode and its length; params double [6][n_ref][N] = amplitude, frequency, offset, phase, width (STEP: the
 * high/low ratio r), roll.  A handle that runs the all-Wiener kernels does not track index and length: both read -1. */
int gemx_refgen_get_params(gemx_refgen *r, int32_t *kind_index_len_out_dev, double *params_out_dev, void *stream);

/* SwitchedReferenceGenerator behind the same handle (new struct and entry points only, ABI number unchanged;
 * reference_generators/switched_reference_generator.py:8-95): a SWITCHED column has n_alt alternatives -- each a complete column
 * description as in gemx_refgen_kinds_config, for the same referenced state -- and runs one of them per SUPER-EPISODE.  A super-episode
 * draws its length, integers(super_len_lo, super_len_hi) (upper bound excluded), and its alternative by the probabilities p.  Per
 * (column, env) the handle keeps the current alternative, the super-episode's step counter sk and length slen and the number of
 * super-episodes drawn so far, beside the sub-episode state of a gemx_refgen_create_kinds lane.
 *   reset (gemx_refgen_reset, a done byte): a new super-episode is drawn and the chosen alternative is reset WITHOUT an initial reference
 *     (WIENER draws its initial value, every other kind restarts from 0).  The next generated value is the alternative's own first value:
 *     it is not counted in sk and not tested against slen, so the super-episode after a reset shows slen + 1 values, every later one slen
 *     (the reference's behaviour).  Between the reset and that value sk reads -1.
 *   step: sk >= slen -> a new super-episode is drawn, sk = 0, and the chosen alternative restarts WITH the value shown last as its initial
 *     reference (a WIENER or LAPLACE walk continues from it, WIENER draws no initial value); a new sub-episode starts at once and its first
 *     value is this step's output.  Otherwise the current alternative advances as a plain column does.  Then sk += 1.
 *   Alternatives that are not current keep no state.  A CONST alternative emits its value and draws nothing.
 * Random streams: the super-episode draws are Philox blocks of a draw kind of their own, indexed by the lane's super-episode count (word 0:
 * the length, word 1: the choice by the inverse distribution function of p); the sub-episode, step and reset draws are those of a plain column
 * and their counters run on across the switches, so no block is used twice.  All keyed by the global env index.
 * n_alt[g] = 0: column g is PLAIN -- alternative 0 is its description, and it makes the draws and the arithmetic, hence the bits, of
 * column g of a gemx_refgen_create_kinds handle with the same seed.  A config without a switched column gives exactly that handle (and its
 * kernels).  Every call that takes a gemx_refgen takes these handles with the same invariants.  Alternative a of column g sits at index
 * g * GEMX_MAX_ALT + a of the per-alternative arrays.  GEMX_ERR_ARG: n_alt outside [0, GEMX_MAX_ALT], p negative or not summing to 1
 * within 1e-9, super_len_lo < 1 or super_len_hi <= super_len_lo, and what gemx_refgen_create_kinds refuses, per alternative. */
#define GEMX_MAX_ALT 5
typedef struct gemx_refgen_switched_config {
    int32_t struct_size; /* = sizeof(gemx_refgen_switched_config) */
    int32_t n_ref;       /* 1..GEMX_MAX_REF columns */
    uint64_t seed;
    int64_t env_base;
    double tau;
    int32_t n_alt[GEMX_MAX_REF];                                   /* 0: plain column; 1..GEMX_MAX_ALT: switched, that many alternatives */
    int32_t super_len_lo[GEMX_MAX_REF], super_len_hi[GEMX_MAX_REF]; /* super_episode_length, default (100, 10000) */
    double p[GEMX_MAX_REF * GEMX_MAX_ALT];                         /* probabilities of the alternatives */
    int32_t kind[GEMX_MAX_REF * GEMX_MAX_ALT];                     /* per alternative, as in gemx_refgen_kinds_config: */
    int32_t episode_len_lo[GEMX_MAX_REF * GEMX_MAX_ALT], episode_len_hi[GEMX_MAX_REF * GEMX_MAX_ALT];
    double margin_lo[GEMX_MAX_REF * GEMX_MAX_ALT], margin_hi[GEMX_MAX_REF * GEMX_MAX_ALT];
    double sigma_lo[GEMX_MAX_REF * GEMX_MAX_ALT], sigma_hi[GEMX_MAX_REF * GEMX_MAX_ALT];
    double initial_lo[GEMX_MAX_REF * GEMX_MAX_ALT], initial_hi[GEMX_MAX_REF * GEMX_MAX_ALT];
    double amplitude_lo[GEMX_MAX_REF * GEMX_MAX_ALT], amplitude_hi[GEMX_MAX_REF * GEMX_MAX_ALT];
    double frequency_lo[GEMX_MAX_REF * GEMX_MAX_ALT], frequency_hi[GEMX_MAX_REF * GEMX_MAX_ALT];
    double offset_lo[GEMX_MAX_REF * GEMX_MAX_ALT], offset_hi[GEMX_MAX_REF * GEMX_MAX_ALT];
    double reference_value[GEMX_MAX_REF * GEMX_MAX_ALT];
} gemx_refgen_switched_config;
int gemx_refgen_create_switched(const gemx_refgen_switched_config *cfg, int64_t n_envs, int device, int dtype, gemx_refgen **out);
/* debug / test access to the super-episode state, int32 [4][n_ref][N]: the current alternative, sk, slen, the super-episodes drawn so
 * far.  A plain column reads 0, 0, 0, 0.  GEMX_ERR_ARG for a handle without a switched column.  On a handle with one,
 * gemx_refgen_get_params reports the kind of the lane's CURRENT alternative (index and length of a CONST one: -1). */
int gemx_refgen_get_switch_state(gemx_refgen *r, int32_t *alt_sk_slen_nsuper_out_dev, void *stream);

/* Checkpoint of a handle's whole device state (new entry points only, ABI number unchanged): one opaque blob of
 * gemx_refgen_state_bytes(r) bytes in device memory -- a header of GEMX_REFGEN_BLOB_HEADER_BYTES, then EVERY per-(column, env) array the
 * handle owns, in this order, each a section of n_envs * n_ref * (bytes per lane) bytes padded to a multiple of 8:
 *   every handle:                          value 8, sigma 8, left 4, n_sub 4, n_reset 4, t 8
 *   + gemx_refgen_create_kinds handles:    len 4, par 48
 *   + handles with a switched column:      alt 4, sk 4, slen 4, n_super 4
 * (value, sigma, steps left, sub-episodes and resets drawn so far, index of the step draws; sub-episode length, the six waveform
 * parameters; alternative, super-episode step counter and length, super-episodes drawn so far.)  The header names n_envs, n_ref, which of
 * the three groups follow, the columns' kinds and env_base.  A handle of the same configuration that takes the blob continues the
 * streams bit for bit; the references shown last are the caller's tensor and travel beside it.
 *   gemx_refgen_get_blob: asynchronous copies on `stream`; equal states give equal blobs.
 *   gemx_refgen_set_blob: copies the header alone to the host (synchronises `stream`) and checks it BEFORE anything is enqueued:
 *     GEMX_ERR_ARG, with the mismatch named in gemx_last_error, for a blob of another n_envs, n_ref, handle or column kind, or shard
 *     (env_base), and the handle is untouched; then asynchronous copies on `stream`.  The caller guarantees the blob's size.
 * For the same build and the same configuration, as the blob of gemx_get_aux_state is. */
#define GEMX_REFGEN_BLOB_HEADER_BYTES 64
int64_t gemx_refgen_state_bytes(gemx_refgen *r);
int gemx_refgen_get_blob(gemx_refgen *r, void *out_dev, void *stream);
int gemx_refgen_set_blob(gemx_refgen *r, const void *in_dev, void *stream);

/* Device-side OBSERVATION STAGE: the observation-side physical-system wrappers of the reference (CurrentSumProcessor,
 * physical_system_wrappers/current_sum_processor.py:40-57; CosSinProcessor, cos_sin_processor.py:52-66), the env shell's state_filter
 * (core.py:273-276, 317, 366) and the flat (state || reference) vector FlattenObservation makes of the shell's Tuple, in ONE pass over the
 * state rows the stepping kernels wrote.  A handle holds a COLUMN PROGRAM: output column c of a row is
 *   GEMX_OBS_COPY   in[src]                                                          (the same bits)
 *   GEMX_OBS_SUM    the sum of in[j] over the set bits j of mask, added in ascending j with plain adds: no fused multiply-add, no
 *                   reassociation -- numpy's sequential float32 / float64 sum, bit for bit
 *   GEMX_OBS_COSPI  cos(pi * in[src]) }  evaluated in half-turns: the state's epsilon IS an angle in units of pi (limit pi), and it is
 *   GEMX_OBS_SINPI  sin(pi * in[src]) }  never multiplied by a rounded pi first: +-1 and +-0.5 give 0 / +-1 exactly
 * The program is one level deep (every source is an input column).  It is uniform over the rows and travels as a kernel argument.
 *   gemx_obsproc_apply: state_dev [rows][n_in] R (a trajectory [K][N][n_in] is rows = K * N contiguous rows) -> out_dev
 *   [rows][n_post] R, or with flat = 1 [rows][n_post + n_ref] R: the processed state followed by that row's n_ref references from
 *   refs_dev [rows][n_ref] R (flat = 0: refs_dev is not read and may be NULL; so it may with n_ref = 0).  The tensors need the alignment
 *   of R only (a 4-byte aligned fp32 base is legal); in and out must not overlap.  One kernel launch, nothing else: no per-call host
 *   state, no device counters, no allocation, no synchronisation -- a captured call replays.  rows = 0 is a no-op.
 * GEMX_ERR_ARG at create: a null pointer, struct_size, n_in outside [1, GEMX_MAX_OUT], n_post outside [1, GEMX_OBS_MAX_POST], n_ref
 * outside [0, GEMX_MAX_REF], flat not 0 | 1, an unknown op, a src or a mask bit >= n_in, a SUM with an empty mask. */
#define GEMX_OBS_MAX_POST 32
enum { GEMX_OBS_COPY = 0, GEMX_OBS_SUM = 1, GEMX_OBS_COSPI = 2, GEMX_OBS_SINPI = 3 };
typedef struct gemx_obsproc_entry {
    int32_t op;    /* GEMX_OBS_* */
    int32_t src;   /* input column (COPY, COSPI, SINPI); ignored by SUM */
    uint32_t mask; /* SUM: bit j set = input column j is a summand; ignored by the others */
} gemx_obsproc_entry;
typedef struct gemx_obsproc_config {
    int32_t struct_size; /* = sizeof(gemx_obsproc_config) */
    int32_t n_in;        /* columns of a state row: 1..GEMX_MAX_OUT */
    int32_t n_post;      /* processed-state columns: 1..GEMX_OBS_MAX_POST */
    int32_t n_ref;       /* reference columns appended when flat = 1: 0..GEMX_MAX_REF */
    int32_t flat;        /* 1: out rows are (processed state || references) */
    gemx_obsproc_entry entries[GEMX_OBS_MAX_POST];
} gemx_obsproc_config;
typedef struct gemx_obsproc gemx_obsproc;
int gemx_obsproc_create(const gemx_obsproc_config *cfg, int dtype, int device, gemx_obsproc **out);
int gemx_obsproc_apply(gemx_obsproc *p, const void *state_dev, const void *refs_dev, int64_t rows, void *out_dev, void *stream);
int gemx_obsproc_destroy(gemx_obsproc *p);

/* Device-side FLUX OBSERVER and flux-oriented dq actions for the induction machines (new struct and entry points only, ABI number
 * unchanged): the reference's FluxObserver (physical_system_wrappers/flux_observer.py:80-102) and the 'SCIM' / 'DFIM' variants of its
 * DqToAbcActionProcessor (dq_to_abc_action_processor.py:57-148) as a stage of its own behind the stepping kernels.  Per env a handle
 * keeps the rotor-flux estimate Psi (complex, ALWAYS double: the explicit Euler recursion
 *   Psi += tau [(i_alpha + j i_beta) k_current - Psi (k_flux - j omega p)],   (i_alpha, i_beta) = t_23 of the three named currents,
 * runs for the whole episode) and the frame(s) the NEXT action will be rotated by; the two new columns and the frames are evaluated from
 * Psi in the row's precision R:
 *   psi_abs = |Psi| / psi_limit,   psi_angle = arg(Psi) / pi
 *   SCIM: frame 0 = arg(Psi) + angle_advance tau omega p
 *   DFIM: frame 0 = epsilon + angle_advance tau omega p (stator),   frame 1 = arg(Psi) - frame 0 (rotor)
 * A reset sets Psi = 0 and the frames to those of the system's constant reset observation (psi_angle = 0, reset_omega, reset_epsilon).
 *   gemx_fluxobs_step: ONE control step.  state_dev [N][n_in] R (the row the stepping kernel wrote) -> ext_out_dev [N][n_in + 2] R: the
 *     row unchanged (the same bits), then psi_abs, psi_angle; the lane's next frames are stored; LAST, lanes with done_dev[env] != 0 are
 *     reset when auto_reset = 1 (the terminating step still shows the updated flux, as the reference's does before its reset()).
 *     done_dev may be NULL.
 *   gemx_fluxobs_rows: the same recursion over a stored trajectory state_dev [K][N][n_in], done_dev [K][N] (or NULL) -> ext_out_dev
 *     [K][N][n_in + 2] in ONE launch; a lane walks its K rows in order and the handle is left exactly where K calls of _step leave it,
 *     rows and state bit for bit (both run one __device__ function per row).
 *   gemx_fluxobs_actions: abc_out_dev [N][3] = t_32(q(dq_dev [N][2], frame 0)); DFIM: dq_dev [N][4] -> abc_out_dev [N][6], the second
 *     pair rotated by frame 1.  Continuous actions, not clipped (the inner converter clips, as in the reference).
 *   gemx_fluxobs_reset: all lanes, or those with mask_dev[env] != 0.
 *   gemx_fluxobs_get_state / _set_state: double [4][N] -- Psi re, Psi im, frame 0, frame 1 -- for a checkpoint.
 * The tensors need the alignment of R only (a view at an odd element offset is legal); in and out must not overlap.  Every call is
 * kernel launches (get / set: one device-to-device copy) on `stream`: no host state, no allocation, no synchronisation -- capturable.
 * GEMX_ERR_ARG at create: a null pointer, struct_size, n_in outside [4, GEMX_MAX_OUT], a column index outside [0, n_in) (epsilon_index
 * is read for GEMX_FLUX_ACT_DFIM only), an unknown action_mode, auto_reset not 0 | 1, psi_limit or tau not positive, n_envs < 1. */
enum { GEMX_FLUX_ACT_NONE = 0, GEMX_FLUX_ACT_SCIM = 1, GEMX_FLUX_ACT_DFIM = 2 };
typedef struct gemx_fluxobs_config {
    int32_t struct_size;      /* = sizeof(gemx_fluxobs_config) */
    int32_t n_in;             /* columns of a state row: 4..GEMX_MAX_OUT */
    int32_t omega_index;      /* column of omega */
    int32_t current_index[3]; /* columns of the three observed currents (current_names) */
    int32_t epsilon_index;    /* column of epsilon (GEMX_FLUX_ACT_DFIM) */
    int32_t action_mode;      /* GEMX_FLUX_ACT_* */
    int32_t auto_reset;       /* 1: a done lane restarts on its own (the system's auto_reset) */
    int32_t reserved;
    double omega_limit, current_limit[3], epsilon_limit; /* PhysicalSystem.limits of those columns */
    double psi_limit;         /* l_m * limits[i_sd] */
    double p, tau;            /* pole pairs, control period */
    double k_current;         /* r_r l_m / l_r,  l_r = l_m + l_sigr */
    double k_flux;            /* r_r / l_r */
    double angle_advance;     /* in control steps: 0.5 + dead time */
    double reset_omega, reset_epsilon; /* the NORMALISED omega (and epsilon) of the constant reset observation */
} gemx_fluxobs_config;
typedef struct gemx_fluxobs gemx_fluxobs;
int gemx_fluxobs_create(const gemx_fluxobs_config *cfg, int64_t n_envs, int dtype, int device, gemx_fluxobs **out);
int gemx_fluxobs_destroy(gemx_fluxobs *h);
int gemx_fluxobs_reset(gemx_fluxobs *h, const uint8_t *mask_dev, void *stream);
int gemx_fluxobs_step(gemx_fluxobs *h, const void *state_dev, const uint8_t *done_dev, void *ext_out_dev, void *stream);
int gemx_fluxobs_rows(gemx_fluxobs *h, const void *state_dev, const uint8_t *done_dev, int32_t K, void *ext_out_dev, void *stream);
int gemx_fluxobs_actions(gemx_fluxobs *h, const void *dq_dev, void *abc_out_dev, void *stream);
int gemx_fluxobs_get_state(gemx_fluxobs *h, double *out_dev, void *stream);
int gemx_fluxobs_set_state(gemx_fluxobs *h, const double *in_dev, void *stream);

/* Device-side STATE NOISE (new struct and entry points only, ABI number unchanged): the reference's StateNoiseProcessor
 * (physical_system_wrappers/state_noise_processor.py:62-92) and what its env shell then evaluates on the NOISY state (core.py:344-350) --
 * the constraint monitor and the reward -- as one stage behind a stepping kernel that runs WITHOUT constraints, auto-reset and reward.
 * The caller feeds done_out back as the mask of gemx_reset before its next gemx_step.
 *   gemx_noise_step: ONE launch.  state_in_dev [N][n_in] R -> state_out_dev [N][n_in] R = the row plus, on column index[j], the draw of
 *     (env, slot j, position), evaluated in double and rounded to R before the add; every other column keeps its bits.  state_in_dev ==
 *     state_out_dev is allowed (any other overlap is not).  done_out_dev [N] uint8 = the constraints of limit_mask / squared_mask (as in
 *     gemx_config) on the noisy row, with the expressions and the term order of the stepping kernels.  reward_out_dev [N] R (may be NULL;
 *     needs has_reward) = the reward description evaluated on the noisy row against refs_dev [N][n_ref] R with the arithmetic of
 *     gemx_reward_rows, violation_reward where done.  Then the position advances by one.
 *   gemx_noise_draws: out_dev [K][N][n_noisy] R = the draws of positions step0 .. step0 + K - 1, as gemx_noise_step adds them; the
 *     position does not move (cf. gemx_synthetic_actions).
 *   gemx_noise_get_position (synchronises `stream`) / gemx_noise_set_position: the stream position, for a checkpoint.
 * Distributions, per slot: NORMAL(param0 = loc, param1 = scale) by Box-Muller, UNIFORM(param0 = low, param1 = high) and
 * LAPLACE(param0 = loc, param1 = scale) by the inverse distribution function, from counter-based Philox4x32-10 words: the draw is a pure
 * function of (seed, env_base + env, position, slot) -- shards by env_base draw what the whole job draws; parity with numpy's streams is
 * distributional.  The position lives in device memory: a call allocates nothing, never synchronises and can be captured in a HIP graph
 * whose replays advance the stream.  The tensors need the alignment of R only.
 * GEMX_ERR_ARG at create: a null pointer, struct_size, n_in outside [1, GEMX_MAX_OUT], n_noisy outside [0, n_in], an index outside
 * [0, n_in) or listed twice, an unknown distribution, a negative scale or high < low, a mask bit >= n_in, has_reward not 0 | 1, and what
 * gemx_set_reward refuses of the reward description. */
enum { GEMX_NOISE_NORMAL = 0, GEMX_NOISE_UNIFORM = 1, GEMX_NOISE_LAPLACE = 2 };
typedef struct gemx_noise_config {
    int32_t struct_size;         /* = sizeof(gemx_noise_config) */
    int32_t n_in;                /* columns of a state row: 1..GEMX_MAX_OUT */
    int32_t n_noisy;             /* noisy columns (slots): 0..n_in */
    int32_t has_reward;          /* 1: `reward` below is evaluated on the noisy row; 0: no reward */
    int32_t index[GEMX_MAX_OUT]; /* column of slot j */
    int32_t dist[GEMX_MAX_OUT];  /* GEMX_NOISE_* of slot j */
    double param0[GEMX_MAX_OUT], param1[GEMX_MAX_OUT]; /* loc, scale | low, high */
    uint64_t seed;
    int64_t env_base;            /* global index of env 0 (see gemx_config.env_base) */
    uint32_t limit_mask, squared_mask; /* the constraints, as in gemx_config, evaluated on the noisy row */
    gemx_reward_config reward;
} gemx_noise_config;
typedef struct gemx_noise gemx_noise;
int gemx_noise_create(const gemx_noise_config *cfg, int64_t n_envs, int dtype, int device, gemx_noise **out);
int gemx_noise_destroy(gemx_noise *h);
int gemx_noise_step(gemx_noise *h, const void *state_in_dev, const void *refs_dev, void *state_out_dev, uint8_t *done_out_dev,
                    void *reward_out_dev, void *stream);
int gemx_noise_draws(gemx_noise *h, uint64_t step0, int32_t K, void *out_dev, void *stream);
int gemx_noise_get_position(gemx_noise *h, uint64_t *position_host, void *stream);
int gemx_noise_set_position(gemx_noise *h, uint64_t position, void *stream);

/* Device-side EPISODE TIME LIMIT and EPISODE STATISTICS (new struct and entry points only, ABI number unchanged): gymnasium's TimeLimit and
 * RecordEpisodeStatistics around an env, as one stage behind the launch that wrote a step's done byte and reward.  Per env the handle keeps
 * length (i32), ret (f64: the return accumulates in double whatever R is), last_length, last_ret (the totals of the episode that ended
 * last) and n_finished (u32).  One step of one env:
 *     length += 1, ret += (double)reward
 *     truncated = max_steps > 0 && length >= max_steps && !done      (terminating AND reaching the limit in one step: terminated)
 *     ended = done | truncated;  where ended: last_length = length, last_ret = ret, n_finished += 1, length = 0, ret = 0
 *   gemx_episode_step: ONE launch, one lane per env.  done_dev [N] uint8, reward_dev [N] R (given exactly when has_reward) ->
 *     truncated_out_dev, ended_out_dev [N] uint8 and reset_mask_out_dev [N] uint8 (may be NULL) = truncated when auto_reset_in_kernel (the
 *     stepping kernel restarts terminated envs itself) and ended when not: the mask of the gemx_reset in front of the caller's next
 *     gemx_step.  Every lane reads its inputs before it writes: done_dev and reset_mask_out_dev MAY BE THE SAME BUFFER (no other overlap).
 *   gemx_episode_rows: the same arithmetic over stored rows done_dev [K][N], reward_dev [K][N] in one pass (a lane scans its env's K rows in
 *     order): afterwards the handle holds what K calls of gemx_episode_step leave, bit for bit.  ended_out_dev [K][N] uint8;
 *     finished_return_out_dev [K][N] double and finished_length_out_dev [K][N] int32 (each may be NULL): the episode's totals at the row
 *     where it ended, 0 elsewhere.  The outputs must not overlap the inputs.
 *   gemx_episode_get_state / gemx_episode_set_state (both synchronise `stream`): all five fields as ONE device blob of
 *     GEMX_EPISODE_STATE_BYTES * N bytes, 8-byte aligned: ret [N] double, last_ret [N] double, length [N] int32, last_length [N] int32,
 *     n_finished [N] uint32, in that order.
 * state_dev at create: NULL (the handle allocates the blob, zeroed) or the caller's own zeroed blob of that layout, which it keeps alive as
 * long as the handle: the handle then works IN that memory (the Python holder hands out views of it, nothing is copied).
 * A step or rows call allocates nothing, keeps no host state, issues no memset and never synchronises: it can be captured in a HIP graph.
 * GEMX_ERR_ARG: a null pointer, struct_size, max_steps < 0, a flag not 0 | 1, n_envs < 1, K < 1, a misaligned tensor, reward_dev not
 * matching has_reward. */
#define GEMX_EPISODE_STATE_BYTES 28
typedef struct gemx_episode_config {
    int32_t struct_size;          /* = sizeof(gemx_episode_config) */
    int32_t max_steps;            /* the time limit in control steps; 0: none (statistics only) */
    int32_t auto_reset_in_kernel; /* 1: the stepping kernel restarts terminated envs itself -> reset_mask = truncated; 0: reset_mask = ended */
    int32_t has_reward;           /* 1: the calls read a reward; 0: ret stays 0 */
} gemx_episode_config;
typedef struct gemx_episode gemx_episode;
int gemx_episode_create(const gemx_episode_config *cfg, int64_t n_envs, int dtype, int device, void *state_dev, gemx_episode **out);
int gemx_episode_destroy(gemx_episode *h);
int gemx_episode_step(gemx_episode *h, const uint8_t *done_dev, const void *reward_dev, uint8_t *truncated_out_dev, uint8_t *ended_out_dev,
                      uint8_t *reset_mask_out_dev, void *stream);
int gemx_episode_rows(gemx_episode *h, const uint8_t *done_dev, const void *reward_dev, int32_t K, uint8_t *ended_out_dev,
                      double *finished_return_out_dev, int32_t *finished_length_out_dev, void *stream);
int gemx_episode_get_state(gemx_episode *h, void *out_dev, void *stream);
int gemx_episode_set_state(gemx_episode *h, const void *in_dev, void *stream);

/* Device-side PROFILE REFERENCES (new struct and entry points only, ABI number unchanged): given reference trajectories -- drive cycles,
 * recorded set-point profiles -- shown per env from a table in device memory, as a stage with a handle of its own.  The table is R
 * [n_rows][n_ref] shared by all envs (per_env = 0) or [n_rows][N][n_ref], one profile per env (per_env = 1), in normalised units; it is
 * BORROWED: the handle keeps the device pointer and the caller keeps the memory alive and unchanged as long as the handle.  Per env the
 * handle keeps k (int32: steps shown since the episode began), s (int32: the episode's start row) and e (uint32: episodes begun so far).
 *   position   p = s + k * (tau / profile_tau), evaluated in double from the integers every time (a product rounded once, then a sum
 *              rounded once): never accumulated, step 10 000 carries no drift
 *   rows       i = floor(p), w = p - i;  END_HOLD: p >= n_rows - 1 shows row n_rows - 1;  END_WRAP: rows modulo n_rows, the partner of
 *              row n_rows - 1 is row 0
 *   value      INTERP_HOLD, or w == 0: the table entry of row i, the same bits;  INTERP_LINEAR: fma((R)w, b - a, a) in R, a and b the
 *              entries of row i and of its partner
 *   restart    k = 0, e += 1, and with START_RANDOM s = min(int(u * n_rows), n_rows - 1), u the first word of the Philox4x32-10 block
 *              keyed by (seed, env_base + env, e): a function of the global env index and the episode number alone, so shards by env_base
 *              show what the whole job shows.  START_ZERO: s = 0.  A fresh handle has k = s = e = 0.
 *   gemx_refprofile_reset: restarts the envs with mask_dev[env] != 0 (NULL: all).
 *   gemx_refprofile_step: ONE launch, the contract of gemx_refgen_step: envs with done_dev[env] != 0 (NULL: none) restart FIRST, then
 *     refs_dev [N][n_ref] R receives the values at p(k) and k advances.
 *   gemx_refprofile_rollout / _rollout_shell: K rows refs_out_dev [K][N][n_ref] with done_dev [K][N] (or NULL) in one launch, a lane
 *     walking its env's rows in order; _rollout restarts AFTER row k (gemx_refgen_rollout's order), _rollout_shell BEFORE it: one call ==
 *     K x gemx_refprofile_step(done[k]), row for row and bit for bit (one __device__ row function serves all three).
 *   gemx_refprofile_get_state: int32 [3][N] = k, s, e (one device-to-device copy).
 *   gemx_refprofile_state_bytes / _get_blob / _set_blob: the checkpoint, a header of GEMX_REFPROFILE_BLOB_HEADER_BYTES and the 12 N
 *     bytes of state; _set_blob copies the header alone to the host (synchronises `stream`) and checks it BEFORE anything is enqueued:
 *     GEMX_ERR_ARG, the mismatch named in gemx_last_error, for a blob of another n_envs, n_ref, n_rows, table layout or shard
 *     (env_base); the handle is then untouched.  The table itself is configuration and does not travel.
 * Reset, step and the rollouts are one kernel launch each: no host state, no allocation, no synchronisation -- a captured call replays
 * and advances the counters.  refs tensors need the alignment of R only.
 * GEMX_ERR_ARG at create: a null pointer, struct_size, n_ref outside [1, GEMX_MAX_REF], n_rows < 1, a flag outside its enum, tau or
 * profile_tau not positive and finite, tau / profile_tau above 2^20, n_envs < 1, a misaligned table. */
enum { GEMX_PROFILE_INTERP_HOLD = 0, GEMX_PROFILE_INTERP_LINEAR = 1 };
enum { GEMX_PROFILE_END_HOLD = 0, GEMX_PROFILE_END_WRAP = 1 };
enum { GEMX_PROFILE_START_ZERO = 0, GEMX_PROFILE_START_RANDOM = 1 };
#define GEMX_REFPROFILE_BLOB_HEADER_BYTES 64
typedef struct gemx_refprofile_config {
    int32_t struct_size;   /* = sizeof(gemx_refprofile_config) */
    int32_t n_ref;         /* 1..GEMX_MAX_REF columns */
    int32_t n_rows;        /* T: rows of a profile, >= 1 */
    int32_t per_env;       /* 0: table [n_rows][n_ref], shared; 1: table [n_rows][N][n_ref] */
    int32_t interpolation; /* GEMX_PROFILE_INTERP_* */
    int32_t end;           /* GEMX_PROFILE_END_* */
    int32_t start;         /* GEMX_PROFILE_START_* */
    int32_t reserved;
    uint64_t seed;         /* START_RANDOM */
    int64_t env_base;      /* global index of env 0 (see gemx_config.env_base) */
    double tau;            /* control period of the physical system */
    double profile_tau;    /* sampling time of the table's rows */
} gemx_refprofile_config;
typedef struct gemx_refprofile gemx_refprofile;
int gemx_refprofile_create(const gemx_refprofile_config *cfg, const void *table_dev, int64_t n_envs, int device, int dtype, gemx_refprofile **out);
int gemx_refprofile_destroy(gemx_refprofile *h);
int gemx_refprofile_reset(gemx_refprofile *h, const uint8_t *mask_dev, void *stream);
int gemx_refprofile_step(gemx_refprofile *h, const uint8_t *done_dev, void *refs_dev, void *stream);
int gemx_refprofile_rollout(gemx_refprofile *h, const uint8_t *done_dev, int32_t K, void *refs_out_dev, void *stream);
int gemx_refprofile_rollout_shell(gemx_refprofile *h, const uint8_t *done_dev, int32_t K, void *refs_out_dev, void *stream);
int gemx_refprofile_get_state(gemx_refprofile *h, int32_t *k_s_e_out_dev, void *stream);
int64_t gemx_refprofile_state_bytes(gemx_refprofile *h);
int gemx_refprofile_get_blob(gemx_refprofile *h, void *out_dev, void *stream);
int gemx_refprofile_set_blob(gemx_refprofile *h, const void *in_dev, void *stream);

/* Device-side DISCOUNTED RETURNS and GENERALISED ADVANTAGE ESTIMATES, GAE(lambda), over the stored rows of a rollout (new struct and
 * entry point only, ABI number unchanged): the reverse scan over K per env that every learner runs on reward [K][N], done [K][N] and a
 * critic's value [K][N], as ONE launch.  No per-env state survives a call: there is no handle.  Per env, for k = K-1 ... 0, with one
 * double accumulator A and everything converted to double first:
 *     term = terminated[k] != 0;  end = ended[k] != 0 (ended_dev NULL: end = term);  trunc = end && !term
 *     v      = value[k]
 *     v_next = k == K-1 ? last_value : value[k+1]                          (last_value_dev NULL: 0)
 *     if (end)  v_next = trunc && final_value ? final_value[k] : 0         (final_value_dev is read at rows with end && !term ONLY)
 *     t1 = gamma * v_next;  delta = (reward[k] + t1) - v
 *     t2 = gamma * lam;     t3 = t2 * A;   A = end ? delta : delta + t3
 *     advantage[k] = (R)A;  return[k] = (R)(A + v)
 *   A starts as carry_in (carry_in_dev NULL: 0); carry_out_dev (may be NULL) receives it after row 0.  A long trajectory can be scanned
 *   in pieces, the later rows first: rows [k0, K) and then rows [0, k0) with carry_out -> carry_in and last_value = value[k0] are one
 *   scan, bit for bit.  A TRUNCATED ROW WITHOUT final_value_dev IS TREATED AS TERMINATED.  Every product and sum above is rounded on its
 *   own, in double, with no FMA across them: a float64 host restatement of these operations gives the same bits, and an fp32 output is
 *   that double rounded to nearest.
 *   value_dev NULL: the plain discounted return-to-go, the same rows with v = 0 and v_next = 0 everywhere and lam taken as 1 (cfg->lam
 *   is ignored); A starts as carry_in if given, else as (double)last_value if given, else as 0 -- giving both is GEMX_ERR_ARG;
 *   return_out_dev is the only output and final_value_dev must be NULL.  return[k] = reward[k] + gamma * return[k+1], cut at `end`.
 *   reward_dev, value_dev, final_value_dev, advantage_out_dev, return_out_dev: [K][N] R, contiguous; last_value_dev [N] R;
 *   terminated_dev (the env's done), ended_dev (terminated | truncated: what gemx_episode_* hands out) [K][N] uint8;
 *   carry_in_dev, carry_out_dev [N] double.  The outputs must not overlap the inputs or each other.
 * One kernel launch on `stream`: no allocation, no host state, no memset, no synchronisation -- the call can be captured in a HIP graph.
 * GEMX_ERR_ARG: cfg NULL, struct_size, flags != 0, gamma or (with value_dev) lam outside [0, 1], reward_dev or terminated_dev NULL, no
 * output, the value_dev-NULL restrictions above, K < 1, n_envs < 1, a misaligned tensor, an unknown dtype or device. */
typedef struct gemx_returns_config {
    int32_t struct_size; /* = sizeof(gemx_returns_config) */
    double gamma;        /* discount, [0, 1] */
    double lam;          /* GAE lambda, [0, 1]; ignored (taken as 1) without value_dev */
    int32_t flags;       /* reserved: 0 */
} gemx_returns_config;
int gemx_returns_rows(const gemx_returns_config *cfg, int64_t n_envs, int32_t K, int dtype, int device, const void *reward_dev, const void *value_dev,
                      const void *last_value_dev, const uint8_t *terminated_dev, const uint8_t *ended_dev, const void *final_value_dev,
                      const double *carry_in_dev, double *carry_out_dev, void *advantage_out_dev, void *return_out_dev, void *stream);

/* PER-ENV MOTOR, LOAD AND SUPPLY PARAMETERS: domain randomisation inside one handle (new struct and entry points only, ABI number
 * unchanged).  gemx_set_env_params gives every env its own machine: host float64 arrays, one entry per env, of the quantities gemx_config
 * carries per handle -- `model` as gemx_config.model ([n_envs][GEMX_MODEL_ROWS * GEMX_MODEL_COLS]), `torque_coef` ([n_envs][4]), `j_total`,
 * `load_a`, `load_b`, `load_c`, `u_nominal` ([n_envs]).  A NULL array means the handle's own value for every env.  The library derives, with
 * the double-precision expressions gemx_create uses for the handle's own parameters, a device table [F][n_envs] of R, field-major:
 *     the system's structurally non-zero model entries | tc0..tc3 | 1 / j_total, a, b, c, omega_lim, lin_factor, 1 / tau_decay | u_sup
 * (F = gemx_env_params_fields(h)), rounded to R once.  From then on gemx_step, gemx_rollout and gemx_rollout_reward run
 * envparams_step_kernel / envparams_rollout_kernel (gemx_last_launch names them), in which lane e computes, bit for bit, what a handle
 * created with env e's values computes.  Everything else stays one value per handle: tau, the pole pair number, the limits the
 * observations are normalised by, the initial state (gemx_reset and the reset observation are unchanged), the constraint set, the
 * solver, the action frame.  The one-step map of the constant-speed loads is never taken with a table (it belongs to one parameter set).
 * GEMX_ERR_ARG, naming per-env parameters, and nothing changed, for: a NULL argument, struct_size, n_envs other than the handle's, a value
 * that is not finite, j_total <= 0, a model entry outside the system's sparsity pattern or a pole pair entry other than the handle's; and
 * for handles the per-env kernels do not serve: fp64, the Dormand-Prince solver (fixed step or GEMX_SOLVER_ADAPTIVE), interlocking_time > 0,
 * action_delay > 0, GEMX_SUPPLY_RC, random initial states.  While a table is set gemx_rollout_synthetic, gemx_rollout_half and
 * gemx_rollout(obs_every = 0) return GEMX_ERR_ARG before anything is launched.
 * gemx_set_env_params copies synchronously (not inside a stream capture); calling it again replaces the table's contents in place, so a
 * captured graph keeps working with the new values.  gemx_clear_env_params synchronises the device, frees the table and returns the handle
 * to the kernels it ran before.  gemx_get_env_params copies the table as it sits on the device to out_dev ([F][n_envs] R) on `stream`. */
typedef struct gemx_env_params {
    int32_t struct_size; /* = sizeof(gemx_env_params) */
    int64_t n_envs;      /* length of every array: the handle's n_envs */
    const double *model;
    const double *torque_coef;
    const double *j_total, *load_a, *load_b, *load_c;
    const double *u_nominal;
} gemx_env_params;
int gemx_set_env_params(gemx_handle *h, const gemx_env_params *p);
int gemx_clear_env_params(gemx_handle *h);
int gemx_get_env_params(gemx_handle *h, void *out_dev, void *stream);
int gemx_env_params_fields(const gemx_handle *h);

/* EPISODIC ROLLOUT: K fused control steps WITH the episode time limit inside the launch (new entry point only, ABI number unchanged).
 * Truncation is `length >= max_steps && !done`, and an env's `length` depends on its own done history alone, so the kernel produces the
 * mask it restarts on.  Per env and step, behind the control step (gemx_episode_step's rule):
 *     length += 1;  truncated = length >= max_steps && !done;  ended = done | truncated;  where ended: length = 0, the env restarts
 * Every ended env restarts from the handle's initial state, whatever auto_reset says (with a time limit the stepped path restarts them all:
 * in the stepping kernel or by the masked gemx_reset).  The switching state survives, as it does there.
 *   actions_dev  [K][N][A] R | [K][N] uint8, as gemx_rollout reads them
 *   length_dev   [N] int32: every env's steps in its running episode (the episode stage's `length` field).  READ ONLY: run
 *                gemx_episode_rows behind this call on terminated_out_dev (and the rewards) with the same max_steps; it moves the counters
 *                by the same rule from the same value
 *   obs_out_dev  [K][N][S_out] | [K][S_out][N] R (16-byte aligned): the row of a step that ended is the final state, not the reset state
 *   terminated_out_dev, truncated_out_dev, ended_out_dev   [K][N] uint8; each may be NULL
 * With a parameter table (gemx_set_env_params) every lane steps with its column, as envparams_step_kernel does; without one the lane takes
 * the code path of gemx_step's kernel (the one-step map of the constant-speed loads included).  Either way the rows equal, bit for bit, K
 * calls of gemx_step with gemx_episode_step and the masked gemx_reset between them.  The kernels live in libgemx_tl<S>_<C>.so beside the
 * library, loaded by the first call that needs one; gemx_last_launch names episodic_rollout_kernel and that unit.
 * Asynchronous on `stream`, allocates nothing, can be captured in a HIP graph (a FIRST launch of a handle that is being captured goes
 * without the one-step map, as a captured first gemx_step does).
 * GEMX_ERR_ARG, naming the episodic rollout, before anything is launched: a NULL handle / actions / length / obs, K < 1, max_steps < 1, a
 * misaligned obs_out_dev or length_dev, and handles the kernel does not serve: fp64, the Dormand-Prince solver (fixed step or
 * GEMX_SOLVER_ADAPTIVE), interlocking_time > 0, action_delay > 0, GEMX_SUPPLY_RC, random initial states. */
int gemx_rollout_episodic(gemx_handle *h, const void *actions_dev, int32_t K, const int32_t *length_dev, int32_t max_steps, void *obs_out_dev,
                          uint8_t *terminated_out_dev, uint8_t *truncated_out_dev, uint8_t *ended_out_dev, void *stream);

/* POLICY ROLLOUT: the episodic rollout with the ACTOR inside the launch (new structs and entry points only, ABI number unchanged).
 * A policy is an MLP of 1..GEMX_POLICY_MAX_LAYERS layers, every width <= GEMX_POLICY_MAX_WIDTH, input width <= GEMX_POLICY_MAX_INPUT,
 * float32: weights[l] is [width[l]][fan-in] row-major, biases[l] [width[l]] (HOST pointers).  Its weights live in one device blob;
 * setting them again copies into the same blob (synchronously, not inside a stream capture), so a captured launch sees them at its next
 * replay.  The action of control step k is computed in front of the step from the row step k - 1 wrote:
 *     x = [obs_prev[columns[0..n_cols)], references[k]];  out = W_L act(... act(W_1 x + b_1)) + b_L   (act: hidden layers only)
 *     continuous converters (width[L-1] = action components): action = squash(out + noise[k]), tanh or clip to [-1, 1]
 *     finite converters (width[L-1] = number of actions):     action = the lowest index among the maxima of out + noise[k]
 * obs_prev is obs0_dev's row at k = 0 and the handle's reset observation behind a step that ended the episode.  Every dot product is an
 * fp32 fma chain from the bias over the inputs in ascending order: the selected columns in ascending column order, then the references.
 *   obs0_dev [N][S_out] | [S_out][N] R;  refs_dev [K][N][n_ref] R (NULL with n_ref = 0);  noise_dev [K][N][width[L-1]] R or NULL
 *   actions_out_dev [K][N][A] R | [K][N] uint8: the actions taken; feeding them to the episodic rollout gives the same rows, bit for bit
 *   length_dev, max_steps, obs_out_dev, terminated / truncated / ended: as the episodic rollout takes them
 * The kernels live in libgemx_pl<S>_<C>.so beside the library.  Asynchronous on `stream`, allocates nothing, can be captured.
 * GEMX_ERR_ARG, naming the policy rollout, before anything is launched: what the episodic rollout refuses; struct_size; a NULL policy /
 * obs0 / actions_out; n_cols + n_ref != the policy's input width; n_ref outside [0, GEMX_MAX_REF]; a column outside the row or selected
 * twice; an output width that is not the converter's; a policy on another device.  The tanh probe runs the actor's tanh over n floats. */
#define GEMX_POLICY_MAX_LAYERS 3
#define GEMX_POLICY_MAX_WIDTH 64
#define GEMX_POLICY_MAX_INPUT 48
enum { GEMX_POLICY_RELU = 0, GEMX_POLICY_TANH = 1 };
enum { GEMX_POLICY_SQUASH_TANH = 0, GEMX_POLICY_SQUASH_CLIP = 1 };
typedef struct gemx_policy_config {
    int32_t struct_size; /* = sizeof(gemx_policy_config) */
    int32_t n_layers;
    int32_t n_in;        /* input width of layer 0 */
    int32_t width[GEMX_POLICY_MAX_LAYERS];
    int32_t activation;  /* GEMX_POLICY_RELU | GEMX_POLICY_TANH */
    int32_t squash;      /* GEMX_POLICY_SQUASH_* (continuous converters) */
} gemx_policy_config;
typedef struct gemx_policy_call {
    int32_t struct_size; /* = sizeof(gemx_policy_call) */
    int32_t K;
    int32_t n_cols, n_ref;
    int32_t columns[GEMX_POLICY_MAX_INPUT];
    int32_t max_steps;
    int32_t reserved;
    const void *obs0_dev, *refs_dev, *noise_dev;
    const int32_t *length_dev;
    void *obs_out_dev, *actions_out_dev;
    uint8_t *terminated_out_dev, *truncated_out_dev, *ended_out_dev;
} gemx_policy_call;
typedef struct gemx_policy gemx_policy;
int gemx_policy_create(const gemx_policy_config *cfg, const float *const *weights, const float *const *biases, int device, gemx_policy **out);
int gemx_policy_set_weights(gemx_policy *p, const float *const *weights, const float *const *biases);
int gemx_policy_destroy(gemx_policy *p);
int gemx_rollout_policy(gemx_handle *h, const gemx_policy *p, const gemx_policy_call *call, void *stream);
int gemx_policy_tanh_probe(gemx_handle *h, const float *x_dev, float *y_dev, int64_t n, void *stream);

/* POLICY ROLLOUT OF THE COMPLETE ENV: the policy rollout with the env's own reference generators stepped INSIDE the launch (one new entry
 * point, ABI number unchanged).  The call is a gemx_policy_call read differently in two fields: refs_dev is [N][n_ref] R, the references
 * shown in front of step 0 (not [K][N][n_ref]), and n_ref is the generator's column count (>= 1).  Step k's actor input is
 * [obs_prev[columns], refs_prev]: refs_prev is refs_dev's row at k = 0 and refs_out_dev[k - 1] afterwards.  Behind the row store of step k
 * the lane restarts the generators of an env whose episode ended (terminated or truncated), advances them and writes
 * refs_out_dev[k] -- the row gemx_refgen_rollout_shell / gemx_refprofile_rollout_shell produce on the ENDED rows, bit for bit, and the
 * generator handle is left in the state they leave it in.  Exactly one generator handle is given, the other NULL:
 *   refgen      an all-Wiener handle of gemx_refgen_create (its standard normals are drawn by a launch in front, into refs_out_dev)
 *   refprofile  a gemx_refprofile handle: shared or per-env table, both interpolations, end rules and start rules
 *   refs_out_dev [K][N][n_ref] R
 * The kernels live in libgemx_pc<S>_<C>.so beside the library (loaded by the first call).  Asynchronous on `stream`, allocates nothing,
 * can be captured.  GEMX_ERR_ARG, naming the complete policy rollout, before anything is launched: what gemx_rollout_policy refuses;
 * both handles or neither; a gemx_refgen of gemx_refgen_create_kinds or gemx_refgen_create_switched (kinds, mixed, switched); a generator
 * handle of another n_envs, dtype, device, env_base or column count; a NULL or misaligned refs_out_dev. */
int gemx_rollout_policy_complete(gemx_handle *h, const gemx_policy *p, const gemx_policy_call *call, void *refs_out_dev, gemx_refgen *refgen,
                                 gemx_refprofile *refprofile, void *stream);

/* LOOKAHEAD ROLLOUT OF THE COMPLETE ENV: one-step finite-control-set predictive control inside the fused launch (one new entry point, no
 * new struct, ABI number unchanged).  In control step k every one of the finite converter's n_actions switching actions (the flat index of
 * a multi-converter) is stepped ONCE from the state the step starts at -- the episodic rollout's control step -- and scored with the
 * handle's reward (gemx_set_reward) against the references shown in front of step k:
 *     score[a] = reward(row_a, refs_prev, done_a);   action = the lowest index among the maxima of score[a] + noise[k][a]
 * (best = 0; for a = 1 .. n_actions - 1: if (s[a] > s[best]) best = a -- the policy rollout's rule; a -inf noise entry masks an action).
 * The chosen trial is committed as it was computed, then the step proceeds as gemx_rollout_policy_complete's: the episode rule, the row
 * store, the generators (restart where the episode ended, advance, refs_out_dev[k]).  Fed to gemx_rollout_episodic, actions_out_dev gives
 * the same rows bit for bit; gemx_reward_rows over them gives reward[k] == score[actions[k]] bit for bit.
 * The call is a gemx_policy_call read as gemx_rollout_policy_complete reads it, without an actor: K, n_ref, max_steps, refs_dev [N][n_ref]
 * (the references shown in front of step 0), length_dev, obs_out_dev, terminated / truncated / ended are read; n_cols must be 0 and
 * obs0_dev, noise_dev, actions_out_dev NULL -- the outputs and the noise of this entry point are arguments:
 *   refs_out_dev     [K][N][n_ref] R
 *   actions_out_dev  [K][N] uint8
 *   scores_out_dev   [K][N][n_actions] R, the scores in front of `+ noise`; may be NULL
 *   noise_dev        [K][N][n_actions] R; may be NULL
 *   refgen | refprofile   exactly one, as gemx_rollout_policy_complete takes them
 * The kernels live in libgemx_la<S>_<C>.so beside the library (finite converters only; loaded by the first call).  Asynchronous on
 * `stream`, allocates nothing, can be captured.  GEMX_ERR_ARG, naming the lookahead rollout, before anything is launched: what
 * gemx_rollout_policy_complete refuses of the handle, the call and the generator; a continuous converter (no finite action set); a handle
 * without a reward or with GEMX_OBS_SOA; n_ref other than the reward's; actor fields of the call that are set. */
int gemx_rollout_lookahead_complete(gemx_handle *h, const gemx_policy_call *call, void *refs_out_dev, uint8_t *actions_out_dev, void *scores_out_dev,
                                    const void *noise_dev, gemx_refgen *refgen, gemx_refprofile *refprofile, void *stream);

/* POLICY EVALUATION OVER STORED ROWS: an MLP of gemx_policy_create on every row of a stored policy rollout, with the rollout kernels' own
 * arithmetic, as ONE launch (new struct and entry point only, ABI number unchanged).  No physics, no env handle: the pass reads the policy's
 * device blob (no second copy of the weights) and the tensors a rollout handed out.  Row (k, env), k < K, one lane each:
 *     x[k] = [o[k][columns[0..n_cols)], r[k]];   out[k] = W_L act(... act(W_1 x[k] + b_1)) + b_L
 * every dot product the fp32 fma chain gemx_rollout_policy documents (from the bias, the selected columns in ascending column order, then
 * the references), so for rows and a policy that came from a policy rollout out[k] is, bit for bit, the value that rollout had in front of
 * `+ noise[k]`.
 *   GEMX_EVAL_SEEN  o[0] = obs0_dev's row;  o[k] = ended_dev[k-1] ? the reset observation : rows_dev[k-1]
 *                   r[k] = refs_dev[k] (refs0_dev NULL: the physics-only form), or  r[0] = refs0_dev's row, r[k] = refs_dev[k-1] (refs0_dev
 *                   given: the complete form, gemx_rollout_policy_complete's refs_dev [N][n_ref] and refs_out_dev)
 *                   GEMX_EVAL_LAST: one more row, k = K: o[K] as above, r[K] = last_refs_dev's row, or refs_dev[K-1] in the complete form;
 *                   it goes to the *_last_dev outputs -- a critic's row K is the last_value of gemx_returns_rows
 *   GEMX_EVAL_NEXT  o[k] = rows_dev[k] without reset substitution, r[k] = refs_dev[k]: a critic's rows are the final_value of
 *                   gemx_returns_rows.  obs0_dev, ended_dev, reset_obs_dev, refs0_dev, last_refs_dev must be NULL, GEMX_EVAL_LAST clear
 * Heads: each reads the fp32 out, computes in double with every operation rounded on its own (no FMA across them, as gemx_returns_rows)
 * and rounds the result once to out_dtype (GEMX_F32 | GEMX_F64):
 *   GEMX_EVAL_HEAD_NONE         out_dev [K][N][n_out] float (n_out = the last layer's width); out_last_dev [N][n_out] float
 *   GEMX_EVAL_HEAD_VALUE        n_out == 1: value_out_dev [K][N] = out[0]; value_last_dev [N]
 *   GEMX_EVAL_HEAD_CATEGORICAL  a = actions_dev[k] ([K][N] uint8);  m = max_i out_i;  s = sum_i exp(out_i - m) (ascending i, from 0);
 *                               lse = m + log(s);  l_i = out_i - lse;  log_prob = l_a;  entropy = -(sum_i exp(l_i) * l_i) (ascending i, from 0).
 *                               a >= n_out: log_prob = NaN, and GEMX_ERRFLAG_ACTION is set in the error word of error_handle (a gemx_handle
 *                               on the policy's device; may be NULL: not reported), where gemx_error_flags finds it
 *   GEMX_EVAL_HEAD_GAUSSIAN     u = pre_squash_dev[k] ([K][N][n_out] float: out_old + noise, what was squashed into the stored action),
 *                               ls = log_std_dev ([n_out] float, DEVICE memory: a captured launch reads new values at its next replay):
 *                               per j ascending, from 0:  sg = exp(ls_j);  d = u_j - out_j;  q = (d * d) / (2 * (sg * sg));
 *                                   log_prob += ((-q) - ls_j) - 0.5 log(2 pi);   entropy += ls_j + 0.5 log(2 pi e)
 *                               GEMX_EVAL_SQUASH_CORRECTION: c += 2 * ((log 2 - u_j) - softplus(-2 u_j)), log_prob = log_prob - c (the tanh
 *                               change of variables); softplus(t) = max(t, 0) + log1p(exp(-|t|))
 *                               log_prob_out_dev, entropy_out_dev [K][N] of out_dtype; either may be NULL, not both
 * rows_dev [K][N][n_state] float;  reset_obs_dev [n_state] float, or [N][n_state] with reset_per_env = 1;  obs0_dev [N][n_state] float.
 * One kernel launch on `stream`: no allocation, no host state, no synchronisation -- the call can be captured in a HIP graph.
 * GEMX_ERR_ARG, naming the policy evaluation, before anything is launched: a NULL policy or call, struct_size, an unknown mode, head, flag
 * or out_dtype, K < 1, n_envs < 1, n_state outside [1, GEMX_MAX_OUT], n_ref outside [0, GEMX_MAX_REF], n_cols + n_ref != the policy's input
 * width, a column outside the row or selected twice, a tensor the mode / head needs that is NULL or one it does not read that is given,
 * the VALUE head with n_out != 1, GEMX_EVAL_LAST with the CATEGORICAL or GAUSSIAN head, a misaligned tensor, a policy or an error_handle on
 * another device. */
enum { GEMX_EVAL_SEEN = 0, GEMX_EVAL_NEXT = 1 };
enum { GEMX_EVAL_HEAD_NONE = 0, GEMX_EVAL_HEAD_VALUE = 1, GEMX_EVAL_HEAD_CATEGORICAL = 2, GEMX_EVAL_HEAD_GAUSSIAN = 3 };
enum { GEMX_EVAL_LAST = 1, GEMX_EVAL_SQUASH_CORRECTION = 2 };
typedef struct gemx_policy_eval_call {
    int32_t struct_size; /* = sizeof(gemx_policy_eval_call) */
    int32_t mode;        /* GEMX_EVAL_SEEN | GEMX_EVAL_NEXT */
    int32_t head;        /* GEMX_EVAL_HEAD_* */
    int32_t flags;       /* GEMX_EVAL_LAST | GEMX_EVAL_SQUASH_CORRECTION */
    int32_t out_dtype;   /* GEMX_F32 | GEMX_F64: the head outputs (out_dev is float whatever it says) */
    int32_t n_state;     /* columns of a stored row */
    int32_t n_cols, n_ref;
    int32_t columns[GEMX_POLICY_MAX_INPUT];
    int32_t reset_per_env; /* 0: reset_obs_dev [n_state]; 1: [N][n_state] */
    int32_t reserved;      /* 0 */
    const float *obs0_dev, *rows_dev, *reset_obs_dev;
    const uint8_t *ended_dev;
    const float *refs_dev, *refs0_dev, *last_refs_dev;
    const uint8_t *actions_dev;
    const float *pre_squash_dev, *log_std_dev;
    float *out_dev, *out_last_dev;
    void *value_out_dev, *value_last_dev, *log_prob_out_dev, *entropy_out_dev;
    gemx_handle *error_handle;
} gemx_policy_eval_call;
int gemx_policy_eval_rows(const gemx_policy *p, const gemx_policy_eval_call *call, int64_t n_envs, int32_t K, int device, void *stream);

/* Checkpoint / parity access to the ODE state, SoA [S_ode, N] of R in physical units (angle in rad; the fp32 build keeps the
 * angle as a 32-bit fraction of a turn internally, so a get/set round trip rounds it to fp32 radians, ~1e-7 rad), plus the
 * per-env packed converter switching state, 2 bits per half-bridge: [N] uint8, or [2][N] uint8 (row 0 = bits 0..7,
 * row 1 = bits 8..11) for the 6 half-bridges of GEMX_CONV_FINITE_2XB6; gemx_n_switch_bytes() = bytes per env.
 * (There is no per-env step counter: PhysicalSystem.k belongs to the binding; the handle's launched-steps count is in the blob below.)
 * Everything else a resumed handle needs is ONE opaque device blob (gemx_aux_state_bytes() bytes, 16-byte aligned): the
 * RCVoltageSupply's two rows (capacitor voltage, time since its last update; voltage_supplies.py:100-123), the DeadTimeProcessor's
 * action queue and its phase (dead_time_processor.py:63-85), the per-env reset counters of the random initialisers (the counter-based
 * streams continue where they were), the exact angle words (see above: gemx_get_state rounds them) and the launched-steps count.
 * A checkpoint = get_state + get_switch_state + get_aux_state, restored in that order (the blob's angle words overwrite the rounded ones);
 * restored into a fresh handle of the SAME configuration (checked: gemx_set_aux_state fails with GEMX_ERR_ARG otherwise, and
 * synchronises `stream` to read the blob's header) the next launches continue bit for bit. */
int gemx_n_switch_bytes(const gemx_handle *h);
int gemx_get_state(gemx_handle *h, void *soa_out_dev, void *stream);
int gemx_set_state(gemx_handle *h, const void *soa_in_dev, void *stream);
int gemx_get_switch_state(gemx_handle *h, uint8_t *out_dev, void *stream);
int gemx_set_switch_state(gemx_handle *h, const uint8_t *in_dev, void *stream);
int64_t gemx_aux_state_bytes(const gemx_handle *h);
int gemx_get_aux_state(gemx_handle *h, void *blob_out_dev, void *stream);
int gemx_set_aux_state(gemx_handle *h, const void *blob_in_dev, void *stream);

/* Tuning: number of control steps whose observations are staged in LDS between global-memory bursts inside
 * gemx_rollout (0 = heuristic from N, S_out and the LDS size; also settable with env GEMX_STEPS_PER_BLOCK). */
int gemx_set_steps_per_block(gemx_handle *h, int32_t steps);

/* Which kernel instantiation / geometry the most recent gemx_step / gemx_rollout on this handle launched (for
 * profiling reports): e.g. "gemx::advance_pipe_kernel<sys=1,conv=1,load=0,solver=1,il=0,f32,D=8> grid=256 x 192 ...". */
const char *gemx_last_launch(const gemx_handle *h);

/* Sticky device error word (synchronises `stream`), GEMX_ERRFLAG_* bits:
 *   ACTION       a discrete action outside the action space was seen (the reference asserts action_space.contains(action),
 *                converters.py:204-206; the kernel masks it into range);
 *   OMEGA_MOVED  a launch specialised for "omega of every env == its initial value" (dc_stream_kernel, constant-speed loads) found
 *                another omega in device memory -- e.g. enqueued on a different stream than a preceding gemx_set_state: the
 *                observations of that launch are invalid;
 *   TOLERANCE    GEMX_SOLVER_ADAPTIVE took a step at its floor (1/1024 of a segment) whose error estimate exceeded the tolerance. */
#define GEMX_ERRFLAG_ACTION 1u
#define GEMX_ERRFLAG_OMEGA_MOVED 2u
#define GEMX_ERRFLAG_TOLERANCE 4u
int gemx_error_flags(gemx_handle *h, uint32_t *flags_host, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GEMX_H */
