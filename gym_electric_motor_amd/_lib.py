"""ctypes binding of include/gemx.h.  The product path has NO fallback: if `libgemx.so` is missing or no
HIP device is visible, creating a system raises."""
import ctypes as C
import os

from . import build as _build

MAX_ODE, MAX_OUT, MODEL_ROWS, MODEL_COLS = 8, 24, 5, 11
ABI_VERSION = 9

SYS_DC_PERMEX, SYS_SYNC, SYS_SCIM, SYS_DC_SERIES, SYS_DC_SHUNT, SYS_DC_EXTEX, SYS_EESM, SYS_DFIM = 0, 1, 2, 3, 4, 5, 6, 7
CONV_CONT_4QC, CONV_FINITE_B6, CONV_CONT_B6, CONV_FINITE_4QC = 0, 1, 2, 3
ACT_ABC, ACT_DQ_SPACE, ACT_DQ_PROCESSOR = 0, 1, 2
SUPPLY_IDEAL, SUPPLY_RC = 0, 1
INIT_CONST, INIT_UNIFORM, INIT_GAUSSIAN = 0, 1, 2
MAX_DELAY = 8
CONV_CONT_2X4QC, CONV_FINITE_2X4QC, CONV_CONT_B6_4QC, CONV_FINITE_B6_4QC, CONV_CONT_2XB6, CONV_FINITE_2XB6 = 4, 5, 6, 7, 8, 9
LOAD_CONST_SPEED, LOAD_POLY_STATIC = 0, 1
SOLVER_EULER, SOLVER_RK4, SOLVER_DP5 = 0, 1, 2
SOLVER_SPLIT_KINKS, SOLVER_ADAPTIVE = 1, 2
F32, F64 = 0, 1
OBS_AOS, OBS_SOA = 0, 1
ERRFLAG_ACTION, ERRFLAG_OMEGA_MOVED, ERRFLAG_TOLERANCE = 1, 2, 4  # gemx_error_flags bits (GEMX_ERRFLAG_*)


class GemxConfig(C.Structure):
    """Mirror of `gemx_config` (include/gemx.h)."""

    _fields_ = [
        ("struct_size", C.c_int32), ("abi_version", C.c_int32),
        ("system_kind", C.c_int32), ("converter_kind", C.c_int32), ("load_kind", C.c_int32),
        ("solver_kind", C.c_int32), ("solver_nsteps", C.c_int32), ("solver_flags", C.c_int32),
        ("dtype", C.c_int32), ("obs_layout", C.c_int32), ("auto_reset", C.c_int32),
        ("limit_mask", C.c_uint32), ("squared_mask", C.c_uint32),
        ("action_frame", C.c_int32), ("action_delay", C.c_int32),
        ("supply_kind", C.c_int32), ("init_kind", C.c_int32), ("init_flux_mode", C.c_int32), ("init_flux", C.c_double * 8),
        ("seed", C.c_uint64), ("env_base", C.c_int64),
        ("init_lo", C.c_double * MAX_ODE), ("init_hi", C.c_double * MAX_ODE), ("init_mu", C.c_double * MAX_ODE),
        ("init_sigma", C.c_double * MAX_ODE),
        ("supply_r", C.c_double), ("supply_c", C.c_double), ("action_delay_reset", C.c_double * 6), ("solver_rtol", C.c_double), ("solver_atol", C.c_double), ("solver_atol_omega", C.c_double),
        ("tau", C.c_double), ("interlocking_time", C.c_double), ("u_nominal", C.c_double),
        ("model", C.c_double * (MODEL_ROWS * MODEL_COLS)),
        ("torque_coef", C.c_double * 4),
        ("j_total", C.c_double), ("load_a", C.c_double), ("load_b", C.c_double), ("load_c", C.c_double),
        ("tau_decay", C.c_double),
        ("limits", C.c_double * MAX_OUT),
        ("init_state", C.c_double * MAX_ODE),
    ]


class GemxError(RuntimeError):
    pass


_lib = None

MAX_REF = 4


class GemxRewardConfig(C.Structure):
    """Mirror of `gemx_reward_config` (include/gemx.h)."""

    _fields_ = [
        ("struct_size", C.c_int32), ("n_ref", C.c_int32), ("ref_index", C.c_int32 * MAX_REF),
        ("weight", C.c_double * MAX_OUT), ("power", C.c_double * MAX_OUT), ("state_length", C.c_double * MAX_OUT),
        ("bias", C.c_double), ("violation_reward", C.c_double),
    ]


class GemxRefgenConfig(C.Structure):
    """Mirror of `gemx_refgen_config` (include/gemx.h)."""

    _fields_ = [
        ("struct_size", C.c_int32), ("n_ref", C.c_int32), ("seed", C.c_uint64), ("env_base", C.c_int64),
        ("episode_len_lo", C.c_int32), ("episode_len_hi", C.c_int32),
        ("sigma_lo", C.c_double * MAX_REF), ("sigma_hi", C.c_double * MAX_REF),
        ("margin_lo", C.c_double * MAX_REF), ("margin_hi", C.c_double * MAX_REF),
        ("initial_lo", C.c_double * MAX_REF), ("initial_hi", C.c_double * MAX_REF),
    ]


REF_WIENER, REF_LAPLACE, REF_SINUS, REF_STEP, REF_TRIANGULAR, REF_SAWTOOTH, REF_CONST = range(7)  # GEMX_REF_*


class GemxRefgenKindsConfig(C.Structure):
    """Mirror of `gemx_refgen_kinds_config` (include/gemx.h)."""

    _fields_ = [
        ("struct_size", C.c_int32), ("n_ref", C.c_int32), ("seed", C.c_uint64), ("env_base", C.c_int64), ("tau", C.c_double),
        ("kind", C.c_int32 * MAX_REF), ("episode_len_lo", C.c_int32 * MAX_REF), ("episode_len_hi", C.c_int32 * MAX_REF),
        ("margin_lo", C.c_double * MAX_REF), ("margin_hi", C.c_double * MAX_REF),
        ("sigma_lo", C.c_double * MAX_REF), ("sigma_hi", C.c_double * MAX_REF),
        ("initial_lo", C.c_double * MAX_REF), ("initial_hi", C.c_double * MAX_REF),
        ("amplitude_lo", C.c_double * MAX_REF), ("amplitude_hi", C.c_double * MAX_REF),
        ("frequency_lo", C.c_double * MAX_REF), ("frequency_hi", C.c_double * MAX_REF),
        ("offset_lo", C.c_double * MAX_REF), ("offset_hi", C.c_double * MAX_REF),
        ("reference_value", C.c_double * MAX_REF),
    ]


MAX_ALT = 5  # GEMX_MAX_ALT
_ALT = MAX_REF * MAX_ALT


class GemxRefgenSwitchedConfig(C.Structure):
    """Mirror of `gemx_refgen_switched_config` (include/gemx.h): alternative a of column g at index g * MAX_ALT + a."""

    _fields_ = [
        ("struct_size", C.c_int32), ("n_ref", C.c_int32), ("seed", C.c_uint64), ("env_base", C.c_int64), ("tau", C.c_double),
        ("n_alt", C.c_int32 * MAX_REF), ("super_len_lo", C.c_int32 * MAX_REF), ("super_len_hi", C.c_int32 * MAX_REF),
        ("p", C.c_double * _ALT),
        ("kind", C.c_int32 * _ALT), ("episode_len_lo", C.c_int32 * _ALT), ("episode_len_hi", C.c_int32 * _ALT),
        ("margin_lo", C.c_double * _ALT), ("margin_hi", C.c_double * _ALT),
        ("sigma_lo", C.c_double * _ALT), ("sigma_hi", C.c_double * _ALT),
        ("initial_lo", C.c_double * _ALT), ("initial_hi", C.c_double * _ALT),
        ("amplitude_lo", C.c_double * _ALT), ("amplitude_hi", C.c_double * _ALT),
        ("frequency_lo", C.c_double * _ALT), ("frequency_hi", C.c_double * _ALT),
        ("offset_lo", C.c_double * _ALT), ("offset_hi", C.c_double * _ALT),
        ("reference_value", C.c_double * _ALT),
    ]


REFGEN_BLOB_HEADER_BYTES = 64  # GEMX_REFGEN_BLOB_HEADER_BYTES
# bytes per (column, env) lane of the arrays a generator handle owns, in the blob's order (include/gemx.h, gemx_refgen_get_blob):
# every handle | + a gemx_refgen_create_kinds handle | + a handle with a switched column
REFGEN_LANE_BYTES = dict(all=(8, 8, 4, 4, 4, 8), kinds=(4, 48), switched=(4, 4, 4, 4))


def refgen_state_bytes(n_envs, n_ref, kinds=False, switched=False):
    """`gemx_refgen_state_bytes` restated: the header, then one section per array, each padded to a multiple of 8 bytes."""
    rows = REFGEN_LANE_BYTES["all"] + (REFGEN_LANE_BYTES["kinds"] if kinds or switched else ()) + (REFGEN_LANE_BYTES["switched"] if switched else ())
    return REFGEN_BLOB_HEADER_BYTES + sum((int(n_envs) * int(n_ref) * b + 7) // 8 * 8 for b in rows)


OBS_MAX_POST = 32
OBS_COPY, OBS_SUM, OBS_COSPI, OBS_SINPI = range(4)  # GEMX_OBS_*


class GemxObsprocEntry(C.Structure):
    """Mirror of `gemx_obsproc_entry` (include/gemx.h)."""

    _fields_ = [("op", C.c_int32), ("src", C.c_int32), ("mask", C.c_uint32)]


class GemxObsprocConfig(C.Structure):
    """Mirror of `gemx_obsproc_config` (include/gemx.h)."""

    _fields_ = [
        ("struct_size", C.c_int32), ("n_in", C.c_int32), ("n_post", C.c_int32), ("n_ref", C.c_int32), ("flat", C.c_int32),
        ("entries", GemxObsprocEntry * OBS_MAX_POST),
    ]


FLUX_ACT_NONE, FLUX_ACT_SCIM, FLUX_ACT_DFIM = range(3)  # GEMX_FLUX_ACT_*


class GemxFluxobsConfig(C.Structure):
    """Mirror of `gemx_fluxobs_config` (include/gemx.h)."""

    _fields_ = [
        ("struct_size", C.c_int32), ("n_in", C.c_int32), ("omega_index", C.c_int32), ("current_index", C.c_int32 * 3), ("epsilon_index", C.c_int32),
        ("action_mode", C.c_int32), ("auto_reset", C.c_int32), ("reserved", C.c_int32),
        ("omega_limit", C.c_double), ("current_limit", C.c_double * 3), ("epsilon_limit", C.c_double), ("psi_limit", C.c_double),
        ("p", C.c_double), ("tau", C.c_double), ("k_current", C.c_double), ("k_flux", C.c_double), ("angle_advance", C.c_double),
        ("reset_omega", C.c_double), ("reset_epsilon", C.c_double),
    ]


NOISE_NORMAL, NOISE_UNIFORM, NOISE_LAPLACE = range(3)  # GEMX_NOISE_*


class GemxNoiseConfig(C.Structure):
    """Mirror of `gemx_noise_config` (include/gemx.h)."""

    _fields_ = [
        ("struct_size", C.c_int32), ("n_in", C.c_int32), ("n_noisy", C.c_int32), ("has_reward", C.c_int32),
        ("index", C.c_int32 * MAX_OUT), ("dist", C.c_int32 * MAX_OUT), ("param0", C.c_double * MAX_OUT), ("param1", C.c_double * MAX_OUT),
        ("seed", C.c_uint64), ("env_base", C.c_int64), ("limit_mask", C.c_uint32), ("squared_mask", C.c_uint32),
        ("reward", GemxRewardConfig),
    ]


class GemxEpisodeConfig(C.Structure):
    """Mirror of `gemx_episode_config` (include/gemx.h)."""

    _fields_ = [("struct_size", C.c_int32), ("max_steps", C.c_int32), ("auto_reset_in_kernel", C.c_int32), ("has_reward", C.c_int32)]


EPISODE_STATE_BYTES = 28  # GEMX_EPISODE_STATE_BYTES

PROFILE_INTERP_HOLD, PROFILE_INTERP_LINEAR = 0, 1  # GEMX_PROFILE_INTERP_*
PROFILE_END_HOLD, PROFILE_END_WRAP = 0, 1  # GEMX_PROFILE_END_*
PROFILE_START_ZERO, PROFILE_START_RANDOM = 0, 1  # GEMX_PROFILE_START_*
REFPROFILE_BLOB_HEADER_BYTES = 64  # GEMX_REFPROFILE_BLOB_HEADER_BYTES


class GemxRefprofileConfig(C.Structure):
    """Mirror of `gemx_refprofile_config` (include/gemx.h)."""

    _fields_ = [
        ("struct_size", C.c_int32), ("n_ref", C.c_int32), ("n_rows", C.c_int32), ("per_env", C.c_int32),
        ("interpolation", C.c_int32), ("end", C.c_int32), ("start", C.c_int32), ("reserved", C.c_int32),
        ("seed", C.c_uint64), ("env_base", C.c_int64), ("tau", C.c_double), ("profile_tau", C.c_double),
    ]


class GemxReturnsConfig(C.Structure):
    """Mirror of `gemx_returns_config` (include/gemx.h)."""

    _fields_ = [("struct_size", C.c_int32), ("gamma", C.c_double), ("lam", C.c_double), ("flags", C.c_int32)]


POLICY_MAX_LAYERS, POLICY_MAX_WIDTH, POLICY_MAX_INPUT = 3, 64, 48  # GEMX_POLICY_MAX_*
POLICY_RELU, POLICY_TANH = 0, 1  # GEMX_POLICY_RELU / GEMX_POLICY_TANH
POLICY_SQUASH_TANH, POLICY_SQUASH_CLIP = 0, 1  # GEMX_POLICY_SQUASH_*


class GemxPolicyConfig(C.Structure):
    """Mirror of `gemx_policy_config` (include/gemx.h)."""

    _fields_ = [("struct_size", C.c_int32), ("n_layers", C.c_int32), ("n_in", C.c_int32), ("width", C.c_int32 * POLICY_MAX_LAYERS),
                ("activation", C.c_int32), ("squash", C.c_int32)]


class GemxPolicyCall(C.Structure):
    """Mirror of `gemx_policy_call` (include/gemx.h)."""

    _fields_ = [("struct_size", C.c_int32), ("K", C.c_int32), ("n_cols", C.c_int32), ("n_ref", C.c_int32), ("columns", C.c_int32 * POLICY_MAX_INPUT),
                ("max_steps", C.c_int32), ("reserved", C.c_int32), ("obs0_dev", C.c_void_p), ("refs_dev", C.c_void_p), ("noise_dev", C.c_void_p),
                ("length_dev", C.c_void_p), ("obs_out_dev", C.c_void_p), ("actions_out_dev", C.c_void_p), ("terminated_out_dev", C.c_void_p),
                ("truncated_out_dev", C.c_void_p), ("ended_out_dev", C.c_void_p)]


EVAL_SEEN, EVAL_NEXT = 0, 1  # GEMX_EVAL_SEEN / GEMX_EVAL_NEXT
EVAL_HEAD_NONE, EVAL_HEAD_VALUE, EVAL_HEAD_CATEGORICAL, EVAL_HEAD_GAUSSIAN = range(4)  # GEMX_EVAL_HEAD_*
EVAL_LAST, EVAL_SQUASH_CORRECTION = 1, 2  # gemx_policy_eval_call.flags


class GemxPolicyEvalCall(C.Structure):
    """Mirror of `gemx_policy_eval_call` (include/gemx.h)."""

    _fields_ = [("struct_size", C.c_int32), ("mode", C.c_int32), ("head", C.c_int32), ("flags", C.c_int32), ("out_dtype", C.c_int32), ("n_state", C.c_int32),
                ("n_cols", C.c_int32), ("n_ref", C.c_int32), ("columns", C.c_int32 * POLICY_MAX_INPUT), ("reset_per_env", C.c_int32), ("reserved", C.c_int32),
                ("obs0_dev", C.c_void_p), ("rows_dev", C.c_void_p), ("reset_obs_dev", C.c_void_p), ("ended_dev", C.c_void_p),
                ("refs_dev", C.c_void_p), ("refs0_dev", C.c_void_p), ("last_refs_dev", C.c_void_p), ("actions_dev", C.c_void_p),
                ("pre_squash_dev", C.c_void_p), ("log_std_dev", C.c_void_p), ("out_dev", C.c_void_p), ("out_last_dev", C.c_void_p),
                ("value_out_dev", C.c_void_p), ("value_last_dev", C.c_void_p), ("log_prob_out_dev", C.c_void_p), ("entropy_out_dev", C.c_void_p),
                ("error_handle", C.c_void_p)]


def refprofile_state_bytes(n_envs):
    """`gemx_refprofile_state_bytes` restated: the header, then k, s, e as int32 [3][N]."""
    return REFPROFILE_BLOB_HEADER_BYTES + 12 * int(n_envs)


EXPORTS = (
    "gemx_abi_version", "gemx_sizeof_config", "gemx_last_error", "gemx_device_count", "gemx_create", "gemx_destroy",
    "gemx_n_envs", "gemx_n_ode", "gemx_n_out", "gemx_n_action", "gemx_action_itemsize", "gemx_n_switch_bytes", "gemx_reset_observation", "gemx_set_reward", "gemx_rollout_reward", "gemx_refgen_create", "gemx_refgen_destroy", "gemx_refgen_reset",
    "gemx_refgen_rollout", "gemx_refgen_get_state", "gemx_refgen_step", "gemx_refgen_create_kinds", "gemx_refgen_get_params",
    "gemx_reset", "gemx_step", "gemx_rollout", "gemx_rollout_half", "gemx_get_state", "gemx_set_state", "gemx_get_switch_state",
    "gemx_set_switch_state", "gemx_aux_state_bytes", "gemx_get_aux_state", "gemx_set_aux_state", "gemx_reset_again", "gemx_rollout_synthetic", "gemx_synthetic_actions", "gemx_set_rate_limiter", "gemx_set_steps_per_block", "gemx_last_launch", "gemx_error_flags", "gemx_debug_read",
    "gemx_obsproc_create", "gemx_obsproc_apply", "gemx_obsproc_destroy",
    "gemx_refgen_rollout_shell", "gemx_reward_rows",
    "gemx_refgen_create_switched", "gemx_refgen_get_switch_state",
    "gemx_refgen_state_bytes", "gemx_refgen_get_blob", "gemx_refgen_set_blob",
    "gemx_fluxobs_create", "gemx_fluxobs_destroy", "gemx_fluxobs_reset", "gemx_fluxobs_step", "gemx_fluxobs_rows", "gemx_fluxobs_actions",
    "gemx_fluxobs_get_state", "gemx_fluxobs_set_state",
    "gemx_noise_create", "gemx_noise_destroy", "gemx_noise_step", "gemx_noise_draws", "gemx_noise_get_position", "gemx_noise_set_position",
    "gemx_episode_create", "gemx_episode_destroy", "gemx_episode_step", "gemx_episode_rows", "gemx_episode_get_state", "gemx_episode_set_state",
    "gemx_refprofile_create", "gemx_refprofile_destroy", "gemx_refprofile_reset", "gemx_refprofile_step", "gemx_refprofile_rollout",
    "gemx_refprofile_rollout_shell", "gemx_refprofile_get_state", "gemx_refprofile_state_bytes", "gemx_refprofile_get_blob", "gemx_refprofile_set_blob",
    "gemx_returns_rows",
    "gemx_set_env_params", "gemx_clear_env_params", "gemx_get_env_params", "gemx_env_params_fields",
    "gemx_rollout_episodic",
    "gemx_policy_create", "gemx_policy_set_weights", "gemx_policy_destroy", "gemx_rollout_policy", "gemx_policy_tanh_probe",
    "gemx_rollout_policy_complete",
    "gemx_rollout_lookahead_complete",
    "gemx_policy_eval_rows",
)


def library_path():
    """In-tree libgemx.so; GEMX_LIBRARY names another build of the SAME library (A/B runs of kernel variants)."""
    return os.environ.get("GEMX_LIBRARY") or _build.LIB


def load():
    """Load libgemx.so (built in-tree by `__graft_entry__.build()` / `gym_electric_motor_amd.build.build_library()`)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise GemxError(
            f"{path} is missing: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    # torch bundles its own libamdhip64.so.7; libgemx.so depends on the same SONAME.  Import torch FIRST so that
    # one HIP runtime serves both (loading the system runtime first and torch's second breaks device discovery).
    import torch  # noqa: F401

    L = C.CDLL(path)
    L.gemx_last_error.restype = C.c_char_p
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.gemx_create.argtypes = [C.POINTER(GemxConfig), i64, C.c_int, C.POINTER(vp)]
    L.gemx_destroy.argtypes = [vp]
    L.gemx_n_envs.argtypes = [vp, C.POINTER(i64)]
    for f in ("gemx_n_ode", "gemx_n_out", "gemx_n_action", "gemx_action_itemsize"):
        getattr(L, f).argtypes = [vp]
    L.gemx_reset_observation.argtypes = [vp, C.POINTER(C.c_double)]
    L.gemx_reset.argtypes = [vp, vp, vp, vp]
    L.gemx_reset_again.argtypes = [vp, vp, vp, vp]
    L.gemx_aux_state_bytes.argtypes = [vp]
    L.gemx_aux_state_bytes.restype = i64
    L.gemx_rollout_synthetic.argtypes = [vp, C.c_uint64, C.c_uint32, i32, vp, vp, vp]
    L.gemx_set_rate_limiter.argtypes = [vp, i32, C.c_double]
    L.gemx_synthetic_actions.argtypes = [vp, C.c_uint64, C.c_uint32, i32, vp, vp]
    L.gemx_get_aux_state.argtypes = [vp, vp, vp]
    L.gemx_set_aux_state.argtypes = [vp, vp, vp]
    L.gemx_step.argtypes = [vp, vp, vp, vp, vp]
    L.gemx_rollout.argtypes = [vp, vp, i32, vp, vp, i32, vp]
    L.gemx_rollout_half.argtypes = [vp, vp, i32, vp, vp, vp]
    L.gemx_set_reward.argtypes = [vp, C.POINTER(GemxRewardConfig)]
    L.gemx_refgen_create.argtypes = [C.POINTER(GemxRefgenConfig), i64, C.c_int, C.c_int, C.POINTER(vp)]
    L.gemx_refgen_create_kinds.argtypes = [C.POINTER(GemxRefgenKindsConfig), i64, C.c_int, C.c_int, C.POINTER(vp)]
    L.gemx_refgen_get_params.argtypes = [vp, vp, vp, vp]
    L.gemx_refgen_create_switched.argtypes = [C.POINTER(GemxRefgenSwitchedConfig), i64, C.c_int, C.c_int, C.POINTER(vp)]
    L.gemx_refgen_get_switch_state.argtypes = [vp, vp, vp]
    L.gemx_refgen_state_bytes.argtypes = [vp]
    L.gemx_refgen_state_bytes.restype = i64
    L.gemx_refgen_get_blob.argtypes = [vp, vp, vp]
    L.gemx_refgen_set_blob.argtypes = [vp, vp, vp]
    L.gemx_refgen_destroy.argtypes = [vp]
    L.gemx_refgen_reset.argtypes = [vp, vp, vp]
    L.gemx_refgen_rollout.argtypes = [vp, vp, i32, vp, vp]
    L.gemx_refgen_get_state.argtypes = [vp, vp, vp, vp, vp]
    L.gemx_refgen_step.argtypes = [vp, vp, vp, vp]
    L.gemx_refgen_rollout_shell.argtypes = [vp, vp, i32, vp, vp]
    L.gemx_reward_rows.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp]
    L.gemx_obsproc_create.argtypes = [C.POINTER(GemxObsprocConfig), C.c_int, C.c_int, C.POINTER(vp)]
    L.gemx_obsproc_apply.argtypes = [vp, vp, vp, i64, vp, vp]
    L.gemx_obsproc_destroy.argtypes = [vp]
    L.gemx_fluxobs_create.argtypes = [C.POINTER(GemxFluxobsConfig), i64, C.c_int, C.c_int, C.POINTER(vp)]
    L.gemx_fluxobs_destroy.argtypes = [vp]
    L.gemx_fluxobs_reset.argtypes = [vp, vp, vp]
    L.gemx_fluxobs_step.argtypes = [vp, vp, vp, vp, vp]
    L.gemx_fluxobs_rows.argtypes = [vp, vp, vp, i32, vp, vp]
    L.gemx_fluxobs_actions.argtypes = [vp, vp, vp, vp]
    L.gemx_fluxobs_get_state.argtypes = [vp, vp, vp]
    L.gemx_fluxobs_set_state.argtypes = [vp, vp, vp]
    L.gemx_noise_create.argtypes = [C.POINTER(GemxNoiseConfig), i64, C.c_int, C.c_int, C.POINTER(vp)]
    L.gemx_noise_destroy.argtypes = [vp]
    L.gemx_noise_step.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.gemx_noise_draws.argtypes = [vp, C.c_uint64, i32, vp, vp]
    L.gemx_noise_get_position.argtypes = [vp, C.POINTER(C.c_uint64), vp]
    L.gemx_noise_set_position.argtypes = [vp, C.c_uint64, vp]
    L.gemx_episode_create.argtypes = [C.POINTER(GemxEpisodeConfig), i64, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.gemx_episode_destroy.argtypes = [vp]
    L.gemx_episode_step.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.gemx_episode_rows.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    L.gemx_episode_get_state.argtypes = [vp, vp, vp]
    L.gemx_episode_set_state.argtypes = [vp, vp, vp]
    L.gemx_refprofile_create.argtypes = [C.POINTER(GemxRefprofileConfig), vp, i64, C.c_int, C.c_int, C.POINTER(vp)]
    L.gemx_refprofile_destroy.argtypes = [vp]
    L.gemx_refprofile_reset.argtypes = [vp, vp, vp]
    L.gemx_refprofile_step.argtypes = [vp, vp, vp, vp]
    L.gemx_refprofile_rollout.argtypes = [vp, vp, i32, vp, vp]
    L.gemx_refprofile_rollout_shell.argtypes = [vp, vp, i32, vp, vp]
    L.gemx_refprofile_get_state.argtypes = [vp, vp, vp]
    L.gemx_refprofile_state_bytes.argtypes = [vp]
    L.gemx_refprofile_state_bytes.restype = i64
    L.gemx_refprofile_get_blob.argtypes = [vp, vp, vp]
    L.gemx_refprofile_set_blob.argtypes = [vp, vp, vp]
    L.gemx_returns_rows.argtypes = [C.POINTER(GemxReturnsConfig), i64, i32, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gemx_rollout_reward.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.gemx_set_env_params.argtypes = [vp, vp]
    L.gemx_clear_env_params.argtypes = [vp]
    L.gemx_get_env_params.argtypes = [vp, vp, vp]
    L.gemx_env_params_fields.argtypes = [vp]
    L.gemx_rollout_episodic.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.gemx_policy_create.argtypes = [C.POINTER(GemxPolicyConfig), vp, vp, C.c_int, C.POINTER(vp)]
    L.gemx_policy_set_weights.argtypes = [vp, vp, vp]
    L.gemx_policy_destroy.argtypes = [vp]
    L.gemx_rollout_policy.argtypes = [vp, vp, C.POINTER(GemxPolicyCall), vp]
    L.gemx_policy_tanh_probe.argtypes = [vp, vp, vp, i64, vp]
    L.gemx_rollout_policy_complete.argtypes = [vp, vp, C.POINTER(GemxPolicyCall), vp, vp, vp, vp]
    L.gemx_rollout_lookahead_complete.argtypes = [vp, C.POINTER(GemxPolicyCall), vp, vp, vp, vp, vp, vp, vp]
    L.gemx_policy_eval_rows.argtypes = [vp, C.POINTER(GemxPolicyEvalCall), i64, i32, C.c_int, vp]
    L.gemx_get_state.argtypes = [vp, vp, vp]
    L.gemx_set_state.argtypes = [vp, vp, vp]
    L.gemx_get_switch_state.argtypes = [vp, vp, vp]
    L.gemx_set_switch_state.argtypes = [vp, vp, vp]
    L.gemx_set_steps_per_block.argtypes = [vp, i32]
    L.gemx_last_launch.argtypes = [vp]
    L.gemx_last_launch.restype = C.c_char_p
    L.gemx_error_flags.argtypes = [vp, C.POINTER(C.c_uint32), vp]
    if L.gemx_abi_version() != ABI_VERSION or L.gemx_sizeof_config() != C.sizeof(GemxConfig):
        raise GemxError("libgemx.so ABI does not match gym_electric_motor_amd._lib.GemxConfig; rebuild the library")
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = load().gemx_last_error().decode()
        if rc == -1:
            raise ValueError(msg)
        raise GemxError(msg)


def bound_call(fn, owner, args, keep=(), result=None):
    """-> zero-argument launch() of `fn(owner._handle, *args)` with everything resolved once: a call is the FFI call and nothing else.
    The handle is read per call (None after `owner.close()` -> the C ABI's "null handle" error, not a stale pointer), a non-zero
    status goes through `check`, `result` is returned; `keep` holds the tensors and the stream behind the raw pointers in `args` for
    as long as the launcher lives."""

    def launch(_fn=fn, _owner=owner, _args=args, _result=result, _keep=keep):
        rc = _fn(_owner._handle, *_args)
        if rc:
            check(rc)
        return _result

    return launch


def counting_call(fn, owner, steps, args, keep=(), result=None):
    """`bound_call` for the launches that advance the physics: every call also moves the owner's host step counter `_k` by `steps`."""

    def launch(_fn=fn, _owner=owner, _steps=steps, _args=args, _result=result, _keep=keep):
        rc = _fn(_owner._handle, *_args)
        if rc:
            check(rc)
        _owner._k += _steps
        return _result

    return launch


def sequence(*launches, result=None):
    """-> zero-argument launch() that runs the given launchers in order (None entries are left out) and returns `result`; None when
    there is nothing to run.  (One launcher and no `result`: that launcher itself -- no frame of its own around it.)"""
    launches = tuple(f for f in launches if f is not None)
    if len(launches) < 2 and result is None:
        return launches[0] if launches else None

    def launch(_launches=launches, _result=result):
        for f in _launches:
            f()
        return _result

    return launch
