"""Batched SCML physical systems behind GEM's `PhysicalSystem` plugin surface.

`BatchedSCMLSystem` keeps the constructor and the property/method surface of the reference's `SCMLSystem`
(physical_systems/physical_systems.py:13-287) and of `gym_electric_motor.core.PhysicalSystem`
(core.py:589-705): `simulate(action)`, `reset()`, `tau`, `k`, `state_names`, `state_positions`,
`action_space`, `state_space`, `limits`, `nominal_state`, `unwrapped`, `close()`, `supply`, `converter`,
`electrical_motor`, `mechanical_load`, the `*_IDX` tables and the abc/alphabeta/dq helper transforms.
All physics runs in the HIP kernels of `libgemx.so` through the C ABI in include/gemx.h -- there is no CPU path.

* `n_envs == 1`: `simulate(action)` / `reset()` take and return 1-D numpy arrays exactly like the reference,
  so the instance drops into the unmodified `ElectricMotorEnvironment(physical_system=...)` and its wrappers.
* `n_envs > 1`: `simulate(actions[N, A])` returns a device tensor `[N, S_out]`; `done` holds the constraint
  mask of the last step; `rollout(actions[K, N, A])` runs K fused steps in one launch.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from . import components as comp
from .spaces import Box

try:  # derive from the reference's plugin base when GEM is importable, so isinstance() checks hold
    from gym_electric_motor.core import PhysicalSystem as _PhysicalSystemBase  # pragma: no cover
except Exception:

    class _PhysicalSystemBase:
        """Stand-alone equivalent of gym_electric_motor.core.PhysicalSystem (core.py:589-705)."""

        def __init__(self, action_space, state_space, state_names, tau):
            self._action_space = action_space
            self._state_space = state_space
            self._state_names = state_names
            self._state_positions = {key: index for index, key in enumerate(self._state_names)}
            self._tau = tau
            self._k = 0

        tau = property(lambda self: self._tau)
        unwrapped = property(lambda self: self)
        k = property(lambda self: self._k)
        state_names = property(lambda self: self._state_names)
        state_positions = property(lambda self: self._state_positions)
        action_space = property(lambda self: self._action_space)
        state_space = property(lambda self: self._state_space)

        def close(self):
            pass


def _is_a(obj, *names):
    """Duck typing across this package's and the reference's component classes (by class name in the MRO)."""
    mro = {c.__name__ for c in type(obj).__mro__}
    return any(n in mro for n in names)


def _torch():
    import torch

    return torch


class LimitConstraint:
    """constraints.py:31-68: violation if any observed |state| > 1 (normalised)."""

    def __init__(self, observed_state_names="all_states"):
        self.observed_state_names = observed_state_names


class SquaredConstraint:
    """constraints.py:71-98: violation if the sum of squares of the normalised states > 1."""

    def __init__(self, states=()):
        self.states = tuple(states)


def _device_index(device):
    """GPU ordinal from 0, "0", "cuda", "cuda:1" or a torch.device."""
    if isinstance(device, int):
        return device
    name = str(device)
    if name.isdigit():
        return int(name)
    kind, _, idx = name.partition(":")
    if kind != "cuda":
        raise ValueError(f"device must be a GPU ordinal or 'cuda[:i]' (there is no CPU path), got {device!r}")
    return int(idx) if idx else 0


class BatchedSCMLSystem(_PhysicalSystemBase):
    """N independent Supply-Converter-Motor-Load systems stepped in lockstep on one MI355X."""

    OMEGA_IDX = 0
    TORQUE_IDX = 1
    CURRENTS_IDX = []
    VOLTAGES_IDX = []
    U_SUP_IDX = -1

    _SYSTEM_KIND = None

    def __init__(self, converter, motor, load, supply, ode_solver, tau=1e-4, calc_jacobian=None, n_envs=1, device=0,
                 dtype="float32", constraints=(), auto_reset=None, obs_layout="aos", control_space="abc", action_frame=None,
                 action_delay=0, action_delay_reset=None, seed=0, env_base=0, env_parameters=None, _defer_create=False):
        """
        Args (first six as in SCMLSystem.__init__, physical_systems.py:54-65):
            converter, motor, load, supply: component instances (this package's or the reference's).
            ode_solver: EulerSolver(nsteps) | RK4Solver(nsteps) | DormandPrince5Solver(); scipy-backed reference
                solvers are refused (they are the CPU oracle path).
            tau(float): control step.
            calc_jacobian: accepted and ignored (explicit solvers need no Jacobian).
            n_envs(int): number of env instances advanced in lockstep.
            device(int): HIP device ordinal.
            dtype: 'float32' (product path) | 'float64' (diagnostic).
            constraints: iterable of state names (LimitConstraint), LimitConstraint / SquaredConstraint objects
                (this package's or the reference's).  They are evaluated in-kernel into the `done` mask.
            auto_reset(bool): restart an env from its initial state on the step after `done`.
                Default: True when n_envs > 1 and constraints are given, else False.
            obs_layout: 'aos' -> observations [N, S_out] (reference contract); 'soa' -> [S_out, N].
            control_space: 'abc' | 'dq' as in SynchronousMotorSystem / SquirrelCageInductionMotorSystem
                (physical_systems.py:423-435, 701-710): actions are (u_d, u_q) in the step-start (field) angle's frame.
            action_frame: None (from control_space) | 'abc' | 'dq' | 'dq_processor' -- the latter is the reference's
                DqToAbcActionProcessor wrapper folded into the kernel (angle advanced by 0.5 + action_delay steps).
            action_delay(int): DeadTimeProcessor(steps) folded into the kernel: the converter sees the action submitted
                `action_delay` steps earlier (the reset action right after a reset).
            action_delay_reset: the ONE action every reset refills that queue with (DeadTimeProcessor(reset_action=...)), in the
                action space of the system the processor wraps; None = zeros, the reference's default.
            seed(int): key of every device-side random stream (random initialisers; `rollout_synthetic` takes its own).
            env_base(int): GLOBAL index of this system's env 0.  The streams are keyed by (seed, env_base + i, ...), so the shards of
                one job (`distributed.make_sharded` sets env_base to the shard's first env) draw, env by env, what one unsharded
                system draws -- the reference gives every env object its own branch of the seed sequence (core.py:373-385,
                physical_systems.py:164-169, random_component.py:60-87).
            env_parameters: None | EnvParameters(motor=, load=, supply=) -- per-env motor, load and supply parameters (env_parameters.py):
                every env steps with its own machine; limits, initial state, p, tau, constraints and solver stay the system's own.
        """
        if control_space not in ("abc", "dq"):
            raise ValueError(f"control_space must be 'abc' or 'dq', got {control_space!r}")
        if action_frame is None:
            action_frame = "dq" if control_space == "dq" else "abc"
        if action_frame not in ("abc", "dq", "dq_processor"):
            raise ValueError(f"action_frame must be 'abc', 'dq' or 'dq_processor', got {action_frame!r}")
        self._seed = int(seed) & (2**64 - 1)
        self._env_base = int(env_base)
        if self._env_base < 0:
            raise ValueError(f"env_base must be >= 0, got {env_base!r}")
        self._action_frame = action_frame
        self._action_delay = int(action_delay)
        if not 0 <= self._action_delay <= _lib.MAX_DELAY:
            raise ValueError(f"action_delay must be in [0, {_lib.MAX_DELAY}]")
        self._action_delay_reset = None if action_delay_reset is None else [float(x) for x in np.atleast_1d(action_delay_reset).ravel()]
        self._converter = converter
        self._electrical_motor = motor
        self._mechanical_load = load
        self._supply = supply
        self._ode_solver = ode_solver
        self.control_space = control_space
        self._n_envs = int(n_envs)
        self._device = _device_index(device)
        self._dtype_name = {"float32": "float32", "float64": "float64", "f32": "float32", "f64": "float64"}[str(dtype).replace("torch.", "")]
        self._obs_layout = obs_layout
        # line 83: load.set_j_rotor(j_rotor).  The reference's set_j_rotor ADDS to j_total (mechanical_load.py:188-193),
        # so a load instance that already served another SCMLSystem must not be bumped a second time.
        j_rotor = self._electrical_motor.motor_parameter["j_rotor"]
        j_load = getattr(self._mechanical_load, "_j_load", None)
        if j_load is None or abs(self._mechanical_load.j_total - (j_load + j_rotor)) > 1e-15 * max(1.0, abs(j_load + j_rotor)):
            self._mechanical_load.set_j_rotor(j_rotor)
        state_names = self._build_state_names()
        self._set_indices()
        # PhysicalSystem.__init__ (core.py:662-676)
        action_space = self._converter.action_space
        if action_frame != "abc":
            # physical_systems.py:431-435: dq-control space is only available for continuous converters
            assert isinstance(action_space, Box), "dq-control space is only available for Continuous Controlled Converters"
            n_dq = int(action_space.shape[0]) - 1  # (u_a, u_b, u_c[, u_e]) -> (u_d, u_q[, u_e])
            action_space = Box(-1, 1, shape=(n_dq,), dtype=np.float64)
        _PhysicalSystemBase.__init__(self, action_space, None, state_names, tau)
        self._state_space = self._build_state_space(state_names)
        self._limits = np.zeros(len(state_names), dtype=float)
        self._nominal_state = np.zeros(len(state_names), dtype=float)
        self._set_limits()
        self._set_nominal_state()
        self._converter.tau = self.tau  # line 103
        self._constraints = tuple(constraints)
        limit_mask, squared_mask = self._constraint_masks(self._constraints)
        if auto_reset is None:
            auto_reset = self._n_envs > 1 and bool(limit_mask or squared_mask)
        self._auto_reset = bool(auto_reset)
        self._cfg = self._build_config(limit_mask, squared_mask)
        self._handle = None
        self._env_parameters = self._env_parameter_arrays = None
        if env_parameters is not None:
            self.set_env_parameters(env_parameters)
        if not _defer_create:  # (_defer_create: host-side config only, used by the CPU unit tests)
            self._create()

    # ------------------------------------------------------------------ reference-compatible metadata
    limits = property(lambda self: self._limits)
    nominal_state = property(lambda self: self._nominal_state)
    supply = property(lambda self: self._supply)
    converter = property(lambda self: self._converter)
    electrical_motor = property(lambda self: self._electrical_motor)
    mechanical_load = property(lambda self: self._mechanical_load)
    n_envs = property(lambda self: self._n_envs)
    env_base = property(lambda self: self._env_base, doc="global index of env 0 (the key of every device random stream is env_base + i)")
    device = property(lambda self: self._device)
    dead_time = property(lambda self: self._action_delay)  # DeadTimeProcessor.dead_time (dead_time_processor.py:43-46)

    def _set_limits(self):
        """physical_systems.py:105-113."""
        for ind, state in enumerate(self._state_names):
            motor_lim = self._electrical_motor.limits.get(state, np.inf)
            mechanical_lim = self._mechanical_load.limits.get(state, np.inf)
            self._limits[ind] = min(motor_lim, mechanical_lim)
        self._limits[self._state_positions["u_sup"]] = self.supply.u_nominal

    def _set_nominal_state(self):
        """physical_systems.py:115-123."""
        for ind, state in enumerate(self._state_names):
            motor_nom = self._electrical_motor.nominal_values.get(state, np.inf)
            mechanical_nom = self._mechanical_load.nominal_values.get(state, np.inf)
            self._nominal_state[ind] = min(motor_nom, mechanical_nom)
        self._nominal_state[self._state_positions["u_sup"]] = self.supply.u_nominal

    def _build_state_names(self):
        raise NotImplementedError

    def _build_state_space(self, state_names):
        raise NotImplementedError

    def _set_indices(self):
        raise NotImplementedError

    # ------------------------------------------------------------------ per-env parameters (env_parameters.py)
    env_parameters = property(lambda self: self._env_parameters, doc="the EnvParameters holder of this system, or None")

    def set_env_parameters(self, env_parameters):
        """Give every env its own motor, load and supply parameters (`EnvParameters`), or replace them.  Everything is checked -- what the
        per-env kernels do not serve, lengths, finiteness, j_total > 0, p -- before the handle changes."""
        from . import env_parameters as ep

        if not isinstance(env_parameters, ep.EnvParameters):
            raise ValueError("env_parameters: an EnvParameters(motor=, load=, supply=) holder")
        why = getattr(self, "_env_parameters_refusal", None) or ep.refusal(self)  # (the first: set by an env that runs a FluxObserver on this system)
        if why is not None:
            raise NotImplementedError(why)
        arrays = env_parameters.resolve(self)
        if self._handle is not None:
            ep.install(self, arrays)
        self._env_parameters, self._env_parameter_arrays = env_parameters, arrays

    def clear_env_parameters(self):
        """Back to one parameter set for every env: the system's own (`gemx_clear_env_params`)."""
        if self._handle is not None:
            _lib.check(self._L.gemx_clear_env_params(self._handle))
        self._env_parameters = self._env_parameter_arrays = None

    def get_env_parameter_table(self):
        """The device table [F, N] as it sits on the device (`gemx_get_env_params`; field order: include/gemx.h), or None without one."""
        if self._env_parameters is None:
            return None
        from .env_parameters import table_fields

        out = _torch().empty((table_fields(self._SYSTEM_KIND), self._n_envs), dtype=self._tdtype, device=self._tdev)
        _lib.check(self._L.gemx_get_env_params(self._handle, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def _refuse_with_env_parameters(self, what):
        if self._env_parameters is not None:
            from .env_parameters import REFUSAL

            raise NotImplementedError(REFUSAL + what)

    def _check_env_parameters_checkpoint(self, ckpt):
        """The checkpoint's table and this system's agree in presence, shape and, on a created system, value (before anything is restored)."""
        from .env_parameters import table_fields

        tab = ckpt.get("env_parameters")
        if (tab is None) != (self._env_parameters is None):
            raise ValueError("checkpoint and system disagree on per-env parameters: " +
                             ("the checkpoint carries a parameter table, this system has none" if tab is not None else
                              "this system has a parameter table (env_parameters=), the checkpoint carries none"))
        if tab is not None and tuple(tab.shape) != (table_fields(self._SYSTEM_KIND), self._n_envs):
            raise ValueError(f"checkpoint per-env parameter table has shape {tuple(tab.shape)}, this system's is "
                             f"{(table_fields(self._SYSTEM_KIND), self._n_envs)}: it was taken from a system of another n_envs or motor")
        if tab is not None and self._handle is not None:  # the same machines, value for value: a run continues only on the parameters it ran on
            torch = _torch()
            own = self.get_env_parameter_table()
            if not torch.equal(torch.as_tensor(tab).to(device=own.device, dtype=own.dtype), own):
                raise ValueError("checkpoint per-env parameter table differs in value from this system's: the checkpoint was taken with other "
                                 "per-env parameters (build the system with the env_parameters= of the run it continues)")

    # ------------------------------------------------------------------ config extraction
    def _constraint_masks(self, constraints):
        """Map the env's `constraints` argument (core.py:256-262) onto bit masks over the system state."""
        pos = {n: i for i, n in enumerate(self._build_state_names())}
        limit_mask = squared_mask = 0

        def bit(n):
            if n not in pos:  # (also the columns a wrapper appends behind the system's own, 'i_sum', 'cos(epsilon)': not evaluated in-kernel)
                raise ValueError(f"constraint on {n!r}: not a state of this system {tuple(pos)}")
            return 1 << pos[n]

        for c in constraints:
            if isinstance(c, str):
                names = list(pos) if c == "all_states" else [c]
                for n in names:
                    limit_mask |= bit(n)
            elif _is_a(c, "LimitConstraint"):
                names = getattr(c, "observed_state_names", None)
                if names is None:
                    names = getattr(c, "_observed_state_names", [])
                if isinstance(names, str):
                    names = [names]
                if "all_states" in names:
                    names = list(pos)
                for n in names:
                    limit_mask |= bit(n)
            elif _is_a(c, "SquaredConstraint"):
                if squared_mask:
                    raise ValueError("only one SquaredConstraint is supported in-kernel")
                names = getattr(c, "states", None) or getattr(c, "_states", ())
                for n in names:
                    squared_mask |= bit(n)
            else:
                raise ValueError(f"constraint {c!r} cannot be evaluated in-kernel (supported: state names, "
                                 "LimitConstraint, SquaredConstraint)")
        return limit_mask, squared_mask

    def _converter_kind(self):
        c = self._converter
        if _is_a(c, "ContMultiConverter", "FiniteMultiConverter"):
            subs = list(getattr(c, "_sub_converters", ()))
            names = tuple(next((n for n in ("ContFourQuadrantConverter", "FiniteFourQuadrantConverter", "ContB6BridgeConverter",
                                            "FiniteB6BridgeConverter") if _is_a(sc, n)), type(sc).__name__) for sc in subs)
            kinds = {("ContFourQuadrantConverter", "ContFourQuadrantConverter"): _lib.CONV_CONT_2X4QC,
                     ("FiniteFourQuadrantConverter", "FiniteFourQuadrantConverter"): _lib.CONV_FINITE_2X4QC,
                     ("ContB6BridgeConverter", "ContFourQuadrantConverter"): _lib.CONV_CONT_B6_4QC,
                     ("FiniteB6BridgeConverter", "FiniteFourQuadrantConverter"): _lib.CONV_FINITE_B6_4QC,
                     ("ContB6BridgeConverter", "ContB6BridgeConverter"): _lib.CONV_CONT_2XB6,
                     ("FiniteB6BridgeConverter", "FiniteB6BridgeConverter"): _lib.CONV_FINITE_2XB6}
            if names not in kinds:
                raise ValueError(f"multi converter of {names} is not on the accelerated path (supported: 2 x 4QC for the externally "
                                 "excited DC motor, B6 + 4QC for the EESM, 2 x B6 for the DFIM)")
            return kinds[names]
        if _is_a(c, "ContFourQuadrantConverter"):
            return _lib.CONV_CONT_4QC
        if _is_a(c, "FiniteB6BridgeConverter"):
            return _lib.CONV_FINITE_B6
        if _is_a(c, "FiniteFourQuadrantConverter"):
            return _lib.CONV_FINITE_4QC
        if _is_a(c, "ContB6BridgeConverter"):
            return _lib.CONV_CONT_B6
        raise ValueError(f"converter {type(c).__name__} is not on the accelerated path "
                         "(supported: ContFourQuadrantConverter, FiniteFourQuadrantConverter, FiniteB6BridgeConverter, ContB6BridgeConverter)")

    def _interlocking_time(self):
        """converter dead time.  A MultiConverter's own value is never used by the reference (converters.py:498-740): its
        sub-converters' values are; the kernels take one value, so they must agree."""
        c = self._converter
        subs = getattr(c, "_sub_converters", None)
        if subs is None:
            return float(getattr(c, "_interlocking_time", 0.0))
        tils = {float(getattr(sc, "_interlocking_time", 0.0)) for sc in subs}
        if len(tils) != 1:
            raise ValueError(f"the sub-converters of a multi converter must share one interlocking_time on the accelerated path, got {sorted(tils)}")
        return tils.pop()

    def _adaptive_tolerances(self):
        """(rtol, atol) if the solver is the error-controlled one: this package's ScipyOdeSolver, or the REFERENCE's own
        ScipyOdeSolver('dopri5', **kwargs) instance (solvers.py:139-184; scipy's defaults rtol 1e-6, atol 1e-12 -> device floor 1e-9)."""
        s = self._ode_solver
        if getattr(s, "_adaptive", False):
            return float(s._rtol), float(s._atol)
        if _is_a(s, "ScipyOdeSolver") and getattr(s, "_integrator", None) == "dopri5":
            kw = dict(getattr(s, "_solver_args", {}) or {})
            return float(kw.get("rtol", 1e-6)), max(float(kw.get("atol", 1e-12)), 1e-9)
        return None

    def _solver_kind(self):
        s = self._ode_solver
        if self._adaptive_tolerances() is not None:
            return _lib.SOLVER_DP5, 1
        nsteps = int(getattr(s, "_nsteps", 1))
        if _is_a(s, "EulerSolver"):
            return _lib.SOLVER_EULER, nsteps
        if _is_a(s, "RK4Solver"):
            return _lib.SOLVER_RK4, nsteps
        if _is_a(s, "DormandPrince5Solver"):
            return _lib.SOLVER_DP5, nsteps
        raise ValueError(f"ode_solver {type(s).__name__} is a CPU (scipy) solver; the GPU path takes EulerSolver, RK4Solver, "
                         "DormandPrince5Solver or ScipyOdeSolver('dopri5') (error-controlled Dormand-Prince on the device)")

    def _load_params(self):
        ld = self._mechanical_load
        if _is_a(ld, "ConstantSpeedLoad"):
            return _lib.LOAD_CONST_SPEED, 0.0, 0.0, 0.0, 1e-3, float(ld.omega_fixed)
        if _is_a(ld, "PolynomialStaticLoad"):
            lp = ld.load_parameter
            init = getattr(ld, "initializer", {}) or {}
            omega0 = float((init.get("states") or {}).get("omega", 0.0))
            return _lib.LOAD_POLY_STATIC, float(lp["a"]), float(lp["b"]), float(lp["c"]), float(ld.tau_decay), omega0
        raise ValueError(f"load {type(ld).__name__} is not on the accelerated path (supported: ConstantSpeedLoad, PolynomialStaticLoad)")

    def _torque_coefficients(self):
        from . import components as comp

        m = self._electrical_motor
        return comp.torque_coefficients(m, comp.derived_parameters(m, m.motor_parameter))

    def _initial_motor_state(self):
        m = self._electrical_motor
        if hasattr(m, "initial_motor_state"):
            return m.initial_motor_state()
        init = getattr(m, "initializer", None) or {}
        states = init.get("states") or {}
        n_motor = self._n_ode - 1
        vals = [float(v) for v in states.values()]
        return vals if len(vals) == n_motor else [0.0] * n_motor

    def _build_config(self, limit_mask, squared_mask):
        cfg = _lib.GemxConfig()
        cfg.struct_size = C.sizeof(_lib.GemxConfig)
        cfg.abi_version = _lib.ABI_VERSION
        cfg.system_kind = self._SYSTEM_KIND
        cfg.converter_kind = self._converter_kind()
        one_u = (_lib.CONV_CONT_4QC, _lib.CONV_FINITE_4QC)
        b6 = (_lib.CONV_CONT_B6, _lib.CONV_FINITE_B6)
        allowed = {_lib.SYS_DC_PERMEX: one_u, _lib.SYS_DC_SERIES: one_u, _lib.SYS_DC_SHUNT: one_u, _lib.SYS_SYNC: b6, _lib.SYS_SCIM: b6,
                   _lib.SYS_DC_EXTEX: (_lib.CONV_CONT_2X4QC, _lib.CONV_FINITE_2X4QC),
                   _lib.SYS_EESM: (_lib.CONV_CONT_B6_4QC, _lib.CONV_FINITE_B6_4QC),
                   _lib.SYS_DFIM: (_lib.CONV_CONT_2XB6, _lib.CONV_FINITE_2XB6)}[self._SYSTEM_KIND]
        if cfg.converter_kind not in allowed:  # (gemx_create refuses it as well)
            raise ValueError(f"converter {type(self._converter).__name__} does not fit {type(self).__name__} with a "
                             f"{type(self._electrical_motor).__name__}: it is not on the accelerated path")
        cfg.solver_kind, cfg.solver_nsteps = self._solver_kind()
        cfg.solver_flags = _lib.SOLVER_SPLIT_KINKS if getattr(self._ode_solver, "_split_kinks", False) else 0
        tol = self._adaptive_tolerances()
        if tol is not None:  # ScipyOdeSolver: error-controlled DP5
            # (kinks in closed form unless the caller opts out -- ScipyOdeSolver(split_kinks=False); the reference's own instance has no such
            # attribute and gets the default.  Ignored by the library for loads without a kink.)
            cfg.solver_flags = _lib.SOLVER_ADAPTIVE | (_lib.SOLVER_SPLIT_KINKS if getattr(self._ode_solver, "_split_kinks", True) else 0)
            cfg.solver_rtol, cfg.solver_atol = tol
            cfg.solver_atol_omega = float(getattr(self._ode_solver, "_atol_omega", 0.0))  # (0: atol x the speed limit)
        cfg.dtype = _lib.F64 if self._dtype_name == "float64" else _lib.F32
        cfg.obs_layout = {"aos": _lib.OBS_AOS, "soa": _lib.OBS_SOA}[self._obs_layout]
        cfg.auto_reset = int(self._auto_reset)
        cfg.limit_mask, cfg.squared_mask = limit_mask, squared_mask
        cfg.action_frame = {"abc": _lib.ACT_ABC, "dq": _lib.ACT_DQ_SPACE, "dq_processor": _lib.ACT_DQ_PROCESSOR}[self._action_frame]
        cfg.action_delay = self._action_delay
        if self._action_delay_reset is not None:
            # validated against the WRAPPED system's action space, entry by entry (advisor finding, round 4: a short continuous row was
            # zero-padded in silence, values beyond the bounds and MultiDiscrete components beyond theirs -- [n0, 0] aliases the flat
            # index of [0, 1] -- were accepted)
            row = list(np.atleast_1d(np.asarray(self._action_delay_reset, dtype=float)).ravel())
            space = self.action_space
            nvec = getattr(space, "nvec", None)
            if nvec is not None:  # MultiDiscrete([n0, n1]): the pair, or the flat index the kernel reads (include/gemx.h)
                nv = [int(v) for v in nvec]
                if len(row) == len(nv):
                    if any(not (float(v).is_integer() and 0 <= v < n) for v, n in zip(row, nv)):
                        raise ValueError(f"action_delay_reset {row} is not an element of {space}")
                    row = [row[0] + nv[0] * row[1]]
                elif not (len(row) == 1 and float(row[0]).is_integer() and 0 <= row[0] < int(np.prod(nv))):
                    raise ValueError(f"action_delay_reset {row} is neither an element of {space} nor a flat index below {int(np.prod(nv))}")
            elif hasattr(space, "n"):  # Discrete(n)
                if not (len(row) == 1 and float(row[0]).is_integer() and 0 <= row[0] < int(space.n)):
                    raise ValueError(f"action_delay_reset {row} is not an element of {space}")
            else:  # Box: exact length, inside the bounds
                lo, hi = np.asarray(space.low, dtype=float).ravel(), np.asarray(space.high, dtype=float).ravel()
                if self._action_frame == "dq_processor":  # the DeadTimeProcessor sits INSIDE the dq processor: it wraps the abc system
                    n_abc = 4 if self._SYSTEM_KIND == _lib.SYS_EESM else 3  # duty cycles (u_a, u_b, u_c[, u_e]) in [-1, 1]
                    lo, hi = -np.ones(n_abc), np.ones(n_abc)
                if len(row) != len(lo) or any(not (l <= v <= h_) for v, l, h_ in zip(row, lo, hi)):
                    raise ValueError(f"action_delay_reset {row} is not an element of {space} (length {len(lo)}, bounds [{lo.min()}, {hi.max()}])")
            for i, v in enumerate(row):
                cfg.action_delay_reset[i] = float(v)
        if self._action_frame != "abc":
            sysk, convk = self._SYSTEM_KIND, self._converter_kind()
            ok = (self._action_frame == "dq" and sysk in (_lib.SYS_SYNC, _lib.SYS_SCIM) and convk == _lib.CONV_CONT_B6) or \
                 (self._action_frame == "dq_processor" and ((sysk == _lib.SYS_SYNC and convk == _lib.CONV_CONT_B6) or
                                                           (sysk == _lib.SYS_EESM and convk == _lib.CONV_CONT_B6_4QC)))
            if not ok:  # (gemx_create refuses it as well)
                raise ValueError(f"action_frame={self._action_frame!r} is not available for {type(self).__name__} with a "
                                 f"{type(self._converter).__name__}: control_space='dq' needs a synchronous or squirrel-cage system, "
                                 "the dq processor a synchronous or EESM system, both a continuous B6 converter")
        cfg.tau = float(self.tau)
        cfg.interlocking_time = self._interlocking_time()
        cfg.u_nominal = float(self._supply.u_nominal)
        if _is_a(self._supply, "RCVoltageSupply"):
            cfg.supply_kind, cfg.supply_r, cfg.supply_c = _lib.SUPPLY_RC, float(self._supply._r), float(self._supply._c)
        elif not _is_a(self._supply, "IdealVoltageSupply"):
            raise ValueError(f"supply {type(self._supply).__name__} is not on the accelerated path (supported: IdealVoltageSupply, RCVoltageSupply)")
        model = np.zeros((_lib.MODEL_ROWS, _lib.MODEL_COLS))
        mc = np.asarray(self._electrical_motor._model_constants, dtype=float)
        model[: mc.shape[0], : mc.shape[1]] = mc
        for i, v in enumerate(model.ravel()):
            cfg.model[i] = v
        for i, v in enumerate(self._torque_coefficients()):
            cfg.torque_coef[i] = v
        kind, a, b, c_, tau_decay, omega0 = self._load_params()
        cfg.load_kind = kind
        cfg.j_total = float(self._mechanical_load.j_total)
        cfg.load_a, cfg.load_b, cfg.load_c, cfg.tau_decay = a, b, c_, tau_decay
        for i, v in enumerate(self._limits):
            cfg.limits[i] = float(v)
        init = [omega0] + list(self._initial_motor_state())
        assert len(init) == self._n_ode
        for i, v in enumerate(init):
            cfg.init_state[i] = float(v)
        self._fill_random_init(cfg)
        return cfg

    def _fill_random_init(self, cfg):
        """Random initialisers (`motor_initializer` / `load_initializer` with random_init='uniform' | 'gaussian'): per-ODE-state
        sampling bounds exactly as electric_motor.py:199-227 / mechanical_load.py:117-130 derive them -- upper = nominal value of the
        state, lower = upper * state_space.low, both clipped to `interval` -- in the ODE slot order the reference fills (the VALUES of
        the `states` dict in dict order, electric_motor.py:270-285).
        Induction machines (electric_motor.py:197-211: bounds from `_initial_limits` = the nominal values, lower = -upper for every
        state): the stator currents and the angle are static bounds like everyone else's; the two FLUX bounds are re-derived at every
        reset from a random field angle (induction_motor.py:174-185, 250-285) -- gemx_config.init_flux_mode / init_flux carry what
        that needs, and the flux slots' init_lo / init_hi hold the user's `interval` only."""
        pos, low = self._state_positions, np.asarray(self._state_space.low, dtype=float)
        kinds = set()
        mot = self._electrical_motor
        induction = _is_a(mot, "SquirrelCageInductionMotor") or _is_a(mot, "DoublyFedInductionMotor") or _is_a(mot, "InductionMotor")

        def bounds(component, nominal_of, slot0, symmetric=False):
            ini = getattr(component, "initializer", None) or {}
            dist = ini.get("random_init")
            if dist is None:
                return
            kinds.add("uniform" if dist == "uniform" else "gaussian")
            names = list((ini.get("states") or {}).keys())
            interval = ini.get("interval")
            mue, sigma = (ini.get("random_params") or (None, None))
            for k_, name in enumerate(names):
                flux = symmetric and name.startswith("psi_")
                if flux:
                    lo, up = -math.inf, math.inf  # this reset's +-psi_d_max (|cos|, |sin|) on the device, clipped to the interval below
                else:
                    up = abs(float(nominal_of(name))) if symmetric else float(nominal_of(name))
                    lo = -up if symmetric else (up * low[pos[name]] if name in pos else -up)  # epsilon etc. are system states too
                if interval is not None:
                    iv = np.asarray(interval, dtype=float).reshape(-1, 2)
                    lo, up = max(lo, iv[k_][0]), min(up, iv[k_][1])
                j = slot0 + k_
                cfg.init_lo[j], cfg.init_hi[j] = lo, up
                cfg.init_mu[j] = float(mue) if mue else (math.nan if flux else (up - lo) / 2 + lo)  # (NaN: the middle of this reset's bounds)
                cfg.init_sigma[j] = float(sigma) if sigma else 1.0

        ld = self._mechanical_load
        bounds(ld, lambda n: self._nominal_state[pos[n]], 0)
        bounds(mot, lambda n: mot.nominal_values[n], 1, symmetric=induction)
        if len(kinds) > 1:
            raise ValueError("motor and load initialisers must use the same distribution on the accelerated path")
        cfg.init_kind = {"uniform": _lib.INIT_UNIFORM, "gaussian": _lib.INIT_GAUSSIAN}[kinds.pop()] if kinds else _lib.INIT_CONST
        cfg.seed = self._seed
        cfg.env_base = self._env_base
        if induction and (getattr(mot, "initializer", None) or {}).get("random_init") is not None:
            names = list(((mot.initializer or {}).get("states") or {}).keys())
            if names[:4] != ["i_salpha", "i_sbeta", "psi_ralpha", "psi_rbeta"]:
                raise ValueError(f"induction-motor initialiser states {names}: the accelerated path expects the reference's order "
                                 "i_salpha, i_sbeta, psi_ralpha, psi_rbeta, epsilon (induction_motor.py:107-118)")
            mp, nv = mot.motor_parameter, mot.nominal_values
            l_s, l_r = mp["l_m"] + mp["l_sigs"], mp["l_m"] + mp["l_sigr"]
            l_mr = mp["l_m"] / l_r
            sigma_l = (l_s * l_r - mp["l_m"] ** 2) / (l_s * l_r)
            u_rq = float(nv.get("u_rq", 0.0)) if _is_a(mot, "DoublyFedInductionMotor") else 0.0  # doubly_fed_induction_motor.py:158-163
            vals = [mp["l_m"] * nv["i_sd"], mp["p"], sigma_l * l_s, mp["r_s"] + mp["r_r"] * l_mr ** 2, nv["u_sq"] + l_mr * u_rq, l_mr, mp["l_m"], 0.0]
            cfg.init_flux_mode = 1
            for i, v in enumerate(vals):
                cfg.init_flux[i] = float(v)

    # ------------------------------------------------------------------ device plumbing (torch = memory + streams)
    def _create(self):
        torch = _torch()
        L = _lib.load()
        if L.gemx_device_count() <= 0 or not torch.cuda.is_available():
            raise _lib.GemxError("no HIP device visible: gym_electric_motor_amd has no CPU fallback "
                                 "(the CPU restatement under oracle/ is test infrastructure, not a product path)")
        h = C.c_void_p()
        _lib.check(L.gemx_create(C.byref(self._cfg), self._n_envs, self._device, C.byref(h)))
        self._handle = h
        self._L = L
        self._tdev = torch.device("cuda", self._device)
        self._tdtype = torch.float64 if self._dtype_name == "float64" else torch.float32
        self._n_out = L.gemx_n_out(h)
        self._n_act = L.gemx_n_action(h)
        self._discrete = L.gemx_action_itemsize(h) == 1
        shape = (self._n_envs, self._n_out) if self._obs_layout == "aos" else (self._n_out, self._n_envs)
        self._obs = torch.empty(shape, dtype=self._tdtype, device=self._tdev)
        self._done = torch.zeros(self._n_envs, dtype=torch.uint8, device=self._tdev)
        self._obs_ptr, self._done_ptr = self._obs.data_ptr(), self._done.data_ptr()
        ro = (C.c_double * _lib.MAX_OUT)()
        _lib.check(L.gemx_reset_observation(h, ro))
        self._reset_obs = np.array(ro[: self._n_out], dtype=float)
        # the internal observation buffer starts out as the reset observation of every env (reset(mask) returns it for rows outside the mask)
        # (random initialisers: gemx_create left draw #1 in place with the counters at 1; gemx_reset_again re-creates that draw -- the same
        # states, now with their observation rows -- without advancing, so the user's first reset() and an env's first in-kernel auto-reset
        # are both draw #2.  Launched on the stream that is current at construction and waited for, so that a caller stepping on another
        # stream later needs no event.)
        _lib.check(L.gemx_reset_again(h, None, C.c_void_p(self._obs.data_ptr()), self._stream()))
        torch.cuda.current_stream(self._tdev).synchronize()
        # closed-loop hot path (simulate() on a device tensor): everything a call needs, bound once
        self._Tensor = torch.Tensor
        self._want_dtype = torch.uint8 if self._discrete else self._tdtype
        self._act_numel = self._n_envs * (1 if self._discrete else self._n_act)
        self._gemx_step = L.gemx_step
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # the current stream's handle without a Stream object
        self._cur_stream = torch.cuda.current_stream
        if getattr(self, "_env_parameter_arrays", None) is not None:  # (a system re-created after close() keeps its table)
            from .env_parameters import install

            install(self, self._env_parameter_arrays)

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self._tdev).cuda_stream)

    def close(self):
        if getattr(self, "_handle", None) is not None:
            self._L.gemx_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _actions_to_device(self, actions, leading):
        """-> contiguous device tensor of shape leading + (A,) (float R) or leading (uint8)."""
        torch = _torch()
        want_dtype = torch.uint8 if self._discrete else self._tdtype
        if torch.is_tensor(actions) and actions.dtype == want_dtype and actions.device == self._tdev and actions.is_contiguous():
            n = 1
            for d in leading:
                n *= d
            if actions.numel() == n * (1 if self._discrete else self._n_act):
                return actions  # fast path: already what the kernel reads (no torch ops on the hot path)
        nvec = getattr(self.action_space, "nvec", None)
        if self._discrete and nvec is not None:
            # MultiDiscrete([n0, n1]) of a FiniteMultiConverter: [..., 2] sub-actions -> the flat index a0 + n0 * a1 the kernel
            # reads (include/gemx.h); an already flat tensor of shape `leading` passes through
            n0, n1 = int(nvec[0]), int(nvec[1])
            if not torch.is_tensor(actions):
                arr = np.asarray(actions)
                if arr.shape[-1:] == (2,) and arr.size == 2 * int(np.prod(leading)):
                    if arr.size and (arr.min() < 0 or (arr[..., 0] >= n0).any() or (arr[..., 1] >= n1).any()):
                        raise AssertionError(f"The selected action {arr.reshape(-1, 2)[0]} is not a valid element of the action space {self.action_space}.")
                    arr = arr[..., 0] + n0 * arr[..., 1]
                elif arr.size and (arr.min() < 0 or arr.max() >= n0 * n1):
                    raise AssertionError(f"The selected flat action is not a valid element of the action space {self.action_space}.")
                actions = torch.as_tensor(arr.astype(np.uint8))
            elif actions.shape[-1:] == (2,) and actions.numel() == 2 * int(np.prod(leading)):
                actions = actions[..., 0] + n0 * actions[..., 1]
            return actions.to(device=self._tdev, dtype=torch.uint8).reshape(leading).contiguous()
        if self._discrete:
            if not torch.is_tensor(actions):
                arr = np.asarray(actions)
                nmax = int(self.action_space.n) - 1
                if arr.size and (arr.min() < 0 or arr.max() > nmax):
                    bad = arr.ravel()[(arr.ravel() < 0) | (arr.ravel() > nmax)][0]
                    raise AssertionError(f"The selected action {bad} is not a valid element of the action space {self.action_space}.")
                actions = torch.as_tensor(arr.astype(np.uint8))
            t = actions.to(device=self._tdev, dtype=torch.uint8).reshape(leading).contiguous()
        else:
            if not torch.is_tensor(actions):
                actions = torch.as_tensor(np.asarray(actions, dtype=np.float64))
            t = actions.to(device=self._tdev, dtype=self._tdtype).reshape(leading + (self._n_act,)).contiguous()
        return t

    # ------------------------------------------------------------------ the plugin surface
    @property
    def done(self):
        """uint8 device tensor [N]: constraint violation (`terminated`, core.py:350) of the last simulate()."""
        return self._done

    @property
    def reward(self):
        """[N] device tensor: reward of the last `simulate(action, references=...)` (fused WeightedSumOfErrors)."""
        return None if getattr(self, "_reward_buf", None) is None else self._reward_buf[0]

    @property
    def reset_observation(self):
        """Normalised state every env shows right after a reset (constant initialiser), numpy [S_out]."""
        return self._reset_obs.copy()

    def simulate(self, action, *_, references=None, **__):
        """One control step.  n_envs == 1: 1-D numpy in / out (reference contract, physical_systems.py:171-203).
        Otherwise `action` is [N, A] (float) or [N] (discrete) and the returned device tensor ([N, S_out]) is an
        internal buffer that the next call overwrites.
        references [N, n_ref] (after `set_reward`): the step's reward is evaluated in the same launch -> `self.reward` [N]."""
        # hot path of a closed loop (policy -> simulate -> policy ...): a contiguous device tensor of the dtype the kernel reads goes
        # straight to the C ABI -- one type test, four tensor attributes, one ctypes call (the launch itself is ~3.9 us of HIP runtime)
        if references is None and type(action) is self._Tensor and action.dtype is self._want_dtype and action.numel() == self._act_numel \
                and action.is_contiguous() and action.device == self._tdev and self._n_envs > 1:
            rs = self._raw_stream
            rc = self._gemx_step(self._handle, action.data_ptr(), self._obs_ptr, self._done_ptr,
                                 rs(self._device) if rs is not None else self._cur_stream(self._tdev).cuda_stream)
            if rc:
                _lib.check(rc)
            self._k += 1
            return self._obs
        if references is not None:
            torch = _torch()
            a = self._actions_to_device(action, (self._n_envs,))
            if getattr(self, "_reward_buf", None) is None:
                self._reward_buf = torch.empty((1, self._n_envs), dtype=self._tdtype, device=self._tdev)
            self._rollout_reward(a.reshape((1,) + tuple(a.shape)), 1, self._obs.reshape((1,) + tuple(self._obs.shape)),
                                 self._done.reshape(1, -1), torch.as_tensor(references).reshape(1, self._n_envs, -1), self._reward_buf)
            return self._obs
        single = self._n_envs == 1 and not _torch().is_tensor(action)
        if single and self._discrete and not hasattr(self.action_space, "nvec"):
            assert self.action_space.contains(action), (  # converters.py:204-206
                f"The selected action {action} is not a valid element of the action space {self.action_space}.")
        a = self._actions_to_device(action, (self._n_envs,))
        rc = self._L.gemx_step(self._handle, a.data_ptr(), self._obs_ptr, self._done_ptr,
                               _torch().cuda.current_stream(self._tdev).cuda_stream)
        if rc:
            _lib.check(rc)
        self._k += 1
        if single:
            return self._obs.reshape(-1).double().cpu().numpy()
        return self._obs

    def bind_step(self, action_buffer, stream=None):
        """A zero-argument `step()` for a closed loop that reuses ONE action tensor (the policy writes into it): everything a launch needs
        -- handle, the action / observation / done pointers, the stream -- is resolved here, once, so a call is nothing but the FFI call
        `gemx_step` (about 0.5 us of Python less than `simulate(action)`, which has to look at its argument every time).  Returns
        `(step, obs, done)`: `step()` advances every env by one control step with the actions currently in `action_buffer` and returns
        `obs` -- the internal observation tensor [N, S_out], overwritten by every step, like simulate()'s; `done` [N] uint8 likewise.
        `stream`: a torch.cuda.Stream to launch on (default: the stream current NOW; a stepper bound to one stream keeps using it)."""
        torch = _torch()
        a = action_buffer
        if not (torch.is_tensor(a) and a.device == self._tdev and a.is_contiguous() and a.dtype is self._want_dtype and a.numel() == self._act_numel):
            raise ValueError(f"bind_step needs a contiguous {self._want_dtype} tensor of {self._act_numel} elements on {self._tdev}")
        stream = stream if stream is not None else torch.cuda.current_stream(self._tdev)  # (the Stream OBJECT is kept: its raw handle must not dangle)
        args = (C.c_void_p(a.data_ptr()), C.c_void_p(self._obs_ptr), C.c_void_p(self._done_ptr), C.c_void_p(stream.cuda_stream))
        # (the buffers behind the raw pointers stay alive as long as the stepper does; the handle is read per call: _lib.bound_call)
        return _lib.counting_call(self._gemx_step, self, 1, args, (a, stream), self._obs), self._obs, self._done

    def bind_rollout(self, actions, obs_out, done_out, stream=None):
        """A zero-argument `launch()` for a loop that reuses its tensors (a fixed action chunk -- or one the policy overwrites -- and fixed
        output buffers): what `rollout(actions, obs_out=..., done_out=...)` checks and converts on every call -- dtype, device, shape,
        contiguity, pointers, the stream -- is resolved here, once, and a call is the FFI call `gemx_rollout` and nothing else.  Python's
        share of a `rollout()` call is 8-12 us, which is what a short launch costs on the device as well (BASELINE config 2: 4096 envs x
        1000 steps = 18.5 us of kernel): without this the host sets the pace there.  Returns `launch`; `launch()` returns
        `(obs_out, done_out)`.  `stream`: a torch.cuda.Stream to launch on (default: the stream current NOW).  (Observations of every step,
        no fused reward: those launches take `rollout(..., references=...)`.)"""
        torch = _torch()
        if not torch.is_tensor(actions) or actions.dim() < 1:
            raise ValueError("bind_rollout needs a device tensor of actions [K, N, A] / [K, N]")
        K = int(actions.shape[0])
        a = actions
        half = a.dtype is torch.float16 and not self._discrete and self._tdtype == torch.float32 and K >= 2  # (narrow action tensor: gemx_rollout_half)
        if half:
            self._refuse_with_env_parameters("a half-precision action tensor (fp32 actions)")
        if not (a.device == self._tdev and a.is_contiguous() and (a.dtype is self._want_dtype or half) and a.numel() == K * self._act_numel):
            raise ValueError(f"bind_rollout needs a contiguous {self._want_dtype} (continuous converters, fp32: or float16) tensor of {K} x {self._act_numel} elements on {self._tdev}")
        oshape, dshape = (K,) + tuple(self._obs.shape), (K, self._n_envs)
        if not (torch.is_tensor(obs_out) and tuple(obs_out.shape) == oshape and obs_out.is_contiguous() and obs_out.dtype == self._tdtype and obs_out.device == self._tdev):
            raise ValueError(f"bind_rollout: obs_out must be a contiguous {self._tdtype} tensor of shape {oshape} on {self._tdev}")
        if not (torch.is_tensor(done_out) and tuple(done_out.shape) == dshape and done_out.is_contiguous() and done_out.dtype == torch.uint8 and done_out.device == self._tdev):
            raise ValueError(f"bind_rollout: done_out must be a contiguous uint8 tensor of shape {dshape} on {self._tdev}")
        stream = stream if stream is not None else torch.cuda.current_stream(self._tdev)  # (the Stream OBJECT is kept: its raw handle must not dangle)
        args = (C.c_void_p(a.data_ptr()), K, C.c_void_p(obs_out.data_ptr()), C.c_void_p(done_out.data_ptr())) + (() if half else (1,)) + (C.c_void_p(stream.cuda_stream),)
        # (the buffers and the stream behind the raw pointers stay alive as long as the launcher does)
        return _lib.counting_call(self._L.gemx_rollout_half if half else self._L.gemx_rollout, self, K, args, (a, obs_out, done_out, stream), (obs_out, done_out))

    def bind_rollout_episodic(self, actions, length, max_steps, obs_out, terminated_out, truncated_out, ended_out, stream=None):
        """A zero-argument `launch()` of `gemx_rollout_episodic` on fixed tensors: K fused control steps with the episode time limit
        `max_steps` INSIDE the launch (csrc/gemx_episodic.hip) -- per env `length += 1; truncated = length >= max_steps and not
        terminated`, and every ended env restarts from the reset state within the launch.  actions [K, N, A] / [K, N] as `bind_rollout`
        takes them (no float16); length [N] int32, the steps of every env's running episode, READ only (the episode stage's rows pass
        behind this launch moves the counters: episodes.py); obs_out [K, N, S_out] (or [K, S_out, N]); terminated_out, truncated_out,
        ended_out [K, N] uint8.  The tensors are the caller's to get right -- contiguous, of these dtypes, on the system's device: the
        envs' `*_episodic` methods validate them and raise what the kernel does not serve before anything is launched; called directly,
        the C ABI refuses such a handle.  `launch()` returns `(obs_out, terminated_out, truncated_out, ended_out)`."""
        from .episodes import check_max_episode_steps

        M = check_max_episode_steps(max_steps)
        if M is None:
            raise ValueError("bind_rollout_episodic needs max_steps >= 1")
        if self._handle is None:
            raise _lib.GemxError("the physical system has no device handle (built with _defer_create, or closed)")
        torch = _torch()
        K, a = int(actions.shape[0]), actions
        stream = stream if stream is not None else torch.cuda.current_stream(self._tdev)  # (the Stream OBJECT is kept: its raw handle must not dangle)
        args = (C.c_void_p(a.data_ptr()), K, C.c_void_p(length.data_ptr()), M, C.c_void_p(obs_out.data_ptr()), C.c_void_p(terminated_out.data_ptr()),
                C.c_void_p(truncated_out.data_ptr()), C.c_void_p(ended_out.data_ptr()), C.c_void_p(stream.cuda_stream))
        out = (obs_out, terminated_out, truncated_out, ended_out)
        return _lib.counting_call(self._L.gemx_rollout_episodic, self, K, args, (a, length, stream) + out, out)

    def rollout(self, actions, obs_out=None, done_out=None, last_only=False, references=None, reward_out=None):
        """K fused control steps in one launch.  actions: [K, N, A] / [K, N]; returns (obs [K, N, S_out], done [K, N])
        device tensors (or the last step's [N, S_out], [N] with last_only=True).
        references [K, N, n_ref] (after `set_reward`): additionally returns reward [K, N] computed in the same launch."""
        torch = _torch()
        K = int(actions.shape[0])
        if references is not None or reward_out is not None:
            return self._rollout_reward(actions, K, obs_out, done_out, references, reward_out)
        # a HALF action tensor (continuous converters, fp32 systems): taken as it is -- gemx_rollout_half widens the values while they are
        # staged (6 instead of 12 bytes per env-step for three duty cycles; the results are those of the same values fed as fp32)
        half = (torch.is_tensor(actions) and actions.dtype == torch.float16 and not self._discrete and self._tdtype == torch.float32 and not last_only)
        if last_only:
            self._refuse_with_env_parameters("last-step-only launches (last_only=True)")
        if half:
            self._refuse_with_env_parameters("a half-precision action tensor (fp32 actions)")
            if not (actions.device == self._tdev and actions.is_contiguous() and actions.numel() == K * self._act_numel and K >= 2):
                raise ValueError(f"rollout: a float16 action tensor must be a contiguous device tensor of {K} x {self._act_numel} elements on {self._tdev}, K >= 2")
            a = actions
        else:
            a = self._actions_to_device(actions, (K, self._n_envs))
        if last_only:
            oshape, dshape = tuple(self._obs.shape), (self._n_envs,)
        else:
            oshape = (K,) + tuple(self._obs.shape)
            dshape = (K, self._n_envs)
        if obs_out is None:
            obs_out = torch.empty(oshape, dtype=self._tdtype, device=self._tdev)
        if done_out is None:
            done_out = torch.empty(dshape, dtype=torch.uint8, device=self._tdev)
        assert tuple(obs_out.shape) == oshape and obs_out.is_contiguous() and obs_out.dtype == self._tdtype
        assert tuple(done_out.shape) == dshape and done_out.is_contiguous() and done_out.dtype == torch.uint8
        if half:
            _lib.check(self._L.gemx_rollout_half(self._handle, C.c_void_p(a.data_ptr()), K, C.c_void_p(obs_out.data_ptr()),
                                                 C.c_void_p(done_out.data_ptr()), self._stream()))
        else:
            _lib.check(self._L.gemx_rollout(self._handle, C.c_void_p(a.data_ptr()), K, C.c_void_p(obs_out.data_ptr()),
                                            C.c_void_p(done_out.data_ptr()), 0 if last_only else 1, self._stream()))
        self._k += K
        return obs_out, done_out

    def set_rate_limiter(self, mode="closed", target_gbps=None):
        """The large-batch rate limiter of the fused rollout (include/gemx.h, gemx_set_rate_limiter) for THIS system: mode 'off' |
        'open' (the built-in target of the launch's family and size) | 'closed' (the default on a whole gfx950: the handle times its own
        launches and keeps the best of a bracket around that target); `target_gbps` replaces the built-in target (open loop).  Results
        never depend on it.  Turn it off for systems that share the chip with other work."""
        modes = {"off": 0, "open": 1, "closed": 2}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)}, not {mode!r}")
        _lib.check(self._L.gemx_set_rate_limiter(self._handle, modes[mode], float(target_gbps) if target_gbps else 0.0))

    # ------------------------------------------------------------------ fused reward
    def synthetic_actions(self, K, seed=0, step0=None):
        """The device's synthetic action stream as a tensor: [K, N, A] (continuous, uniform on (-1, 1)) or [K, N] uint8 (uniform over the
        converter's action set; MultiDiscrete: the flat index) for stream positions step0 .. step0 + K - 1 (default step0: the step count
        `k`).  `rollout(synthetic_actions(K, seed, s))` and `rollout_synthetic(K, seed, s)` give the same bits."""
        torch = _torch()
        K = int(K)
        s0 = int(self._k if step0 is None else step0) & 0xFFFFFFFF
        shape = (K, self._n_envs) if self._discrete else (K, self._n_envs, self._n_act)
        out = torch.empty(shape, dtype=self._want_dtype, device=self._tdev)
        _lib.check(self._L.gemx_synthetic_actions(self._handle, int(seed) & (2**64 - 1), s0, K, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def rollout_synthetic(self, K, seed=0, step0=None, obs_out=None, done_out=None):
        """K fused control steps on SYNTHETIC random actions generated inside the launch (no action tensor is read: include/gemx.h,
        gemx_rollout_synthetic) -- random-action rollouts of the continuous converters at large batch sizes run 15-20 % faster without
        the action stream coming from the HBM between the observation stores.  Returns (obs [K, N, S_out], done [K, N])."""
        self._refuse_with_env_parameters("rollout_synthetic (synthetic_actions + rollout)")
        torch = _torch()
        K = int(K)
        s0 = int(self._k if step0 is None else step0) & 0xFFFFFFFF
        oshape, dshape = (K,) + tuple(self._obs.shape), (K, self._n_envs)
        if obs_out is None:
            obs_out = torch.empty(oshape, dtype=self._tdtype, device=self._tdev)
        if done_out is None:
            done_out = torch.empty(dshape, dtype=torch.uint8, device=self._tdev)
        # (the checks of bind_rollout -- incl. the DEVICE: a host or other-GPU tensor would hand the kernel a foreign pointer; advisor, round 5)
        if not (torch.is_tensor(obs_out) and tuple(obs_out.shape) == oshape and obs_out.is_contiguous() and obs_out.dtype == self._tdtype and obs_out.device == self._tdev):
            raise ValueError(f"rollout_synthetic: obs_out must be a contiguous {self._tdtype} tensor of shape {oshape} on {self._tdev}")
        if not (torch.is_tensor(done_out) and tuple(done_out.shape) == dshape and done_out.is_contiguous() and done_out.dtype == torch.uint8 and done_out.device == self._tdev):
            raise ValueError(f"rollout_synthetic: done_out must be a contiguous uint8 tensor of shape {dshape} on {self._tdev}")
        _lib.check(self._L.gemx_rollout_synthetic(self._handle, int(seed) & (2**64 - 1), s0, K, C.c_void_p(obs_out.data_ptr()),
                                                  C.c_void_p(done_out.data_ptr()), self._stream()))
        self._k += K
        return obs_out, done_out

    def set_reward(self, reward_weights=None, referenced_states=(), normed_reward_weights=False, violation_reward=None, gamma=0.9,
                   reward_power=1, bias=0.0):
        """Install a WeightedSumOfErrors reward (reward_functions/weighted_sum_of_errors.py:9-129; same arguments, same defaults)
        that `rollout(..., references=...)` / `simulate(..., references=...)` evaluate in-kernel.

        referenced_states: names of the states the caller's reference tensor carries, i.e. the reference generator's
            `referenced_states`; the tensor's last axis follows the order of `state_names`.  All other states are compared
            with 0, as the reference's generators return 0 there (core.py:346).
        Pass reward_weights=False to remove the reward function."""
        if reward_weights is False:
            _lib.check(self._L.gemx_set_reward(self._handle, None))
            self._reward_cfg = None
            return None
        rc = self._build_reward_config(reward_weights, referenced_states, normed_reward_weights, violation_reward, gamma, reward_power, bias)
        if self._handle is not None:
            _lib.check(self._L.gemx_set_reward(self._handle, C.byref(rc)))
        self._reward_cfg = rc
        return rc

    def _build_reward_config(self, reward_weights, referenced_states, normed, violation_reward, gamma, reward_power, bias):
        names = list(self._state_names)
        n = len(names)

        def state_array(v):  # utils.set_state_array (utils.py:40-70)
            if isinstance(v, dict):
                arr = np.zeros(n)
                for k_, x in v.items():
                    arr[names.index(k_)] = x
                return arr
            if np.ndim(v) == 0:
                return np.full(n, float(v))
            arr = np.asarray(v, dtype=float)
            assert len(arr) == n
            return arr

        ref_idx = sorted(names.index(r) for r in referenced_states)
        if len(ref_idx) > _lib.MAX_REF:
            raise ValueError(f"at most {_lib.MAX_REF} referenced states")
        if reward_weights is None:  # set_modules, lines 97-112: equal weights over the referenced states (or over all states)
            sel = ref_idx if ref_idx else list(range(n))
            w = np.zeros(n)
            w[sel] = 1 / len(sel)
        else:
            w = state_array(reward_weights)
        powers = state_array(reward_power)
        length = self._state_space.high - self._state_space.low
        rw_sum = float(sum(w))
        if normed:  # lines 117-127
            if bias == "positive":
                bias = 1
            w = w / rw_sum
            rng = (-1 + bias, bias)
        else:
            if bias == "positive":
                bias = rw_sum
            rng = (-rw_sum + bias, bias)
        if violation_reward is None:
            violation_reward = min(rng[0] / (1.0 - gamma), 0)
        rc = _lib.GemxRewardConfig()
        rc.struct_size = C.sizeof(_lib.GemxRewardConfig)
        rc.n_ref = len(ref_idx)
        for j, i in enumerate(ref_idx):
            rc.ref_index[j] = i
        for i in range(n):
            rc.weight[i], rc.power[i], rc.state_length[i] = float(w[i]), float(powers[i]), float(length[i])
        rc.bias, rc.violation_reward = float(bias), float(violation_reward)
        self.reward_range = rng
        return rc

    def _rollout_reward(self, actions, K, obs_out, done_out, references, reward_out):
        torch = _torch()
        if getattr(self, "_reward_cfg", None) is None:
            raise ValueError("no reward function installed: call set_reward(...) first")
        n_ref = int(self._reward_cfg.n_ref)
        a = self._actions_to_device(actions, (K, self._n_envs))
        r = None
        if n_ref:
            r = torch.as_tensor(references).to(device=self._tdev, dtype=self._tdtype).reshape(K, self._n_envs, n_ref).contiguous()
        oshape = (K,) + tuple(self._obs.shape)
        if obs_out is None:
            obs_out = torch.empty(oshape, dtype=self._tdtype, device=self._tdev)
        if done_out is None:
            done_out = torch.empty((K, self._n_envs), dtype=torch.uint8, device=self._tdev)
        if reward_out is None:
            reward_out = torch.empty((K, self._n_envs), dtype=self._tdtype, device=self._tdev)
        assert tuple(obs_out.shape) == oshape and obs_out.is_contiguous() and obs_out.dtype == self._tdtype
        assert tuple(reward_out.shape) == (K, self._n_envs) and reward_out.is_contiguous() and reward_out.dtype == self._tdtype
        _lib.check(self._L.gemx_rollout_reward(self._handle, C.c_void_p(a.data_ptr()), K, C.c_void_p(r.data_ptr()) if r is not None else None,
                                               C.c_void_p(obs_out.data_ptr()), C.c_void_p(done_out.data_ptr()),
                                               C.c_void_p(reward_out.data_ptr()), self._stream()))
        self._k += K
        return obs_out, done_out, reward_out

    def reset(self, mask=None, *_):
        """PhysicalSystem.reset (core.py:678-685).  mask: optional [N] bool/uint8 selecting the envs to reset.
        Returns the internal observation buffer with the rows of the reset envs replaced by their reset observation.  Rows outside
        `mask` hold what simulate() last wrote there (the reset observation before the first step); rollout() writes to ITS output
        tensors and does not update this buffer -- after a rollout take the unmasked rows from the rollout's last row."""
        torch = _torch()
        m = None
        if mask is not None and not (self._n_envs == 1 and not torch.is_tensor(mask) and np.ndim(mask) == 0):
            m = torch.as_tensor(mask).to(device=self._tdev, dtype=torch.uint8).contiguous()
        # the kernel writes the reset observation of every env it resets into the internal buffer (masked-out rows untouched)
        _lib.check(self._L.gemx_reset(self._handle, C.c_void_p(m.data_ptr()) if m is not None else None,
                                      C.c_void_p(self._obs.data_ptr()), self._stream()))
        if m is None:
            self._k = 0
        if self._n_envs == 1:
            if self._cfg.init_kind != _lib.INIT_CONST:
                # random initialisers: the observation of the state the kernel just drew, not the constant initial state's
                return self._obs.reshape(-1).double().cpu().numpy()
            return self._reset_obs.copy()
        return self._obs

    def last_launch(self):
        """Description of the kernel instantiation / geometry the last simulate() / rollout() launched."""
        return self._L.gemx_last_launch(self._handle).decode()

    def check_errors(self):
        """Synchronises.  Raises like the reference (converters.py:204-206) if a discrete action left 0..7."""
        flags = C.c_uint32(0)
        _lib.check(self._L.gemx_error_flags(self._handle, C.byref(flags), self._stream()))
        if flags.value & _lib.ERRFLAG_ACTION:
            raise AssertionError(f"An action outside the action space {self.action_space} was passed to simulate()/rollout().")
        if flags.value & _lib.ERRFLAG_OMEGA_MOVED:
            raise _lib.GemxError("a launch specialised for envs at their initial speed (dc_stream_kernel) found another omega in device memory: "
                                 "set_state() and the rollout were enqueued on different streams without synchronisation; the observations "
                                 "of that launch are invalid")
        if flags.value & _lib.ERRFLAG_TOLERANCE:
            import warnings

            warnings.warn("the error-controlled solver (ScipyOdeSolver) took a step at its floor of 1/1024 of a segment whose error estimate "
                          "exceeded the tolerance: some trajectory since the last check is less accurate than asked for", RuntimeWarning)

    # ------------------------------------------------------------------ checkpoint / parity access
    def get_state(self):
        """ODE state [S_ode, N] (physical units, angle in rad) as a new device tensor."""
        torch = _torch()
        out = torch.empty((self._n_ode, self._n_envs), dtype=self._tdtype, device=self._tdev)
        _lib.check(self._L.gemx_get_state(self._handle, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def set_state(self, state):
        torch = _torch()
        s = torch.as_tensor(state).to(device=self._tdev, dtype=self._tdtype).reshape(self._n_ode, self._n_envs).contiguous()
        _lib.check(self._L.gemx_set_state(self._handle, C.c_void_p(s.data_ptr()), self._stream()))
        torch.cuda.current_stream(self._tdev).synchronize()

    def get_switch_state(self):
        """Packed half-bridge states (2 bits each): uint8 [N], or [2, N] for the six half-bridges of a 2 x Finite-B6C."""
        torch = _torch()
        rows = self._L.gemx_n_switch_bytes(self._handle)
        out = torch.empty(self._n_envs if rows == 1 else (rows, self._n_envs), dtype=torch.uint8, device=self._tdev)
        _lib.check(self._L.gemx_get_switch_state(self._handle, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def set_switch_state(self, sw):
        torch = _torch()
        s = torch.as_tensor(sw).to(device=self._tdev, dtype=torch.uint8).contiguous()
        _lib.check(self._L.gemx_set_switch_state(self._handle, C.c_void_p(s.data_ptr()), self._stream()))
        torch.cuda.current_stream(self._tdev).synchronize()


    def get_checkpoint(self):
        """Everything a resumed system needs, as device tensors: the ODE state, the converters' leg states, and the opaque `aux` blob
        (RCVoltageSupply rows, DeadTimeProcessor queue + phase, reset counters of the random initialisers: include/gemx.h,
        gemx_get_aux_state) plus the step counter `k` (PhysicalSystem._k).  The reference keeps the same things in
        solvers.py:44-45, converters.py:193-197, dead_time_processor.py:63-72, voltage_supplies.py:100-123."""
        torch = _torch()
        nb = int(self._L.gemx_aux_state_bytes(self._handle))
        aux = torch.empty(nb, dtype=torch.uint8, device=self._tdev)  # (gemx_get_aux_state zeroes the sections' padding itself: equal states, equal blobs)
        _lib.check(self._L.gemx_get_aux_state(self._handle, C.c_void_p(aux.data_ptr()), self._stream()))
        ck = {"state": self.get_state(), "switch_state": self.get_switch_state(), "aux": aux, "k": int(self._k)}
        if self._env_parameters is not None:  # the table as the device holds it (the parameters themselves are a construction argument)
            ck["env_parameters"] = self.get_env_parameter_table()
        return ck

    def check_checkpoint(self, ckpt):
        """The size checks of `set_checkpoint`, which restore nothing -> the aux blob on this system's device."""
        self._check_env_parameters_checkpoint(ckpt)
        torch = _torch()
        aux = torch.as_tensor(ckpt["aux"]).to(device=self._tdev, dtype=torch.uint8).contiguous()
        if aux.numel() != int(self._L.gemx_aux_state_bytes(self._handle)):
            raise ValueError(f"checkpoint aux blob has {aux.numel()} bytes, this system needs {int(self._L.gemx_aux_state_bytes(self._handle))}: "
                             "it was taken from a system of another configuration")
        if torch.as_tensor(ckpt["state"]).numel() != self._n_ode * self._n_envs:
            raise ValueError(f"checkpoint state has shape {tuple(torch.as_tensor(ckpt['state']).shape)}, this system's is {(self._n_ode, self._n_envs)}: "
                             "it was taken from a system of another n_envs or motor")
        return aux

    def set_checkpoint(self, ckpt):
        """Restore `get_checkpoint()` of a system of the SAME configuration (n_envs, dtype, converter, supply, wrappers, initialisers;
        checked by the library): the next simulate() / rollout() continues bit for bit."""
        aux = self.check_checkpoint(ckpt)
        self.set_state(ckpt["state"])
        self.set_switch_state(ckpt["switch_state"])
        _lib.check(self._L.gemx_set_aux_state(self._handle, C.c_void_p(aux.data_ptr()), self._stream()))
        self._k = int(ckpt["k"])


class BatchedDcMotorSystem(BatchedSCMLSystem):
    """DcMotorSystem (physical_systems.py:290-318) for N envs: permanently excited, series and shunt DC motors
    (one converter voltage) with Cont-4QC or Finite-4QC; externally excited DC motor with a Cont/FiniteMultiConverter
    of two 4QCs (armature, excitation)."""

    def __init__(self, converter, motor, *args, **kwargs):
        if _is_a(motor, "DcSeriesMotor"):
            self._SYSTEM_KIND = _lib.SYS_DC_SERIES
        elif _is_a(motor, "DcShuntMotor"):
            self._SYSTEM_KIND = _lib.SYS_DC_SHUNT
        elif _is_a(motor, "DcPermanentlyExcitedMotor"):
            self._SYSTEM_KIND = _lib.SYS_DC_PERMEX
        elif _is_a(motor, "DcExternallyExcitedMotor"):
            self._SYSTEM_KIND = _lib.SYS_DC_EXTEX
        else:
            raise ValueError(f"motor {type(motor).__name__} is not on the accelerated path for DcMotorSystem "
                             "(supported: DcPermanentlyExcitedMotor, DcSeriesMotor, DcShuntMotor, DcExternallyExcitedMotor)")
        self._n_ode = 1 + len(motor.CURRENTS)
        super().__init__(converter, motor, *args, **kwargs)

    def _build_state_names(self):
        return self._mechanical_load.state_names + ["torque"] + list(self._electrical_motor.CURRENTS) + list(self._electrical_motor.VOLTAGES) + ["u_sup"]

    def _set_indices(self):
        """physical_systems.py:141-162."""
        n_c, n_v = len(self._electrical_motor.CURRENTS), len(self._electrical_motor.VOLTAGES)
        self.OMEGA_IDX = 0
        self.TORQUE_IDX = 1
        self.CURRENTS_IDX = list(range(2, 2 + n_c))
        self.VOLTAGES_IDX = list(range(2 + n_c, 2 + n_c + n_v))
        self.U_SUP_IDX = [2 + n_c + n_v]

    def _build_state_space(self, state_names):
        """physical_systems.py:305-318."""
        low, high = self._electrical_motor.get_state_space(self._converter.currents, self._converter.voltages)
        low_mech, high_mech = self._mechanical_load.get_state_space((low["omega"], high["omega"]))
        low, high = dict(low), dict(high)
        low.update(low_mech)
        high.update(high_mech)
        high["u_sup"] = self._supply.supply_range[1] / self._supply.u_nominal
        if self._supply.supply_range[0] != self._supply.supply_range[1]:
            low["u_sup"] = self._supply.supply_range[0] / self._supply.u_nominal
        else:
            low["u_sup"] = 0
        return Box(np.array([low[n] for n in state_names], dtype=float), np.array([high[n] for n in state_names], dtype=float), dtype=np.float64)


class _BatchedThreePhaseMotorSystem(BatchedSCMLSystem):
    """ThreePhaseMotorSystem helper transforms (physical_systems.py:321-415), host-side numpy, for user code."""

    _T23 = 2 / 3 * np.array([[1, -0.5, -0.5], [0, 0.5 * np.sqrt(3), -0.5 * np.sqrt(3)]])
    _T32 = np.array([[1, 0], [-0.5, 0.5 * np.sqrt(3)], [-0.5, -0.5 * np.sqrt(3)]])

    @staticmethod
    def _q(quantities, epsilon):
        c, s = math.cos(epsilon), math.sin(epsilon)
        return c * quantities[0] - s * quantities[1], s * quantities[0] + c * quantities[1]

    def abc_to_alphabeta_space(self, abc_quantities):
        return np.matmul(self._T23, abc_quantities)

    def alphabeta_to_abc_space(self, alphabeta_quantities):
        return np.matmul(self._T32, alphabeta_quantities)

    def abc_to_dq_space(self, abc_quantities, epsilon_el, normed_epsilon=False):
        if normed_epsilon:
            epsilon_el *= np.pi
        return self._q(np.matmul(self._T23, abc_quantities), -epsilon_el)

    def dq_to_abc_space(self, dq_quantities, epsilon_el, normed_epsilon=False):
        if normed_epsilon:
            epsilon_el *= np.pi
        return np.matmul(self._T32, self._q(dq_quantities, epsilon_el))

    def alphabeta_to_dq_space(self, alphabeta_quantities, epsilon_el, normed_epsilon=False):
        if normed_epsilon:
            epsilon_el *= np.pi
        return self._q(alphabeta_quantities, -epsilon_el)

    def dq_to_alphabeta_space(self, dq_quantities, epsilon_el, normed_epsilon=False):
        if normed_epsilon:
            epsilon_el *= np.pi
        return self._q(dq_quantities, epsilon_el)

    def _set_indices(self):
        """physical_systems.py:462-485 / 737-763."""
        self.OMEGA_IDX = 0
        self.TORQUE_IDX = 1
        self.CURRENTS_IDX = list(range(2, 7))
        self.VOLTAGES_IDX = list(range(7, 12))
        self.EPSILON_IDX = 12
        self.U_SUP_IDX = [13]

    def _build_state_space(self, state_names):
        """physical_systems.py:437-442 / 712-717."""
        low = -1 * np.ones(len(state_names), dtype=float)
        low[self.U_SUP_IDX] = 0.0
        high = np.ones(len(state_names), dtype=float)
        return Box(low, high, dtype=np.float64)


class BatchedSynchronousMotorSystem(_BatchedThreePhaseMotorSystem):
    """SynchronousMotorSystem (physical_systems.py:418-561) for N envs (PMSM, SynRM)."""

    _SYSTEM_KIND = _lib.SYS_SYNC
    _n_ode = 4

    def _build_state_names(self):
        return self._mechanical_load.state_names + ["torque", "i_a", "i_b", "i_c", "i_sd", "i_sq", "u_a", "u_b", "u_c",
                                                    "u_sd", "u_sq", "epsilon", "u_sup"]


class BatchedExternallyExcitedSynchronousMotorSystem(_BatchedThreePhaseMotorSystem):
    """ExternallyExcitedSynchronousMotorSystem (physical_systems.py:564-691) for N envs: EESM behind a
    Cont/FiniteMultiConverter of a B6 bridge (stator) and a 4QC (excitation).  No converter dead time (the reference's
    interlocking branch for this system cannot execute)."""

    _SYSTEM_KIND = _lib.SYS_EESM
    _n_ode = 5

    def _build_state_names(self):
        return self._mechanical_load.state_names + ["torque", "i_a", "i_b", "i_c", "i_sd", "i_sq", "i_e", "u_a", "u_b", "u_c",
                                                    "u_sd", "u_sq", "u_e", "epsilon", "u_sup"]

    def _set_indices(self):
        """physical_systems.py:595-617."""
        self.OMEGA_IDX = 0
        self.TORQUE_IDX = 1
        self.CURRENTS_IDX = list(range(2, 8))
        self.VOLTAGES_IDX = list(range(8, 14))
        self.EPSILON_IDX = 14
        self.U_SUP_IDX = [15]


class BatchedDoublyFedInductionMotorSystem(_BatchedThreePhaseMotorSystem):
    """DoublyFedInductionMotorSystem (physical_systems.py:850-1113) for N envs: stator and rotor each behind a B6 bridge of a
    Cont/FiniteMultiConverter; 24 system states."""

    _SYSTEM_KIND = _lib.SYS_DFIM
    _n_ode = 6

    def _build_state_names(self):
        return self._mechanical_load.state_names + [
            "torque", "i_sa", "i_sb", "i_sc", "i_sd", "i_sq", "i_ra", "i_rb", "i_rc", "i_rd", "i_rq",
            "u_sa", "u_sb", "u_sc", "u_sd", "u_sq", "u_ra", "u_rb", "u_rc", "u_rd", "u_rq", "epsilon", "u_sup"]

    def _set_indices(self):
        """physical_systems.py:911-916."""
        self.OMEGA_IDX = 0
        self.TORQUE_IDX = 1
        self.CURRENTS_IDX = list(range(2, 12))
        self.VOLTAGES_IDX = list(range(12, 22))
        self.EPSILON_IDX = 22
        self.U_SUP_IDX = [23]


class BatchedSquirrelCageInductionMotorSystem(_BatchedThreePhaseMotorSystem):
    """SquirrelCageInductionMotorSystem (physical_systems.py:696-847) for N envs."""

    _SYSTEM_KIND = _lib.SYS_SCIM
    _n_ode = 6

    def _build_state_names(self):
        return self._mechanical_load.state_names + ["torque", "i_sa", "i_sb", "i_sc", "i_sd", "i_sq", "u_sa", "u_sb", "u_sc",
                                                    "u_sd", "u_sq", "epsilon", "u_sup"]
