"""Per-env motor, load and supply parameters: domain randomisation inside ONE batched system.

    ga.make("Cont-CC-PMSM-v0", n_envs=N, env_parameters=ga.EnvParameters(
        motor={"r_s": r_s, "l_d": l_d},                 # any key of the motor's motor_parameter dict but p
        load={"j_load": j_load, "a": a, "b": b, "c": c},
        supply={"u_nominal": u}))

A value is a scalar or an array / tensor of n_envs entries; a key that is absent keeps the env's own parameter.  The per-env model
constants, torque coefficients and j_total are the component classes' own derivations (components.py) evaluated in float64 on the arrays,
handed to `gemx_set_env_params` (include/gemx.h), which derives the device table.  Lane e then computes, bit for bit, what a uniform system
built with env e's parameters computes (tests/test_gpu_env_parameters.py).  One value per system stay: tau, the pole pair number p, the
limits the observations are normalised by (those of the system's OWN parameters), the initial state, constraints, solver, action frame.
"""
import numpy as np

from . import _lib

REFUSAL = "per-env parameters (env_parameters=) are not available with "
_LOAD_KEYS = ("j_load", "a", "b", "c")
_SUPPLY_KEYS = ("u_nominal",)
_TAIL_FIELDS = ("tc0", "tc1", "tc2", "tc3", "inv_j", "la", "lb", "lc", "omega_lim", "lin_factor", "inv_tau_decay", "u_sup")
# structurally non-zero model entries per system kind (gemx_capi.hip: pack_model), the table's leading fields
_N_MODEL = {_lib.SYS_DC_PERMEX: 3, _lib.SYS_DC_SERIES: 3, _lib.SYS_DC_SHUNT: 5, _lib.SYS_DC_EXTEX: 5, _lib.SYS_SYNC: 7, _lib.SYS_EESM: 14,
            _lib.SYS_SCIM: 14, _lib.SYS_DFIM: 18}


def table_fields(system_kind):
    """Number of fields F of the device table [F, N] of a system kind (gemx_env_params_fields)."""
    return _N_MODEL[system_kind] + len(_TAIL_FIELDS)


def _as_array(value, what):
    if hasattr(value, "detach"):  # a torch tensor, wherever it lives
        value = value.detach().cpu().numpy()
    arr = np.asarray(value, dtype=np.float64)
    if arr.ndim > 1:
        raise ValueError(f"env_parameters: {what} must be a scalar or a one-dimensional array of n_envs values, got shape {arr.shape}")
    return arr


class EnvParameters:
    """Holder of per-env parameter overrides: `motor`, `load`, `supply` dicts of scalars or [n_envs] arrays (see the module docstring)."""

    def __init__(self, motor=None, load=None, supply=None):
        self.motor = {k: _as_array(v, f"motor[{k!r}]") for k, v in dict(motor or {}).items()}
        self.load = {k: _as_array(v, f"load[{k!r}]") for k, v in dict(load or {}).items()}
        self.supply = {k: _as_array(v, f"supply[{k!r}]") for k, v in dict(supply or {}).items()}
        if "p" in self.motor and self.motor["p"].ndim > 0:
            raise ValueError("env_parameters: the pole pair number p is one value per system (per-env parameters do not cover it): pass a scalar "
                             "through the motor's motor_parameter instead of an array")
        for k in self.load:
            if k not in _LOAD_KEYS:
                raise ValueError(f"env_parameters: load key {k!r} is not one of {_LOAD_KEYS}")
        for k in self.supply:
            if k not in _SUPPLY_KEYS:
                raise ValueError(f"env_parameters: supply key {k!r} is not one of {_SUPPLY_KEYS}")

    def _groups(self):
        return (("motor", self.motor), ("load", self.load), ("supply", self.supply))

    def shard(self, lo, hi, n_total):
        """The holder of envs [lo, hi) of a job of n_total envs (`distributed.make_sharded`): arrays are cut by GLOBAL env index."""
        out = EnvParameters()
        for name, group in self._groups():
            dst = getattr(out, name)
            for k, v in group.items():
                if v.ndim == 1:
                    if len(v) != n_total:
                        raise ValueError(f"env_parameters: {name}[{k!r}] has {len(v)} entries, the job has {n_total} envs")
                    v = v[lo:hi].copy()
                dst[k] = v
        return out

    def check(self, n_envs, motor):
        """Raises ValueError for a wrong length, a value that is not finite, or a motor key the motor does not have."""
        for name, group in self._groups():
            for k, v in group.items():
                if v.ndim == 1 and len(v) != n_envs:
                    raise ValueError(f"env_parameters: {name}[{k!r}] has {len(v)} entries, the system has {n_envs} envs")
                if not np.all(np.isfinite(v)):
                    raise ValueError(f"env_parameters: {name}[{k!r}] holds a value that is not finite")
        for k in self.motor:
            if k not in motor.motor_parameter or k in getattr(motor, "DERIVED_PARAMETERS", ()):
                raise ValueError(f"env_parameters: {type(motor).__name__} has no motor parameter {k!r} (it has {sorted(motor.motor_parameter)})")

    def resolve(self, system):
        """-> dict of float64 arrays for `gemx_set_env_params`, one entry per env: model [N, MODEL_ROWS * MODEL_COLS], torque_coef [N, 4],
        j_total, load_a, load_b, load_c, u_nominal [N] -- the component classes' derivations on arrays, no loop over envs.  Absent keys
        take the system's own components' values."""
        from . import components as comp

        n = system.n_envs
        motor, load, supply = system.electrical_motor, system.mechanical_load, system.supply
        self.check(n, motor)
        base = {k: v for k, v in motor.motor_parameter.items() if k not in getattr(motor, "DERIVED_PARAMETERS", ())}
        mp = dict(base)
        for k, v in self.motor.items():
            mp[k] = np.broadcast_to(v, (n,)) if k != "p" else float(v)
        if "p" in self.motor and float(self.motor["p"]) != float(base["p"]):
            raise ValueError("env_parameters: the pole pair number p is one value per system and differs from the motor's own")
        mc = np.asarray(comp.model_constants(motor, mp), dtype=np.float64)
        mc = np.broadcast_to(mc, (n,) + mc.shape[-2:])
        model = np.zeros((n, _lib.MODEL_ROWS, _lib.MODEL_COLS))
        model[:, : mc.shape[1], : mc.shape[2]] = mc
        tc = np.zeros((n, 4))
        for i, v in enumerate(comp.torque_coefficients(motor, comp.derived_parameters(motor, mp))):
            tc[:, i] = v
        lp = getattr(load, "load_parameter", None) or {}
        polynomial = type(load).__name__ == "PolynomialStaticLoad" or any(c.__name__ == "PolynomialStaticLoad" for c in type(load).__mro__)
        if not polynomial and any(k in self.load for k in ("a", "b", "c")):
            raise ValueError(f"env_parameters: load keys a, b, c belong to a PolynomialStaticLoad, the system has a {type(load).__name__}")

        def per_env(group, key, own):
            return np.array(np.broadcast_to(group[key] if key in group else np.float64(own), (n,)), dtype=np.float64)

        j_load = per_env(self.load, "j_load", getattr(load, "_j_load", 0.0))
        j_rotor = np.broadcast_to(np.asarray(mp["j_rotor"], dtype=np.float64), (n,))
        j_total = j_load + j_rotor  # _MechanicalLoad.set_j_rotor
        if "j_load" not in self.load and "j_rotor" not in self.motor:
            j_total = np.full(n, float(load.j_total))
        if not np.all(j_total > 0):
            raise ValueError("env_parameters: j_total = j_load + j_rotor must be positive for every env")
        out = dict(model=np.ascontiguousarray(model.reshape(n, -1)), torque_coef=np.ascontiguousarray(tc), j_total=np.ascontiguousarray(j_total),
                   load_a=per_env(self.load, "a", lp.get("a", 0.0) if polynomial else 0.0), load_b=per_env(self.load, "b", lp.get("b", 0.0) if polynomial else 0.0),
                   load_c=per_env(self.load, "c", lp.get("c", 0.0) if polynomial else 0.0), u_nominal=per_env(self.supply, "u_nominal", supply.u_nominal))
        return out


def refusal(system):
    """None, or the message of what a system with per-env parameters cannot have (raised by the system before anything is created)."""
    cfg = system._cfg
    if cfg.dtype == _lib.F64:
        return REFUSAL + "dtype='float64' (the fp64 build is a diagnostic of one parameter set)"
    if cfg.solver_flags & _lib.SOLVER_ADAPTIVE:
        return REFUSAL + "the error-controlled Dormand-Prince solver (ScipyOdeSolver): EulerSolver or RK4Solver"
    if cfg.solver_kind not in (_lib.SOLVER_EULER, _lib.SOLVER_RK4):
        return REFUSAL + "DormandPrince5Solver: EulerSolver or RK4Solver"
    if cfg.interlocking_time > 0:
        return REFUSAL + "a converter interlocking time (dead time)"
    if cfg.action_delay > 0:
        return REFUSAL + "a DeadTimeProcessor"
    if cfg.supply_kind != _lib.SUPPLY_IDEAL:
        return REFUSAL + "an RCVoltageSupply (IdealVoltageSupply with a per-env u_nominal)"
    if cfg.init_kind != _lib.INIT_CONST:
        return REFUSAL + "random initial states (the initial state is one per system)"
    return None


class GemxEnvParams(_lib.C.Structure):
    """Mirror of `gemx_env_params` (include/gemx.h)."""

    _fields_ = [("struct_size", _lib.C.c_int32), ("n_envs", _lib.C.c_int64), ("model", _lib.C.c_void_p), ("torque_coef", _lib.C.c_void_p),
                ("j_total", _lib.C.c_void_p), ("load_a", _lib.C.c_void_p), ("load_b", _lib.C.c_void_p), ("load_c", _lib.C.c_void_p),
                ("u_nominal", _lib.C.c_void_p)]


def install(system, arrays):
    """`gemx_set_env_params` on a created system with the arrays of `EnvParameters.resolve`."""
    C = _lib.C
    p = GemxEnvParams()
    p.struct_size = C.sizeof(GemxEnvParams)
    p.n_envs = system.n_envs
    keep = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    for k, v in keep.items():
        setattr(p, k, v.ctypes.data)
    _lib.check(system._L.gemx_set_env_params(system._handle, C.byref(p)))
