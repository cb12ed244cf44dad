"""Shared by tests/test_env_parameters_cpu.py and tests/test_gpu_env_parameters.py: the envs, the four parameter sets per env, the
seeded actions, and the fp64 oracle run once per (env, set).

Shape: N = 197 envs (three full waves and a partial one), K = 48 steps, set index = env % 4 (every wave holds all four sets).  A set is
the default machine with its resistances, its inductances, J_load and u_nominal scaled by factors in [0.6, 1.6].  The factors and the
action amplitude of every env were chosen on the CPU with the fp64 oracle so that within the 48 steps at least one set violates its
constraint (and auto-resets) and at least one never does; `oracle_runs` lets the tests assert exactly that."""
import functools
import json

import numpy as np

import gym_electric_motor_amd as ga
from oracle import oracle as orc

N, K, NSETS = 197, 48, 4

# per set: (resistances, inductances, J_load, u_nominal), each in [0.6, 1.6]
FACTORS = ((1.0, 1.0, 1.0, 1.0), (1.6, 1.5, 0.6, 0.6), (0.6, 0.7, 1.6, 1.6), (1.3, 0.6, 1.2, 0.8))

_RES = ("r_a", "r_e", "r_s", "r_r")
_IND = ("l_a", "l_e", "l_e_prime", "l_d", "l_q", "l_m", "l_sigs", "l_sigr")

# env id -> make() keywords, the seeded actions (continuous: bias + amp * U(-1, 1); discrete: uniform over the action set, each draw held for
# `hold` steps) and whether the load is a PolynomialStaticLoad (else a uniform system may take the one-step linear map)
CASES = {
    "Cont-CC-PermExDc-v0": dict(kw=dict(ode_solver=ga.EulerSolver()), amp=0.02, bias=0.275, poly=False),
    "Finite-CC-PMSM-v0": dict(kw=dict(ode_solver=ga.RK4Solver(), tau=1e-4), amp=None, poly=False),
    "Cont-SC-SCIM-v0": dict(kw=dict(), amp=1.0, poly=True),
    "Cont-CC-EESM-v0": dict(kw=dict(), amp=0.25, poly=False),
    "Finite-TC-DFIM-v0": dict(kw=dict(tau=1e-4), amp=None, hold=8, poly=False),
    "Cont-SC-SeriesDc-v0": dict(kw=dict(tau=4e-4), amp=0.3, bias=0.7, poly=True),
    "dq-PMSM": dict(env_id="Cont-SC-PMSM-v0", kw=dict(control_space="dq"), amp=0.6, poly=True),
}


def env_id_of(case):
    return CASES[case].get("env_id", case)


def make_kwargs(case):
    return dict(CASES[case]["kw"])


@functools.lru_cache(maxsize=None)
def base_env(case):
    """The env without a table, host side only (no device needed): the source of the default parameters."""
    return ga.make(env_id_of(case), n_envs=N, _defer_create=True, **make_kwargs(case))


def set_values(case, s):
    """-> (motor overrides, load overrides, supply overrides) of set s as scalars."""
    ps = base_env(case).physical_system
    fr, fl, fj, fu = FACTORS[s]
    mp = ps.electrical_motor.motor_parameter
    motor = {k: mp[k] * fr for k in _RES if k in mp}
    motor.update({k: mp[k] * fl for k in _IND if k in mp})
    j_load = float(getattr(ps.mechanical_load, "_j_load", 0.0))
    return motor, {"j_load": j_load * fj}, {"u_nominal": float(ps.supply.u_nominal) * fu}


def env_parameters(case, n=N, sets=None):
    """EnvParameters with set index = env % 4 (or `sets` [n]: the set of every env)."""
    sets = np.arange(n) % NSETS if sets is None else np.asarray(sets)
    vals = [set_values(case, s) for s in range(NSETS)]
    groups = []
    for g in range(3):
        groups.append({k: np.array([vals[s][g][k] for s in range(NSETS)])[sets] for k in vals[0][g]})
    return ga.EnvParameters(motor=groups[0], load=groups[1], supply=groups[2])


def uniform_kwargs(case, s):
    """make() keywords of the uniform env built with set s."""
    motor, load, supply = set_values(case, s)
    ps = base_env(case).physical_system
    kw = make_kwargs(case)
    kw["motor"] = dict(motor_parameter=motor)
    ld = ps.mechanical_load
    if type(ld).__name__ == "PolynomialStaticLoad":
        kw["load"] = dict(load_parameter=dict(ld.load_parameter, j_load=load["j_load"]))
    kw["supply"] = dict(u_nominal=supply["u_nominal"])
    return kw


def actions(case, seed=11):
    """Seeded actions [K, N, A] float32 / [K, N] uint8."""
    ps = base_env(case).physical_system
    rng = np.random.default_rng(seed)
    amp = CASES[case]["amp"]
    space = ps.action_space
    if amp is None:
        n = int(np.prod(space.nvec)) if hasattr(space, "nvec") else int(space.n)
        hold = CASES[case].get("hold", 1)
        return np.repeat(rng.integers(0, n, ((K + hold - 1) // hold, N)), hold, axis=0)[:K].astype(np.uint8)
    return np.clip(CASES[case].get("bias", 0.0) + amp * rng.uniform(-1.0, 1.0, (K, N, int(space.shape[0]))), -1.0, 1.0).astype(np.float32)


def _converter_name(conv):
    subs = getattr(conv, "_sub_converters", None)
    name = type(conv).__name__
    return name if subs is None else name + "[" + ",".join(type(c).__name__ for c in subs) + "]"


def oracle_params(case, s):
    """OrcParams of set s: the uniform env's components, normalised by the COMMON limits (those of the env without a table)."""
    base = base_env(case).physical_system
    env = ga.make(env_id_of(case), n_envs=1, _defer_create=True, **uniform_kwargs(case, s))
    ps = env.physical_system
    solver = type(ps._ode_solver).__name__
    solver = {"EulerSolver": "euler", "RK4Solver": "rk4_kink" if getattr(ps._ode_solver, "_split_kinks", False) and CASES[case]["poly"] else "rk4"}[solver]
    meta = dict(system=type(ps).__name__.replace("Batched", ""), motor=type(ps.electrical_motor).__name__, converter=_converter_name(ps.converter),
                load=type(ps.mechanical_load).__name__, solver=solver, episodic=True, tau=float(ps.tau), interlocking_time=0.0,
                u_nominal=float(ps.supply.u_nominal), motor_parameter={k: float(v) for k, v in ps.electrical_motor.motor_parameter.items()},
                j_total=float(ps.mechanical_load.j_total), load_parameter=dict(getattr(ps.mechanical_load, "load_parameter", {}) or {}),
                tau_decay=float(getattr(ps.mechanical_load, "tau_decay", 1e-3)), limits=[float(v) for v in base.limits],
                state_names=list(ps.state_names), action_frame=ps._action_frame, supply="IdealVoltageSupply")
    if meta["load"] == "ConstantSpeedLoad":
        meta["omega_fixed"] = float(ps.mechanical_load.omega_fixed)
    return orc.params_from_meta(json.loads(json.dumps(meta)))


@functools.lru_cache(maxsize=None)
def oracle_runs(case):
    """fp64 oracle, once per (set, lane of that set): -> obs [K, N, S_out], done [K, N] with lane e run under set e % 4 and lane e's actions."""
    a = actions(case)
    nvec = getattr(base_env(case).physical_system.action_space, "nvec", None)
    if nvec is not None:  # MultiDiscrete: the device reads the flat index a0 + n0 * a1, the oracle one entry per sub-converter
        a = np.stack([a % int(nvec[0]), a // int(nvec[0])], axis=-1)
    obs = done = None
    for s in range(NSETS):
        p = oracle_params(case, s)
        for e in range(s, N, NSETS):
            env = orc.OracleEnv(p)
            env.reset()
            o, d = env.rollout(a[:, e].astype(np.float64), auto_reset=True)
            if obs is None:
                obs, done = np.zeros((K, N, o.shape[-1])), np.zeros((K, N), dtype=bool)
            obs[:, e], done[:, e] = o, d
    return obs, done
