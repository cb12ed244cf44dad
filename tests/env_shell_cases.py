"""The cases of tests/test_gpu_env_shell.py, as data and builders that need no device, so that tests/test_env_shell_cpu.py can run the
host shell alone on exactly these inputs (the close-call cap).  Every third lane holds the action that drives its machine over the
current limit (tests/test_gpu_pipeline_forms.py: PMSM abc (1, -1, -1) passes it in the eighth step, SCIM in the third, as dq (1, 1) too;
the PermExDc under switch state 2 in the sixth: |i| 0.94, 1.12 in steps five and six of the fp64 oracle); the lanes behind them hold it for the first half of
the run only -- they terminate, then run into the time limit; the others never leave the neighbourhood of zero and only truncate.
The time limit M lies above the hot lanes' episode length, so terminations and truncations meet in one run, and the noise scales are a few
per cent of the step the deciding expression takes per control step, so that the noise decides some terminations but close calls stay rare."""
import numpy as np

import env_shell_restatement as esr

GEN_KW = dict(episode_lengths=(6, 12), frequency_range=(500, 2000), amplitude_range=(0.1, 0.4), offset_range=(-0.2, 0.2))
PMSM_OBSERVED = ["omega", "i_sd", "i_sq", "cos(epsilon)", "sin(epsilon)"]
SCIM_OBSERVED = ["omega", "i_sd", "i_sq", "psi_abs", "psi_angle"]
COSSIN = [dict(kind="CosSinProcessor", angle="epsilon", remove_angle=True)]

CASES = {
    # Case A, once per distribution: make() takes ONE StateNoiseProcessor and it has one distribution
    "A-normal": dict(env_id="Cont-CC-PMSM-v0", golden="default_cont_cc_pmsm_dopri5", N=70, K=20, M=10, hot=(1.0, -1.0, -1.0),
                     noise=(["i_sd", "i_sq", "epsilon"], "normal", dict(scale=[0.03, 0.03, 0.01])), generators=(("step", "i_sd"), ("sinusoidal", "i_sq")),
                     chain=COSSIN, observed=PMSM_OBSERVED, squared=("i_sd", "i_sq")),
    "A-uniform": dict(env_id="Cont-CC-PMSM-v0", golden="default_cont_cc_pmsm_dopri5", N=300, K=20, M=10, hot=(1.0, -1.0, -1.0),
                      noise=(["i_sd", "i_sq", "epsilon"], "uniform", dict(low=[-0.05, -0.05, -0.02], high=[0.05, 0.05, 0.02])),
                      generators=(("step", "i_sd"), ("sinusoidal", "i_sq")), chain=COSSIN, observed=PMSM_OBSERVED, squared=("i_sd", "i_sq")),
    "A-laplace": dict(env_id="Cont-CC-PMSM-v0", golden="default_cont_cc_pmsm_dopri5", N=70, K=20, M=10, hot=(1.0, -1.0, -1.0),
                      noise=(["i_sd", "i_sq", "epsilon"], "laplace", dict(scale=[0.02, 0.02, 0.01])), generators=(("step", "i_sd"), ("sinusoidal", "i_sq")),
                      chain=COSSIN, observed=PMSM_OBSERVED, squared=("i_sd", "i_sq")),
    # (N = 300: the noise stage's second 256-row tile together with the flux observer; C keeps the single partial tile)
    "B": dict(env_id="Cont-CC-SCIM-v0", golden="default_cont_cc_scim_dopri5", N=300, K=12, M=5, hot=(1.0, -1.0, -1.0),
              noise=(["i_sa", "i_sd", "i_sq"], "normal", dict(scale=[0.02, 0.1, 0.1])), generators=(("sinusoidal", "i_sd"), ("sinusoidal", "i_sq")),
              observer=True, observed=SCIM_OBSERVED, squared=("i_sd", "i_sq")),
    "C": dict(env_id="Cont-CC-SCIM-v0", golden="default_cont_cc_scim_dopri5", N=70, K=12, M=5, hot=(1.0, 1.0),
              noise=(["i_sa", "i_sd", "i_sq"], "normal", dict(scale=[0.02, 0.1, 0.1])), generators=(("sinusoidal", "i_sd"), ("sinusoidal", "i_sq")),
              observer=True, dq=True, observed=SCIM_OBSERVED, squared=("i_sd", "i_sq")),
    "D": dict(env_id="Finite-CC-PermExDc-v0", golden="default_finite_cc_permexdc_dopri5", N=300, K=16, M=8, hot=2,
              noise=(["i", "omega"], "laplace", dict(scale=[0.04, 0.01])), generators=(("triangular", "i"),), limit=("i",), auto_reset=False),
    "E": dict(env_id="Cont-CC-PMSM-v0", golden="default_cont_cc_pmsm_dopri5", N=70, K=20, M=10, hot=(1.0, -1.0, -1.0), noise=None,
              generators=(("step", "i_sd"), ("sinusoidal", "i_sq")), chain=COSSIN, observed=PMSM_OBSERVED, squared=("i_sd", "i_sq")),
}
SEED = 17


def actions(spec):
    """[K, N, A] float64 (continuous) | [K, N] int64 (discrete)."""
    K, N = spec["K"], spec["N"]
    rng = np.random.default_rng(SEED)
    lane, k = np.arange(N)[None, :], np.arange(K)[:, None]
    hot = (lane % 3 == 0) | ((lane % 3 == 1) & (k < K // 2))
    if np.ndim(spec["hot"]) == 0:
        return np.where(hot, spec["hot"], rng.choice([0, 3], (K, N))).astype(np.int64)
    cold = 0.005 * rng.uniform(-1.0, 1.0, (K, N, len(spec["hot"])))
    return np.where(hot[..., None], np.array(spec["hot"], dtype=np.float64), cold)


def make_kwargs(ga, spec, dtype, **extra):
    """What a user hands to `ga.make(env_id, ...)` for this case."""
    wrappers = []
    if spec.get("noise"):
        states, dist, kw = spec["noise"]
        wrappers.append(ga.StateNoiseProcessor(states, dist, kw))
    if spec.get("observer"):
        wrappers.append(ga.FluxObserver())
    if spec.get("dq"):
        wrappers.append(ga.FluxOrientedDqToAbcActionProcessor("SCIM"))
    if spec.get("chain"):
        wrappers.append(ga.CosSinProcessor(remove_angle=True))
    gens = [getattr(ga, kind.capitalize() + "ReferenceGenerator")(reference_state=state, **GEN_KW) for kind, state in spec["generators"]]
    kw = dict(n_envs=spec["N"], dtype=dtype, seed=SEED, physical_system_wrappers=tuple(wrappers), reference_generator=gens,
              max_episode_steps=spec["M"], episode_statistics=True)
    if spec.get("observed"):
        kw.update(observed_states=spec["observed"], flatten_observation=True)
    if "auto_reset" in spec:
        kw["auto_reset"] = spec["auto_reset"]
    kw.update(extra)
    return kw


def build_shell(ga, spec, param_sets, n_envs=None):
    """The host shell of a case.  Everything but the observer's host restatement comes from the fp64 golden's description of the
    reference env (oracle.params_from_meta), not from the package."""
    from oracle import oracle as orc

    _, meta = orc.load_golden(spec["golden"])
    names = meta["state_names"]
    solver = "rk4"  # make() hands the CC envs (ConstantSpeedLoad) one classical RK4 step: test_gpu_parity._oracle_solver_for
    assert meta["load"] == "ConstantSpeedLoad"
    margin = {s: float(meta["nominal_state"][names.index(s)] / meta["limits"][names.index(s)]) for _, s in spec["generators"]}
    gens = sorted((dict(kind=kind, state=s, margin=(-margin[s], margin[s])) for kind, s in spec["generators"]), key=lambda g: names.index(g["state"]))
    n = len(names)
    observer = None
    if spec.get("observer"):  # the flux observer's float64 host restatement: an env that never touches a device
        w = (ga.FluxObserver(),) + ((ga.FluxOrientedDqToAbcActionProcessor("SCIM"),) if spec.get("dq") else ())
        observer = ga.make(spec["env_id"], n_envs=1, _defer_create=True, physical_system_wrappers=w).flux
    return esr.EnvShell(orc.params_from_meta(meta, solver=solver, episodic=False), n_envs or spec["N"], names,
                        limit_columns=[names.index(s) for s in spec.get("limit", ())], squared_columns=[names.index(s) for s in spec.get("squared", ())],
                        noise_columns=[names.index(s) for s in spec["noise"][0]] if spec.get("noise") else None,
                        reward=esr.reward_description(names, -np.ones(n), np.ones(n), [g["state"] for g in gens]),  # (the referenced currents span [-1, 1])
                        generators=gens, param_sets=param_sets, tau=meta["tau"], max_steps=spec["M"], restart=True, observer=observer,
                        dq_actions=bool(spec.get("dq")), chain=spec.get("chain", ()), observed_states=spec.get("observed"), flatten=bool(spec.get("observed")))


def standin_draws(spec, rng):
    """numpy draws of the case's distribution and scales, [K + 1, N, n_noisy], standing in for the device's stream."""
    states, dist, kw = spec["noise"]
    return getattr(rng, dist)(size=(spec["K"] + 1, spec["N"], len(states)), **kw)


def standin_param_sets(spec, shell, rng, n_sets=12):
    """Parameter sets drawn with numpy from the ranges the reference's generators draw from (e.g. sinusoidal_reference_generator.py:50-64),
    standing in for the device's: param_sets[column][env] = list of dicts."""
    out = []
    for g in shell.generators:
        lo, hi = g["margin"]
        per_env = []
        for _ in range(shell.n):
            sets = []
            for _ in range(n_sets):
                a = rng.uniform(*np.clip(GEN_KW["amplitude_range"], 0, (hi - lo) / 2))
                f = rng.uniform(*GEN_KW["frequency_range"])
                b = esr.rw.offset_bounds(g["kind"], a, np.clip(GEN_KW["offset_range"], lo, hi), (lo, hi))
                sets.append(dict(length=int(rng.uniform(*GEN_KW["episode_lengths"])), amplitude=a, frequency=f, offset=rng.uniform(min(b), max(b)),
                                 phase=rng.uniform() * 2 * np.pi, width=rng.triangular(0, 0.5, 1), roll=esr.rw.step_roll(f, shell.tau, rng.uniform())))
            per_env.append(sets)
        out.append(per_env)
    return out
