"""Batched env factory for the env ids on the accelerated path.

`make(env_id, n_envs=N, **kwargs)` mirrors `gym_electric_motor.make` (reference __init__.py:27, core.py:291-292)
for the env ids whose physical system is built from supported components, with the same per-id defaults as the
reference env classes (supply voltage, converter, motor, load, tau, constraints):

    {Finite,Cont}-{CC,TC,SC}-{PermExDc,SeriesDc,ShuntDc}-v0   envs/gym_dcm/{permex,series,shunt}_dc_motor_env/*.py
    {Finite,Cont}-{CC,TC,SC}-{PMSM,SynRM}-v0                  envs/gym_pmsm/*.py, envs/gym_synrm/*.py
    {Finite,Cont}-{CC,TC,SC}-SCIM-v0                          envs/gym_im/squirrel_cage_induction_motor_envs/*.py
    {Finite,Cont}-{CC,TC,SC}-ExtExDc-v0                       envs/gym_dcm/extex_dc_motor_env/*.py   (MultiConverter 2 x 4QC)
    {Finite,Cont}-{CC,TC,SC}-EESM-v0                          envs/gym_eesm/*.py                     (MultiConverter B6 + 4QC)
    {Finite,Cont}-{CC,TC,SC}-DFIM-v0                          envs/gym_im/doubly_fed_induction_motor_envs/*.py (MultiConverter 2 x B6)
(all 54 env ids of the reference.)

`make(env_id, n_envs=N)` alone gives the physical system + constraint monitor (done mask): `step()` returns `reward=None` and an
observation without a reference.  Naming `reference_generator=` and / or `reward_function=` gives the COMPLETE env, with the per-id
defaults of the reference's env classes (`default_env_modules`): device-side Wiener reference generators, the fused
WeightedSumOfErrors reward, and the reference's shell semantics (core.py:300-371):

    env = ga.make("Cont-CC-PMSM-v0", n_envs=4096, reference_generator="default", seed=3)
    (state, ref), _ = env.reset()                       # ref [N, n_ref]: initial value advanced once (core.py:313, 485-505)
    (state, ref), reward, terminated, _, _ = env.step(actions)

    step k:  launch 1  physics + reward against the references the PREVIOUS observation showed     (core.py:344-349)
             launch 2  generators of terminated envs restart, every generator advances, `ref` rewritten  (core.py:351)

Two kernel launches per step, no host round trip; `bind_step` resolves everything once and can be captured in a HIP graph.
K steps in one call: `state, refs, reward, done = env.rollout_complete(actions [K, N, A])` -- what K calls of `step` return, stacked, bit for
bit, in three launches (physics rollout; generators in the shell's order on its done mask; reward pass over the stored rows); also
`rollout_complete_synthetic(K)` and the pre-bound, graph-capturable `bind_rollout_complete(...)`.
The reference's other generator kinds (sinusoidal, step, triangular, sawtooth, Laplace process, constant) run on the same path: pass a
holder named after the reference's class, a list of them or a `BatchedMultipleReferenceGenerator` as `reference_generator=`;
`ga.SwitchedReferenceGenerator(holders, p=..., super_episode_length=...)` is such a holder: a waveform kind per super-episode and env.

The observation side runs on the device too (observation.py, csrc/gemx_obsproc.hip): `physical_system_wrappers=` may hold
`CurrentSumProcessor` / `CosSinProcessor` holders (`"default"`: what the reference's env class wraps its system in -- the `i_sum` column
of the six shunt envs), `observed_states=[names]` is the reference's `state_filter`, `flatten_observation=True` hands out ONE
`[N, n_post + n_ref]` tensor, the processed state followed by the references.  One more launch per step, after the generators:

    env = ga.make("Cont-CC-PMSM-v0", n_envs=4096, reference_generator="default", flatten_observation=True,
                  physical_system_wrappers=(ga.CosSinProcessor(remove_angle=True),), observed_states=["omega", "i_sd", "i_sq", "cos(epsilon)", "sin(epsilon)"])
    obs, _ = env.reset()                                # [N, 5 + 2], ready for the policy

Field-oriented control of the induction machines (flux_observer.py, csrc/gemx_fluxobs.hip): `ga.FluxObserver()` appends `psi_abs` and
`psi_angle` to the state of a SCIM / DFIM system, `ga.FluxOrientedDqToAbcActionProcessor("SCIM" | "DFIM")` listed after it turns the env's
actions into (u_d, u_q) pairs in the estimated flux frame.  A step is then four launches: dq -> abc actions, the physics, the observer,
the observation stage (when it is not the identity).  The K-step rollouts run with a `FluxObserver` and abc actions (physics, then ONE
pass of the observer over the stored rows, then the stage); with the flux-oriented action processor they raise: each step's angle depends
on the previous step's observation.  The order of the launches behind the physics is written down once, for every entry point of both
env classes: `ObservationPipeline.bind_after_step` / `bind_after_rollout` (observation.py) and, for the complete rollouts, `_tail` below.

    env = ga.make("Cont-CC-SCIM-v0", n_envs=4096, physical_system_wrappers=(ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor("SCIM")))
    state, _ = env.reset()                              # [N, 14 + 2]
    state, _, terminated, _, _ = env.step(dq_actions)   # dq_actions [N, 2]

Measurement noise (state_noise.py, csrc/gemx_statenoise.hip): `ga.StateNoiseProcessor(states, random_dist, random_kwargs)` -- 'normal',
'uniform' or 'laplace' -- listed before every observation-side processor.  The reference checks the constraints and computes the reward
on the NOISY state, so the physics then runs without constraints, auto-reset and fused reward and a step is: the masked reset of the envs
the last noisy row terminated, the physics, ONE launch that adds the noise and decides `terminated` and the reward on the noisy row, then
the generators and the other stages as above -- two launches more than without the wrapper (one with `auto_reset=False`).  `terminated`,
`reward` and the returned state are the noisy ones; `reset()` noises the reset state too.  The fused K-step rollouts raise: a K-step
launch cannot restart an env on a done mask it has not seen.

    env = ga.make("Cont-CC-PMSM-v0", n_envs=4096, reference_generator="default",
                  physical_system_wrappers=(ga.StateNoiseProcessor(["i_sd", "i_sq"], "normal", dict(scale=0.01)),))

Episode time limit and episode statistics (episodes.py, csrc/gemx_episode.hip): `max_episode_steps=M` is gymnasium's TimeLimit on the device,
`episode_statistics=True` its RecordEpisodeStatistics -- ONE launch more per step, directly behind the launch that writes reward and
`terminated` and before the generators.  With a time limit `step()` hands out `truncated` [N] (bool) in the fourth slot; the observation
of a truncating step is the final state, and the truncated envs restart in front of the next step's physics (one more launch: the masked
reset), their generators and flux observer with them.  A step that terminates and reaches the limit at once counts as terminated.
`env.episode_statistics()` -> dict(length, ret, last_length, last_ret, n_finished): [N] device tensors, views of the stage's state; the
return accumulates in float64.  The K-step rollouts run the statistics as one pass over their stored rows (`episode_statistics=True`:
a fifth result, dict(ended, finished_return, finished_length) [K, N]); with a time limit they raise: a K-step launch cannot restart an
env on a mask it has not seen.  The physics-only env counts lengths (it has no reward of its own: `ret` stays 0).

    env = ga.make("Cont-CC-PMSM-v0", n_envs=4096, reference_generator="default", max_episode_steps=1000, episode_statistics=True)
    obs, reward, terminated, truncated, _ = env.step(actions)
    stats = env.episode_statistics()                    # stats["last_ret"][stats["n_finished"] > 0].mean()

Outside the accelerated path: reward weights or constraints on appended columns (`i_sum`,
`cos(...)`, `psi_abs`, `psi_angle`) and visualisation; an instance of the reference's own `SwitchedReferenceGenerator` is refused (pass the holder of that
name).  For a full single-env GEM environment pass a `BatchedSCMLSystem(n_envs=1)` as
`physical_system=` to the reference's own `ElectricMotorEnvironment`.
"""
import re

import numpy as np

from .spaces import Box
from . import components as comp
from . import physical_systems as bps
from .reference_generators import BatchedMultipleReferenceGenerator, BatchedWienerProcessReferenceGenerator, ProfileReferences, ReplayReferenceGenerator

_ID = re.compile(r"^(Finite|Cont)-(CC|TC|SC)-(PermExDc|SeriesDc|ShuntDc|ExtExDc|PMSM|SynRM|SCIM|EESM|DFIM)-v0$")


def _initialize(arg, default_class, default_args):
    """utils.initialize (utils.py:5-16): instance | dict of overrides | None."""
    if arg is None:
        return default_class(**default_args)
    if isinstance(arg, type):
        raise Exception("Need initialization value")
    if type(arg) is str:
        raise Exception("Deprecated in version 3.0.0")
    if type(arg) is dict:
        args = dict(default_args)
        args.update(arg)
        return default_class(**args)
    return arg


# speed-control (SC) envs: PolynomialStaticLoad parameters per env class (e.g. cont_sc_permex_dc_env.py:159,
# finite_sc_permex_dc_env.py:160, cont_sc_series_dc_env.py:157, finite_sc_series_dc_env.py:157, cont_sc_shunt_dc_env.py:159,
# cont_sc_pmsm_env.py:153, cont_sc_synrm_env.py:153, cont_sc_scim_env.py:161)
_SC_LOAD = {
    ("Cont", "PermExDc"): dict(a=0.0, b=0.0, c=0.0, j_load=1e-4), ("Finite", "PermExDc"): dict(a=0.0, b=0.0, c=0.0, j_load=1e-3),
    ("Cont", "SeriesDc"): dict(a=0.01, b=0.05, c=0.0, j_load=1e-4), ("Finite", "SeriesDc"): dict(a=0.15, b=0.05, c=0.0, j_load=1e-4),
    ("Cont", "ShuntDc"): dict(a=0.05, b=0.01, c=0.0, j_load=1e-4), ("Finite", "ShuntDc"): dict(a=0.05, b=0.01, c=0.0, j_load=1e-4),
    # cont_sc_extex_dc_env.py:161, finite_sc_extex_dc_env.py:162; cont_sc_eesm_env.py:165 (-> the fall-through default below),
    # finite_sc_eesm_env.py:160 (PolynomialStaticLoad's own defaults)
    ("Cont", "ExtExDc"): dict(a=0.0, b=0.0, c=0.0, j_load=1e-4), ("Finite", "ExtExDc"): dict(a=0.0, b=0.0, c=0.0, j_load=1e-4),
    ("Finite", "EESM"): dict(),
}
# the one env class whose ConstantSpeedLoad does not turn at 100 rad/s (cont_tc_shunt_dc_env.py:155)
_OMEGA_FIXED = {"Cont-TC-ShuntDc-v0": 230.0}
# supply voltages that differ from the family default (60 V DC motors, 420 V three-phase)
_U_NOMINAL = {"Cont-CC-PMSM-v0": 300.0, "Finite-CC-SeriesDc-v0": 420.0, "Finite-TC-SeriesDc-v0": 420.0, "Cont-CC-EESM-v0": 300.0}


def default_components(env_id):
    """Per-id defaults, read off the reference env classes (e.g. cont_cc_permex_dc_env.py:146-160,
    finite_cc_pmsm_env.py:148-166, cont_sc_scim_env.py:153-170, cont_cc_series_dc_env.py:144-160,
    cont_cc_shunt_dc_env.py:145-161, cont_cc_synrm_env.py:152-160)."""
    m = _ID.match(env_id)
    if not m:
        raise KeyError(f"{env_id!r} is not on the accelerated path; supported: "
                       "(Finite|Cont)-(CC|TC|SC)-(PermExDc|SeriesDc|ShuntDc|ExtExDc|PMSM|SynRM|SCIM|EESM|DFIM)-v0")
    action, control, motor = m.groups()
    finite = action == "Finite"
    dc = motor.endswith("Dc")
    d_conv_args = dict()
    if motor == "ExtExDc":  # cont_cc_extex_dc_env.py:146-160: MultiConverter of two 4QCs
        sub = comp.FiniteFourQuadrantConverter if finite else comp.ContFourQuadrantConverter
        d = dict(system=bps.BatchedDcMotorSystem, supply=dict(u_nominal=60.0), motor=comp.DcExternallyExcitedMotor,
                 converter=comp.FiniteMultiConverter if finite else comp.ContMultiConverter, constraints=("i_a", "i_e"))
        d_conv_args = dict(subconverters=(sub, sub))
    elif motor == "EESM":  # cont_cc_eesm_env.py:153-170: B6 bridge + 4QC
        subs = (comp.FiniteB6BridgeConverter, comp.FiniteFourQuadrantConverter) if finite else (comp.ContB6BridgeConverter, comp.ContFourQuadrantConverter)
        d = dict(system=bps.BatchedExternallyExcitedSynchronousMotorSystem, supply=dict(u_nominal=420.0),
                 motor=comp.ExternallyExcitedSynchronousMotor, converter=comp.FiniteMultiConverter if finite else comp.ContMultiConverter,
                 constraints=(bps.SquaredConstraint(("i_sq", "i_sd")), bps.LimitConstraint(("i_e",))))
        d_conv_args = dict(subconverters=subs)
    elif motor == "DFIM":  # cont_cc_dfim_env.py:160-180: stator and rotor B6 bridges
        sub = comp.FiniteB6BridgeConverter if finite else comp.ContB6BridgeConverter
        d = dict(system=bps.BatchedDoublyFedInductionMotorSystem, supply=dict(u_nominal=420.0), motor=comp.DoublyFedInductionMotor,
                 converter=comp.FiniteMultiConverter if finite else comp.ContMultiConverter,
                 constraints=(bps.SquaredConstraint(("i_sq", "i_sd")),))
        d_conv_args = dict(subconverters=(sub, sub))
    elif dc:
        motor_cls = {"PermExDc": comp.DcPermanentlyExcitedMotor, "SeriesDc": comp.DcSeriesMotor, "ShuntDc": comp.DcShuntMotor}[motor]
        d = dict(system=bps.BatchedDcMotorSystem, supply=dict(u_nominal=60.0), motor=motor_cls,
                 converter=comp.FiniteFourQuadrantConverter if finite else comp.ContFourQuadrantConverter,
                 constraints=("i_a", "i_e") if motor == "ShuntDc" else ("i",))
        # (the reference's shunt envs additionally wrap the system in a CurrentSumProcessor: default_physical_system_wrappers)
    else:
        motor_cls = {"PMSM": comp.PermanentMagnetSynchronousMotor, "SynRM": comp.SynchronousReluctanceMotor,
                     "SCIM": comp.SquirrelCageInductionMotor}[motor]
        system = bps.BatchedSquirrelCageInductionMotorSystem if motor == "SCIM" else bps.BatchedSynchronousMotorSystem
        d = dict(system=system, supply=dict(u_nominal=420.0), motor=motor_cls,
                 converter=comp.FiniteB6BridgeConverter if finite else comp.ContB6BridgeConverter,
                 constraints=(bps.SquaredConstraint(("i_sq", "i_sd")),))
    if env_id in _U_NOMINAL:
        d["supply"] = dict(u_nominal=_U_NOMINAL[env_id])
    if control == "SC":
        d["load"] = (comp.PolynomialStaticLoad, dict(load_parameter=_SC_LOAD.get((action, motor), dict(a=0.01, b=0.01, c=0.0))))
    else:
        d["load"] = (comp.ConstantSpeedLoad, dict(omega_fixed=_OMEGA_FIXED.get(env_id, 100.0)))
    d["tau"] = 1e-5 if finite else 1e-4
    d["converter_args"] = d_conv_args
    return d


# Wiener generators whose arguments differ from WienerProcessReferenceGenerator's defaults (sigma_range (1e-3, 1e-1), limit_margin None =
# nominal / limit): cont_cc_permex_dc_env.py:164, finite_cc_permex_dc_env.py:164, cont_tc_permex_dc_env.py:165, finite_tc_permex_dc_env.py:164,
# cont_sc_permex_dc_env.py:169, finite_sc_permex_dc_env.py:170, cont_sc_series_dc_env.py:167, finite_sc_series_dc_env.py:167,
# cont_sc_shunt_dc_env.py:169, finite_sc_shunt_dc_env.py:169, cont_sc_synrm_env.py:163, finite_sc_synrm_env.py:169, cont_sc_scim_env.py:171,
# finite_sc_scim_env.py:176, cont_sc_dfim_env.py:181, finite_sc_dfim_env.py:181
_SIGMA_RANGE = {
    "Cont-CC-PermExDc-v0": (1e-2, 1e-1), "Finite-CC-PermExDc-v0": (1e-2, 1e-1), "Cont-TC-PermExDc-v0": (1e-2, 1e-1), "Finite-TC-PermExDc-v0": (1e-2, 1e-1),
    "Cont-SC-PermExDc-v0": (1e-3, 5e-2), "Finite-SC-PermExDc-v0": (1e-3, 5e-3), "Cont-SC-SeriesDc-v0": (1e-3, 2e-2), "Finite-SC-SeriesDc-v0": (1e-3, 5e-3),
    "Cont-SC-ShuntDc-v0": (1e-3, 3e-2), "Finite-SC-ShuntDc-v0": (1e-3, 5e-3), "Cont-SC-SynRM-v0": (1e-3, 1e-2), "Finite-SC-SynRM-v0": (1e-3, 1e-2),
    "Cont-SC-SCIM-v0": (1e-3, 1e-2), "Finite-SC-SCIM-v0": (1e-3, 1e-2), "Cont-SC-DFIM-v0": (1e-3, 1e-2), "Finite-SC-DFIM-v0": (1e-3, 1e-2),
}
# cont_cc_eesm_env.py:153 (the excitation current's reference stays positive), cont_tc_shunt_dc_env.py:164
_LIMIT_MARGIN = {"Cont-CC-EESM-v0": dict(i_e=(0, 1)), "Cont-TC-ShuntDc-v0": dict(torque=(0, 0.8))}


def default_env_modules(env_id):
    """Per-id defaults of the reference generator and the reward function, read off the reference env classes the way
    `default_components` is (e.g. cont_cc_pmsm_env.py:146-152, cont_cc_eesm_env.py:149-156, cont_cc_extex_dc_env.py:149-155,
    cont_tc_pmsm_env.py:151, cont_sc_pmsm_env.py:151): CC envs reference the current(s) with one WienerProcessReferenceGenerator each
    (MultipleReferenceGenerator), TC envs the torque, SC envs omega; WeightedSumOfErrors with equal weights over the referenced
    states, gamma 0.9, power 1, no bias, the derived violation reward.
    -> dict(reference_states, generator=dict(BatchedWienerProcessReferenceGenerator arguments), reward=dict(set_reward keywords))."""
    m = _ID.match(env_id)
    if not m:
        default_components(env_id)  # (raises the KeyError that names the supported ids)
    _, control, motor = m.groups()
    if control == "TC":
        states = ("torque",)
    elif control == "SC":
        states = ("omega",)
    elif motor in ("PermExDc", "SeriesDc"):
        states = ("i",)
    elif motor == "ShuntDc":
        states = ("i_a",)
    elif motor == "ExtExDc":
        states = ("i_a", "i_e")
    elif motor == "EESM":
        states = ("i_sd", "i_sq", "i_e")
    else:
        states = ("i_sd", "i_sq")
    gen = dict(sigma_range=_SIGMA_RANGE.get(env_id, (1e-3, 1e-1)), episode_lengths=(500, 2000), limit_margin=_LIMIT_MARGIN.get(env_id), initial_range=None)
    reward = dict(reward_weights={s: 1.0 / len(states) for s in states}, gamma=0.9, reward_power=1, bias=0.0, violation_reward=None,
                  normed_reward_weights=False)
    return dict(reference_states=states, generator=gen, reward=reward)


def default_physical_system_wrappers(env_id):
    """The physical-system wrappers the reference's env class puts around its system when the caller names none: the six shunt envs'
    `CurrentSumProcessor(("i_a", "i_e"))` (envs/gym_dcm/shunt_dc_motor_env/*.py, e.g. cont_cc_shunt_dc_env.py:187), nothing elsewhere."""
    from .physical_system_wrappers import CurrentSumProcessor

    m = _ID.match(env_id)
    if not m:
        default_components(env_id)  # (raises the KeyError that names the supported ids)
    return (CurrentSumProcessor(("i_a", "i_e")),) if m.group(3) == "ShuntDc" else ()


def default_ode_solver(env_id, tau=None, load=None):
    """The solver `make(env_id)` uses when the caller names none.  The reference's default is scipy's ADAPTIVE dopri5 (rtol 1e-6,
    solvers.py:139-184); the device integrates with fixed steps, so the default is chosen per env such that the fp32 trajectories stay
    within the 1e-4 contract of the reference's default-solver runs.  Measured on the GPU over every one of the reference's 54 env ids
    exactly as `gem.make(env_id)` builds them plus ~100 further recorded dopri5 runs (tests/solver_scan.py -> profiles/r04a_solver_scan.md):

    * ConstantSpeedLoad (the CC / TC envs): one classical RK4 step per control step -- the electrical subsystem is linear there and the
      step is the exact one-step map of the scheme: <= 1.8e-5 on the envs as shipped (free runs far beyond the limits: < 1e-4).
      More sub-steps make fp32 WORSE here (rounding accumulates: 8 sub-steps reach 2.7e-3 on a free-running EESM), so none;
    * PolynomialStaticLoad (the SC envs: omega is a state, the load torque has kinks at |omega| = a tau_decay / J): RK4 with every step
      corrected for those kinks in closed form (split_kinks; the adaptive reference solver rejects and splits such steps): <= 6.3e-6 on
      every recorded run with such a load (plain RK4: up to 7.9e-5 -- Cont-SC-ShuntDc-v0 --, 6.8e-5 on the SCIM), ONE pass of the
      scheme (rounds 2-3: up to three), at plain RK4's rate wherever the launch is bandwidth bound (BASELINE config 4).

    `tau` / `load` (instance, class or class name): what the env is actually built with, when it differs from the env id's defaults."""
    d = default_components(env_id)
    if load is None:
        load = d["load"][0]
    lname = load if isinstance(load, str) else (load.__name__ if isinstance(load, type) else type(load).__name__)
    return comp.RK4Solver(split_kinks=lname != "ConstantSpeedLoad")


class BatchedElectricMotorEnv:
    """Vector-env style shell around a batched physical system (physics + done mask only)."""

    def __init__(self, physical_system, observation=None, _n_ref=0, _defer_create=False, flux_action=None, state_noise=None, _reward_config=None,
                 episodes=None, _episode_reward=False):
        """episodes: None | dict(max_steps=, statistics=) -- the episode stage (`make(max_episode_steps=, episode_statistics=)`).
        flux_action: None | 'SCIM' | 'DFIM' -- the flux-oriented dq action processor (needs a FluxObserver in the observation chain).
        state_noise: None | the StateNoiseProcessor's spec with the constraint masks and the auto-reset asked for (`make` builds it; the
        system itself then has no constraints and no auto-reset): `terminated` and the returned state are the noisy ones.
        observation: None, or dict(chain=, observed_states=, flatten=) for a device-side `ObservationStage` behind the system: `reset()`,
        `step()` and `rollout()` then return the PROCESSED state, `state_space` / `state_names` describe it; `physical_system` stays raw.
        Everything behind the physics is the `pipeline` (observation.py: ObservationPipeline)."""
        from .observation import ObservationPipeline

        self.physical_system = physical_system
        self.n_envs = physical_system.n_envs
        pipe = self.pipeline = ObservationPipeline(physical_system, observation, _n_ref, flux_action, _defer_create, noise=state_noise,
                                                   reward_config=_reward_config, episode=episodes, episode_reward=_episode_reward)
        self.episodes = pipe.episode
        self.observation_stage, self.flux, self.flux_action, self._flux_only = pipe.stage, pipe.flux, pipe.flux_action, pipe.flux_only
        if pipe.flux is not None:  # the observer holds ONE machine's parameters: the system refuses a table now and later (set_env_parameters)
            from .env_parameters import REFUSAL as EP_REFUSAL

            why = EP_REFUSAL + "a FluxObserver or a FluxOrientedDqToAbcActionProcessor (the observer holds one machine's parameters)"
            if getattr(physical_system, "env_parameters", None) is not None:
                raise NotImplementedError(why)
            physical_system._env_parameters_refusal = why
        self.state_noise = pipe.noise
        self.action_space = pipe.action_space
        self.state_space = physical_system.state_space if pipe.stage is None else pipe.stage.observation_space
        self.state_names = list(physical_system.state_names if pipe.stage is None else pipe.stage.observation_names)

    truncated = property(lambda self: self.pipeline.truncated, doc="[N] bool: the envs the last step truncated (False without a time limit)")

    def episode_statistics(self):
        """-> dict(length, ret, last_length, last_ret, n_finished): [N] device tensors, views of the episode stage's state -- the running
        episode's steps and return (float64), the totals of the episode that ended last, the number of finished episodes."""
        if self.episodes is None or not self.episodes.statistics:
            raise ValueError("this env keeps no episode statistics: build it with make(..., episode_statistics=True)")
        return self.episodes.fields()

    def get_checkpoint(self):
        """`physical_system.get_checkpoint()`, plus the flux observer's per-env state (`flux_observer`: float64 [4, N]) when the env has one,
        plus, with a StateNoiseProcessor, `state_noise`: the stream position and the done mask whose envs restart in front of the next step,
        plus, with an episode stage, `episodes`: its state blob and the mask of the reset in front of the next step."""
        ck = self.physical_system.get_checkpoint()
        if self.flux is not None:
            ck["flux_observer"] = self.flux.get_state()
        if self.state_noise is not None:
            ck["state_noise"] = dict(position=self.state_noise.get_position(), done=self.physical_system._done.clone())
        if self.episodes is not None:
            ck["episodes"] = dict(state=self.episodes.get_state(), reset_mask=self.episodes.reset_mask.clone())
        return ck

    def _checkpoint_keys(self):
        """The entries `set_checkpoint` reads beside the physical system's, by the stages this env has."""
        return [k for k, part in (("flux_observer", self.flux), ("state_noise", self.state_noise), ("episodes", self.episodes)) if part is not None]

    def _check_checkpoint(self, ckpt):
        """What is checked before anything is restored: every entry this env reads is there."""
        missing = [k for k in ["state", "switch_state", "aux", "k"] + self._checkpoint_keys() if k not in ckpt]
        if missing:
            raise ValueError(f"the checkpoint lacks {missing}: it was taken from an env without these stages, or is not a get_checkpoint() result")

    def set_checkpoint(self, ckpt):
        """Restore `get_checkpoint()` of an env of the same configuration: the next `step()` continues bit for bit.  An entry this env needs
        and the checkpoint lacks raises before anything is restored."""
        self._check_checkpoint(ckpt)
        self.physical_system.set_checkpoint(ckpt)
        if self.flux is not None:
            self.flux.set_state(ckpt["flux_observer"])
        if self.state_noise is not None:
            self.state_noise.set_position(ckpt["state_noise"]["position"])
            self.physical_system._done.copy_(ckpt["state_noise"]["done"])
        if self.episodes is not None:
            self.episodes.set_state(ckpt["episodes"]["state"])
            self.episodes.reset_mask.copy_(ckpt["episodes"]["reset_mask"])

    @property
    def unwrapped(self):
        return self

    # the pipeline's buffers under the names they had on the env
    _ext = property(lambda self: self.pipeline.rows)
    _raw_scratch = property(lambda self: self.pipeline.raw_scratch)
    _ext_scratch_buf = property(lambda self: self.pipeline.ext_scratch)

    def _shown(self, raw):
        """What the env hands out for the system's `raw` state (n_envs == 1 with numpy in / out keeps numpy)."""
        if self.observation_stage is None and self.state_noise is None:
            return raw
        out = self.pipeline.state
        return out.reshape(-1).double().cpu().numpy() if isinstance(raw, np.ndarray) else out

    def reset(self, seed=None, options=None):
        """All envs to the initial state; returns (observations, {})."""
        raw = self.physical_system.reset()
        self.pipeline.reset()
        return self._shown(raw), {}

    def step(self, actions, references=None):
        """-> (obs [N, S_out], reward, terminated [N] uint8, truncated, {}); truncated: False, or with a time limit [N] bool.  reward: [N] device tensor when a reward function is
        installed (`physical_system.set_reward`) and `references [N, n_ref]` are passed, else None.  With auto_reset (default for
        n_envs > 1) an env that terminated restarts from the reset state on its next step; the state it shows
        right after that restart is `physical_system.reset_observation`."""
        ps, pipe = self.physical_system, self.pipeline
        if self.state_noise is not None and references is not None:
            raise NotImplementedError("step(actions, references=...) with a StateNoiseProcessor: the reward is computed on the noisy state by the complete "
                                      "env (make(..., reward_function=...)), not by the physics launch")
        if self.flux_action:  # launch 1 of 4: the dq actions rotated into the frame the last observation left
            pipe.bind_actions(pipe.dq_to_device(actions))()
            actions = pipe.abc
        pipe.before_step()  # (a StateNoiseProcessor: the envs the last noisy row terminated restart; a time limit: the truncated ones)
        obs = ps.simulate(actions, references=references) if references is not None else ps.simulate(actions)
        pipe.after_step()
        return self._shown(obs), (ps.reward if references is not None else None), ps.done, pipe.truncated, {}

    def _rollout(self, physics, K, obs_out, kw):
        """A physics rollout into the pipeline's raw rows, then its launches: ONE pass over the stored rows writes the processed
        `[K, N, n_post]` trajectory (into `obs_out`, when given)."""
        pipe = self.pipeline
        pipe.refuse_rollout()
        want = kw.pop("episode_statistics", None)
        if pipe.episode is None and want:
            pipe.bind_episode_rows(None, outputs=want)  # (raises: the env has no stage)
        res = physics(obs_out=pipe.raw_rows(K, obs_out, kw.get("last_only", False)), **kw)
        episodes, stats = pipe.bind_episode_rows(res[1], outputs=want)  # (the physics-only env: lengths, no reward)
        episodes, rows = self._tail(K, res[0], (obs_out, res[1]), res[1], episodes, None)
        if episodes is not None:
            episodes()
        return (res[0] if rows is None else rows(),) + tuple(res[1:]) + ((stats,) if want else ())

    def rollout(self, actions, obs_out=None, **kw):
        """PhysicalSystem.rollout; with an observation stage the raw trajectory goes into a scratch tensor and ONE `apply` writes the
        processed `[K, N, n_post]` trajectory (into `obs_out`, when given).  episode_statistics=True (an env with the episode stage): one
        more result, dict(ended, finished_return, finished_length) [K, N] in the pipeline's scratch."""
        return self._rollout(lambda **k: self.physical_system.rollout(actions, **k), len(actions), obs_out, kw)

    def rollout_synthetic(self, K, obs_out=None, **kw):
        """K fused steps on random actions generated on the device (PhysicalSystem.rollout_synthetic)."""
        return self._rollout(lambda **k: self.physical_system.rollout_synthetic(K, **k), K, obs_out, kw)

    def bind_rollout(self, actions, obs_out, done_out, stream=None, episode_statistics=None):
        """-> zero-argument launch(): the pre-bound `gemx_rollout` call for fixed tensors (PhysicalSystem.bind_rollout); with an
        observation stage `obs_out` is the processed `[K, N, n_post]` tensor and a launch is the rollout plus the pipeline's launches.
        episode_statistics: dict(ended=, finished_return=, finished_length=) of [K, N] tensors the episode stage's pass writes."""
        ps, pipe = self.physical_system, self.pipeline
        pipe.refuse_rollout()
        if pipe.stage is None and pipe.episode is None and not episode_statistics:
            return ps.bind_rollout(actions, obs_out, done_out, stream=stream)
        return self._bind("bind_rollout", True, actions, (obs_out, done_out), stream, episode_statistics)

    # ------------------------------------------------------------------ K-step rollouts over stored rows: one table, one check, one allocator, one plan
    def _specs(self, K, complete=False, episodic=False, actions_out=False):
        """-> (the `actions` spec, the ordered output specs) of one family of stored-rows rollouts -- physics-only or complete, episodic
        (the time limit inside the launch) or not, with or without the policy's `actions_out`.  An output spec is (name, dtype, shape);
        the actions are checked by their element count, (name, dtype, numel) -- None for the physics-only rollout without a time limit,
        whose actions `PhysicalSystem.bind_rollout` checks itself (it takes float16 tensors too).  Needs no device."""
        torch = bps._torch()
        ps, stage = self.physical_system, self.observation_stage
        N = ps.n_envs
        real = getattr(ps, "_tdtype", None) or getattr(torch, ps._dtype_name)
        space = ps.action_space
        discrete = hasattr(space, "n") or hasattr(space, "nvec")
        n_act = 1 if discrete else int(space.shape[0])
        n_state = len(ps.state_names) if stage is None else stage.n_out
        mask = (torch.uint8, (K, N))
        specs = [("state_out" if complete else "obs_out", real, (K, N, n_state) if getattr(ps, "_obs_layout", "aos") == "aos" else (K, n_state, N))]
        if complete:
            specs += [("refs_out", real, (K, N, len(self.reference_names))), ("reward_out", real, (K, N))]
        if actions_out:  # (what the policy kernel writes: the action rows as the physics reads them)
            specs.append(("actions_out",) + (mask if discrete else (torch.float32, (K, N, n_act))))
        specs.append(("terminated_out" if episodic else "done_out",) + mask)
        if episodic:
            specs.append(("truncated_out",) + mask)
        return ("actions", torch.uint8 if discrete else real, K * N * n_act) if complete or episodic else None, specs

    def _check_tensor(self, what, t, name, dtype, shape=None, numel=None):
        """One tensor of a bound or eager call: dtype, shape, contiguity, device, in this order (needs no device)."""
        torch = bps._torch()
        ps = self.physical_system
        tdev = getattr(ps, "_tdev", None) or torch.device("cuda", ps._device)
        if not torch.is_tensor(t):
            raise ValueError(f"{what}: {name} must be a tensor")
        if t.dtype != dtype:
            raise ValueError(f"{what}: {name} must have dtype {dtype}, not {t.dtype}")
        if (shape is not None and tuple(t.shape) != shape) or (numel is not None and t.numel() != numel):
            raise ValueError(f"{what}: {name} must have shape {shape if shape is not None else f'of {numel} elements'}, not {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
        if t.device != tdev:
            raise ValueError(f"{what}: {name} must be on device {tdev}, not {t.device}")

    def _need_device(self):
        if getattr(self.physical_system, "_handle", None) is None:
            raise bps._lib.GemxError("the physical system has no device handle (built with _defer_create, or closed)")

    def _check_call(self, what, K, actions, outs, bound, episode_statistics=None, **family):
        """What every stored-rows entry point `what` checks before anything is launched, in one order -> (K, the output specs of
        `_specs(K, **family)`): the family's refusal; `actions` (K is None: K is their first dimension) have a shape; K >= 1; a bound launch
        allocates nothing, so every output is given and `episode_statistics` is not True; every tensor given, in table order -- the
        actions of a bound launch first (the eager entry points convert what `rollout` takes); a bound launch cannot carry a
        ReplayReferenceGenerator; the system has a device handle.  Everything but the last needs no device."""
        torch = bps._torch()
        episodic = family.get("episodic", False)
        if episodic:
            self.pipeline.need_episodic()
            if torch.is_tensor(actions) and actions.dtype is torch.float16:
                from .episodes import episodic_refusal

                raise NotImplementedError(episodic_refusal(self.physical_system, "a half-precision action tensor (fp32 actions)"))
        else:
            self.pipeline.refuse_rollout()
        if K is None:
            if not hasattr(actions, "shape") or len(actions.shape) < 1:
                raise ValueError(f"{what} needs {'a device tensor of ' if bound and not episodic else ''}actions [K, N, A] / [K, N]")
            K = actions.shape[0]
        K = int(K)
        if K < 1:
            raise ValueError(f"{what}: K must be >= 1, not {K}")
        actions_spec, specs = self._specs(K, **family)
        if bound:
            for t, (name, _, _) in zip(outs, specs):
                if t is None:
                    raise ValueError(f"{what}: {name} must be given (a bound launch allocates nothing)")
            if episode_statistics is True:
                raise ValueError(f"{what}: episode_statistics must be a dict of tensors (a bound launch allocates nothing)")
            if actions is not None and actions_spec is not None:  # (a policy rollout reads no action tensor)
                self._check_tensor(what, actions, *actions_spec[:2], numel=actions_spec[2])
        for t, (name, dtype, shape) in zip(outs, specs):
            if t is not None:
                self._check_tensor(what, t, name, dtype, shape)
        if bound and family.get("complete") and isinstance(self.reference_generator, ReplayReferenceGenerator):
            self.reference_generator.bind_rollout_shell(outs[3], outs[1])  # (raises: cannot be captured)
        self._need_device()
        return K, specs

    def _allocate(self, specs, given):
        """-> `given` with a fresh tensor of the spec's dtype and shape in the place of every None."""
        torch, device = bps._torch(), self.physical_system._tdev
        return tuple(torch.empty(shape, dtype=dtype, device=device) if t is None else t for t, (_, dtype, shape) in zip(given, specs))

    def _tail(self, K, raw, outs, restart, episodes, stream, eager=False, generators=True):
        """-> the launchers behind the physics of a stored-rows rollout, in order: the episode stage's pass over the rows, the pipeline's
        launches over the stored rows.  The one thing the complete env does differently."""
        return episodes, self.pipeline.bind_after_rollout(raw, restart, None, outs[0], stream)

    def _plan(self, physics, K, outs, truncated_out, stream, episode_statistics, eager=False, extra=(), generators=True):
        """-> launch() of any stored-rows rollout on fixed tensors, all on `stream` (default: the current one): `physics(raw, done |
        terminated, truncated, ended, stream)` -> its launcher; `_tail` (the complete env: generators and reward pass first, the
        references shown last); with a time limit (`truncated_out` given) row K-1 into the episode stage's bytes, its `reset_mask`
        cleared.  outs: (obs_out, done_out) or (state_out, refs_out, reward_out, done_out); `launch()` returns outs but the last, `extra`
        (a policy rollout's actions_out), the last of outs, truncated_out and the statistics dict, as far as they exist -- the order of
        `_specs`.  generators=False: the physics has written refs_out and the generator state itself (the complete policy rollout).  Decided here, once: where the physics writes, which rows
        the episode stage's pass reads and writes, and the rows everything behind it restarts on -- ENDED with a time limit, else done."""
        ps, pipe = self.physical_system, self.pipeline
        stream = stream if stream is not None else bps._torch().cuda.current_stream(ps._tdev)
        done = outs[-1]
        raw = pipe.raw_rows(K, outs[0])
        episodes, stats = pipe.bind_episode_rows(done, outs[2] if len(outs) == 4 else None, episode_statistics, stream)  # (no reward rows: lengths only)
        ended, last, result = done, None, outs[:-1] + tuple(extra) + outs[-1:]
        if truncated_out is not None:
            ended = stats["ended"] if stats else pipe.ended_scratch
            last, result = pipe.episode.bind_after_episodic_rollout(truncated_out, ended, stream), result + (truncated_out,)
        return bps._lib.sequence(physics(raw, done, truncated_out, ended, stream), *self._tail(K, raw, outs, ended, episodes, stream, eager, generators), last,
                                 result=result + ((stats,) if stats else ()))

    def _episodic_physics(self, a, raw, terminated, truncated, ended, stream):
        """-> the first two launches of every episodic rollout: the reset a truncating `step()` left pending in the stage's `reset_mask`
        (the masked `gemx_reset`), then the episodic physics reading the stage's `length`."""
        pipe = self.pipeline
        return bps._lib.sequence(pipe.bind_before_step(stream),
                                 self.physical_system.bind_rollout_episodic(a, pipe.episode.length, pipe.episode.max_steps, raw, terminated, truncated, ended, stream=stream))

    def _bind(self, what, bound, actions, outs, stream, episode_statistics, **family):
        """-> launch() of the entry point `what` of a family that reads an action tensor: check, allocate what an eager call (bound=False)
        did not give, plan.  A bound entry point returns the launch; its eager counterpart -- which takes the actions as `rollout` takes
        them -- calls it once: both reach the device by the same code."""
        K, specs = self._check_call(what, None, actions, outs, bound, episode_statistics, **family)
        ps = self.physical_system
        a = actions if bound else ps._actions_to_device(actions, (K, ps._n_envs))
        outs = self._allocate(specs, outs)
        if family.get("episodic"):
            return self._plan(lambda *t: self._episodic_physics(a, *t), K, outs[:-1], outs[-1], stream, episode_statistics, eager=not bound)
        return self._plan(lambda raw, done, _truncated, _ended, st: ps.bind_rollout(a, raw, done, stream=st), K, outs, None, stream, episode_statistics, eager=not bound)

    def bind_rollout_episodic(self, actions, obs_out, terminated_out, truncated_out, stream=None, episode_statistics=None):
        """-> zero-argument launch() of `rollout_episodic` on fixed tensors (every output must be given: a bound launch allocates
        nothing); `launch()` returns `(obs_out, terminated_out, truncated_out[, stats])`.  Every launch goes to ONE stream and nothing
        lives on the host, so it can be captured with `torch.cuda.graph` and replayed: the counters carry from replay to replay.
        episode_statistics: dict(ended=, finished_return=, finished_length=) of [K, N] tensors the episode stage's pass writes."""
        return self._bind("bind_rollout_episodic", True, actions, (obs_out, terminated_out, truncated_out), stream, episode_statistics, episodic=True)

    # ------------------------------------------------------------------ policy rollouts: the actor inside the episodic launch
    def _bind_policy(self, what, bound, policy, K, outs, obs0, references, noise, stream, episode_statistics, complete=False):
        """-> launch() of the policy entry point `what`: the policy's own checks (no device call), then what `_bind` does -- check,
        allocate what an eager call did not give, plan.  outs: (obs_out, actions_out, terminated_out, truncated_out); complete (the
        complete env's own references and reward in the loop): (state_out, refs_out, reward_out, actions_out, terminated_out,
        truncated_out), no `references` -- the generator must be one the kernel steps in the lane."""
        from .episodes import episodic_refusal
        from .policy import MLPPolicy

        pipe, ps = self.pipeline, self.physical_system
        pipe.need_episodic()
        torch = bps._torch()
        if not isinstance(policy, MLPPolicy):
            raise ValueError(f"{what}: policy must be an MLPPolicy")
        if isinstance(K, bool) or not isinstance(K, int) or K < 1:
            raise ValueError(f"{what}: K must be an integer >= 1, not {K!r}")
        if pipe.stage is not None or pipe.flux is not None:
            raise NotImplementedError(f"{what} is not available with a FluxObserver or any observation-side processor: the policy reads the raw state row")
        if getattr(ps, "_obs_layout", "aos") != "aos":
            raise NotImplementedError(f"{what} is not available with obs_layout='soa': the tensors are [K, N, S_out]")
        if complete:
            self._policy_generator(what)
        n_state, N = len(ps.state_names), ps.n_envs
        columns = list(range(n_state)) if policy.columns is None else list(policy.columns)
        if any(c >= n_state for c in columns):
            raise ValueError(f"{what}: the policy selects column {max(columns)}, the state row has {n_state} columns")
        for name, t in (("obs0", obs0), ("references", references), ("noise", noise), ("actions_out", outs[3 if complete else 1])):
            if torch.is_tensor(t) and t.dtype in (torch.float16, torch.bfloat16):
                raise NotImplementedError(episodic_refusal(ps, f"a half-precision {name} tensor (fp32 tensors)"))
        n_ref = len(self.reference_names) if complete else 0
        if references is not None:
            if not torch.is_tensor(references) or references.dim() != 3:
                raise ValueError(f"{what}: references must be a tensor [K, N, n_ref]")
            n_ref = int(references.shape[2])
            if not 1 <= n_ref <= 4:
                raise ValueError(f"{what}: references has {n_ref} columns; 1 to 4 (GEMX_MAX_REF)")
            self._check_tensor(what, references, "references", torch.float32, (K, N, n_ref))
        if len(columns) + n_ref != policy.n_in:
            raise ValueError(f"{what}: {len(columns)} observation columns + {n_ref} references = {len(columns) + n_ref} inputs, the policy's first layer takes {policy.n_in}")
        space = ps.action_space
        discrete = hasattr(space, "n") or hasattr(space, "nvec")
        n_logit = int(getattr(space, "n", 0) or np.prod(getattr(space, "nvec", [0]))) if discrete else int(space.shape[0])
        if policy.n_out != n_logit:
            raise ValueError(f"{what}: the policy's output width is {policy.n_out}, the converter takes {n_logit} "
                             f"({'one logit per discrete action' if discrete else 'one output per action component'})")
        if noise is not None:
            self._check_tensor(what, noise, "noise", torch.float32, (K, N, n_logit))
        if obs0 is not None:
            self._check_tensor(what, obs0, "obs0", torch.float32, (N, n_state))
        _, specs = self._check_call(what, K, None, outs, bound, episode_statistics, complete=complete, episodic=True, actions_out=True)
        if complete:
            state_out, refs_out, reward_out, actions_out, terminated_out, truncated_out = self._allocate(specs, outs)
            return self._plan(lambda *t: self._policy_physics(policy, K, columns, n_ref, obs0, self._refs, noise, actions_out, *t, refs_out=refs_out), K,
                              (state_out, refs_out, reward_out, terminated_out), truncated_out, stream, episode_statistics, eager=not bound, extra=(actions_out,),
                              generators=False)
        obs_out, actions_out, terminated_out, truncated_out = self._allocate(specs, outs)
        return self._plan(lambda *t: self._policy_physics(policy, K, columns, n_ref, obs0, references, noise, actions_out, *t), K, (obs_out, terminated_out),
                          truncated_out, stream, episode_statistics, eager=not bound, extra=(actions_out,))

    def _policy_physics(self, policy, K, columns, n_ref, obs0, references, noise, actions_out, raw, terminated, truncated, ended, stream, refs_out=None):
        """-> the pending masked reset, then `gemx_rollout_policy` on fixed tensors (the policy counterpart of `_episodic_physics`).
        refs_out given: `gemx_rollout_policy_complete` -- `references` is then the [N, n_ref] row shown now, and the env's generator handle
        goes with the call: the launch writes refs_out and advances the generators itself."""
        import ctypes as C

        ps, pipe = self.physical_system, self.pipeline
        lib = bps._lib
        call = lib.GemxPolicyCall()
        call.struct_size, call.K, call.n_cols, call.n_ref, call.max_steps = C.sizeof(call), K, len(columns), n_ref, pipe.episode.max_steps
        for i, c in enumerate(columns):
            call.columns[i] = c
        obs0 = ps._obs if obs0 is None else obs0
        call.obs0_dev, call.refs_dev, call.noise_dev = obs0.data_ptr(), (references.data_ptr() if references is not None else None), (noise.data_ptr() if noise is not None else None)
        call.length_dev, call.obs_out_dev, call.actions_out_dev = pipe.episode.length.data_ptr(), raw.data_ptr(), actions_out.data_ptr()
        call.terminated_out_dev, call.truncated_out_dev, call.ended_out_dev = terminated.data_ptr(), truncated.data_ptr(), ended.data_ptr()
        args = (policy._on_device(ps._device), C.byref(call), C.c_void_p(stream.cuda_stream))
        keep = (call, policy, obs0, references, noise, actions_out, raw, terminated, truncated, ended, stream, pipe.episode.length)
        entry = ps._L.gemx_rollout_policy
        if refs_out is not None:
            gen = self.reference_generator
            profile = isinstance(gen, ProfileReferences)
            args = args[:2] + (C.c_void_p(refs_out.data_ptr()), None if profile else gen._handle, gen._handle if profile else None) + args[2:]
            keep, entry = keep + (refs_out, gen), ps._L.gemx_rollout_policy_complete
        return lib.sequence(pipe.bind_before_step(stream), lib.counting_call(entry, ps, K, args, keep))

    def bind_rollout_policy_episodic(self, policy, K, obs_out, actions_out, terminated_out, truncated_out, obs0=None, references=None, noise=None, stream=None,
                                     episode_statistics=None):
        """-> zero-argument launch() of `rollout_policy_episodic` on fixed tensors (every output must be given); `launch()` returns
        `(obs_out, actions_out, terminated_out, truncated_out[, stats])`.  One stream, nothing on the host: capturable with
        `torch.cuda.graph`; `policy.set_weights` between replays changes the weights the next replay reads."""
        return self._bind_policy("bind_rollout_policy_episodic", True, policy, K, (obs_out, actions_out, terminated_out, truncated_out), obs0, references, noise,
                                 stream, episode_statistics)

    def rollout_policy_episodic(self, policy, K, obs0=None, references=None, noise=None, obs_out=None, actions_out=None, terminated_out=None, truncated_out=None,
                                episode_statistics=None):
        """K fused control steps of an env built with `max_episode_steps=M`, each on the action `policy` (an `MLPPolicy`) computes inside
        the launch from the row the previous step wrote (csrc/gemx_policy.hip): -> (traj [K, N, S_out], actions [K, N, A] or [K, N] uint8,
        terminated, truncated[, stats]).  Step k's input is `[obs_prev[columns], references[k]]`: obs_prev is `obs0` at k = 0 (default: the
        system's internal observation buffer), the previous row afterwards, and the reset observation behind a step that ended the episode.
        `noise [K, N, out]` is added to the output in front of the squash / the argmax (Gaussian: exploration; Gumbel: categorical
        sampling); the kernel has no random stream of its own.  The physics rows are bit for bit `rollout_episodic(actions)`'s; the
        launches around the physics are the same.  On an env without a time limit: ValueError (pass a large M for none).
        The default `obs0` is the buffer `reset()` and `step()` write; the rollouts themselves do not update it, and the masked reset a
        truncating `step()` left pending writes no observation: after an episodic or policy rollout (pass `traj[-1]`, or the reset
        observation where row K-1 ended) and after a `step()` that truncated, give `obs0` explicitly."""
        return self._bind_policy("rollout_policy_episodic", False, policy, K, (obs_out, actions_out, terminated_out, truncated_out), obs0, references, noise,
                                 None, episode_statistics)()

    def _evaluate_policy(self, what, policy, outputs, n_lead, head, mode, obs0, kw):
        """The common part of `evaluate_policy_rollout` / `evaluate_policy_complete_rollout`: the policy and the tuple a rollout returned
        checked, `ended`, `reset_obs` and the stored actions filled in -> the keyword arguments of `MLPPolicy.evaluate_rollout`."""
        from .policy import MLPPolicy

        torch = bps._torch()
        ps = self.physical_system
        if not isinstance(policy, MLPPolicy):
            raise ValueError(f"{what}: policy must be an MLPPolicy")
        if not isinstance(outputs, (tuple, list)) or len(outputs) not in (n_lead + 3, n_lead + 4) or not all(torch.is_tensor(t) for t in outputs[:n_lead + 3]):
            raise ValueError(f"{what}: rollout_outputs must be the tuple the policy rollout returned ({n_lead + 3} tensors, then the statistics dict if it gave one)")
        actions, terminated, truncated = outputs[n_lead:n_lead + 3]
        traj = outputs[0]
        if head == "categorical":
            kw["actions"] = actions
        if mode == "seen":
            stats = outputs[n_lead + 3] if len(outputs) == n_lead + 4 else None
            kw["ended"] = stats["ended"] if stats else torch.bitwise_or(terminated, truncated)
            kw["reset_obs"] = torch.as_tensor(ps.reset_observation, dtype=torch.float32).to(traj.device)
            kw["obs0"] = obs0
        elif obs0 is not None:
            raise ValueError(f"{what}: obs0 belongs to mode='seen'")
        return dict(kw, head=head, mode=mode, system=ps)

    def evaluate_policy_rollout(self, policy, rollout_outputs, head="none", mode="seen", obs0=None, **kw):
        """`policy.evaluate_rollout` on what `rollout_policy_episodic` returned, `(traj, actions, terminated, truncated[, stats])`: the
        env fills in `ended` (the statistics' or terminated | truncated), the reset observation, the stored actions of head="categorical"
        and itself as the owner of the error word.  `obs0 [N, S]`: the observation in front of step 0 (mode="seen"; the rollout's own
        `obs0`).  `references` / `last_references` / `references_next`, `pre_squash`, `log_std`, `last`, `dtype`, outputs: as
        `MLPPolicy.evaluate_rollout` takes them.  An eager convenience: every call allocates `ended` (without statistics) and copies the reset
        observation to the device, so it cannot be captured -- a graph goes through `policy.bind_evaluate_rollout` with tensors the caller
        holds (`reset_obs` a device row made once, `ended` written by `torch.bitwise_or(terminated, truncated, out=ended)`)."""
        what = "evaluate_policy_rollout"
        return policy.evaluate_rollout(rollout_outputs[0] if isinstance(rollout_outputs, (tuple, list)) and rollout_outputs else None,
                                       **self._evaluate_policy(what, policy, rollout_outputs, 1, head, mode, obs0, kw))

    def rollout_episodic(self, actions, obs_out=None, terminated_out=None, truncated_out=None, episode_statistics=None):
        """K fused control steps of an env built with `max_episode_steps=M`, the time limit INSIDE the launch (csrc/gemx_episodic.hip):
        -> (traj [K, N, S_out], terminated [K, N], truncated [K, N][, stats]) uint8 masks -- what K calls of `step(actions[k])` return,
        stacked, bit for bit; the row of a step that ended is the final state, and the env restarts within the launch.  The launches, on
        the current stream: the reset a truncating `step()` left pending; the episodic physics; the episode stage's pass over the rows;
        the pipeline's launches (a FluxObserver resets on the ENDED rows); row K-1 into `env.truncated`, with the stage's `reset_mask`
        cleared.  `step()` and further rollouts continue the same episodes.  On an env without a time limit: ValueError.
        episode_statistics (an env built with `episode_statistics=True`): as `rollout` takes it."""
        return self._bind("rollout_episodic", False, actions, (obs_out, terminated_out, truncated_out), None, episode_statistics, episodic=True)()

    def close(self):
        self.pipeline.close()
        self.physical_system.close()


class CompleteBatchedElectricMotorEnv(BatchedElectricMotorEnv):
    """The batched counterpart of the reference's ElectricMotorEnvironment shell (core.py:197-371): physical system + constraint
    monitor + reference generator + reward function, all on the device.  Observations are `(state [N, S_out], ref [N, n_ref])`;
    both and `reward` / `terminated` are internal buffers that the next call overwrites, as `simulate()`'s are.

    The reward of step k is computed against the references the agent saw before acting; then the generators advance and the
    observation carries the advanced values.  An env that terminated in step k shows the first reference of its fresh generator: under
    auto-reset its next step starts from the reset state, and that is the reference its reward will use."""

    _REWARD_KEYS = ("reward_weights", "gamma", "reward_power", "bias", "violation_reward", "normed_reward_weights")

    def __init__(self, physical_system, reference_generator, reward_function=None, default_modules=None, _defer_create=False, observation=None,
                 flux_action=None, state_noise=None, episodes=None):
        ps = physical_system
        d = default_modules or dict(reference_states=(), reward=dict())
        if observation is None and getattr(ps, "_obs_layout", "aos") != "aos":
            raise ValueError("the complete env needs obs_layout='aos' (states [N, S_out])")
        rf = dict(d["reward"]) if reward_function in (None, "default") else dict(reward_function)
        unknown = sorted(set(rf) - set(self._REWARD_KEYS))
        if unknown:
            raise TypeError(f"reward_function: unknown keywords {unknown}; known: {list(self._REWARD_KEYS)}")
        gen = reference_generator
        if isinstance(gen, ReplayReferenceGenerator) or (isinstance(gen, ProfileReferences) and not gen.is_set):
            gen.set_modules(ps, _defer_create=_defer_create, default_states=d["reference_states"])  # its columns are the env id's referenced states unless it names its own
        elif not gen.is_set:  # (a generator the caller has already announced to this system is taken as it is)
            gen.set_modules(ps, _defer_create=_defer_create)
        if gen.n_envs != ps.n_envs:
            raise ValueError(f"the reference generator serves {gen.n_envs} envs, the physical system {ps.n_envs}")
        self.reference_generator = gen
        self.reference_names = list(gen.reference_names)
        if isinstance(rf.get("reward_weights"), dict):  # weights on states the system does not have ('i_sum' of the shunt envs) cannot be served
            missing = sorted(set(rf["reward_weights"]) - set(ps.state_names))
            if missing:
                raise ValueError(f"reward_weights name {missing}, which are not states of the physical system {list(ps.state_names)}")
        if state_noise is None:
            self.reward_config = ps.set_reward(referenced_states=self.reference_names, **rf)
        else:  # the reward is the noise stage's, on the noisy row: nothing is installed in the stepping kernels
            kw = dict(reward_weights=None, normed_reward_weights=False, violation_reward=None, gamma=0.9, reward_power=1, bias=0.0)
            kw.update(rf)
            self.reward_config = ps._build_reward_config(kw["reward_weights"], self.reference_names, kw["normed_reward_weights"], kw["violation_reward"],
                                                         kw["gamma"], kw["reward_power"], kw["bias"])
        self.reward_range = ps.reward_range
        lo, hi = gen.reference_space
        self.reference_space = Box(lo, hi, dtype=float)
        # (after the generator: a flat observation carries its n_ref columns)
        super().__init__(ps, observation, _n_ref=len(self.reference_names), _defer_create=_defer_create, flux_action=flux_action, state_noise=state_noise,
                         _reward_config=self.reward_config if state_noise is not None else None, episodes=episodes, _episode_reward=True)
        flat = self.observation_stage is not None and self.observation_stage.flatten
        self.observation_space = (self.state_space, self.reference_space)  # gymnasium.spaces.Tuple((state box, reference box)), core.py:278
        if flat:  # FlattenObservation of that Tuple: one box, state then reference
            self.observation_space = Box(np.concatenate((self.state_space.low, self.reference_space.low)),
                                         np.concatenate((self.state_space.high, self.reference_space.high)), dtype=float)
        self._bound = None
        if _defer_create:
            return
        self._reward = bps._torch().zeros((1, ps.n_envs), dtype=ps._tdtype, device=ps._tdev)
        ps._reward_buf = self._reward  # (`physical_system.reward` shows the same buffer)
        self._refs = gen.references
        self._obs = self.pipeline.state if flat else (self.pipeline.state, self._refs)

    def get_checkpoint(self):
        """The physics-only env's checkpoint plus `reference_generator`: the generators' whole device state -- one opaque blob: values,
        sub-episode and super-episode counters, the indices of their random streams, the waveform parameters -- and the references shown
        last, which the reward of the next step reads (`reference_generator.get_state()`; a ReplayReferenceGenerator: its host row index)."""
        ck = super().get_checkpoint()
        ck["reference_generator"] = self.reference_generator.get_state()
        return ck

    def set_checkpoint(self, ckpt):
        """Restore `get_checkpoint()` of a complete env of the same configuration (n_envs, shard, generator kinds and columns, stages): the
        next `step()`, `rollout_complete()` or replay of a captured `bind_step` continues the run bit for bit -- state, references, reward,
        terminated, truncated, statistics.  Everything is copied INTO the buffers the env owns, so launchers bound before the restore stay
        valid.  Checked before anything is enqueued: a checkpoint without the `reference_generator` entry (a physics-only env's), of
        another n_envs, generator kind, column count or shard, or with a truncated blob raises ValueError and leaves the env as it was."""
        self._check_checkpoint(ckpt)
        if "reference_generator" not in ckpt:
            raise ValueError("the checkpoint has no 'reference_generator' entry: it was taken from a physics-only env (or by a version that did not "
                             "carry the generators); a complete env cannot continue from it")
        gen = self.reference_generator
        gen.check_state(ckpt["reference_generator"])
        self.physical_system.check_checkpoint(ckpt)
        gen.set_state(ckpt["reference_generator"])  # (the blob's header is checked here, before its first copy is enqueued)
        super().set_checkpoint(ckpt)

    def reset(self, seed=None, options=None):
        """All envs to the initial state, all generators restarted and advanced once (core.py:312-313, 485-505).
        -> ((state, ref), {})."""
        gen = self.reference_generator
        self.physical_system.reset()
        gen.reset()
        gen.step(None)
        self.pipeline.reset(self._refs)
        return self._obs, {}

    def _launchers(self, a, stream):
        """-> zero-argument step() on the action tensor `a` with everything resolved, returning the observation: the dq -> abc actions
        (flux-oriented action processor only), physics + fused reward reading the generator's buffer, then the pipeline's launches
        around the generator step on the fresh done mask (with an episode stage: on `ended`), which writes that same buffer."""
        import ctypes as C

        ps, pipe = self.physical_system, self.pipeline
        to_abc, keep = None, (a, stream)
        if self.flux_action:  # dq [N, 2 | 4] -> the abc scratch the physics reads
            to_abc, a = pipe.bind_actions(a, stream), pipe.abc
        args = (C.c_void_p(a.data_ptr()), 1, C.c_void_p(self._refs.data_ptr()) if int(self.reward_config.n_ref) else None, C.c_void_p(ps._obs_ptr),
                C.c_void_p(ps._done_ptr), C.c_void_p(self._reward.data_ptr()), C.c_void_p(stream.cuda_stream))
        call = ps._L.gemx_rollout_reward
        noisy = self.state_noise is not None
        if noisy:  # the plain physics step: done and reward come from the noise stage behind it, on the noisy row
            args, call = (C.c_void_p(a.data_ptr()), C.c_void_p(ps._obs_ptr), C.c_void_p(ps._done_ptr), C.c_void_p(stream.cuda_stream)), ps._L.gemx_step
        physics = bps._lib.counting_call(call, ps, 1, args, keep)  # (the host's step counter moves with it)
        after = pipe.bind_after_step(self._refs, stream, generators=self.reference_generator.bind_step(pipe.restart_mask, stream=stream),
                                     reward=self._reward[0] if noisy else None, returns=self._reward[0])
        return bps._lib.sequence(to_abc, pipe.bind_before_step(stream), physics, after, result=self._obs)

    def step(self, actions, references=None):
        """-> ((state [N, S_out], ref [N, n_ref]), reward [N], terminated [N] uint8, truncated, {}); truncated: False, or with a time limit
        [N] bool.  Two kernel launches; three with an observation stage, whose processed state (or flat `[N, n_post + n_ref]` observation)
        replaces the raw one."""
        if references is not None:
            raise TypeError("the complete env generates its references: step(actions)")
        ps = self.physical_system
        a = self.pipeline.dq_to_device(actions) if self.flux_action else ps._actions_to_device(actions, (ps._n_envs,))
        stream = bps._torch().cuda.current_stream(ps._tdev)
        key = (a.data_ptr(), stream.cuda_stream)
        if self._bound is None or self._bound[0] != key:  # (a loop that reuses its action tensor and stream resolves the launches once)
            self._bound = (key, self._launchers(a, stream))
        return self._bound[1](), self._reward[0], ps._done, self.pipeline.truncated, {}

    def bind_step(self, action_buffer, stream=None):
        """A zero-argument `step()` for a closed loop that reuses ONE action tensor: -> `(step, (state, ref), reward, done)`; `step()`
        enqueues the two launches (three with an observation stage) and returns the observation.  Nothing is looked up, allocated or synchronised per call, and no step
        index lives on the host, so `step` can be captured with `torch.cuda.graph` (a linear graph) and replayed -- with the Wiener
        and the other device generators; a ReplayReferenceGenerator keeps its row index on the host and refuses to step while a stream is capturing."""
        ps = self.physical_system
        torch = bps._torch()
        a = action_buffer
        numel = ps._n_envs * self.flux.n_action if self.flux_action else ps._act_numel
        if not (torch.is_tensor(a) and a.device == ps._tdev and a.is_contiguous() and a.dtype is ps._want_dtype and a.numel() == numel):
            raise ValueError(f"bind_step needs a contiguous {ps._want_dtype} tensor of {numel} elements on {ps._tdev}")
        if self.flux_action:
            a = a.view(ps._n_envs, self.flux.n_action)
        stream = stream if stream is not None else torch.cuda.current_stream(ps._tdev)
        return self._launchers(a, stream), self._obs, self._reward[0], ps._done

    # ------------------------------------------------------------------ complete K-step rollouts: physics -> references -> reward
    def _complete_shapes(self, K):
        """(state, refs, reward, done) shapes of a complete K-step rollout: the output table's, for the callers that allocate them."""
        return tuple(shape for _, _, shape in self._specs(K, complete=True)[1])

    def _tail(self, K, raw, outs, restart, episodes, stream, eager=False, generators=True):
        """-> the launchers that follow the physics of a complete K-step rollout, in order, on fixed tensors: the generators in the shell's
        order on the `restart` rows; the reward of row k against the references shown before step k; `episodes` (the episode stage's pass
        over the done and reward rows, directly behind the launch that completes them); the pipeline's launches over the stored rows; row
        K-1 into the references shown, on the launch stream (after the reward pass has read the old ones: `step()` and further rollouts
        continue from it).  restart [K, N]: the rows the generators restart on and the flux observer resets on -- `done_out`, or the ENDED
        rows of an episodic rollout, whose reward pass still reads the terminated rows `done_out`.  eager: run once, on the current
        stream, so a ReplayReferenceGenerator (host state) can take part.  generators=False: the physics launch has stepped the generators
        in the lane and written refs_out (the complete policy rollout); their replay on the restart rows drops out, nothing else."""
        if len(outs) != 4:  # (the inherited physics-only rollouts: no references, no reward)
            return super()._tail(K, raw, outs, restart, episodes, stream, eager)
        torch = bps._torch()
        ps, gen = self.physical_system, self.reference_generator
        state_out, refs_out, reward_out, done_out = outs
        if not generators:
            generators = None
        elif eager and isinstance(gen, ReplayReferenceGenerator):  # (host state: cannot be bound)
            generators = lambda: gen.rollout_shell(K, restart, out=refs_out)  # noqa: E731
        else:
            generators = gen.bind_rollout_shell(restart, refs_out, stream=stream)
        reward = self.bind_reward_rows(raw, refs_out, done_out, reward_out, stream=stream)
        shown, last = self._refs, refs_out[K - 1]

        def show(_current=torch.cuda.current_stream, _on=torch.cuda.stream):
            if _current(ps._tdev) == stream:  # one device-to-device copy on the launch stream
                shown.copy_(last)
            else:
                with _on(stream):
                    shown.copy_(last)

        return generators, reward, episodes, self.pipeline.bind_after_rollout(raw, restart, refs_out, state_out, stream), show

    def bind_reward_rows(self, rows, refs_rows, done, reward_out, stream=None):
        """-> zero-argument launch() of the reward pass (`gemx_reward_rows`) on fixed tensors: the base system's rows [K, N, S] of a
        physics rollout, rewarded against the references shown now (row 0) and refs_rows [K, N, n_ref] (row k + 1 against refs_rows[k]),
        with done [K, N] -> reward_out [K, N].  The tensors are the caller's to get right: contiguous, of the env's dtype, on its device."""
        import ctypes as C

        ps = self.physical_system
        stream = stream if stream is not None else bps._torch().cuda.current_stream(ps._tdev)
        n_ref = int(self.reward_config.n_ref)
        args = (C.c_void_p(rows.data_ptr()), C.c_void_p(self._refs.data_ptr()) if n_ref else None, C.c_void_p(refs_rows.data_ptr()) if n_ref else None,
                C.c_void_p(done.data_ptr()), int(rows.shape[0]), C.c_void_p(reward_out.data_ptr()), C.c_void_p(stream.cuda_stream))
        return bps._lib.bound_call(ps._L.gemx_reward_rows, ps, args, (rows, refs_rows, done, reward_out, stream))

    def rollout_complete(self, actions, state_out=None, refs_out=None, reward_out=None, done_out=None, episode_statistics=None):
        """K complete control steps in THREE launches (four with an observation stage) instead of K x (two or three):
        -> (state [K, N, S_out], refs [K, N, n_ref], reward [K, N], done [K, N]) -- exactly what K calls of `step(actions[k])` return,
        stacked, bit for bit.  The physics rollout writes the states and the done mask; the generators replay the shell's order on that
        mask (`rollout_shell`); the reward pass (`gemx_reward_rows`) rewards row k against the references shown before step k.  With an
        observation stage `state` is the processed trajectory; with `flatten_observation=True` it is the flat `[K, N, n_post + n_ref]`
        tensor, and `refs` is still returned.  Afterwards `reference_generator.references` holds row K-1: `step()` and further rollouts
        continue the same sequence.  (`physical_system.done` / `.reward` and the internal state buffer keep what the last `step()` wrote,
        as after `rollout()`.)  actions: [K, N, A] / [K, N], as `rollout` takes them.
        episode_statistics (an env built with `episode_statistics=True`; its counters follow every rollout either way): True -> a fifth
        result dict(ended [K, N] uint8, finished_return [K, N] float64, finished_length [K, N] int32) -- an episode's totals at the row where
        it ended, 0 elsewhere -- in the pipeline's scratch (the next rollout overwrites it), or a dict of the caller's tensors."""
        return self._bind("rollout_complete", False, actions, (state_out, refs_out, reward_out, done_out), None, episode_statistics, complete=True)()

    def rollout_complete_synthetic(self, K, seed=0, step0=None, state_out=None, refs_out=None, reward_out=None, done_out=None, episode_statistics=None):
        """`rollout_complete` on the device-side action source (`physical_system.rollout_synthetic(K, seed, step0)`): no action tensor is
        read.  Equal, bit for bit, to `rollout_complete(physical_system.synthetic_actions(K, seed, step0))`."""
        outs = (state_out, refs_out, reward_out, done_out)
        K, specs = self._check_call("rollout_complete_synthetic", K, None, outs, False, complete=True)
        ps = self.physical_system
        physics = lambda raw, done, *_: lambda: ps.rollout_synthetic(K, seed=seed, step0=step0, obs_out=raw, done_out=done)  # noqa: E731 (no bound synthetic launch)
        return self._plan(physics, K, self._allocate(specs, outs), None, None, episode_statistics, eager=True)()

    def bind_rollout_complete(self, actions, state_out, refs_out, reward_out, done_out, stream=None, episode_statistics=None):
        """-> zero-argument launch() of `rollout_complete` on fixed tensors; `launch()` returns `(state_out, refs_out, reward_out,
        done_out)`.  Everything -- handles, pointers, the stream -- is resolved here, once: a call allocates nothing and never
        synchronises, and every launch goes to ONE stream, so it can be captured with `torch.cuda.graph` (a linear graph) and replayed;
        replays advance the physics and the generators.  A ReplayReferenceGenerator is refused: its row index lives on the host.
        episode_statistics: dict(ended=, finished_return=, finished_length=) of [K, N] tensors the episode stage's pass writes (a bound
        launch allocates nothing: `True` is refused); `launch()` then returns that dict as a fifth result."""
        return self._bind("bind_rollout_complete", True, actions, (state_out, refs_out, reward_out, done_out), stream, episode_statistics, complete=True)

    # ------------------------------------------------------------------ complete episodic rollouts: the time limit inside the fused launch
    def rollout_complete_episodic(self, actions, state_out=None, refs_out=None, reward_out=None, terminated_out=None, truncated_out=None, episode_statistics=None):
        """`rollout_complete` for an env built with `max_episode_steps=M`, the time limit INSIDE the fused launch (csrc/gemx_episodic.hip):
        -> (state [K, N, S_out], refs [K, N, n_ref], reward [K, N], terminated [K, N], truncated [K, N][, stats]) -- what K calls of
        `step(actions[k])` return, stacked, bit for bit: the row of a step that ended is the final state, an ended env restarts within the
        launch, its generators restart and its flux observer resets with it, and a step that terminates and reaches the limit at once
        counts as terminated.  A reset a truncating `step()` left pending is applied first; afterwards `env.truncated` shows row K-1 and no
        reset is pending, so `step()` and further rollouts continue the same episodes.  `ended = terminated | truncated` is what
        `ga.advantages(..., ended=)` takes.  On an env without a time limit: ValueError; what the kernel does not serve:
        NotImplementedError (episodes.episodic_refusal).  episode_statistics: as `rollout_complete` takes it."""
        return self._bind("rollout_complete_episodic", False, actions, (state_out, refs_out, reward_out, terminated_out, truncated_out), None, episode_statistics,
                          complete=True, episodic=True)()

    def bind_rollout_complete_episodic(self, actions, state_out, refs_out, reward_out, terminated_out, truncated_out, stream=None, episode_statistics=None):
        """-> zero-argument launch() of `rollout_complete_episodic` on fixed tensors; `launch()` returns `(state_out, refs_out, reward_out,
        terminated_out, truncated_out[, stats])`.  Everything is resolved here, once: a call allocates nothing, never synchronises and goes
        to ONE stream, so it can be captured with `torch.cuda.graph` and replayed -- the episode counters, like the physics and the
        generators, carry from replay to replay.  A ReplayReferenceGenerator is refused: its row index lives on the host."""
        return self._bind("bind_rollout_complete_episodic", True, actions, (state_out, refs_out, reward_out, terminated_out, truncated_out), stream,
                          episode_statistics, complete=True, episodic=True)

    # ------------------------------------------------------------------ complete policy rollouts: actor, references and reward in the loop
    def _policy_generator(self, what):
        """The generator of a complete policy rollout is one the kernel steps in the lane: the all-Wiener handle of a
        BatchedWienerProcessReferenceGenerator (what `reference_generator='default'` builds) or a ProfileReferenceGenerator's."""
        gen = self.reference_generator
        if isinstance(gen, (BatchedWienerProcessReferenceGenerator, ProfileReferences)):
            return
        kind = type(gen).__name__
        if isinstance(gen, BatchedMultipleReferenceGenerator):
            kind += " (switched)" if getattr(gen, "_switched", False) else f" of {', '.join(type(h).__name__ for h in gen.sub_generators)}"
        raise NotImplementedError(f"{what} steps the reference generators inside the launch, and serves two kinds: a BatchedWienerProcessReferenceGenerator "
                                  f"(reference_generator='default') and a ProfileReferenceGenerator; this env's generator is a {kind}")

    def bind_rollout_policy_complete_episodic(self, policy, K, state_out, refs_out, reward_out, actions_out, terminated_out, truncated_out, obs0=None, noise=None,
                                              stream=None, episode_statistics=None):
        """-> zero-argument launch() of `rollout_policy_complete_episodic` on fixed tensors (every output must be given); `launch()` returns
        `(state_out, refs_out, reward_out, actions_out, terminated_out, truncated_out[, stats])`.  One stream, nothing on the host: capturable
        with `torch.cuda.graph` (make one launch outside the capture first: it loads the kernel unit and builds the one-step map);
        `policy.set_weights` between replays changes the weights the next replay reads."""
        return self._bind_policy("bind_rollout_policy_complete_episodic", True, policy, K, (state_out, refs_out, reward_out, actions_out, terminated_out, truncated_out),
                                 obs0, None, noise, stream, episode_statistics, complete=True)

    def rollout_policy_complete_episodic(self, policy, K, obs0=None, noise=None, state_out=None, refs_out=None, reward_out=None, actions_out=None,
                                         terminated_out=None, truncated_out=None, episode_statistics=None):
        """K calls of `step()` with the actor `policy` (an `MLPPolicy`) in between, fused: the env's own reference generators are stepped
        inside the launch that steps the env and computes the action (csrc/gemx_policy_complete.hip), the reward pass follows.
        -> (state [K, N, S_out], refs [K, N, n_ref], reward [K, N], actions [K, N, A] or [K, N] uint8, terminated [K, N], truncated [K, N][, stats])
        -- what goes into `ga.advantages`.  Step k's actor input is `[obs_prev[columns], refs_prev]`, so `policy.n_in == len(columns) +
        n_ref`: obs_prev as `rollout_policy_episodic` has it (`obs0`, the previous row, the reset observation behind a step that ended);
        refs_prev is the reference row shown in front of step k -- the env's currently shown references at k = 0, `refs[k - 1]` afterwards,
        the second half of the observation `step()` hands out.  Row k of `refs` is the shell's: the generators of an env that ended in step
        k (terminated or truncated) restart, then every generator advances.  `reward[k]` rewards row k against the references shown before
        step k.  Bit for bit `rollout_complete_episodic(actions)` of a twin env; afterwards the env stands where that leaves it (references
        shown: row K-1; generator state advanced; `env.truncated`: row K-1; no reset pending), so `step()` and every other rollout
        continue the same episodes and the same random streams.  `noise`, `obs0`, episode_statistics: as `rollout_policy_episodic` takes
        them.  Served generators: BatchedWienerProcessReferenceGenerator (`reference_generator='default'`) and ProfileReferenceGenerator;
        any other: NotImplementedError.  An env without a time limit: ValueError."""
        return self._bind_policy("rollout_policy_complete_episodic", False, policy, K, (state_out, refs_out, reward_out, actions_out, terminated_out, truncated_out),
                                 obs0, None, noise, None, episode_statistics, complete=True)()

    # ------------------------------------------------------------------ lookahead rollouts: one-step finite-control-set predictive control in the loop
    def n_lookahead_actions(self, what="rollout_lookahead_complete_episodic"):
        """The size of the finite action set the lookahead enumerates (a multi-converter: its flat action index); a continuous
        converter: NotImplementedError.  Needs no device."""
        space = self.physical_system.action_space
        if not (hasattr(space, "n") or hasattr(space, "nvec")):
            raise NotImplementedError(f"{what} tries every switching action of a finite converter one step ahead; this env's converter is continuous "
                                      f"(action space {space}): it has no finite action set")
        return int(getattr(space, "n", 0) or np.prod(space.nvec))

    def _bind_lookahead(self, what, bound, K, outs, noise, scores, stream, episode_statistics):
        """-> launch() of the lookahead entry point `what`: the refusals of the complete policy rollout and the converter's (no device
        call), the tensors, then what `_bind_policy` does -- allocate what an eager call did not give, plan.  outs: (state_out, refs_out,
        reward_out, actions_out, terminated_out, truncated_out); scores: None | True (eager: allocated) | a [K, N, n_actions] tensor."""
        import ctypes as C

        from .episodes import episodic_refusal

        pipe, ps = self.pipeline, self.physical_system
        pipe.need_episodic()
        torch = bps._torch()
        if isinstance(K, bool) or not isinstance(K, int) or K < 1:
            raise ValueError(f"{what}: K must be an integer >= 1, not {K!r}")
        if pipe.stage is not None or pipe.flux is not None:
            raise NotImplementedError(f"{what} is not available with a FluxObserver or any observation-side processor: the controller scores the raw state row")
        if getattr(ps, "_obs_layout", "aos") != "aos":
            raise NotImplementedError(f"{what} is not available with obs_layout='soa': the tensors are [K, N, S_out]")
        self._policy_generator(what)
        n_actions, N = self.n_lookahead_actions(what), ps.n_envs
        for name, t in (("noise", noise), ("scores_out", scores)):
            if torch.is_tensor(t) and t.dtype in (torch.float16, torch.bfloat16):
                raise NotImplementedError(episodic_refusal(ps, f"a half-precision {name} tensor (fp32 tensors)"))
        if noise is not None:
            self._check_tensor(what, noise, "noise", torch.float32, (K, N, n_actions))
        if scores is True and bound:
            raise ValueError(f"{what}: scores_out must be a tensor (a bound launch allocates nothing)")
        if scores is not None and scores is not True and scores is not False:
            self._check_tensor(what, scores, "scores_out", torch.float32, (K, N, n_actions))
        _, specs = self._check_call(what, K, None, outs, bound, episode_statistics, complete=True, episodic=True, actions_out=True)
        state_out, refs_out, reward_out, actions_out, terminated_out, truncated_out = self._allocate(specs, outs)
        if scores is True:
            scores = torch.empty((K, N, n_actions), dtype=torch.float32, device=ps._tdev)
        elif scores is False:
            scores = None
        n_ref = len(self.reference_names)

        def physics(raw, terminated, truncated, ended, st):
            """the pending masked reset, then `gemx_rollout_lookahead_complete` on fixed tensors (the counterpart of `_policy_physics`)"""
            lib = bps._lib
            call = lib.GemxPolicyCall()
            call.struct_size, call.K, call.n_cols, call.n_ref, call.max_steps = C.sizeof(call), K, 0, n_ref, pipe.episode.max_steps
            call.refs_dev, call.length_dev, call.obs_out_dev = self._refs.data_ptr(), pipe.episode.length.data_ptr(), raw.data_ptr()
            call.terminated_out_dev, call.truncated_out_dev, call.ended_out_dev = terminated.data_ptr(), truncated.data_ptr(), ended.data_ptr()
            gen = self.reference_generator
            profile = isinstance(gen, ProfileReferences)
            args = (C.byref(call), C.c_void_p(refs_out.data_ptr()), C.c_void_p(actions_out.data_ptr()), C.c_void_p(scores.data_ptr()) if scores is not None else None,
                    C.c_void_p(noise.data_ptr()) if noise is not None else None, None if profile else gen._handle, gen._handle if profile else None,
                    C.c_void_p(st.cuda_stream))
            keep = (call, noise, scores, actions_out, refs_out, raw, terminated, truncated, ended, st, pipe.episode.length, self._refs, gen)
            return lib.sequence(pipe.bind_before_step(st), lib.counting_call(ps._L.gemx_rollout_lookahead_complete, ps, K, args, keep))

        launch = self._plan(physics, K, (state_out, refs_out, reward_out, terminated_out), truncated_out, stream, episode_statistics, eager=not bound,
                            extra=(actions_out,), generators=False)
        if scores is None:
            return launch

        def launch_with_scores():
            result = launch()
            return result[:6] + (scores,) + result[6:]

        return launch_with_scores

    def bind_rollout_lookahead_complete_episodic(self, K, state_out, refs_out, reward_out, actions_out, terminated_out, truncated_out, noise=None, scores_out=None,
                                                 stream=None, episode_statistics=None):
        """-> zero-argument launch() of `rollout_lookahead_complete_episodic` on fixed tensors (every output must be given; `scores_out
        [K, N, n_actions]` float32 is optional); `launch()` returns `(state_out, refs_out, reward_out, actions_out, terminated_out,
        truncated_out[, scores_out][, stats])`.  One stream, nothing on the host: capturable with `torch.cuda.graph` (make one launch
        outside the capture first: it loads the kernel unit and builds the one-step map)."""
        return self._bind_lookahead("bind_rollout_lookahead_complete_episodic", True, K, (state_out, refs_out, reward_out, actions_out, terminated_out, truncated_out),
                                    noise, scores_out, stream, episode_statistics)

    def rollout_lookahead_complete_episodic(self, K, noise=None, return_scores=False, state_out=None, refs_out=None, reward_out=None, actions_out=None,
                                            terminated_out=None, truncated_out=None, scores_out=None, episode_statistics=None):
        """K calls of `step()` under one-step finite-control-set model predictive control, fused (csrc/gemx_lookahead.hip): in every
        control step the launch tries each of the finite converter's actions once from the state the step starts at, scores the outcome
        with the env's own reward against the references shown before the step, and takes the lowest index among the maxima of
        `score + noise[k]` -- the policy rollouts' rule; a `-inf` noise entry masks an action, Gumbel noise samples from softmax(score).
        -> (state [K, N, S_out], refs [K, N, n_ref], reward [K, N], actions [K, N] uint8, terminated [K, N], truncated [K, N][, scores
        [K, N, n_actions]][, stats]); `scores` (return_scores=True or `scores_out`) are the scores before the noise, and
        `reward[k, n] == scores[k, n, actions[k, n]]` bit for bit.  A multi-converter's action is its flat index.  Everything else is
        `rollout_policy_complete_episodic`'s: bit for bit `rollout_complete_episodic(actions)` of a twin env, the env afterwards stands
        where that leaves it, the same generators are served and the same configurations refused; a continuous converter has no finite
        action set: NotImplementedError.  An env without a time limit: ValueError."""
        scores = scores_out if scores_out is not None else bool(return_scores)
        return self._bind_lookahead("rollout_lookahead_complete_episodic", False, K, (state_out, refs_out, reward_out, actions_out, terminated_out, truncated_out),
                                    noise, scores, None, episode_statistics)()

    def evaluate_policy_complete_rollout(self, policy, rollout_outputs, head="none", mode="seen", obs0=None, shown0=None, **kw):
        """`policy.evaluate_rollout` on what `rollout_policy_complete_episodic` returned, `(state, refs, reward, actions, terminated,
        truncated[, stats])`, in the complete form: `refs` from the tuple, `n_ref` from the env, `ended`, the reset observation and the
        stored actions as `evaluate_policy_rollout` fills them.  mode="seen" needs `obs0 [N, S]` and `shown0 [N, n_ref]`, the state row
        and the reference row of the observation in front of the rollout (clones: the rollout moves the env's own buffers on)."""
        what = "evaluate_policy_complete_rollout"
        kw = self._evaluate_policy(what, policy, rollout_outputs, 3, head, mode, obs0, kw)
        if mode == "seen":
            kw["shown0"] = shown0
        elif shown0 is not None:
            raise ValueError(f"{what}: shown0 belongs to mode='seen'")
        return policy.evaluate_rollout(rollout_outputs[0], refs=rollout_outputs[1], n_ref=len(self.reference_names), **kw)

    def close(self):
        self.reference_generator.close()
        super().close()  # (closes the observation pipeline too)


def make(env_id, n_envs=1, device=0, supply=None, converter=None, motor=None, load=None, ode_solver=None, tau=None,
         constraints=None, dtype="float32", auto_reset=None, obs_layout="aos", physical_system_wrappers=(), reference_generator=None,
         reward_function=None, state_filter=None, observed_states=None, flatten_observation=False, max_episode_steps=None, episode_statistics=False,
         **kwargs):
    """Build a batched env.  Component arguments follow the reference's env-arg convention (instance | dict | None).
    physical_system_wrappers: reference-style tuple (innermost first) of DeadTimeProcessor / DqToAbcActionProcessor holders
    (or the reference's own instances), which are folded into the kernel's action stage, and of CurrentSumProcessor / CosSinProcessor
    holders, which become the device-side observation stage, and of FluxObserver / FluxOrientedDqToAbcActionProcessor holders (induction
    machines: the flux-observer stage), and of at most one StateNoiseProcessor holder, listed before the observation-side ones (the
    state-noise stage: constraints, auto-reset and reward then act on the noisy state); 'default': `default_physical_system_wrappers(env_id)`.
    observed_states: None | list of state names of the wrapped system -- the reference's `state_filter`, applied last.
    flatten_observation: the complete env hands out ONE tensor [N, n_post + n_ref], the processed state followed by the references.
    reference_generator: None | 'default' | BatchedWienerProcessReferenceGenerator | BatchedMultipleReferenceGenerator | a holder such as
    StepReferenceGenerator(...) or SwitchedReferenceGenerator([...]), or a list of holders (one per referenced state; the reference's own
    generator instances are read the same way, its SwitchedReferenceGenerator excepted) | ProfileReferenceGenerator(profiles, ...) (given
    trajectories per env, on the device) | ReplayReferenceGenerator;
    reward_function: None | 'default' | dict of `set_reward` keywords.  Naming either one selects the complete env
    (CompleteBatchedElectricMotorEnv), the other then takes the env id's default (`default_env_modules`); `seed` keys the default
    generators, and the generator built from holders, like every other device random stream.  Both None: the physics-only env.
    max_episode_steps: None | int >= 1 -- gymnasium's TimeLimit on the device: `step()` returns `truncated` [N], truncated envs restart in
    front of the next step; episode_statistics: `env.episode_statistics()` hands out per-env episode length and return counters
    (episodes.py).  Both off: nothing is built and nothing more is launched.
    env_parameters (through **kwargs to the system): None | EnvParameters(motor=, load=, supply=) -- per-env motor, load and supply parameters
    (env_parameters.py): every env steps with its own machine, everything behind the physics runs unchanged."""
    from .episodes import check_max_episode_steps
    from .physical_system_wrappers import fold_wrappers

    max_episode_steps = check_max_episode_steps(max_episode_steps)
    episodes = dict(max_steps=max_episode_steps, statistics=bool(episode_statistics)) if max_episode_steps is not None or episode_statistics else None

    if state_filter is not None:
        raise NotImplementedError("state_filter is spelled observed_states=[names] on the accelerated path (a device-side column selection, "
                                  "applied after the physical-system wrappers)")
    if isinstance(physical_system_wrappers, str):
        if physical_system_wrappers != "default":
            raise ValueError("physical_system_wrappers: a tuple of wrapper holders or 'default'")
        physical_system_wrappers = default_physical_system_wrappers(env_id)
    chain = []
    flux_action = state_noise = None
    if physical_system_wrappers:
        folded = fold_wrappers(physical_system_wrappers, observation_chain=chain)
        flux_action = folded.pop("flux_action", None)  # (served by the flux-observer stage, not by the system's action stage)
        state_noise = folded.pop("state_noise", None)  # (served by the state-noise stage behind the physics)
        kwargs = dict(kwargs, **folded)
    if kwargs.get("env_parameters") is not None and (flux_action is not None or any(spec[0] == "flux" for spec in chain)):
        from .env_parameters import REFUSAL as EP_REFUSAL

        raise NotImplementedError(EP_REFUSAL + "a FluxObserver or a FluxOrientedDqToAbcActionProcessor (the observer holds one machine's parameters)")
    if state_noise is not None and obs_layout != "aos":
        from .state_noise import REFUSAL

        raise NotImplementedError(REFUSAL + f"obs_layout={obs_layout!r} was asked for")
    observation = None
    if chain or observed_states is not None or flatten_observation:
        if obs_layout != "aos":
            raise ValueError("the observation stage (observation-side wrappers, observed_states, flatten_observation) reads state rows: "
                             "it needs obs_layout='aos', not 'soa'")
        observation = dict(chain=tuple(chain), observed_states=observed_states, flatten=bool(flatten_observation))
    d = default_components(env_id)
    tau = d["tau"] if tau is None else tau
    conv_cls = d["converter"]
    load = _initialize(load, d["load"][0], d["load"][1])
    if ode_solver is None:
        ode_solver = default_ode_solver(env_id, tau=tau, load=load)
    system = d["system"](
        supply=_initialize(supply, comp.IdealVoltageSupply, d["supply"]),
        converter=_initialize(converter, conv_cls, d["converter_args"]),
        motor=_initialize(motor, d["motor"], dict()),
        load=load,
        ode_solver=_initialize(ode_solver, comp.RK4Solver, dict()),
        tau=tau,
        n_envs=n_envs,
        device=device,
        dtype=dtype,
        # (a StateNoiseProcessor: constraints, auto-reset and reward move behind the noise -- the physics has none of them)
        constraints=() if state_noise is not None else (d["constraints"] if constraints is None else constraints),
        auto_reset=False if state_noise is not None else auto_reset,
        obs_layout=obs_layout,
        **kwargs,
    )
    if state_noise is not None:
        limit_mask, squared_mask = system._constraint_masks(tuple(d["constraints"] if constraints is None else constraints))
        state_noise = dict(state_noise, limit_mask=limit_mask, squared_mask=squared_mask,
                           auto_reset=(n_envs > 1 and bool(limit_mask or squared_mask)) if auto_reset is None else bool(auto_reset))
    if reference_generator is None and reward_function is None:
        return BatchedElectricMotorEnv(system, observation=observation, _defer_create=bool(kwargs.get("_defer_create", False)), flux_action=flux_action,
                                       state_noise=state_noise, episodes=episodes)
    from .reference_generators import (BatchedMultipleReferenceGenerator, BatchedWienerProcessReferenceGenerator, SWITCHED_REFUSAL, _DeviceGenerators, _SubGenerator,
                                       as_profile_holder)

    modules = default_env_modules(env_id)
    if reference_generator is None or (isinstance(reference_generator, str) and reference_generator == "default"):
        reference_generator = BatchedWienerProcessReferenceGenerator(reference_states=modules["reference_states"], seed=kwargs.get("seed", 0),
                                                                     **modules["generator"])
    elif isinstance(reference_generator, (str, type)):
        raise ValueError("reference_generator: 'default', a BatchedWienerProcessReferenceGenerator, a BatchedMultipleReferenceGenerator, generator "
                         "holders (e.g. StepReferenceGenerator(...), or a list of them), a ProfileReferenceGenerator or a ReplayReferenceGenerator instance")
    elif type(reference_generator).__name__ == "SwitchedReferenceGenerator" and not isinstance(reference_generator, _SubGenerator):
        raise NotImplementedError(SWITCHED_REFUSAL)  # (the reference's own instance; the holder of the same name goes on below)
    elif as_profile_holder(reference_generator) is not None:  # given trajectories on the device (a list that mixes them with other kinds is refused)
        reference_generator = ProfileReferences(reference_generator, seed=kwargs.get("seed", 0))
    elif not isinstance(reference_generator, (_DeviceGenerators, ReplayReferenceGenerator)):
        # holders, a list of them, or the reference's own instances: one handle, columns in state order
        reference_generator = BatchedMultipleReferenceGenerator(reference_generator, seed=kwargs.get("seed", 0))
    if not (reward_function is None or isinstance(reward_function, dict) or (isinstance(reward_function, str) and reward_function == "default")):
        raise ValueError("reward_function: 'default' or a dict of set_reward keywords")
    return CompleteBatchedElectricMotorEnv(system, reference_generator, reward_function, default_modules=modules,
                                           _defer_create=bool(kwargs.get("_defer_create", False)), observation=observation, flux_action=flux_action,
                                           state_noise=state_noise, episodes=episodes)
