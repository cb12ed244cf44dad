"""FluxObserver and flux-oriented dq actions, host side: the float64 restatement against the reference's recorded runs, the metadata,
the chain order, folding and every refusal.  No GPU."""
import sys

import numpy as np
import pytest

from flux_fixtures import CASES, DQ_CASES, DQ_RUNS, PARAM_CASES, RUNS, holders, load_any, load_runs, make_kwargs
from parity_contract import FLUX_FLOOR, TOL_FP32

TOL = 1e-12  # what the oracle is held to


def _env(ga, d, **kw):
    return ga.make(d["meta"]["env_id"], n_envs=4, _defer_create=True, physical_system_wrappers=holders(ga, d["meta"]["chain"]), **make_kwargs(d), **kw)


@pytest.mark.parametrize("case", CASES + RUNS)
def test_host_evaluate_reproduces_the_reference(case):
    import gym_electric_motor_amd as ga

    d = load_any(case)
    env = _env(ga, d)
    flux, nb = env.flux, env.flux.n_in
    assert flux.auto_reset and flux.angle_advance == 0.5 + d["meta"]["dead_time"]
    flux.set_reset_observation(d["reset_state"])
    assert np.array_equal(d["reset_state"][nb:], [0.0, 0.0])
    got = env.observation_stage.evaluate(d["state"][:, :nb], done=d["terminated"])
    assert got.shape == d["state"].shape and np.array_equal(got[:, :nb], d["state"][:, :nb])
    err = np.abs(got[:, nb:] - d["state"][:, nb:])
    err[:, 1] = np.minimum(err[:, 1], 2.0 - err[:, 1])  # (an angle in units of pi)
    print(case, "max |psi_abs|, |psi_angle| error", err.max(axis=0))
    assert err.max() <= TOL


@pytest.mark.parametrize("case", DQ_CASES + DQ_RUNS)
def test_host_actions_reproduce_the_reference(case):
    import gym_electric_motor_amd as ga

    d = load_any(case)
    flux = _env(ga, d).flux
    nb = flux.n_in
    flux.set_reset_observation(d["reset_state"])
    flux.host_reset(1)
    worst = 0.0
    for k in range(len(d["actions"])):
        abc = flux.host_actions(d["actions"][k])[0]
        worst = max(worst, float(np.abs(abc - d["abc_actions"][k]).max()))
        flux.evaluate(d["state"][k:k + 1, :nb], done=d["terminated"][k:k + 1])
    print(case, "max abc action error", worst)
    assert worst <= TOL


@pytest.mark.parametrize("case", CASES + RUNS)
def test_metadata_matches_the_reference(case):
    import gym_electric_motor_amd as ga

    d = load_any(case)
    env = _env(ga, d)
    st = env.observation_stage
    assert st.state_names == d["state_names"] and env.state_names == d["state_names"]
    for got, key in ((st.limits, "limits"), (st.nominal_state, "nominal_state"), (st.state_space.low, "state_space_low"), (st.state_space.high, "state_space_high")):
        assert np.allclose(got, d[key], rtol=1e-12, atol=0.0), key
    width = d["actions"].shape[1]
    assert env.action_space.shape == (width,) and np.all(env.action_space.low == -1) and np.all(env.action_space.high == 1)
    assert list(env.physical_system.state_names) == d["state_names"][:-2]  # (the system itself stays raw)


def _host_misses(flux, d):
    """How far the host restatement of `flux` is from one recorded run: (psi_abs, psi_angle -- circular, weighted as the contract weighs
    it --, abc actions), each in the normalised units the tolerances are stated in."""
    nb = flux.n_in
    flux.set_reset_observation(d["reset_state"])
    flux.host_reset(1)
    K = len(d["actions"])
    got, abc = np.empty((K, 2)), 0.0
    for k in range(K):
        if flux.action_mode:
            abc = max(abc, float(np.abs(flux.host_actions(d["actions"][k])[0] - d["abc_actions"][k]).max()))
        got[k] = flux.evaluate(d["state"][k:k + 1, :nb], done=d["terminated"][k:k + 1])[0, nb:]
    ref = d["state"][:, nb:]
    circ = np.abs(got[:, 1] - ref[:, 1])
    circ = np.minimum(circ, 2.0 - circ) * np.minimum(1.0, ref[:, 0] / (FLUX_FLOOR * ref[:, 0].max()))
    return float(np.abs(got[:, 0] - ref[:, 0]).max()), float(circ.max()), abc


def _mutants(flux, d):
    """name -> (attribute, deliberately wrong value | None where the wrong value is the right one) for the stage of one fixture"""
    mp = d["meta"]["overrides"].get("motor", {}).get("motor_parameter", {})
    names = d["state_names"]
    nominal_psi = flux.l_m * float(d["nominal_state"][names.index("i_sd")])
    plain = [names.index(c) for c in ("i_sa", "i_sb", "i_sc")]

    def other(value, wrong):
        return None if value == wrong else wrong

    return {
        "l_r from l_sigs": ("l_r", other(flux.l_r, flux.l_m + mp["l_sigs"]) if mp else None),
        "p = 2": ("p", other(flux.p, 2.0)),
        "tau = 1e-4": ("tau", other(flux.tau, 1e-4)),
        "dead time forgotten": ("angle_advance", other(flux.angle_advance, 0.5)),
        "currents unpermuted": ("current_indices", other(flux.current_indices, plain)),
        "psi_limit from the nominal i_sd": ("psi_limit", other(flux.psi_limit, nominal_psi)),
    }


def test_every_mutant_is_seen_by_a_new_fixture():
    """The new recordings can see a folding mistake: one deliberately wrong attribute on the FluxObserverStage instance (the product code
    stays as it is) puts the host restatement more than 10 * TOL_FP32 away from at least one run, in psi_abs, psi_angle or the abc
    actions -- ten times what the device is allowed, so the GPU comparison against the same recordings sees it as well.  Unmutated, every
    run is reproduced to 1e-12 (test_host_evaluate_reproduces_the_reference, test_host_actions_reproduce_the_reference)."""
    import gym_electric_motor_amd as ga

    need = 10 * TOL_FP32
    worst, seen_by = {}, {}
    for case in PARAM_CASES:
        runs = load_runs(case)
        for name in _mutants(_env(ga, runs[0]).flux, runs[0]):
            for r, d in enumerate(runs):
                flux = _env(ga, d).flux
                attr, wrong = _mutants(flux, d)[name]
                if wrong is None:  # (this fixture's machine has the wrong value as its right one)
                    continue
                setattr(flux, attr, wrong)
                miss = max(_host_misses(flux, d))
                worst[name] = max(worst.get(name, 0.0), miss)
                if miss > need:
                    seen_by.setdefault(name, []).append(f"{case}-run{r}")
    for name, miss in worst.items():
        print(f"mutant '{name}': worst miss {miss:.2e}, seen by {seen_by.get(name, [])}")
    expected = {"l_r from l_sigs", "p = 2", "tau = 1e-4", "dead time forgotten", "currents unpermuted", "psi_limit from the nominal i_sd"}
    if "psi_limit from the nominal i_sd" not in worst:
        print("NOTE: the nominal and the limit of i_sd are equal in every new fixture: the psi_limit mutant cannot be told apart and is skipped")
        expected.discard("psi_limit from the nominal i_sd")
    assert set(worst) >= expected, sorted(expected - set(worst))
    assert all(name in seen_by for name in expected), {n: worst[n] for n in expected if n not in seen_by}
    # each mistake has a fixture made for it: the pole pairs and the control step in every `param` case, the leakage swap in the two
    # with tau = 2e-4 (at 5e-5 the 200 steps are 10 ms, too short for the rotor time constant to show beyond 1e-3), the dead time in the
    # dead-time case, the current order in the permuted one
    for name in ("p = 2", "tau = 1e-4"):
        assert all(any(s.startswith(c) for s in seen_by[name]) for c in PARAM_CASES[:3]), name
    assert all(any(s.startswith(c) for s in seen_by["l_r from l_sigs"]) for c in PARAM_CASES[1:3])
    assert any(s.startswith("flux_param_scim_dq_dead2") for s in seen_by["dead time forgotten"])
    assert any(s.startswith("flux_scim_abc_perm") for s in seen_by["currents unpermuted"])


def test_chain_order():
    import gym_electric_motor_amd as ga

    mk = lambda w, **kw: ga.make("Cont-CC-SCIM-v0", n_envs=4, _defer_create=True, physical_system_wrappers=w, **kw)  # noqa: E731
    base = list(mk(()).state_names)
    env = mk((ga.CurrentSumProcessor(("i_sa", "i_sb", "i_sc")), ga.FluxObserver(), ga.CosSinProcessor("psi_angle")))
    assert env.state_names == base + ["i_sum", "psi_abs", "psi_angle", "cos(psi_angle)", "sin(psi_angle)"]
    st = env.observation_stage
    assert st.n_in == len(base) + 2 and st.program[-2:] == [("cospi", len(base) + 1, 0), ("sinpi", len(base) + 1, 0)]
    env = mk((ga.FluxObserver(), ga.CurrentSumProcessor(("i_sa", "i_sb")), ga.CosSinProcessor("psi_angle", remove_angle=True)), observed_states=["psi_abs", "cos(psi_angle)"], flatten_observation=True)
    assert env.state_names == ["psi_abs", "cos(psi_angle)"] and not env._flux_only
    # the program over the extended row, on the host
    rows = np.random.default_rng(0).uniform(-0.5, 0.5, (5, 4, len(base)))
    ext = env.flux.evaluate(rows)
    env.flux.host_reset()
    got = env.observation_stage.evaluate(rows)
    assert np.allclose(got[..., 0], ext[..., -2]) and np.allclose(got[..., 1], np.cos(np.pi * ext[..., -1]))


def test_folding_from_holders_and_reference_style_classes():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd.physical_system_wrappers import fold_wrappers

    class PhysicalSystemWrapper:
        pass

    class FluxObserver(PhysicalSystemWrapper):
        _current_names = ("i_sa", "i_sb", "i_sc")

    class DqToAbcActionProcessor(PhysicalSystemWrapper):
        pass

    class _ClassicDqToAbcActionProcessor(DqToAbcActionProcessor):
        _angle_name = "psi_angle"

    class _DFIMDqToAbcActionProcessor(DqToAbcActionProcessor):
        _angle_name = "epsilon"

    class DeadTimeProcessor(PhysicalSystemWrapper):
        dead_time, _reset_actions = 2, None

    for dq, kind in ((_ClassicDqToAbcActionProcessor(), "SCIM"), (_DFIMDqToAbcActionProcessor(), "DFIM"), (ga.FluxOrientedDqToAbcActionProcessor(kind := "SCIM"), "SCIM")):
        chain = []
        fo = FluxObserver()
        out = fold_wrappers((DeadTimeProcessor(), fo, dq), observation_chain=chain)
        assert out == dict(action_delay=2, action_frame=None, flux_action=kind) and chain == [("flux", fo)]
    # without a FluxObserver they stay refused, with the message they always had
    for dq in (_ClassicDqToAbcActionProcessor(), _DFIMDqToAbcActionProcessor()):
        with pytest.raises(NotImplementedError, match="need a flux observer"):
            fold_wrappers((dq,), observation_chain=[])
    with pytest.raises(NotImplementedError, match="flux observer"):
        fold_wrappers((ga.FluxOrientedDqToAbcActionProcessor("DFIM"),), observation_chain=[])
    with pytest.raises(NotImplementedError, match="flux observer"):
        ga.DqToAbcActionProcessor.make("SCIM")
    with pytest.raises(ValueError):
        ga.FluxOrientedDqToAbcActionProcessor("PMSM")
    # order: the observer first, a dead time inside the dq processor
    with pytest.raises((ValueError, NotImplementedError)):
        fold_wrappers((ga.FluxOrientedDqToAbcActionProcessor("SCIM"), ga.FluxObserver()), observation_chain=[])
    with pytest.raises(ValueError, match="DeadTimeProcessor"):
        fold_wrappers((ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor("SCIM"), ga.DeadTimeProcessor(1)), observation_chain=[])
    # the stand-ins build an env
    env = ga.make("Cont-CC-DFIM-v0", n_envs=4, _defer_create=True, physical_system_wrappers=(DeadTimeProcessor(), FluxObserver(), _DFIMDqToAbcActionProcessor()))
    assert env.flux_action == "DFIM" and env.action_space.shape == (4,) and env.flux.angle_advance == 2.5 and env.physical_system.dead_time == 2


def test_refusals():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd.flux_observer import FluxObserverStage

    fo, dq = ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor("SCIM")
    mk = lambda env_id="Cont-CC-SCIM-v0", **kw: ga.make(env_id, n_envs=4, _defer_create=True, **kw)  # noqa: E731
    with pytest.raises(NotImplementedError, match="FluxObserver needs an induction machine"):
        mk("Cont-CC-PMSM-v0", physical_system_wrappers=(fo,))
    assert "DEVIATION" in sys.modules[FluxObserverStage.__module__].__doc__  # (the reference raises an AssertionError there)
    with pytest.raises(ValueError, match="soa"):
        mk(physical_system_wrappers=(fo,), obs_layout="soa")
    with pytest.raises(ValueError, match="derived"):  # currents that are derived columns
        mk(physical_system_wrappers=(ga.CurrentSumProcessor(("i_sa", "i_sb")), ga.FluxObserver(("i_sum", "i_sb", "i_sc"))))
    with pytest.raises(ValueError, match="one FluxObserver"):
        mk(physical_system_wrappers=(ga.FluxObserver(), ga.FluxObserver(("psi_abs", "i_sb", "i_sc"))))
    with pytest.raises(ValueError, match="psi_abs"):  # reward weights on the new columns
        mk(physical_system_wrappers=(fo,), reference_generator="default", reward_function=dict(reward_weights=dict(psi_abs=1.0)))
    with pytest.raises((ValueError, KeyError, AssertionError)):  # constraints on the new columns
        mk(physical_system_wrappers=(fo,), constraints=("psi_abs",))
    with pytest.raises(ValueError, match="DFIM|doubly"):
        mk(physical_system_wrappers=(fo, ga.FluxOrientedDqToAbcActionProcessor("DFIM")))
    # random initial states with the flux-oriented action processor
    motor = ga.SquirrelCageInductionMotor(motor_initializer=dict(random_init="uniform"))
    with pytest.raises(NotImplementedError, match="random initial"):
        mk(physical_system_wrappers=(fo, dq), motor=motor)
    assert mk(physical_system_wrappers=(fo,), motor=motor).flux is not None  # (the observer alone takes them)
    # fused rollouts with the flux-oriented action processor
    env = mk(physical_system_wrappers=(fo, dq))
    for call in (lambda: env.rollout(np.zeros((3, 4, 2))), lambda: env.rollout_synthetic(3), lambda: env.bind_rollout(None, None, None)):
        with pytest.raises(NotImplementedError, match="previous step's observation"):
            call()
    env = mk(physical_system_wrappers=(fo, dq), reference_generator="default")
    for call in (lambda: env.rollout_complete(np.zeros((3, 4, 2))), lambda: env.rollout_complete_synthetic(3)):
        with pytest.raises(NotImplementedError, match="previous step's observation"):
            call()
    # the 26-column row of the DFIM is handed out as it is, but the column program reads at most 24 columns
    assert mk("Cont-CC-DFIM-v0", physical_system_wrappers=(fo,))._flux_only
    with pytest.raises(NotImplementedError, match="at most 24 columns"):
        mk("Cont-CC-DFIM-v0", physical_system_wrappers=(fo, ga.CosSinProcessor("psi_angle")))


def test_unchanged_path():
    import gym_electric_motor_amd as ga

    for kw in (dict(), dict(physical_system_wrappers=(ga.DeadTimeProcessor(1),)), dict(physical_system_wrappers=(ga.CosSinProcessor(),), reference_generator="default")):
        env = ga.make("Cont-CC-SCIM-v0", n_envs=4, _defer_create=True, **kw)
        assert env.flux is None and env.flux_action is None and not env._flux_only
        assert env.action_space.shape == (3,) and "psi_abs" not in env.state_names
    from gym_electric_motor_amd import _lib

    assert {"gemx_fluxobs_create", "gemx_fluxobs_step", "gemx_fluxobs_rows", "gemx_fluxobs_actions", "gemx_fluxobs_get_state"} <= set(_lib.EXPORTS)
