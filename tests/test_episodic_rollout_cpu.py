"""Episodic rollouts (the episode time limit inside a fused K-step launch: csrc/gemx_episodic.hip, gemx_rollout_episodic) without a GPU
(`_defer_create=True`): header, binding and build list agree; every refusal is raised before any device call, with its own message; an env
without a time limit raises ValueError; the tensors are validated in `_check_complete`'s order and wording; the old entry points still
refuse a time limit."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mk(ga, env_id="Cont-CC-PMSM-v0", n_envs=8, **kw):
    return ga.make(env_id, n_envs=n_envs, _defer_create=True, **kw)


def test_header_binding_and_abi():
    from gym_electric_motor_amd import _lib

    header = open(os.path.join(REPO, "include", "gemx.h")).read()
    assert re.search(r"^#define GEMX_ABI_VERSION 9\b", header, re.M) and _lib.ABI_VERSION == 9  # a new entry point only
    m = re.search(r"\bint gemx_rollout_episodic\(([^;]*)\);", header)
    assert m, "include/gemx.h does not declare gemx_rollout_episodic"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "actions_dev", "K", "length_dev", "max_steps", "obs_out_dev", "terminated_out_dev",
                                                           "truncated_out_dev", "ended_out_dev", "stream"]
    assert "const int32_t *length_dev" in m.group(1)  # read only: the episode stage owns the counters
    assert "gemx_rollout_episodic" in _lib.EXPORTS and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    src = open(os.path.join(REPO, "gym_electric_motor_amd", "_lib.py")).read()
    bound = re.search(r"L\.gemx_rollout_episodic\.argtypes = \[([^\]]*)\]", src)
    assert bound and [a.strip() for a in bound.group(1).split(",")] == ["vp", "vp", "i32", "vp", "i32", "vp", "vp", "vp", "vp", "vp"]


def test_build_lists_one_episodic_unit_per_per_env_unit():
    from gym_electric_motor_amd import build

    ep, tl = build.ep_libs(), build.tl_libs()
    assert len(tl) == len(ep) == len(build.UNITS) == 19 and len(set(tl)) == 19
    for (s, c), e, t in zip(build.UNITS, ep, tl):
        assert os.path.basename(e) == f"libgemx_ep{s}_{c}.so" and os.path.basename(t) == f"libgemx_tl{s}_{c}.so"
        assert os.path.dirname(t) == os.path.dirname(build.LIB)  # (load_tl_unit looks beside libgemx.so)
    deps = build._DEPS["episodic"]
    assert set(deps) == {"gemx_common.hpp", "gemx_reward.hpp", "gemx_kernels.hpp", "gemx_launch_plan.hpp", "gemx_unit_host.hpp", "gemx_envparams.hpp", "gemx_envparams_dev.hpp", "gemx_episodic.hip"}
    assert "gemx_envparams_dev.hpp" in build._DEPS["envparams"]  # the shared helpers: an edit recompiles both kinds of unit
    assert "gemx_envparams.hpp" in build._DEPS["capi"]  # (the launch kind and the unit's entry point type)
    names = {os.path.basename(p) for p in build.SOURCES}
    assert {"gemx_episodic.hip", "gemx_envparams_dev.hpp"} <= names and all(os.path.exists(p) for p in build.SOURCES)
    for kind, files in build._DEPS.items():
        assert set(files) <= names, kind  # (everything a unit is compiled from is in the stamp and the snapshot)
    src = open(os.path.join(REPO, "gym_electric_motor_amd", "csrc", "gemx_episodic.hip")).read()
    for fn in ("dq_action_stage", "full_step<ST", "constraint_done", "lin_usable", "ep_control_step", "ep_load", "ep_apply"):
        assert fn in src, fn
    capi = open(os.path.join(REPO, "gym_electric_motor_amd", "csrc", "gemx_capi.hip")).read()
    assert "libgemx_%s%d_%d.so" in capi and 'load_side_unit(g_tl_units, "tl"' in capi and "EP_LAUNCH_EPISODIC" in capi


def _calls(env, complete, K=3):
    """The four ways into an episodic rollout of `env`, as thunks (numpy actions: nothing here may reach a device)."""
    n = env.n_envs
    space = env.physical_system.action_space
    a = np.zeros((K, n), dtype=np.uint8) if hasattr(space, "n") or hasattr(space, "nvec") else np.zeros((K, n, int(space.shape[0])))
    if complete:
        return [lambda: env.rollout_complete_episodic(a), lambda: env.bind_rollout_complete_episodic(a, 0, 0, 0, 0, 0)]
    return [lambda: env.rollout_episodic(a), lambda: env.bind_rollout_episodic(a, 0, 0, 0)]


def test_every_refusal_is_raised_before_any_device_call():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd.episodes import EPISODIC_REFUSAL

    noise = (ga.StateNoiseProcessor(["i_sd"], "normal", dict(scale=0.01)),)
    cases = [
        (dict(dtype="float64"), "Cont-CC-PMSM-v0", "float64"),
        (dict(ode_solver=ga.DormandPrince5Solver()), "Cont-CC-PMSM-v0", "DormandPrince5Solver"),
        (dict(ode_solver=ga.ScipyOdeSolver()), "Cont-CC-PMSM-v0", "error-controlled Dormand-Prince"),
        (dict(converter=dict(interlocking_time=1e-6)), "Finite-CC-PMSM-v0", "interlocking time"),
        (dict(physical_system_wrappers=(ga.DeadTimeProcessor(steps=2),)), "Cont-CC-PMSM-v0", "DeadTimeProcessor"),
        (dict(supply=ga.RCVoltageSupply(u_nominal=400.0)), "Cont-CC-PMSM-v0", "RCVoltageSupply"),
        (dict(motor=dict(motor_initializer=dict(random_init="uniform"))), "Cont-CC-PMSM-v0", "random initial states"),
        (dict(physical_system_wrappers=noise), "Cont-CC-PMSM-v0", "StateNoiseProcessor"),
        (dict(physical_system_wrappers=(ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor("SCIM"))), "Cont-CC-SCIM-v0", "FluxOrientedDqToAbcActionProcessor"),
    ]
    for kw, env_id, needle in cases:
        for shell in (dict(), dict(reference_generator="default")):
            env = _mk(ga, env_id, max_episode_steps=5, **kw, **shell)
            assert env.physical_system._handle is None
            for call in _calls(env, bool(shell)):
                with pytest.raises(NotImplementedError) as e:
                    call()
                assert str(e.value).startswith(EPISODIC_REFUSAL) and needle in str(e.value), (needle, str(e.value))
    # messages differ: one each
    msgs = set()
    for kw, env_id, needle in cases:
        with pytest.raises(NotImplementedError) as e:
            _mk(ga, env_id, max_episode_steps=5, **kw).rollout_episodic(np.zeros((2, 8, 3)))
        msgs.add(str(e.value))
    assert len(msgs) == len(cases)


def test_refused_ways_of_calling():
    """Half-precision actions are refused by name; last_only and the synthetic action source have no episodic entry point at all."""
    import inspect

    import torch

    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd.episodes import EPISODIC_REFUSAL

    for shell in (dict(), dict(reference_generator="default")):
        env = _mk(ga, max_episode_steps=5, **shell)
        half = torch.zeros((3, 8, 3), dtype=torch.float16)
        calls = ([lambda: env.rollout_complete_episodic(half), lambda: env.bind_rollout_complete_episodic(half, 0, 0, 0, 0, 0)] if shell else
                 [lambda: env.rollout_episodic(half), lambda: env.bind_rollout_episodic(half, 0, 0, 0)])
        for call in calls:
            with pytest.raises(NotImplementedError) as e:
                call()
            assert str(e.value).startswith(EPISODIC_REFUSAL) and "half-precision" in str(e.value)
        for name in ("rollout_episodic", "bind_rollout_episodic", "rollout_complete_episodic", "bind_rollout_complete_episodic"):
            if hasattr(env, name):
                params = inspect.signature(getattr(env, name)).parameters
                assert "last_only" not in params and "seed" not in params and "step0" not in params, name
        assert not hasattr(env, "rollout_episodic_synthetic") and not hasattr(env, "rollout_complete_episodic_synthetic")
        with pytest.raises(TypeError):
            (env.rollout_complete_episodic if shell else env.rollout_episodic)(np.zeros((3, 8, 3)), last_only=True)


def test_an_env_without_a_time_limit_raises_value_error():
    import gym_electric_motor_amd as ga

    for kw in (dict(), dict(episode_statistics=True)):
        for shell in (dict(), dict(reference_generator="default")):
            env = _mk(ga, **kw, **shell)
            for call in _calls(env, bool(shell)):
                with pytest.raises(ValueError, match="max_episode_steps"):
                    call()


def test_tensor_validation_follows_check_complete():
    import torch

    import gym_electric_motor_amd as ga

    env = _mk(ga, max_episode_steps=5, reference_generator="default")
    n, K, S = 8, 5, len(env.physical_system.state_names)
    n_ref = len(env.reference_names)
    with pytest.raises(ValueError, match="K must be >= 1"):
        env.rollout_complete_episodic(torch.zeros((0, n, 3)))
    with pytest.raises(ValueError, match="actions"):
        env.rollout_complete_episodic(7)
    a = torch.zeros((K, n, 3))
    s_out, r_out, w_out = torch.zeros((K, n, S)), torch.zeros((K, n, n_ref)), torch.zeros((K, n))
    t_out, u_out = torch.zeros((K, n), dtype=torch.uint8), torch.zeros((K, n), dtype=torch.uint8)
    what = "rollout_complete_episodic: "
    with pytest.raises(ValueError, match=what + "state_out must have shape"):
        env.rollout_complete_episodic(a, state_out=torch.zeros((K, n, S - 1)))
    with pytest.raises(ValueError, match=what + "refs_out must have shape"):
        env.rollout_complete_episodic(a, refs_out=torch.zeros((K + 1, n, n_ref)))
    with pytest.raises(ValueError, match=what + "terminated_out must have shape"):
        env.rollout_complete_episodic(a, terminated_out=torch.zeros((n, K), dtype=torch.uint8))
    with pytest.raises(ValueError, match=what + "truncated_out must have shape"):
        env.rollout_complete_episodic(a, truncated_out=torch.zeros((K, n, 1), dtype=torch.uint8))
    with pytest.raises(ValueError, match=what + "state_out must have dtype"):
        env.rollout_complete_episodic(a, state_out=s_out.double())
    with pytest.raises(ValueError, match=what + "truncated_out must have dtype"):
        env.rollout_complete_episodic(a, truncated_out=torch.zeros((K, n), dtype=torch.bool))
    with pytest.raises(ValueError, match=what + "reward_out must be contiguous"):
        env.rollout_complete_episodic(a, reward_out=torch.zeros((n, K)).t())
    with pytest.raises(ValueError, match=what + "state_out must be on device cuda:0"):
        env.rollout_complete_episodic(a, state_out=s_out)
    bound = "bind_rollout_complete_episodic: "
    with pytest.raises(ValueError, match=bound + "actions must have dtype"):
        env.bind_rollout_complete_episodic(a.double(), s_out, r_out, w_out, t_out, u_out)
    with pytest.raises(ValueError, match=bound + "actions must have shape"):
        env.bind_rollout_complete_episodic(torch.zeros((K, n, 2)), s_out, r_out, w_out, t_out, u_out)
    with pytest.raises(ValueError, match=bound + "actions must be on device cuda:0"):
        env.bind_rollout_complete_episodic(a, s_out, r_out, w_out, t_out, u_out)
    with pytest.raises(ValueError, match=bound + "truncated_out must be given"):
        env.bind_rollout_complete_episodic(a, s_out, r_out, w_out, t_out, None)
    with pytest.raises(ValueError, match="must be a dict of tensors"):
        env.bind_rollout_complete_episodic(a, s_out, r_out, w_out, t_out, u_out, episode_statistics=True)
    fin = _mk(ga, "Finite-CC-PMSM-v0", max_episode_steps=5, reference_generator="default")
    with pytest.raises(ValueError, match="actions must have dtype torch.uint8"):
        fin.bind_rollout_complete_episodic(torch.zeros((K, n)), s_out, r_out, w_out, t_out, u_out)

    # the physics-only env, both layouts
    for layout, shape in (("aos", (K, n, S)), ("soa", (K, S, n))):
        env = _mk(ga, max_episode_steps=5, obs_layout=layout)
        with pytest.raises(ValueError, match="rollout_episodic: obs_out must have shape"):
            env.rollout_episodic(a, obs_out=torch.zeros(shape[:2] + (shape[2] + 1,)))
        with pytest.raises(ValueError, match="rollout_episodic: obs_out must be on device cuda:0"):
            env.rollout_episodic(a, obs_out=torch.zeros(shape))
        with pytest.raises(ValueError, match="rollout_episodic: terminated_out must have dtype"):
            env.rollout_episodic(a, terminated_out=torch.zeros((K, n)))
        with pytest.raises(ValueError, match="bind_rollout_episodic: obs_out must be given"):
            env.bind_rollout_episodic(a, None, t_out, u_out)
        with pytest.raises(ValueError, match="bind_rollout_episodic: actions must be on device cuda:0"):
            env.bind_rollout_episodic(a, torch.zeros(shape), t_out, u_out)


def test_the_old_entry_points_still_refuse_a_time_limit():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd.episodes import ROLLOUT_REFUSAL

    assert "time limit" in ROLLOUT_REFUSAL and "mask it has not seen" in ROLLOUT_REFUSAL
    assert "rollout_episodic" in ROLLOUT_REFUSAL and "rollout_complete_episodic" in ROLLOUT_REFUSAL  # (it names the way out)
    env = _mk(ga, max_episode_steps=5)
    for call in (lambda: env.rollout(np.zeros((2, 8, 3))), lambda: env.rollout_synthetic(2), lambda: env.bind_rollout(np.zeros((2, 8, 3)), None, None)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == ROLLOUT_REFUSAL
    env = _mk(ga, max_episode_steps=5, reference_generator="default")
    for call in (lambda: env.rollout_complete(np.zeros((2, 8, 3))), lambda: env.rollout_complete_synthetic(2),
                 lambda: env.bind_rollout_complete(np.zeros((2, 8, 3)), 0, 0, 0, 0)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == ROLLOUT_REFUSAL


@pytest.mark.parametrize("M", [7, 10])
def test_the_host_shell_shows_what_the_oracle_inputs_must_show(M):
    """The float64 host shell alone, on the inputs of tests/test_gpu_episodic_rollout.py::test_against_the_float64_host_shell (numpy
    parameter sets standing in for the device's): at M = 7 every lane truncates and none terminates -- the hot lanes pass the current limit
    in their eighth step --, at M = 10 terminations and truncations meet in one lane and some lanes only ever truncate; truncation rows
    differ between lanes; no lane-step is a close call."""
    import sys

    sys.path.insert(0, os.path.join(REPO, "tests"))
    import env_shell_cases as cases
    import env_shell_restatement as esr
    import episodic_rollout_cases as erc
    import gym_electric_motor_amd as ga
    from parity_contract import DONE_MARGIN

    spec = erc.spec(M)
    assert (spec["N"], spec["K"]) == (197, 48) and M in erc.LIMITS
    shell = cases.build_shell(ga, spec, None)
    shell.param_sets = cases.standin_param_sets(spec, shell, np.random.default_rng(5), n_sets=40)
    _, out = shell.run(cases.actions(spec))
    term, trunc = out["terminated"], out["truncated"]
    only_trunc = ~term.any(axis=0) & trunc.any(axis=0)
    assert not (term & trunc).any()
    if M == 7:
        assert not term.any() and only_trunc.all() and int(trunc.sum()) == 197 * (48 // 7)
    else:
        assert term.any() and only_trunc.any() and (term.any(axis=0) & trunc.any(axis=0)).any()
        assert (trunc != trunc[:, :1]).any()  # a termination restarted some lane's counter
    left_out = 1.0 - float((np.arange(48)[:, None] < esr.first_close_call(out["margin"], DONE_MARGIN)[None, :]).mean())
    assert left_out <= 0.02
