"""The device-side StateNoiseProcessor without a GPU (`_defer_create=True`): folding and order rules, the refusals and their messages,
the holder's defaults against the reference's class, the noise config struct, the physics config under the wrapper, and the agreement of
header, binding and build list."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REFERENCE_SRC = "/root/reference/src"


def _mk(ga, env_id="Cont-CC-PMSM-v0", **kw):
    return ga.make(env_id, n_envs=4, _defer_create=True, **kw)


def test_folding_and_order():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd.physical_system_wrappers import fold_wrappers

    noise = ga.StateNoiseProcessor(["i_sd", "i_sq"], "uniform", dict(low=-0.1, high=[0.1, 0.2]))
    chain = []
    out = fold_wrappers((ga.DeadTimeProcessor(2), noise, ga.CosSinProcessor()), observation_chain=chain)
    assert out["state_noise"] == dict(states=("i_sd", "i_sq"), dist="uniform", kwargs=dict(low=-0.1, high=[0.1, 0.2]))
    assert out["action_delay"] == 2 and chain == [("cossin", "epsilon", False)]
    assert "state_noise" not in fold_wrappers((ga.DeadTimeProcessor(2),))
    # observation-side processors behind the noise read the noisy row: the env has both stages
    env = _mk(ga, physical_system_wrappers=(noise, ga.CosSinProcessor()), observed_states=["i_sd", "cos(epsilon)"])
    assert env.state_noise is not None and env.observation_stage is not None and env.state_names == ["i_sd", "cos(epsilon)"]
    assert env.state_noise.states == ("i_sd", "i_sq") and env.state_noise.indices == [5, 6]
    # an instance read by class name and attributes, as the reference's own is
    class StateNoiseProcessor:
        _states, _random_dist, _random_kwargs = ["omega"], "laplace", dict(scale=0.5)

    env = _mk(ga, physical_system_wrappers=(StateNoiseProcessor(),))
    assert env.state_noise.dist == "laplace" and env.state_noise.indices == [0] and env.state_noise.params[1].tolist() == [0.5]
    assert env.state_names == list(env.physical_system.state_names)


def test_refusals():
    import gym_electric_motor_amd as ga

    noise = lambda *a, **k: ga.StateNoiseProcessor(["i_sd"], *a, **k)  # noqa: E731

    class StateNoiseProcessor:
        pass

    for kw in (dict(physical_system_wrappers=(StateNoiseProcessor(),)),                          # parameters cannot be read
               dict(physical_system_wrappers=(noise("gamma"),)),                                  # another distribution
               dict(physical_system_wrappers=(ga.CosSinProcessor(), noise())),                    # behind an observation-side processor
               dict(physical_system_wrappers=(ga.CurrentSumProcessor(("i_sd", "i_sq")), ga.StateNoiseProcessor(["i_sum"]))),  # appended columns
               dict(physical_system_wrappers=(noise(), noise())),                                 # a second one
               dict(physical_system_wrappers=(noise(),), obs_layout="soa")):
        with pytest.raises(NotImplementedError, match="NOISY state"):
            _mk(ga, **kw)
    with pytest.raises(NotImplementedError, match="NOISY state"):
        _mk(ga, "Cont-CC-SCIM-v0", physical_system_wrappers=(ga.FluxObserver(), noise()))
    for states in (["i_sum"], ["nothing"], "all"):  # not states of the base system: the reference's KeyError ('all' is not implemented there)
        with pytest.raises(KeyError):
            _mk(ga, physical_system_wrappers=(ga.StateNoiseProcessor(states),))
    with pytest.raises(TypeError, match="random_kwargs"):
        _mk(ga, physical_system_wrappers=(noise("normal", dict(low=0.0)),))
    with pytest.raises(ValueError):
        _mk(ga, physical_system_wrappers=(noise("normal", dict(scale=-1.0)),))
    with pytest.raises(ValueError):
        _mk(ga, physical_system_wrappers=(ga.StateNoiseProcessor(["i_sd", "i_sq"], "normal", dict(scale=[1.0, 2.0, 3.0])),))


def test_rollouts_refuse_by_name():
    import gym_electric_motor_amd as ga

    w = (ga.StateNoiseProcessor(["i_sd"]),)
    env = _mk(ga, physical_system_wrappers=w)
    for call in (lambda: env.rollout(np.zeros((2, 4, 3))), lambda: env.rollout_synthetic(2), lambda: env.bind_rollout(np.zeros((2, 4, 3)), None, None)):
        with pytest.raises(NotImplementedError, match="StateNoiseProcessor"):
            call()
    env = _mk(ga, physical_system_wrappers=w, reference_generator="default")
    for call in (lambda: env.rollout_complete(np.zeros((2, 4, 3))), lambda: env.rollout_complete_synthetic(2),
                 lambda: env.bind_rollout_complete(np.zeros((2, 4, 3)), 0, 0, 0, 0)):
        with pytest.raises(NotImplementedError, match="StateNoiseProcessor"):
            call()


_REF_PROBE = '''
import inspect, json, sys
sys.path[:0] = [%r, %r, %r]
from gym_electric_motor.physical_system_wrappers import StateNoiseProcessor as Ref
import gym_electric_motor_amd as ga
sig = lambda cls: [(n, repr(p.default)) for n, p in inspect.signature(cls.__init__).parameters.items()]
inst = Ref(["i_sd", "i_sq"], random_dist="laplace", random_kwargs=dict(loc=0.0, scale=0.1))
env = ga.make("Cont-CC-PMSM-v0", n_envs=4, _defer_create=True, physical_system_wrappers=(inst,))
print(json.dumps(dict(ref=sig(Ref), mine=sig(ga.StateNoiseProcessor), dist=env.state_noise.dist, indices=env.state_noise.indices,
                      scale=env.state_noise.params[1].tolist())))
'''


def test_holder_defaults_equal_the_references():
    """The live class, in a child process (its imports stay out of this session)."""
    import json
    import subprocess

    if not os.path.isdir(REFERENCE_SRC):
        pytest.skip("the reference is not on this machine")
    code = _REF_PROBE % (os.path.join(REPO, "oracle", "gymnasium_standin"), REFERENCE_SRC, REPO)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["mine"] == got["ref"] and [n for n, _ in got["ref"]] == ["self", "states", "random_dist", "random_kwargs", "random_length", "physical_system"]
    # the reference's own instance is read like the holder
    assert got["dist"] == "laplace" and got["indices"] == [5, 6] and got["scale"] == [0.1, 0.1]


def test_config_struct_and_physics_config():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd import _lib

    noise = ga.StateNoiseProcessor(["i_sq", "omega"], "uniform", dict(low=[-0.1, -0.2], high=0.3))
    env = _mk(ga, physical_system_wrappers=(noise,), reference_generator="default", seed=11, env_base=100)
    plain = _mk(ga, reference_generator="default", seed=11, env_base=100)
    cfg, ps = env.state_noise._cfg, env.physical_system
    assert cfg.struct_size == C.sizeof(_lib.GemxNoiseConfig) and cfg.n_in == 14 and cfg.n_noisy == 2
    assert list(cfg.index[:2]) == [6, 0] and list(cfg.dist[:2]) == [_lib.NOISE_UNIFORM] * 2
    assert list(cfg.param0[:2]) == [-0.1, -0.2] and list(cfg.param1[:2]) == [0.3, 0.3]
    assert cfg.seed == 11 and cfg.env_base == 100
    # the physics has no constraint, no auto-reset; the noise config carries what the env without the wrapper gives its physics
    assert ps._cfg.limit_mask == ps._cfg.squared_mask == 0 and ps._cfg.auto_reset == 0
    assert (cfg.limit_mask, cfg.squared_mask) == (plain.physical_system._cfg.limit_mask, plain.physical_system._cfg.squared_mask) == (0, 0x60)
    assert env.state_noise.auto_reset and plain.physical_system._cfg.auto_reset == 1
    assert cfg.has_reward == 1 and bytes(cfg.reward) == bytes(plain.reward_config) and env.reward_range == plain.reward_range
    # defaults of the three distributions, custom constraints, auto_reset=False, the physics-only env
    for dist, kind in (("normal", _lib.NOISE_NORMAL), ("uniform", _lib.NOISE_UNIFORM), ("laplace", _lib.NOISE_LAPLACE)):
        env = _mk(ga, "Cont-CC-PermExDc-v0", physical_system_wrappers=(ga.StateNoiseProcessor(["i"], dist),), constraints=("i", "omega"), auto_reset=False)
        cfg = env.state_noise._cfg
        assert (cfg.dist[0], cfg.param0[0], cfg.param1[0]) == (kind, 0.0, 1.0) and cfg.n_in == 5 and cfg.has_reward == 0
        assert cfg.limit_mask == 0b101 and cfg.squared_mask == 0 and not env.state_noise.auto_reset
        assert env.physical_system._cfg.limit_mask == 0 and env.physical_system._cfg.auto_reset == 0
        assert env.pipeline.bind_before_step() is None  # (auto_reset=False: no reset launch)


def test_build_and_header_agree_with_the_binding():
    from gym_electric_motor_amd import _lib, build

    assert os.path.join(build.CSRC, "gemx_statenoise.hip") in build.SOURCES
    assert ("statenoise", "gemx_statenoise.hip", ["gemx_support.hpp"]) in [u[:3] for u in build.SUPPORT]
    header = open(build.HEADER).read()
    m = re.search(r"enum \{ GEMX_NOISE_NORMAL = (\d+), GEMX_NOISE_UNIFORM = (\d+), GEMX_NOISE_LAPLACE = (\d+) \}", header)
    assert m and tuple(int(x) for x in m.groups()) == (_lib.NOISE_NORMAL, _lib.NOISE_UNIFORM, _lib.NOISE_LAPLACE)
    assert re.search(r"#define GEMX_ABI_VERSION 9\b", header) and _lib.ABI_VERSION == 9
    for name in ("gemx_noise_create", "gemx_noise_destroy", "gemx_noise_step", "gemx_noise_draws", "gemx_noise_get_position", "gemx_noise_set_position"):
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\(", header), name
    # the struct as the header lays it out: 4 int32, two int32 arrays, two double arrays, two 64-bit words, two masks, the reward description
    n = _lib.MAX_OUT
    assert C.sizeof(_lib.GemxNoiseConfig) == 16 + 2 * 4 * n + 2 * 8 * n + 16 + 8 + C.sizeof(_lib.GemxRewardConfig)
    assert _lib.GemxNoiseConfig.reward.offset == 16 + 2 * 4 * n + 2 * 8 * n + 16 + 8
    src = open(os.path.join(build.CSRC, "gemx_statenoise.hip")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["gemx_support.hpp"]
