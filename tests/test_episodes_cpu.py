"""The device-side episode time limit and episode statistics without a GPU (`_defer_create=True`): the keywords of `make()`, the stage's
config, the refusals, the resolved launch order with and without the stage, the numpy restatement of the row function on a hand-written
table, and the agreement of header, binding and build list."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)  # (sibling module: the restatement)


def _mk(ga, env_id="Cont-CC-PMSM-v0", **kw):
    return ga.make(env_id, n_envs=4, _defer_create=True, **kw)


def test_make_builds_the_stage():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd import _lib

    for kw in (dict(), dict(reference_generator="default")):  # both env shells
        env = _mk(ga, max_episode_steps=3, **kw)
        cfg = env.episodes._cfg
        assert cfg.struct_size == C.sizeof(_lib.GemxEpisodeConfig) == 16 and cfg.max_steps == 3 and env.episodes.max_steps == 3
        assert cfg.has_reward == int(bool(kw))  # (the physics-only env has no reward of its own: it counts lengths)
        assert not env.episodes.statistics
        with pytest.raises(ValueError, match="episode_statistics=True"):
            env.episode_statistics()
        env = _mk(ga, episode_statistics=True, **kw)
        assert env.episodes._cfg.max_steps == 0 and env.episodes.statistics and env.truncated is False
        env = _mk(ga, max_episode_steps=np.int64(1000), episode_statistics=True, **kw)
        assert env.episodes._cfg.max_steps == 1000 and env.episodes.statistics


def test_auto_reset_in_kernel_follows_the_physics():
    import gym_electric_motor_amd as ga

    noise = (ga.StateNoiseProcessor(["i_sd"], "normal", dict(scale=0.0)),)
    for kw in (dict(), dict(reference_generator="default")):
        env = _mk(ga, max_episode_steps=3, **kw)
        assert env.physical_system._cfg.auto_reset == 1 and env.episodes._cfg.auto_reset_in_kernel == 1
        env = _mk(ga, max_episode_steps=3, auto_reset=False, **kw)
        assert env.physical_system._cfg.auto_reset == 0 and env.episodes._cfg.auto_reset_in_kernel == 0
        for auto in (None, True, False):  # behind a StateNoiseProcessor the physics never restarts an env itself
            env = _mk(ga, max_episode_steps=3, physical_system_wrappers=noise, auto_reset=auto, **kw)
            assert env.physical_system._cfg.auto_reset == 0 and env.episodes._cfg.auto_reset_in_kernel == 0
    # one env: auto_reset defaults to off
    env = ga.make("Cont-CC-PMSM-v0", n_envs=1, _defer_create=True, max_episode_steps=3)
    assert env.episodes._cfg.auto_reset_in_kernel == 0


def test_bad_time_limits_raise():
    import gym_electric_motor_amd as ga

    for bad in (0, -1, -1000, 2.5, 3.0, "3", True, 2 ** 31):
        for kw in (dict(), dict(reference_generator="default")):
            with pytest.raises(ValueError, match="max_episode_steps"):
                _mk(ga, max_episode_steps=bad, **kw)


def test_fused_rollouts_refuse_a_time_limit():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd.episodes import ROLLOUT_REFUSAL

    assert "time limit" in ROLLOUT_REFUSAL and "mask it has not seen" in ROLLOUT_REFUSAL
    env = _mk(ga, max_episode_steps=5)
    for call in (lambda: env.rollout(np.zeros((2, 4, 3))), lambda: env.rollout_synthetic(2), lambda: env.bind_rollout(np.zeros((2, 4, 3)), None, None)):
        with pytest.raises(NotImplementedError, match="episode time limit") as e:
            call()
        assert str(e.value) == ROLLOUT_REFUSAL
    env = _mk(ga, max_episode_steps=5, episode_statistics=True, reference_generator="default")
    for call in (lambda: env.rollout_complete(np.zeros((2, 4, 3))), lambda: env.rollout_complete_synthetic(2),
                 lambda: env.bind_rollout_complete(np.zeros((2, 4, 3)), 0, 0, 0, 0)):
        with pytest.raises(NotImplementedError, match="episode time limit") as e:
            call()
        assert str(e.value) == ROLLOUT_REFUSAL
    # statistics alone do not refuse; outputs asked of an env without the stage do
    _mk(ga, episode_statistics=True).pipeline.refuse_rollout()
    with pytest.raises(ValueError, match="episode_statistics=True"):
        _mk(ga).pipeline.bind_episode_rows(None, outputs=True)


def test_launch_order_with_and_without_the_stage():
    """Without the keywords `make()` builds no stage and resolves the launches it resolved before (the lists are written out here)."""
    import gym_electric_motor_amd as ga

    noise = (ga.StateNoiseProcessor(["i_sd"], "normal", dict(scale=0.01)),)
    flux = (ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor("SCIM"))
    parent = [
        (dict(), False, ["physics"]),
        (dict(reference_generator="default"), True, ["physics", "generators"]),
        (dict(reference_generator="default", flatten_observation=True), True, ["physics", "generators", "program"]),
        (dict(reference_generator="default", physical_system_wrappers=noise), True, ["reset", "physics", "noise", "generators"]),
        (dict(reference_generator="default", physical_system_wrappers=noise, auto_reset=False), True, ["physics", "noise", "generators"]),
        (dict(env_id="Cont-CC-SCIM-v0", reference_generator="default", physical_system_wrappers=flux), True, ["actions", "physics", "observer", "generators"]),
        (dict(env_id="Cont-CC-SCIM-v0", physical_system_wrappers=flux[:1] + (ga.CosSinProcessor(angle="psi_angle"),)), False, ["physics", "observer", "program"]),
    ]
    for kw, gens, want in parent:
        kw = dict(kw)
        env = _mk(ga, kw.pop("env_id", "Cont-CC-PMSM-v0"), **kw)
        assert env.episodes is None and env.pipeline.episode is None and env.truncated is False
        assert env.pipeline.launch_order(generators=gens) == want, kw
    with_stage = [
        (dict(episode_statistics=True), False, ["physics", "episode"]),
        (dict(max_episode_steps=9), False, ["reset", "physics", "episode"]),
        (dict(reference_generator="default", episode_statistics=True), True, ["physics", "episode", "generators"]),
        (dict(reference_generator="default", max_episode_steps=9, flatten_observation=True), True, ["reset", "physics", "episode", "generators", "program"]),
        (dict(reference_generator="default", max_episode_steps=9, physical_system_wrappers=noise), True, ["reset", "physics", "noise", "episode", "generators"]),
        (dict(reference_generator="default", max_episode_steps=9, physical_system_wrappers=noise, auto_reset=False), True,
         ["reset", "physics", "noise", "episode", "generators"]),
        (dict(reference_generator="default", episode_statistics=True, physical_system_wrappers=noise, auto_reset=False), True,
         ["physics", "noise", "episode", "generators"]),
        (dict(env_id="Cont-CC-SCIM-v0", reference_generator="default", max_episode_steps=9, physical_system_wrappers=flux), True,
         ["actions", "reset", "physics", "episode", "observer", "generators"]),
    ]
    for kw, gens, want in with_stage:
        kw = dict(kw)
        env = _mk(ga, kw.pop("env_id", "Cont-CC-PMSM-v0"), **kw)
        assert env.pipeline.launch_order(generators=gens) == want, kw
    # the order is written down once, and the stage sits directly behind what produces reward and done, before the generators
    from gym_electric_motor_amd.observation import ObservationPipeline

    assert ObservationPipeline.AFTER_STEP == ("noise", "episode", "observer", "generators", "program")
    # a time limit restarts every ended env: the flux observer follows even when the physics has no auto-reset
    env = _mk(ga, "Cont-CC-SCIM-v0", physical_system_wrappers=flux[:1], max_episode_steps=9, auto_reset=False)
    assert env.flux.auto_reset
    env = _mk(ga, "Cont-CC-SCIM-v0", physical_system_wrappers=flux[:1], episode_statistics=True, auto_reset=False)
    assert not env.flux.auto_reset


def test_restatement_on_a_hand_written_table():
    """6 steps, 3 envs, a limit of 3: env 0 only ever truncates; env 1 terminates at step 2 and truncates at step 5; env 2 terminates at
    step 3, where it also reaches the limit -- that counts as terminated, not truncated -- and truncates at step 6."""
    from episode_restatement import Episodes

    done = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.uint8)
    reward = np.array([[1, 0.5, -1], [2, 0.5, -1], [3, 0.5, -1], [4, 0.5, -1], [5, 0.5, -1], [6, 0.5, -1]], np.float32)
    truncated = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [1, 0, 1]], np.uint8)
    ended = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 1], [0, 0, 0], [0, 1, 0], [1, 0, 1]], np.uint8)
    fin_ret = np.array([[0, 0, 0], [0, 1.0, 0], [6, 0, -3], [0, 0, 0], [0, 1.5, 0], [15, 0, -3]], np.float64)
    fin_len = np.array([[0, 0, 0], [0, 2, 0], [3, 0, 3], [0, 0, 0], [0, 3, 0], [3, 0, 3]], np.int32)
    for in_kernel in (False, True):
        ep = Episodes(3, max_steps=3, auto_reset_in_kernel=in_kernel)
        got = ep.rows(done, reward)
        assert np.array_equal(got["truncated"], truncated) and np.array_equal(got["ended"], ended)
        assert np.array_equal(got["reset_mask"], truncated if in_kernel else ended)
        assert np.array_equal(got["finished_return"], fin_ret) and got["finished_return"].dtype == np.float64
        assert np.array_equal(got["finished_length"], fin_len)
        f = ep.fields()
        assert f["length"].tolist() == [0, 1, 0] and f["ret"].tolist() == [0.0, 0.5, 0.0]
        assert f["last_length"].tolist() == [3, 3, 3] and f["last_ret"].tolist() == [15.0, 1.5, -3.0] and f["n_finished"].tolist() == [2, 2, 2]
    # no limit: ended is done, nothing truncates, the return keeps summing
    ep = Episodes(3)
    got = ep.rows(done, reward)
    assert not got["truncated"].any() and np.array_equal(got["ended"], done)
    assert ep.fields()["ret"].tolist() == [21.0, 2.0, -3.0] and ep.fields()["length"].tolist() == [6, 4, 3]
    # the sum is sequential float64 over float32 rewards
    ep = Episodes(1)
    r = np.array([[1e8], [1.0], [-1e8]], np.float32)
    ep.rows(np.zeros((3, 1), np.uint8), r)
    assert ep.ret[0] == (np.float64(r[0, 0]) + np.float64(r[1, 0])) + np.float64(r[2, 0]) == 1.0


def test_build_and_header_agree_with_the_binding():
    from gym_electric_motor_amd import _lib, build

    assert os.path.join(build.CSRC, "gemx_episode.hip") in build.SOURCES
    assert ("episode", "gemx_episode.hip", ["gemx_support.hpp"]) in [u[:3] for u in build.SUPPORT]
    header = open(build.HEADER).read()
    assert re.search(r"#define GEMX_ABI_VERSION 9\b", header) and _lib.ABI_VERSION == 9  # new struct and entry points only
    assert re.search(r"#define GEMX_EPISODE_STATE_BYTES (\d+)", header).group(1) == str(_lib.EPISODE_STATE_BYTES) == "28"
    for name in ("gemx_episode_create", "gemx_episode_destroy", "gemx_episode_step", "gemx_episode_rows", "gemx_episode_get_state", "gemx_episode_set_state"):
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\(", header), name
    m = re.search(r"typedef struct gemx_episode_config \{(.*?)\} gemx_episode_config;", header, re.S)
    assert re.findall(r"int32_t (\w+);", m.group(1)) == [f[0] for f in _lib.GemxEpisodeConfig._fields_] == ["struct_size", "max_steps", "auto_reset_in_kernel", "has_reward"]
    src = open(os.path.join(build.CSRC, "gemx_episode.hip")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["gemx_support.hpp"]
    # ONE row function, called by both kernels
    assert len(re.findall(r"episode_row\(s, max_steps", src)) == 2 and len(re.findall(r"uint32_t episode_row\(", src)) == 1
