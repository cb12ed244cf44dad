"""The lookahead rollout (csrc/gemx_lookahead.hip, gemx_rollout_lookahead_complete) without a GPU: every refusal before any device call,
each with its own message; the shape, dtype and device checks of `noise`, `scores_out` and the bound tensors; the selection rule's numpy
restatement on ties, -inf and all-equal scores; the source-level contract of the units and the C ABI."""
import os
import re

import numpy as np
import pytest

import gym_electric_motor_amd as ga
from gym_electric_motor_amd import _lib, build
import lookahead_restatement as lr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gym_electric_motor_amd", "csrc")
N = 8


def _mk(env_id="Finite-CC-PMSM-v0", reference_generator="default", **kw):
    kw.setdefault("max_episode_steps", 5)
    return ga.make(env_id, n_envs=N, device=0, _defer_create=True, reference_generator=reference_generator, **kw)


def test_refusals_need_no_device():
    import torch

    env = _mk()
    n_state, n_ref, na = len(env.physical_system.state_names), len(env.reference_names), 8
    assert env.n_lookahead_actions() == na and n_ref == 2
    seen = set()

    def raises(exc, fn):
        with pytest.raises(exc) as e:
            fn()
        seen.add(str(e.value))
        return str(e.value)

    roll, bind = env.rollout_lookahead_complete_episodic, env.bind_rollout_lookahead_complete_episodic
    # the new refusal: a continuous converter has no finite action set
    for env_id in ("Cont-CC-PMSM-v0", "Cont-SC-PermExDc-v0"):
        msg = raises(NotImplementedError, lambda: _mk(env_id).rollout_lookahead_complete_episodic(4))
        assert "continuous" in msg and "finite action set" in msg
        with pytest.raises(NotImplementedError, match="finite action set"):
            _mk(env_id).bind_rollout_lookahead_complete_episodic(4, None, None, None, None, None, None)  # (before the outputs are looked at)
    # what rollout_policy_complete_episodic refuses
    assert "time limit" in raises(ValueError, lambda: _mk(max_episode_steps=None).rollout_lookahead_complete_episodic(4))
    assert "K must be" in raises(ValueError, lambda: roll(0))
    assert "K must be" in raises(ValueError, lambda: roll(True))
    assert "float64" in raises(NotImplementedError, lambda: _mk(dtype="float64").rollout_lookahead_complete_episodic(4))
    e = _mk("Finite-SC-SCIM-v0", physical_system_wrappers=(ga.FluxObserver(),))
    assert "FluxObserver" in raises(NotImplementedError, lambda: e.rollout_lookahead_complete_episodic(4))
    assert "observation-side processor" in raises(NotImplementedError, lambda: _mk(flatten_observation=True).rollout_lookahead_complete_episodic(4))
    e = _mk(physical_system_wrappers=(ga.StateNoiseProcessor(states=["i_sd"], random_dist="normal", random_kwargs=dict(scale=0.01)),))
    assert "StateNoiseProcessor" in raises(NotImplementedError, lambda: e.rollout_lookahead_complete_episodic(4))
    gen = ga.StepReferenceGenerator(reference_state="i")
    msg = raises(NotImplementedError, lambda: _mk("Finite-CC-PermExDc-v0", reference_generator=gen).rollout_lookahead_complete_episodic(4))
    assert "StepReferenceGenerator" in msg and "BatchedWienerProcessReferenceGenerator" in msg and "ProfileReferenceGenerator" in msg
    # noise and scores: dtype, shape, contiguity, device
    assert "noise must have dtype" in raises(ValueError, lambda: roll(4, noise=torch.zeros((4, N, na), dtype=torch.float64)))
    assert "noise must have shape" in raises(ValueError, lambda: roll(4, noise=torch.zeros((4, N, na - 1))))
    assert "noise must be contiguous" in raises(ValueError, lambda: roll(4, noise=torch.zeros((4, N, 2 * na))[:, :, ::2]))
    assert "noise must be on device" in raises(ValueError, lambda: roll(4, noise=torch.zeros((4, N, na))))
    assert "noise must be a tensor" in raises(ValueError, lambda: roll(4, noise=np.zeros((4, N, na), np.float32)))
    assert "half-precision noise" in raises(NotImplementedError, lambda: roll(4, noise=torch.zeros((4, N, na), dtype=torch.float16)))
    assert "scores_out must have dtype" in raises(ValueError, lambda: roll(4, scores_out=torch.zeros((4, N, na), dtype=torch.float64)))
    assert "scores_out must have shape" in raises(ValueError, lambda: roll(4, scores_out=torch.zeros((4, N))))
    assert "scores_out must be on device" in raises(ValueError, lambda: roll(4, scores_out=torch.zeros((4, N, na))))
    assert "half-precision scores_out" in raises(NotImplementedError, lambda: roll(4, scores_out=torch.zeros((4, N, na), dtype=torch.bfloat16)))
    # the outputs, in the table's order
    assert "state_out must have shape" in raises(ValueError, lambda: roll(4, state_out=torch.zeros((4, N, n_state + 1))))
    assert "refs_out must have dtype" in raises(ValueError, lambda: roll(4, refs_out=torch.zeros((4, N, n_ref), dtype=torch.float64)))
    assert "reward_out must have shape" in raises(ValueError, lambda: roll(4, reward_out=torch.zeros((4, N, 1))))
    assert "actions_out must have dtype" in raises(ValueError, lambda: roll(4, actions_out=torch.zeros((4, N))))
    assert "terminated_out must have dtype" in raises(ValueError, lambda: roll(4, terminated_out=torch.zeros((4, N))))
    assert "truncated_out must be on device" in raises(ValueError, lambda: roll(4, truncated_out=torch.zeros((4, N), dtype=torch.uint8)))
    # a bound call allocates nothing
    assert "state_out must be given" in raises(ValueError, lambda: bind(4, None, None, None, None, None, None))
    u8 = torch.zeros((4, N), dtype=torch.uint8)
    t = [torch.zeros((4, N, n_state)), torch.zeros((4, N, n_ref)), torch.zeros((4, N)), u8, u8]
    assert "truncated_out must be given" in raises(ValueError, lambda: bind(4, *t, None))
    assert "scores_out must be a tensor" in raises(ValueError, lambda: bind(4, *t, u8, scores_out=True))
    assert "episode_statistics must be a dict" in raises(ValueError, lambda: bind(4, *t, u8, episode_statistics=True))
    # everything past the checks needs the device handle, which a deferred env has not got: nothing was launched before
    for kw in (dict(), dict(return_scores=True)):
        with pytest.raises(_lib.GemxError, match="no device handle"):
            roll(4, **kw)
    profile = ga.ProfileReferenceGenerator(np.zeros((37, 2), np.float32), reference_states=["i_sd", "i_sq"])
    with pytest.raises(_lib.GemxError, match="no device handle"):
        _mk(reference_generator=profile).rollout_lookahead_complete_episodic(4)
    assert len(seen) >= 29  # each refusal has its own message


def test_action_set_sizes():
    for env_id, na in (("Finite-CC-PMSM-v0", 8), ("Finite-SC-PermExDc-v0", 4), ("Finite-TC-ExtExDc-v0", 16), ("Finite-SC-SCIM-v0", 8), ("Finite-CC-EESM-v0", 32),
                       ("Finite-CC-DFIM-v0", 64)):
        assert _mk(env_id).n_lookahead_actions() == na, env_id


def test_selection_rule_restatement():
    inf = np.float32(np.inf)
    pick = lambda *s: int(lr.select(np.array(s, np.float32)))  # noqa: E731
    assert pick(1, 2, 3) == 2 and pick(3, 2, 1) == 0
    assert pick(1, 5, 5, 2) == 1 and pick(5, 1, 5, 5) == 0  # ties: the lowest index
    assert pick(7, 7, 7, 7) == 0 and pick(-inf, -inf, -inf) == 0  # all equal, all masked: action 0
    assert pick(-inf, -inf, -3, -inf) == 2 and pick(-inf, 0, 0) == 1  # masks
    assert pick(np.nan, 1, 2) == 0 and pick(1, np.nan, 2) == 2 and pick(1, 2, np.nan) == 1  # a NaN never wins, and is never beaten at index 0
    # noise is added in float32, and a -inf entry masks whatever the score
    scores = np.array([[-0.25, -0.5, -0.125, -0.125]], np.float32)
    noise = np.array([[0, 0, -inf, 0]], np.float32)
    assert lr.select(lr.noisy(scores)).tolist() == [2] and lr.select(lr.noisy(scores, noise)).tolist() == [3]
    assert lr.noisy(scores, noise).dtype == np.float32 and lr.select(lr.noisy(scores)).dtype == np.uint8
    # against the loop itself on random rows with many ties
    rng = np.random.default_rng(0)
    s = rng.integers(-2, 3, (500, 16)).astype(np.float32)
    s[rng.random(s.shape) < 0.2] = -inf
    want = []
    for row in s:
        best = 0
        for a in range(1, len(row)):
            if row[a] > row[best]:
                best = a
        want.append(best)
    assert lr.select(s).tolist() == want


def test_units_headers_and_abi():
    la = build.la_libs()
    assert len(la) == 8 == len(set(la)) and all(re.search(r"libgemx_la\d+_\d+\.so$", p) for p in la)
    assert set(build.LA_UNITS) <= set(build.UNITS) and all(c in (1, 3, 5, 7, 9) for _, c in build.LA_UNITS)  # finite converters only
    assert {(s, c) for s, c in build.UNITS if c % 2 == 1 and c < 10} == set(build.LA_UNITS)
    names = {os.path.basename(p) for p in build.SOURCES}
    assert {"gemx_lookahead.hip", "gemx_lookahead.hpp"} <= names and all(os.path.exists(p) for p in build.SOURCES)
    deps = set(build._DEPS["lookahead"])
    assert {"gemx_lookahead.hip", "gemx_lookahead.hpp", "gemx_reward.hpp", "gemx_refgen_lane.hpp", "gemx_refprofile_lane.hpp", "gemx_refprofile.hip", "gemx_unit_host.hpp",
            "gemx_envparams_dev.hpp", "gemx_kernels.hpp"} <= deps
    assert "gemx_lookahead.hpp" in build._DEPS["capi"]
    header = open(os.path.join(REPO, "include", "gemx.h")).read()
    assert re.search(r"^#define GEMX_ABI_VERSION 9\b", header, re.M) and _lib.ABI_VERSION == 9  # one new entry point, no struct changed
    m = re.search(r"\bint gemx_rollout_lookahead_complete\(([^;]*)\);", header)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")] == [
        "h", "call", "refs_out_dev", "actions_out_dev", "scores_out_dev", "noise_dev", "refgen", "refprofile", "stream"]
    assert "gemx_rollout_lookahead_complete" in _lib.EXPORTS and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    unit = open(os.path.join(CSRC, "gemx_lookahead.hip")).read()
    # the action loop is rolled, the reward is THE definition, the generators are the lane functions, the pin is there where the trial is merged
    assert "#pragma unroll 1\n        for (uint32_t ai = 0; ai < (uint32_t)NA; ++ai)" in unit and "reward_row<R>(H, &W" in unit
    for fn in ("reset_generator(G", "new_subepisode(G", "walk_step(G", "profile_restart(P", "profile_row<float>(P", "ensure_linmap<", "fill_unit_kargs<", "dispatch_load_solver("):
        assert fn in unit, fn
    assert 'asm volatile("" : "+v"(yt[j]))' in unit and 'asm volatile("" : "+v"(y[j]))' in unit and "__shared__" not in unit and "__syncthreads" not in unit
    capi = open(os.path.join(CSRC, "gemx_capi.hip")).read()
    assert 'load_side_unit(g_la_units, "la"' in capi and "EP_LAUNCH_LOOKAHEAD" in capi and "lookahead_rollout_kernel<%d" in capi
    assert capi.count("episodic_family_refusals(") == 3  # one list of refusals: its definition, the policy rollouts, the lookahead
