"""The policy rollout (csrc/gemx_policy.hip, gemx_rollout_policy, ga.MLPPolicy) without a GPU: validation and refusals before any device
call, the margin of the finite-action test's excuse, and the source-level contract of the units and the C ABI."""
import os
import re

import numpy as np
import pytest

import gym_electric_motor_amd as ga
from gym_electric_motor_amd import _lib, build
import policy_restatement as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mk(env_id, **kw):
    kw.setdefault("max_episode_steps", 5)
    return ga.make(env_id, n_envs=8, device=0, _defer_create=True, **kw)


def _policy(n_in, widths, **kw):
    return ga.MLPPolicy(pr.make_layers(np.random.default_rng(0), n_in, widths), **kw)


def test_policy_limits_are_value_errors():
    rng = np.random.default_rng(1)
    for bad, msg in (([], "1 to 3"), (pr.make_layers(rng, 4, (8, 8, 8, 2)), "1 to 3"), (pr.make_layers(rng, 4, (65, 2)), "at most 64"),
                     (pr.make_layers(rng, 49, (8,)), "at most 48")):
        with pytest.raises(ValueError, match=msg):
            ga.MLPPolicy(bad)
    good = pr.make_layers(rng, 4, (8, 2))
    with pytest.raises(ValueError, match="activation"):
        ga.MLPPolicy(good, activation="gelu")
    with pytest.raises(ValueError, match="squash"):
        ga.MLPPolicy(good, squash="none")
    with pytest.raises(ValueError, match="distinct"):
        ga.MLPPolicy(good, columns=[1, 1])
    with pytest.raises(ValueError, match="half precision"):
        ga.MLPPolicy([(good[0][0].astype(np.float16), good[0][1]), good[1]])
    with pytest.raises(ValueError, match="layer 1 takes"):
        ga.MLPPolicy([good[0], (np.zeros((2, 7), np.float32), np.zeros(2, np.float32))])
    p = ga.MLPPolicy(good)
    with pytest.raises(ValueError, match="keep their shapes"):
        p.set_weights(pr.make_layers(rng, 4, (16, 2)))


def test_refusals_need_no_device_and_are_distinct():
    import torch

    env = _mk("Cont-CC-PermExDc-v0")
    n_state = len(env.physical_system.state_names)
    seen = set()

    def raises(exc, fn):
        with pytest.raises(exc) as e:
            fn()
        seen.add(str(e.value))
        return str(e.value)

    ok = _policy(n_state, (16, 1))
    assert "time limit" in raises(ValueError, lambda: ga.make("Cont-CC-PermExDc-v0", n_envs=8, device=0, _defer_create=True).rollout_policy_episodic(ok, 4))
    assert "MLPPolicy" in raises(ValueError, lambda: env.rollout_policy_episodic(object(), 4))
    assert "K must be" in raises(ValueError, lambda: env.rollout_policy_episodic(ok, 0))
    assert "output width" in raises(ValueError, lambda: env.rollout_policy_episodic(_policy(n_state, (16, 3)), 4))
    assert "inputs" in raises(ValueError, lambda: env.rollout_policy_episodic(_policy(n_state + 1, (16, 1)), 4))
    assert "selects column" in raises(ValueError, lambda: env.rollout_policy_episodic(_policy(1, (1,), columns=[n_state]), 4))
    assert "references must be a tensor" in raises(ValueError, lambda: env.rollout_policy_episodic(ok, 4, references=np.zeros((4, 8, 1))))
    assert "references must have shape" in raises(ValueError, lambda: env.rollout_policy_episodic(_policy(n_state + 1, (1,)), 4, references=torch.zeros((3, 8, 1))))
    assert "noise must have dtype" in raises(ValueError, lambda: env.rollout_policy_episodic(ok, 4, noise=torch.zeros((4, 8, 1), dtype=torch.float64)))
    assert "noise must be on device" in raises(ValueError, lambda: env.rollout_policy_episodic(ok, 4, noise=torch.zeros((4, 8, 1))))
    assert "obs0 must have shape" in raises(ValueError, lambda: env.rollout_policy_episodic(ok, 4, obs0=torch.zeros((8, n_state + 1))))
    assert "half-precision noise" in raises(NotImplementedError, lambda: env.rollout_policy_episodic(ok, 4, noise=torch.zeros((4, 8, 1), dtype=torch.float16)))
    assert "must be given" in raises(ValueError, lambda: env.bind_rollout_policy_episodic(ok, 4, None, None, None, None))
    # everything episodic_refusal lists, through the same gate
    for kw, word in ((dict(dtype="float64"), "float64"), (dict(ode_solver=ga.DormandPrince5Solver()) if hasattr(ga, "DormandPrince5Solver") else None, "Dormand")):
        if kw is not None:
            e = _mk("Cont-CC-PermExDc-v0", **kw)
            assert word in raises(NotImplementedError, lambda e=e: e.rollout_policy_episodic(ok, 4))
    # an observation-side processor
    e = _mk("Cont-SC-SCIM-v0", physical_system_wrappers=(ga.FluxObserver(),))
    n = len(e.physical_system.state_names)
    assert "FluxObserver" in raises(NotImplementedError, lambda: e.rollout_policy_episodic(_policy(n, (8, int(e.physical_system.action_space.shape[0]))), 4))
    assert len(seen) >= 15


def test_finite_excuse_margin():
    """Every finite case of the GPU test's table, with its weights, references and noise, on synthetic rows in [-1, 1]: the share of
    (row, lane) pairs whose two largest float64 logits are closer than twice the bound stays below 0.2 %, so the GPU test's 1 % cap can
    only be reached by a wrong kernel."""
    rows = np.random.default_rng(7).uniform(-1, 1, (pr.K_STEPS, pr.N_ENVS, 14))
    seen = 0
    for env_id, M, plan, act, squash, use_refs, use_noise in pr.cases():
        if not pr.ENVS[env_id][2]:
            continue
        layers, columns, refs, noise = pr.case_data(env_id, plan, use_refs, use_noise)
        x = rows[:, :, columns] if columns else rows
        if refs is not None:
            x = np.concatenate([x, refs.astype(np.float64)], axis=2)
        out, err = pr.forward(layers, act, x, noise)
        _, excused = pr.finite_action(out, err)
        assert excused.mean() < 0.002, (plan, act, use_refs, use_noise, excused.mean())
        seen += 1
    assert seen == 12


def test_units_and_header():
    assert len(build.pl_libs()) == len(build.UNITS) == len(set(build.pl_libs())) and all(re.search(r"libgemx_pl\d+_\d+\.so$", p) for p in build.pl_libs())
    src = open(os.path.join(REPO, "gym_electric_motor_amd", "build.py")).read()
    assert "gemx_policy.hip" in src and "pl_unit_lib(s, c)" in src
    header = open(os.path.join(REPO, "include", "gemx.h")).read()
    assert re.search(r"^#define GEMX_ABI_VERSION 9\b", header, re.M) and _lib.ABI_VERSION == 9  # new structs and entry points only
    for name in ("gemx_policy_create", "gemx_policy_set_weights", "gemx_policy_destroy", "gemx_rollout_policy", "gemx_policy_tanh_probe"):
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\(", header), name
    unit = open(os.path.join(REPO, "gym_electric_motor_amd", "csrc", "gemx_policy.hip")).read()
    assert '#include "gemx_policy_kernel.hpp"' in unit and "PC_GEN_NONE" in unit  # the kernel: the one both kinds of policy unit include
    kernel = open(os.path.join(REPO, "gym_electric_motor_amd", "csrc", "gemx_policy_kernel.hpp")).read()
    assert 'asm volatile("" : "+v"(y[j]))' in kernel and "ep_control_step" in kernel and "lin_usable" in kernel
