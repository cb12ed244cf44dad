"""The policy rollout of the complete env (csrc/gemx_policy_complete.hip, gemx_rollout_policy_complete) without a GPU: every refusal
before any device call, the documented output table, and the source-level contract of the units, the shared lane headers and the C ABI."""
import os
import re

import numpy as np
import pytest

import gym_electric_motor_amd as ga
from gym_electric_motor_amd import _lib, build
import policy_restatement as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gym_electric_motor_amd", "csrc")
N = 8


def _mk(env_id, reference_generator="default", **kw):
    kw.setdefault("max_episode_steps", 5)
    return ga.make(env_id, n_envs=N, device=0, _defer_create=True, reference_generator=reference_generator, **kw)


def _policy(n_in, widths, **kw):
    return ga.MLPPolicy(pr.make_layers(np.random.default_rng(0), n_in, widths), **kw)


def test_refusals_need_no_device():
    import torch

    env = _mk("Cont-CC-PermExDc-v0")
    n_state, n_ref = len(env.physical_system.state_names), len(env.reference_names)
    assert n_ref == 1
    seen = set()

    def raises(exc, fn):
        with pytest.raises(exc) as e:
            fn()
        seen.add(str(e.value))
        return str(e.value)

    ok = _policy(n_state + n_ref, (16, 1))
    roll = env.rollout_policy_complete_episodic
    # what rollout_policy_episodic refuses
    assert "time limit" in raises(ValueError, lambda: _mk("Cont-CC-PermExDc-v0", max_episode_steps=None).rollout_policy_complete_episodic(ok, 4))
    assert "MLPPolicy" in raises(ValueError, lambda: roll(object(), 4))
    assert "K must be" in raises(ValueError, lambda: roll(ok, 0))
    assert "output width" in raises(ValueError, lambda: roll(_policy(n_state + n_ref, (16, 3)), 4))
    assert "selects column" in raises(ValueError, lambda: roll(_policy(2, (1,), columns=[n_state]), 4))
    # the first layer takes the selected columns AND the env's references; there is no references= argument
    assert f"{n_state} observation columns + {n_ref} references" in raises(ValueError, lambda: roll(_policy(n_state, (16, 1)), 4))
    with pytest.raises(TypeError):
        roll(ok, 4, references=torch.zeros((4, N, 1)))
    # tensors, in _check_call's order
    assert "noise must have dtype" in raises(ValueError, lambda: roll(ok, 4, noise=torch.zeros((4, N, 1), dtype=torch.float64)))
    assert "noise must be on device" in raises(ValueError, lambda: roll(ok, 4, noise=torch.zeros((4, N, 1))))
    assert "obs0 must have shape" in raises(ValueError, lambda: roll(ok, 4, obs0=torch.zeros((N, n_state + 1))))
    assert "half-precision noise" in raises(NotImplementedError, lambda: roll(ok, 4, noise=torch.zeros((4, N, 1), dtype=torch.float16)))
    assert "state_out must have shape" in raises(ValueError, lambda: roll(ok, 4, state_out=torch.zeros((4, N, n_state + 1))))
    assert "refs_out must have dtype" in raises(ValueError, lambda: roll(ok, 4, refs_out=torch.zeros((4, N, n_ref), dtype=torch.float64)))
    assert "reward_out must have shape" in raises(ValueError, lambda: roll(ok, 4, reward_out=torch.zeros((4, N, 1))))
    assert "actions_out must be contiguous" in raises(ValueError, lambda: roll(ok, 4, actions_out=torch.zeros((4, N, 2))[:, :, :1]))
    assert "terminated_out must have dtype" in raises(ValueError, lambda: roll(ok, 4, terminated_out=torch.zeros((4, N))))
    assert "truncated_out must be on device" in raises(ValueError, lambda: roll(ok, 4, truncated_out=torch.zeros((4, N), dtype=torch.uint8)))
    # a bound call allocates nothing
    bind = env.bind_rollout_policy_complete_episodic
    assert "state_out must be given" in raises(ValueError, lambda: bind(ok, 4, None, None, None, None, None, None))
    t = [torch.zeros((4, N, n_state)), torch.zeros((4, N, n_ref)), torch.zeros((4, N)), torch.zeros((4, N, 1)), torch.zeros((4, N), dtype=torch.uint8)]
    assert "truncated_out must be given" in raises(ValueError, lambda: bind(ok, 4, *t, None))
    assert "episode_statistics must be a dict" in raises(ValueError, lambda: bind(ok, 4, *t, t[4], episode_statistics=True))
    # everything past the checks needs the device handle, which a deferred env has not got: nothing was launched before
    with pytest.raises(_lib.GemxError, match="no device handle"):
        roll(ok, 4)
    # what the kernel does not serve, through the episodic gate
    assert "float64" in raises(NotImplementedError, lambda: _mk("Cont-CC-PermExDc-v0", dtype="float64").rollout_policy_complete_episodic(ok, 4))
    e = _mk("Cont-SC-SCIM-v0", physical_system_wrappers=(ga.FluxObserver(),))
    wide = _policy(len(e.physical_system.state_names) + 1, (8, int(e.physical_system.action_space.shape[0])))
    assert "FluxObserver" in raises(NotImplementedError, lambda: e.rollout_policy_complete_episodic(wide, 4))
    e = _mk("Cont-CC-PermExDc-v0", flatten_observation=True)
    assert "observation-side processor" in raises(NotImplementedError, lambda: e.rollout_policy_complete_episodic(ok, 4))
    e = _mk("Cont-CC-PermExDc-v0", physical_system_wrappers=(ga.StateNoiseProcessor(states=["i"], random_dist="normal", random_kwargs=dict(scale=0.01)),))
    assert "StateNoiseProcessor" in raises(NotImplementedError, lambda: e.rollout_policy_complete_episodic(ok, 4))
    assert len(seen) >= 22


def test_generators_that_are_not_stepped_in_the_lane_are_refused_by_name():
    env0 = _mk("Cont-CC-PermExDc-v0")
    n_in = len(env0.physical_system.state_names) + 1
    ok = _policy(n_in, (16, 1))
    others = {
        "StepReferenceGenerator": ga.StepReferenceGenerator(reference_state="i"),
        "WienerProcessReferenceGenerator, ": None,  # (filled below: a multiple of kinds)
        "switched": ga.SwitchedReferenceGenerator([ga.StepReferenceGenerator(reference_state="i"), ga.SinusoidalReferenceGenerator(reference_state="i")]),
        "ReplayReferenceGenerator": ga.ReplayReferenceGenerator(np.zeros((16, N, 1)), reference_states=["i"]),
    }
    for word, gen in others.items():
        if gen is None:
            continue
        env = _mk("Cont-CC-PermExDc-v0", reference_generator=gen)
        with pytest.raises(NotImplementedError) as e:
            env.rollout_policy_complete_episodic(ok, 4)
        msg = str(e.value)
        assert word in msg and "BatchedWienerProcessReferenceGenerator" in msg and "ProfileReferenceGenerator" in msg, msg
        with pytest.raises(NotImplementedError):
            env.bind_rollout_policy_complete_episodic(ok, 4, None, None, None, None, None, None)  # (before the outputs are looked at)
    # a multiple of kinds on a two-column env
    env = _mk("Finite-CC-PMSM-v0", reference_generator=[ga.WienerProcessReferenceGenerator(reference_state="i_sd"), ga.SawtoothReferenceGenerator(reference_state="i_sq")])
    with pytest.raises(NotImplementedError, match="WienerProcessReferenceGenerator, SawtoothReferenceGenerator"):
        env.rollout_policy_complete_episodic(_policy(len(env.physical_system.state_names) + 2, (16, 8)), 4)
    # the two kinds that are served get as far as the missing device handle
    profile = ga.ProfileReferenceGenerator(np.zeros((37, 1), np.float32), reference_states=["i"])
    for gen in ("default", ga.BatchedWienerProcessReferenceGenerator(reference_states=("i",), episode_lengths=(3, 9)), profile):
        with pytest.raises(_lib.GemxError, match="no device handle"):
            _mk("Cont-CC-PermExDc-v0", reference_generator=gen).rollout_policy_complete_episodic(ok, 4)


def test_output_table_of_the_complete_policy_rollout():
    import torch

    for env_id, n_state, n_ref, act in (("Finite-CC-PMSM-v0", 14, 2, (torch.uint8, (6, N))), ("Cont-SC-SCIM-v0", 14, 1, (torch.float32, (6, N, 3)))):
        env = _mk(env_id)
        actions, specs = env._specs(6, complete=True, episodic=True, actions_out=True)
        assert [s[0] for s in specs] == ["state_out", "refs_out", "reward_out", "actions_out", "terminated_out", "truncated_out"]
        assert [s[1:] for s in specs] == [(torch.float32, (6, N, n_state)), (torch.float32, (6, N, n_ref)), (torch.float32, (6, N)), act,
                                          (torch.uint8, (6, N)), (torch.uint8, (6, N))]


def test_units_headers_and_abi():
    pc = build.pc_libs()
    assert len(pc) == len(build.UNITS) == len(set(pc)) and all(re.search(r"libgemx_pc\d+_\d+\.so$", p) for p in pc)
    assert [os.path.basename(p) for p in build.pl_libs()] == [os.path.basename(p).replace("_pc", "_pl") for p in pc]
    names = {os.path.basename(p) for p in build.SOURCES}
    new = {"gemx_policy_complete.hip", "gemx_policy_complete.hpp", "gemx_policy_dev.hpp", "gemx_refgen_lane.hpp", "gemx_refprofile_lane.hpp"}
    assert new <= names and all(os.path.exists(p) for p in build.SOURCES)
    for kind in ("policy_complete", "refgen", "refprofile", "capi"):  # an edit of a lane header recompiles everything that sees it
        assert {"gemx_refgen_lane.hpp", "gemx_refprofile_lane.hpp"} <= set(build._DEPS[kind]), kind
    assert "gemx_policy_dev.hpp" in build._DEPS["policy"] and "gemx_policy_dev.hpp" in build._DEPS["policy_complete"]
    assert {"gemx_policy_kernel.hpp", "gemx_unit_host.hpp"} <= names  # the one kernel of both kinds of policy unit: an edit recompiles both
    assert "gemx_policy_kernel.hpp" in build._DEPS["policy"] and "gemx_policy_kernel.hpp" in build._DEPS["policy_complete"]
    header = open(os.path.join(REPO, "include", "gemx.h")).read()
    assert re.search(r"^#define GEMX_ABI_VERSION 9\b", header, re.M) and _lib.ABI_VERSION == 9  # one new entry point only
    m = re.search(r"\bint gemx_rollout_policy_complete\(([^;]*)\);", header)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")] == ["h", "p", "call", "refs_out_dev", "refgen", "refprofile", "stream"]
    assert "gemx_rollout_policy_complete" in _lib.EXPORTS and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    # the lane functions are defined once, in the headers, and called by the generator units and the new unit alike
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("gemx_refgen.hip", "gemx_refprofile.hip", "gemx_policy_complete.hip", "gemx_refgen_lane.hpp", "gemx_refprofile_lane.hpp")}
    for fn in ("reset_generator", "new_subepisode", "walk_step", "step_normal"):
        assert re.search(rf"__device__ inline \w+ {fn}\(", src["gemx_refgen_lane.hpp"]), fn
        assert not re.search(rf"__device__ inline \w+ {fn}\(", src["gemx_refgen.hip"]) and re.search(rf"\b{fn}(<R>)?\(", src["gemx_refgen.hip"]), fn
    assert re.search(r"__device__ __forceinline__ void profile_restart\(", src["gemx_refprofile_lane.hpp"]) and "void profile_restart(" not in src["gemx_refprofile.hip"]
    # THE row function: declared in the lane header, defined once in gemx_refprofile.hip, in the head section the new unit includes
    assert re.search(r"void profile_row\(.*\);$", src["gemx_refprofile_lane.hpp"], re.M) and len(re.findall(r"void profile_row\(.*\) \{$", src["gemx_refprofile.hip"], re.M)) == 1
    assert src["gemx_refprofile.hip"].index("void profile_row(") < src["gemx_refprofile.hip"].index("#ifndef GEMX_REFPROFILE_ROW_ONLY")
    assert "#define GEMX_REFPROFILE_ROW_ONLY" in src["gemx_policy_complete.hip"] and '#include "gemx_refprofile.hip"' in src["gemx_policy_complete.hip"]
    unit = src["gemx_policy_complete.hip"]
    for fn in ("reset_generator(G", "new_subepisode(G", "walk_step(G", "profile_restart(P", "profile_row<float>(P"):
        assert fn in unit, fn
    kernel = open(os.path.join(CSRC, "gemx_policy_kernel.hpp")).read()  # the unit's kernel: the policy units', with a generator kind
    assert '#include "gemx_policy_kernel.hpp"' in unit and "pc_references<GEN>(" in kernel
    assert 'asm volatile("" : "+v"(y[j]))' in kernel and "ep_control_step" in kernel and "lin_usable" in kernel
    capi = open(os.path.join(CSRC, "gemx_capi.hip")).read()
    assert 'load_side_unit(g_pc_units, "pc"' in capi and "EP_LAUNCH_POLICY_COMPLETE" in capi and "policy_complete_rollout_kernel<%d" in capi
