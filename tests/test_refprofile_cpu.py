"""The device-side profile references without a GPU (`_defer_create=True`): the holder's config derivation, the agreement of header,
binding and build list, the refusals, and the float64 restatement of the row function on hand-computed cases."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)  # (sibling module: the restatement)

from refprofile_restatement import Profiles  # noqa: E402

NEW = ("gemx_refprofile_create", "gemx_refprofile_destroy", "gemx_refprofile_reset", "gemx_refprofile_step", "gemx_refprofile_rollout",
       "gemx_refprofile_rollout_shell", "gemx_refprofile_get_state", "gemx_refprofile_state_bytes", "gemx_refprofile_get_blob", "gemx_refprofile_set_blob")


def _mk(ga, gen, n_envs=4, env_id="Cont-CC-PMSM-v0", **kw):
    return ga.make(env_id, n_envs=n_envs, _defer_create=True, reference_generator=gen, **kw)


def test_config_derivation():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd import _lib

    assert ga.ProfileReferenceGenerator is ga.reference_generators.ProfileReferenceGenerator
    prof = np.stack([np.linspace(0.1, 0.5, 6), np.linspace(-0.5, -0.1, 6)], axis=1)
    # default states: the env id's referenced states, in state order; a shared table sampled at tau
    env = _mk(ga, ga.ProfileReferenceGenerator(prof))
    gen = env.reference_generator
    assert isinstance(gen, ga.ProfileReferences) and env.reference_names == ["i_sd", "i_sq"] and gen._order == [0, 1]
    cfg = gen._cfg
    assert cfg.struct_size == C.sizeof(_lib.GemxRefprofileConfig) == 64
    assert (cfg.n_ref, cfg.n_rows, cfg.per_env) == (2, 6, 0) and cfg.tau == cfg.profile_tau == env.physical_system.tau and gen.ratio == 1.0
    assert cfg.interpolation == _lib.PROFILE_INTERP_HOLD  # (rows at tau: nothing to interpolate)
    assert (cfg.end, cfg.start, cfg.env_base) == (_lib.PROFILE_END_HOLD, _lib.PROFILE_START_ZERO, 0)
    assert tuple(env.reference_space.low) == (-1.0, -1.0) and tuple(env.reference_space.high) == (1.0, 1.0)
    # the caller's columns are reordered to the state order; profile_tau, the choices, the seed and the shard arrive in the config
    tau = env.physical_system.tau
    env = _mk(ga, ga.ProfileReferenceGenerator(prof, reference_states=("i_sq", "i_sd"), profile_tau=2.5 * tau, end="wrap", start="random", seed=7), env_base=35)
    gen = env.reference_generator
    assert env.reference_names == ["i_sd", "i_sq"] and gen._order == [1, 0]
    cfg = gen._cfg
    assert cfg.profile_tau == 2.5 * tau and gen.ratio == tau / (2.5 * tau) and cfg.interpolation == _lib.PROFILE_INTERP_LINEAR
    assert (cfg.end, cfg.start, cfg.seed, cfg.env_base) == (_lib.PROFILE_END_WRAP, _lib.PROFILE_START_RANDOM, 7, 35)
    env = _mk(ga, ga.ProfileReferenceGenerator(prof, profile_tau=2 * tau, interpolation="hold"), seed=11)
    assert env.reference_generator._cfg.interpolation == _lib.PROFILE_INTERP_HOLD and env.reference_generator._cfg.seed == 11  # (make's seed)
    # a table per env; a list of one holder is that holder
    env = _mk(ga, [ga.ProfileReferenceGenerator(np.zeros((5, 4, 2)))])
    cfg = env.reference_generator._cfg
    assert (cfg.n_ref, cfg.n_rows, cfg.per_env) == (2, 5, 1)
    # one column, another state
    env = _mk(ga, ga.ProfileReferenceGenerator(np.zeros((3, 1)), reference_states="omega"))
    assert env.reference_names == ["omega"] and env.reference_generator._cfg.n_ref == 1
    assert _lib.refprofile_state_bytes(70) == 64 + 12 * 70


def test_sharded_envs_slice_a_per_env_table():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd.distributed import make_sharded

    table = np.arange(5 * 70 * 2, dtype=np.float64).reshape(5, 70, 2) / 1000.0
    for rank, (lo, hi) in enumerate(((0, 35), (35, 70))):
        env = make_sharded("Cont-CC-PMSM-v0", 70, rank, 2, 0, reference_generator=ga.ProfileReferenceGenerator(table, start="random", seed=3), _defer_create=True)
        gen = env.reference_generator
        assert gen._cfg.env_base == lo and gen._cfg.per_env == 1 and gen.n_envs == 35
        assert np.array_equal(np.asarray(gen.holder.profiles), table[:, lo:hi])
    shared = ga.ProfileReferenceGenerator(np.zeros((5, 2)))
    env = make_sharded("Cont-CC-PMSM-v0", 70, 1, 2, 0, reference_generator=shared, _defer_create=True)
    assert env.reference_generator.holder is shared and env.reference_generator._cfg.env_base == 35
    with pytest.raises(ValueError, match="profiles"):
        make_sharded("Cont-CC-PMSM-v0", 64, 0, 2, 0, reference_generator=ga.ProfileReferenceGenerator(table), _defer_create=True)


def test_build_and_header_agree_with_the_binding():
    from gym_electric_motor_amd import _lib, build

    assert os.path.join(build.CSRC, "gemx_refprofile.hip") in build.SOURCES
    assert ("refprofile", "gemx_refprofile.hip", ["gemx_support.hpp"]) in [u[:3] for u in build.SUPPORT]
    header = open(build.HEADER).read()
    assert re.search(r"#define GEMX_ABI_VERSION 9\b", header) and _lib.ABI_VERSION == 9  # new struct and entry points only
    assert re.search(r"#define GEMX_REFPROFILE_BLOB_HEADER_BYTES (\d+)", header).group(1) == str(_lib.REFPROFILE_BLOB_HEADER_BYTES)
    for name in NEW:
        assert name in _lib.EXPORTS and re.search(rf"\bint(64_t)? {name}\(", header), name
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    m = re.search(r"typedef struct gemx_refprofile_config \{(.*?)\} gemx_refprofile_config;", header, re.S)
    fields = re.findall(r"^\s*(\w+) (\w+);", m.group(1), re.M)
    ctype = dict(int32_t=C.c_int32, uint64_t=C.c_uint64, int64_t=C.c_int64, double=C.c_double)
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.GemxRefprofileConfig._fields_)
    assert fields[0] == ("int32_t", "struct_size")
    for group, names in (("INTERP", ("HOLD", "LINEAR")), ("END", ("HOLD", "WRAP")), ("START", ("ZERO", "RANDOM"))):
        for name in names:
            value = re.search(rf"GEMX_PROFILE_{group}_{name} = (\d+)", header).group(1)
            assert int(value) == getattr(_lib, f"PROFILE_{group}_{name}")
    src = open(os.path.join(build.CSRC, "gemx_refprofile.hip")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["gemx_support.hpp"]
    # ONE row function, called by the step kernel and the rows kernel; plain C++
    assert len(re.findall(r"profile_row<R>\(P, tab", src)) == 2 and len(re.findall(r"void profile_row\(", src)) == 1
    assert "asm" not in src


def test_refusals_name_the_argument():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd import _lib

    P = ga.ProfileReferenceGenerator
    for bad in (np.zeros(5), np.zeros((5, 2, 2, 2)), 0.5):
        with pytest.raises(ValueError, match="profiles"):
            P(bad)
    with pytest.raises(ValueError, match="profiles.*MAX_REF"):
        P(np.zeros((5, _lib.MAX_REF + 1)))
    with pytest.raises(ValueError, match="profiles.*MAX_REF"):
        P(np.zeros((5, 3, _lib.MAX_REF + 1)))
    with pytest.raises(ValueError, match="profiles: T"):
        P(np.zeros((0, 2)))
    for what in ("end", "interpolation", "start"):
        for bad in ("cubic", None, 1):
            with pytest.raises(ValueError, match=what):
                P(np.zeros((5, 2)), **{what: bad})
    for bad in (0, -1e-4, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="profile_tau"):
            P(np.zeros((5, 2)), profile_tau=bad)
    with pytest.raises(ValueError, match="reference_states names a state twice"):
        P(np.zeros((5, 2)), reference_states=("i_sd", "I_sd"))
    with pytest.raises(ValueError, match="reference_states"):
        P(np.zeros((5, 2)), reference_states=("i_sd",))
    # against the system: N, the states, the default states' count
    with pytest.raises(ValueError, match=r"profiles are for N = 3 envs"):
        _mk(ga, P(np.zeros((5, 3, 2))))
    with pytest.raises(ValueError, match="reference_states"):
        _mk(ga, P(np.zeros((5, 1)), reference_states="psi_nowhere"))
    with pytest.raises(ValueError, match="profiles carry 1 columns"):
        _mk(ga, P(np.zeros((5, 1))))  # (the PMSM current-control env references two states)
    # mixed with other kinds: refused, in make() and by the list generator itself
    step = ga.StepReferenceGenerator(reference_state="i_sq")
    for mixed in ([P(np.zeros((5, 1)), reference_states="i_sd"), step], (step, P(np.zeros((5, 1)), reference_states="i_sd"))):
        with pytest.raises(ValueError, match="cannot be mixed"):
            _mk(ga, mixed)
        with pytest.raises(ValueError, match="cannot be mixed"):
            ga.BatchedMultipleReferenceGenerator(mixed)
    with pytest.raises(ValueError, match="cannot be mixed"):
        ga.SwitchedReferenceGenerator([P(np.zeros((5, 1)), reference_states="i_sd"), step])


TABLE = np.array([[0.0, 1.0], [0.25, 0.5], [0.5, 0.0], [0.75, -0.5], [1.0, -1.0]])  # T = 5


def test_restatement_hold_at_the_end():
    p = Profiles(TABLE, 2)
    got = p.rollout_shell(7)
    assert got.shape == (7, 2, 2)
    assert got[:, 0, 0].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0, 1.0] and got[:, 1, 1].tolist() == [1.0, 0.5, 0.0, -0.5, -1.0, -1.0, -1.0]
    assert p.state()["k"].tolist() == [7, 7] and p.state()["e"].tolist() == [0, 0]


def test_restatement_wrap_and_the_partner_of_the_last_row():
    p = Profiles(TABLE, 1, end="wrap")
    assert p.rollout_shell(7)[:, 0, 0].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0, 0.0, 0.25]
    # half a row per step: between row 4 (1.0, -1.0) and its partner row 0 (0.0, 1.0) the value is their mean
    p = Profiles(TABLE, 1, ratio=0.5, end="wrap")
    got = p.rollout_shell(12)[:, 0]
    assert got[:, 0].tolist() == [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0, 0.5, 0.0, 0.125]
    assert got[9].tolist() == [0.5, 0.0]
    # a start row: the profile is walked from there
    p = Profiles(TABLE, 1, end="wrap")
    p.reset(start=[3])
    assert p.rollout_shell(4)[:, 0, 0].tolist() == [0.75, 1.0, 0.0, 0.25] and p.state()["s"].tolist() == [3] and p.state()["e"].tolist() == [1]


def test_restatement_counter_after_a_done_at_row_2():
    done = np.zeros((5, 2), np.uint8)
    done[2, 0] = 1
    # the shell's order: the restart comes BEFORE row 2 is shown
    p = Profiles(TABLE, 2)
    got = p.rollout_shell(5, done)
    assert got[:, 0, 0].tolist() == [0.0, 0.25, 0.0, 0.25, 0.5] and got[:, 1, 0].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert p.state()["k"].tolist() == [3, 5] and p.state()["e"].tolist() == [1, 0]
    # rollout: AFTER it
    p = Profiles(TABLE, 2)
    got = p.rollout(5, done)
    assert got[:, 0, 0].tolist() == [0.0, 0.25, 0.5, 0.0, 0.25]
    assert p.state()["k"].tolist() == [2, 5] and p.state()["e"].tolist() == [1, 0]
    # K x step == rollout_shell
    p, q = Profiles(TABLE, 2), Profiles(TABLE, 2)
    assert np.array_equal(np.stack([p.step(done[k]) for k in range(5)]), q.rollout_shell(5, done))


def test_restatement_rows_sampled_at_two_and_a_half_tau():
    ratio = 1e-4 / (2.5 * 1e-4)
    assert ratio == 0.4
    # positions 0, .4, .8, 1.2, 1.6, 2, ...: column 0 of TABLE is 0.25 * position up to row 4
    lin = Profiles(TABLE, 1, ratio=ratio).rollout_shell(12)[:, 0]
    want = np.minimum(np.arange(12) * 0.4, 4.0) * 0.25
    assert np.abs(lin[:, 0] - want).max() < 1e-15 and np.abs(lin[:, 1] - (1.0 - 2.0 * want)).max() < 1e-15
    assert lin[5].tolist() == [0.5, 0.0] and lin[10].tolist() == [1.0, -1.0] and lin[11].tolist() == [1.0, -1.0]  # (on a row, and past the end: the entries themselves)
    hold = Profiles(TABLE, 1, ratio=ratio, interpolation="hold").rollout_shell(12)[:, 0, 0]
    assert hold.tolist() == [0.0, 0.0, 0.0, 0.25, 0.25, 0.5, 0.5, 0.5, 0.75, 0.75, 1.0, 1.0]
    # wrap with zero-order hold
    hold = Profiles(TABLE, 1, ratio=ratio, interpolation="hold", end="wrap").rollout_shell(14)[:, 0, 0]
    assert hold[10:].tolist() == [1.0, 1.0, 1.0, 0.0]
    # no drift: the position of step 10 000 is s + k * ratio in one rounding each
    p = Profiles(TABLE, 1, ratio=ratio, end="wrap")
    p.k[:] = 10000
    ia, ib, w = p.rows()
    assert (int(ia[0]), int(ib[0]), float(w[0])) == (0, 1, 0.0)
