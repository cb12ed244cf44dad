"""The observation stage without a GPU (`_defer_create=True`): the metadata of the wrapped system against what the reference's own
wrappers show (tests/golden/obs_stage/metadata.json, recorded by tools/record_obs_stage.py), the resolved column program against the
numpy restatement of the reference's `simulate()` chain (tests/obs_stage_restatement.py) on the recorded raw states, argument handling,
and the header / binding agreement of the new entry points."""
import ctypes as C
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from obs_stage_restatement import simulate_chain, wrapped_names  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "obs_stage")
with open(os.path.join(GOLDEN, "metadata.json")) as _f:
    META = json.load(_f)
RECORDED = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz"))
ENV_IDS = [f"{a}-{c}-{m}-v0" for m in ("PermExDc", "SeriesDc", "ShuntDc", "ExtExDc", "PMSM", "SynRM", "SCIM", "EESM", "DFIM")
           for c in ("CC", "TC", "SC") for a in ("Finite", "Cont")]


def _holders(ga, chain):
    out = []
    for spec in chain:
        if spec["kind"] == "CurrentSumProcessor":
            out.append(ga.CurrentSumProcessor(tuple(spec["currents"]), limit=spec["limit"]))
        else:
            out.append(ga.CosSinProcessor(angle=spec["angle"], remove_angle=spec["remove_angle"]))
    return tuple(out)


def _make(ga, meta, **kw):
    wrappers = "default" if meta["built_by"] == "gem.make" else _holders(ga, meta["chain"])
    return ga.make(meta["env_id"], n_envs=4, physical_system_wrappers=wrappers, observed_states=meta["state_filter_names"], _defer_create=True, **kw)


def test_recorded_cases():
    assert len(META) == 11 and sum(m["built_by"] == "gem.make" for m in META.values()) == 6
    assert RECORDED == ["extex_sum", "pmsm_cossin", "pmsm_cossin_remove", "shunt_cont_cc"]


@pytest.mark.parametrize("case", sorted(META))
def test_metadata_matches_the_reference(case):
    import gym_electric_motor_amd as ga

    meta = META[case]
    env = _make(ga, meta)
    st = env.observation_stage
    assert st.state_names == meta["state_names"]
    assert st.state_positions == meta["state_positions"]
    for got, key in ((st.limits, "limits"), (st.nominal_state, "nominal_state"), (st.state_space.low, "state_space_low"), (st.state_space.high, "state_space_high")):
        assert np.allclose(got, meta[key], rtol=1e-12, atol=0.0), key
    assert st.state_filter == meta["state_filter"]
    assert env.state_names == [meta["state_names"][i] for i in meta["state_filter"]]
    assert np.array_equal(env.state_space.low, np.asarray(meta["state_space_low"])[meta["state_filter"]])
    assert list(env.physical_system.state_names) == meta["inner_state_names"]  # (the system itself stays raw)
    assert st.state_names == wrapped_names(meta["inner_state_names"], meta["chain"])
    # ONE shape everywhere, simulate()'s -- the reference's reset() of a remove_angle processor hands out one column more
    assert st.n_post == len(meta["state_filter"]) and len(st.state_names) == meta["step_state_len"]
    removes = any(s.get("remove_angle") for s in meta["chain"])
    assert meta["reset_state_len"] == meta["step_state_len"] + (1 if removes else 0)
    # the same env as a complete one: the observation space follows
    env = _make(ga, meta, reference_generator="default")
    assert env.observation_space[0].shape == (st.n_post,) and env.observation_space[1] is env.reference_space
    env = _make(ga, meta, reference_generator="default", flatten_observation=True)
    assert env.observation_space.shape == (st.n_post + len(env.reference_names),)
    assert np.array_equal(env.observation_space.low[st.n_post:], env.reference_space.low)


@pytest.mark.parametrize("case", RECORDED)
def test_program_against_the_restatement_on_recorded_states(case):
    import gym_electric_motor_amd as ga

    meta = META[case]
    d = np.load(os.path.join(GOLDEN, case + ".npz"))
    want = simulate_chain(d["raw_state"], meta["inner_state_names"], meta["chain"])
    assert np.abs(want - d["wrapped_state"]).max() <= 1e-12  # the restatement reproduces the reference's wrapped state
    assert np.abs(want[:, meta["state_filter"]] - d["observation_state"]).max() <= 1e-12
    st = _make(ga, meta).observation_stage
    got = st.evaluate(d["raw_state"])
    assert got.shape == d["observation_state"].shape and np.abs(got - want[:, meta["state_filter"]]).max() <= 1e-12
    refs = np.arange(2.0 * len(got)).reshape(len(got), 2)
    flat = ga.ObservationStage(_make(ga, meta).physical_system, st.chain, flatten=True, n_ref=2).evaluate(d["raw_state"], refs)
    assert np.array_equal(flat[:, :st.n_post], got) and np.array_equal(flat[:, st.n_post:], refs)


def test_default_wrappers_per_env_id():
    import gym_electric_motor_amd as ga

    for env_id in ENV_IDS:
        w = ga.default_physical_system_wrappers(env_id)
        if "ShuntDc" in env_id:
            assert len(w) == 1 and isinstance(w[0], ga.CurrentSumProcessor) and tuple(w[0]._currents) == ("i_a", "i_e") and w[0]._limit_name == "max"
        else:
            assert w == ()
    assert sum("ShuntDc" in e for e in ENV_IDS) == 6 and len(ENV_IDS) == 54
    with pytest.raises(KeyError):
        ga.default_physical_system_wrappers("Cont-CC-Nothing-v0")


def test_holders_keep_the_reference_arguments():
    import gym_electric_motor_amd as ga

    with pytest.raises(AssertionError):
        ga.CurrentSumProcessor(("i_a",), limit="mean")
    c = ga.CosSinProcessor()
    assert c.angle == "epsilon" and c._remove_angle is False
    # any position of the tuple; the action-side result is what it was
    from gym_electric_motor_amd.physical_system_wrappers import fold_wrappers

    chain = []
    dq = ga.DqToAbcActionProcessor.make("PMSM")
    both = fold_wrappers((ga.CosSinProcessor(), ga.DeadTimeProcessor(2), ga.CurrentSumProcessor(("i_sd", "i_sq"), limit="sum"), dq), observation_chain=chain)
    assert both == fold_wrappers((ga.DeadTimeProcessor(2), dq))
    assert chain == [("cossin", "epsilon", False), ("sum", ("i_sd", "i_sq"), "sum")]


def test_refusals():
    import gym_electric_motor_amd as ga

    mk = lambda **kw: ga.make("Cont-CC-PMSM-v0", n_envs=4, _defer_create=True, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="i_sum.*derived"):  # nested derived sources, by name
        mk(physical_system_wrappers=(ga.CurrentSumProcessor(("i_sd", "i_sq")), ga.CosSinProcessor(angle="i_sum")))
    with pytest.raises(ValueError, match="cos\\(epsilon\\).*derived"):
        mk(physical_system_wrappers=(ga.CosSinProcessor(), ga.CurrentSumProcessor(("i_sd", "cos(epsilon)"))))
    with pytest.raises(KeyError):  # unknown names: the reference's KeyError
        mk(physical_system_wrappers=(ga.CurrentSumProcessor(("i_a", "i_e")),))
    with pytest.raises(KeyError):
        mk(physical_system_wrappers=(ga.CosSinProcessor(angle="phi"),))
    with pytest.raises(KeyError):  # removed by an inner processor
        mk(physical_system_wrappers=(ga.CosSinProcessor(remove_angle=True), ga.CosSinProcessor()))
    with pytest.raises(ValueError):
        mk(observed_states=["omega", "nothing"])

    class StateNoiseProcessor:  # (class name is what fold_wrappers reads, as for the reference's own instances)
        pass

    with pytest.raises(NotImplementedError, match="NOISY state"):
        mk(physical_system_wrappers=(StateNoiseProcessor(),))

    class FluxObserver:
        pass

    with pytest.raises(NotImplementedError, match="FluxObserver"):
        mk(physical_system_wrappers=(FluxObserver(),))
    for kw in (dict(physical_system_wrappers=(ga.CosSinProcessor(),)), dict(observed_states=["omega"]), dict(flatten_observation=True)):
        with pytest.raises(ValueError, match="soa"):
            mk(obs_layout="soa", **kw)
    with pytest.raises(NotImplementedError, match="state_filter"):
        mk(state_filter=["omega"])
    with pytest.raises(ValueError, match="reward_weights"):  # reward weights on appended columns stay refused
        ga.make("Cont-CC-ShuntDc-v0", n_envs=4, _defer_create=True, physical_system_wrappers="default", reward_function=dict(reward_weights=dict(i_sum=1.0)))


def test_make_without_the_new_keywords_is_unchanged():
    import gym_electric_motor_amd as ga

    for env_id in ("Cont-CC-ShuntDc-v0", "Cont-CC-PMSM-v0"):
        env = ga.make(env_id, n_envs=4, _defer_create=True)
        ps = env.physical_system
        assert env.observation_stage is None and env.state_space is ps.state_space and env.state_names == list(ps.state_names)
        assert "i_sum" not in env.state_names
        env = ga.make(env_id, n_envs=4, reference_generator="default", _defer_create=True)
        ps = env.physical_system
        assert env.observation_stage is None and env.observation_space[0] is ps.state_space and env.observation_space[1] is env.reference_space
        assert env.state_space.shape == (len(ps.state_names),)


def test_header_and_binding_agree():
    from gym_electric_motor_amd import _lib

    spec = importlib.util.spec_from_file_location("gen_integration_sketch", os.path.join(REPO, "tools", "gen_integration_sketch.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    header = open(os.path.join(REPO, "include", "gemx.h")).read()
    consts = gen.header_constants(header)
    assert consts["GEMX_OBS_MAX_POST"] == _lib.OBS_MAX_POST == 32 and consts["GEMX_ABI_VERSION"] == _lib.ABI_VERSION == 9
    ops = re.search(r"enum \{ GEMX_OBS_COPY = (\d), GEMX_OBS_SUM = (\d), GEMX_OBS_COSPI = (\d), GEMX_OBS_SINPI = (\d) \};", header)
    assert tuple(int(g) for g in ops.groups()) == (_lib.OBS_COPY, _lib.OBS_SUM, _lib.OBS_COSPI, _lib.OBS_SINPI)
    ct = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "gemx_obsproc_entry": _lib.GemxObsprocEntry}
    for struct, cls in (("gemx_obsproc_entry", _lib.GemxObsprocEntry), ("gemx_obsproc_config", _lib.GemxObsprocConfig)):
        fields = gen.parse_struct(header, struct)
        assert [f[0] for f in cls._fields_] == [name for _, name, _ in fields], struct
        for (gn, gt), (t, name, n) in zip(cls._fields_, fields):
            assert C.sizeof(gt) == C.sizeof(ct[t]) * (n or 1), (struct, gn)
    for decl in ("int gemx_obsproc_create(const gemx_obsproc_config *cfg, int dtype, int device, gemx_obsproc **out);",
                 "int gemx_obsproc_apply(gemx_obsproc *p, const void *state_dev, const void *refs_dev, int64_t rows, void *out_dev, void *stream);",
                 "int gemx_obsproc_destroy(gemx_obsproc *p);"):
        assert decl in header
    assert {"gemx_obsproc_create", "gemx_obsproc_apply", "gemx_obsproc_destroy"} <= set(_lib.EXPORTS)
    import __graft_entry__ as g

    g.build()
    L = _lib.load()
    assert L.gemx_obsproc_apply.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    # argument errors come before any device is looked for: status GEMX_ERR_ARG and a message
    h = C.c_void_p()
    cfg = _lib.GemxObsprocConfig()
    cfg.struct_size, cfg.n_in, cfg.n_post = C.sizeof(cfg), 6, 1
    for mutate, text in ((lambda c: setattr(c.entries[0], "src", 6), "src"), (lambda c: setattr(c, "n_in", 25), "n_in"),
                         (lambda c: (setattr(c.entries[0], "op", _lib.OBS_SUM), setattr(c.entries[0], "mask", 0)), "SUM over no column"),
                         (lambda c: (setattr(c.entries[0], "op", _lib.OBS_SUM), setattr(c.entries[0], "mask", 1 << 6)), "mask")):
        bad = _lib.GemxObsprocConfig.from_buffer_copy(cfg)
        mutate(bad)
        assert L.gemx_obsproc_create(C.byref(bad), _lib.F32, 0, C.byref(h)) == -1 and text in L.gemx_last_error().decode()
    assert L.gemx_obsproc_create(None, _lib.F32, 0, C.byref(h)) == -1
    assert L.gemx_obsproc_apply(None, None, None, 0, None, None) == -1
