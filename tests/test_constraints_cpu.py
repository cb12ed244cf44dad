"""CPU-only: custom constraint sets (state names, LimitConstraint, one SquaredConstraint, "all_states").

* the oracle's custom-mask path against runs recorded from the live reference with such sets (tests/golden/constraints/, written by
  oracle/make_golden.py:main_constraints);
* the host's mapping of a `constraints=` argument onto the two bit masks, from the package's holders, bare names, "all_states" and the
  reference's own constraint objects, and its refusals;
* the default set written as objects: the config bytes of plain make(env_id) for all nine systems (the device's default / custom
  classification works on hard-coded bit positions);
* a matrix of sets meant for device runs (tests/constraint_cases.py:MATRIX), on the oracle alone: every term of every set fires, lanes
  that terminate repeatedly and lanes that never do, and how many lane-steps sit within 1e-5 of the boundary;
* the comparison helpers of tests/test_gpu_parity.py judging by a custom set's masks.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import constraint_cases as cc  # noqa: E402

import gym_electric_motor_amd as ga  # noqa: E402
from oracle import oracle as orc  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/src"


def test_fixture_inventory_and_the_directory_of_its_own():
    """Eight recorded runs over the machines the issue names, none of them visible to the tests that enrol tests/golden/*.npz."""
    import glob

    assert len(cc.FIXTURES) == 8
    metas = [cc.load_fixture(n)[1] for n in cc.FIXTURES]
    motors = {m["env_id"].split("-")[2] for m in metas}
    assert {"PermExDc", "ExtExDc", "PMSM", "EESM", "SCIM", "DFIM"} <= motors
    assert {m["env_id"].split("-")[0] for m in metas if "PMSM" in m["env_id"]} == {"Cont", "Finite"}
    assert not [f for f in glob.glob(os.path.join(cc.GOLDEN, "*.npz")) if os.path.basename(f).startswith("cs_")]
    for m in metas:
        assert isinstance(m["constraints"], list) and m["solver"] == "euler" and m["every"] == 1 and m["K"] <= 400 and m["episodic"]


@pytest.mark.parametrize("name", cc.FIXTURES)
def test_oracle_reproduces_reference_run_under_a_custom_set(name):
    """The bound of tests/test_oracle_golden.py::test_oracle_reproduces_reference_trajectory for same-solver runs: 1e-9 on normalised
    states (relative where |x| > 1), `terminated` exactly.  Each run terminates at least three times and holds an episode of more than
    50 steps, so the auto-reset and a long stretch under the set are both in it."""
    d, meta = cc.load_fixture(name)
    masks = orc.masks_from_spec(meta, meta["constraints"])
    assert masks != orc.default_masks(meta)
    p = orc.params_from_meta(meta, masks=masks)
    assert (p.limit_mask, p.squared_mask) == masks
    env = orc.OracleEnv(p)
    r = env.reset()
    assert np.abs(r - d["reset_state"]).max() < 1e-14
    obs, done = env.rollout(d["actions"], auto_reset=True)
    ref = d["states"]
    assert np.array_equal(d["state_index"], np.arange(len(ref)))
    diff = np.abs(obs - ref) / np.maximum(1.0, np.abs(ref))
    if meta["system"] in ("DoublyFedInductionMotorSystem", "SquirrelCageInductionMotorSystem"):
        # dq columns of steps that start with zero rotor flux: the reference's field angle is arctan2(rounding noise)
        bad = orc.undefined_field_angle_steps(p, d["actions"])
        assert bad.sum() <= 2 * (1 + d["terminated"].sum())
        cols = [meta["state_names"].index(c) for c in orc.DQ_COLUMNS if c in meta["state_names"]]
        diff[np.ix_(bad, cols)] = 0.0
    assert diff.max() < 1e-9, diff.max()
    assert np.array_equal(done, d["terminated"])
    ends = np.nonzero(done)[0]
    assert len(ends) >= 3 and np.diff(np.concatenate([[-1], ends, [len(done) - 1]])).max() > 50
    # the recorded flags ARE the two sub-expressions on the recorded rows
    lim, sq = cc.term_values(meta, masks, ref)
    assert np.array_equal(d["terminated"], (lim > 1.0) | (sq > 1.0))


def test_params_from_meta_default_behaviour_is_unchanged():
    for name in ("pmsm_epi_held_tau1e-4_euler", "eesm_cont_epi_held_euler", "shunt_cont_epi_held_euler", "permexdc_free_held_euler"):
        _, meta = orc.load_golden(name)
        p = orc.params_from_meta(meta)
        want = orc.default_masks(meta) if meta["episodic"] else (0, 0)
        assert (p.limit_mask, p.squared_mask) == want
        q = orc.params_from_meta(meta, episodic=False, masks=(3, 4))
        assert (q.limit_mask, q.squared_mask) == (0, 0)


def _system(meta, constraints):
    return ga.make(meta["env_id"], n_envs=2, constraints=constraints, _defer_create=True).physical_system


@pytest.mark.parametrize("name", cc.FIXTURES)
def test_host_masks_from_holders_and_bare_names(name):
    _, meta = cc.load_fixture(name)
    want = orc.masks_from_spec(meta, meta["constraints"])
    ps = _system(meta, cc.package_constraints(ga, meta["constraints"]))
    assert list(ps.state_names) == meta["state_names"]
    assert (ps._cfg.limit_mask, ps._cfg.squared_mask) == want
    # every limit term as bare names gives the same limit mask
    bare = tuple(n for c in meta["constraints"] if c["kind"] != "squared" for n in c["states"])
    assert _system(meta, bare)._cfg.limit_mask == want[0]


def test_host_masks_all_states():
    for env_id in ("Cont-CC-PermExDc-v0", "Cont-CC-PMSM-v0", "Finite-CC-DFIM-v0"):
        meta = dict(env_id=env_id)
        full = (1 << len(_system(meta, ()).state_names)) - 1
        for c in (("all_states",), (ga.LimitConstraint(),), (ga.LimitConstraint(("all_states",)),), (ga.LimitConstraint("all_states"), "omega")):
            ps = _system(meta, c)
            assert (ps._cfg.limit_mask, ps._cfg.squared_mask) == (full, 0), (env_id, c)


def test_host_refuses_what_the_kernels_do_not_evaluate():
    meta = dict(env_id="Cont-CC-PMSM-v0")
    with pytest.raises(ValueError, match="one SquaredConstraint"):
        _system(meta, (ga.SquaredConstraint(("i_sd", "i_sq")), ga.SquaredConstraint(("u_sd", "u_sq"))))
    for unknown in (("i_x",), (ga.LimitConstraint(("i_sd", "psi")),), (ga.SquaredConstraint(("i_sd", "i")),)):
        with pytest.raises(ValueError, match="not a state"):
            _system(meta, unknown)
    for foreign in ((object(),), (lambda state: 0.0,), (3,)):
        with pytest.raises(ValueError, match="cannot be evaluated"):
            _system(meta, foreign)
    # columns a wrapper appends behind the system's own are no states of the system
    for appended in ("i_sum", "cos(epsilon)"):
        with pytest.raises(ValueError, match="not a state"):
            ga.make("Cont-CC-ShuntDc-v0", n_envs=2, physical_system_wrappers="default", constraints=(appended,), _defer_create=True)


DEFAULT_AS_OBJECTS = {"PermExDc": lambda: (ga.LimitConstraint(("i",)),), "SeriesDc": lambda: (ga.LimitConstraint(("i",)),),
                      "ShuntDc": lambda: ("i_a", "i_e"), "ExtExDc": lambda: (ga.LimitConstraint(("i_a", "i_e")),),
                      "PMSM": lambda: (ga.SquaredConstraint(("i_sq", "i_sd")),), "SynRM": lambda: (ga.SquaredConstraint(("i_sq", "i_sd")),),
                      "SCIM": lambda: (ga.SquaredConstraint(("i_sq", "i_sd")),), "DFIM": lambda: (ga.SquaredConstraint(("i_sq", "i_sd")),),
                      "EESM": lambda: (ga.SquaredConstraint(("i_sq", "i_sd")), ga.LimitConstraint(("i_e",)))}


@pytest.mark.parametrize("motor", sorted(DEFAULT_AS_OBJECTS))
@pytest.mark.parametrize("prefix", ["Cont-CC", "Finite-SC"])
def test_default_set_written_out_gives_the_plain_config_and_the_hard_coded_bits(motor, prefix):
    """The device classifies a set as the env's default (fast path) by bit positions 2, 3, 5, 6 and 7 (gemx_capi.hip, fill_params): the
    armature / excitation currents of the DC machines sit at 2 (and 3), i_sd / i_sq of every three-phase system at 5 / 6, the EESM's i_e
    at 7 -- held here against the state names of all nine systems."""
    env_id = f"{prefix}-{motor}-v0"
    plain = ga.make(env_id, n_envs=2, _defer_create=True).physical_system
    written = ga.make(env_id, n_envs=2, constraints=DEFAULT_AS_OBJECTS[motor](), _defer_create=True).physical_system
    assert bytes(written._cfg) == bytes(plain._cfg)
    names = list(plain.state_names)
    lim, sq = plain._cfg.limit_mask, plain._cfg.squared_mask
    if motor in ("PermExDc", "SeriesDc"):
        assert names[2] == "i" and (lim, sq) == (1 << 2, 0)
    elif motor in ("ShuntDc", "ExtExDc"):
        assert names[2:4] == ["i_a", "i_e"] and (lim, sq) == ((1 << 2) | (1 << 3), 0)
    else:
        assert names[5:7] == ["i_sd", "i_sq"] and sq == (1 << 5) | (1 << 6)
        assert lim == ((1 << 7) if motor == "EESM" else 0) and (motor != "EESM" or names[7] == "i_e")


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="reference tree only exists in the build container")
def test_host_masks_from_the_reference_constraint_objects():
    """The reference's own LimitConstraint / SquaredConstraint instances (private attribute names) give the masks of the stored sets.  In
    a subprocess, so that the reference / gymnasium stand-in imports do not leak into this session."""
    code = r'''
import os, sys
os.environ["MPLBACKEND"] = "Agg"
sys.path[:0] = [%r, %r, %r, %r]
from gym_electric_motor.constraints import LimitConstraint, SquaredConstraint
import gym_electric_motor_amd as ga
import constraint_cases as cc
from oracle import oracle as orc
for name in cc.FIXTURES:
    _, meta = cc.load_fixture(name)
    cons = []
    for c in meta["constraints"]:
        cons += [LimitConstraint(tuple(c["states"]))] if c["kind"] == "limit" else [SquaredConstraint(tuple(c["states"]))] if c["kind"] == "squared" else list(c["states"])
    ps = ga.make(meta["env_id"], n_envs=2, constraints=tuple(cons), _defer_create=True).physical_system
    assert (ps._cfg.limit_mask, ps._cfg.squared_mask) == orc.masks_from_spec(meta, meta["constraints"]), name
ps = ga.make("Cont-CC-PMSM-v0", n_envs=2, constraints=(LimitConstraint(),), _defer_create=True).physical_system
assert ps._cfg.limit_mask == (1 << len(ps.state_names)) - 1
plain = ga.make("Cont-CC-EESM-v0", n_envs=2, _defer_create=True).physical_system
theirs = ga.make("Cont-CC-EESM-v0", n_envs=2, constraints=(SquaredConstraint(("i_sq", "i_sd")), LimitConstraint(("i_e",))), _defer_create=True).physical_system
assert bytes(plain._cfg) == bytes(theirs._cfg)
try:
    ga.make("Cont-CC-PMSM-v0", n_envs=2, constraints=(SquaredConstraint(("i_sd",)), SquaredConstraint(("i_sq",))), _defer_create=True)
except ValueError:
    print("OK")
''' % (os.path.join(REPO, "oracle", "gymnasium_standin"), REF_SRC, REPO, os.path.join(REPO, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, out.stderr[-3000:]


@pytest.mark.parametrize("case_id", sorted(cc.MATRIX))
def test_matrix_case_on_the_oracle_alone(case_id):
    """What a device run of the case against the oracle relies on, established without a device: the env builds with the oracle's limits and masks;
    every term of the set fires on some lane; some lanes terminate repeatedly and some never; and the count of lane-steps within 1e-5 of
    the boundary -- each one a step where an fp32 device may decide `done` the other way, which ends that lane's comparison.  With ONE
    sampled lane allowed to end so and 90 % of the lane-steps to be compared, more than 5 such steps among the 21 000 of a case would
    make it a gamble: such a set is replaced, not exempted.  A column that IS the constant 1.0 on every row (`u_sup` under an
    ideal supply, in "all_states") sits on the boundary by construction and moves on neither side: it is counted apart."""
    from test_gpu_parity import _make_from_meta

    run = cc.oracle_run(case_id)
    meta, masks = run["meta"], run["masks"]
    ps = _make_from_meta(meta, 2, solver="euler", _defer_create=True).physical_system
    assert list(ps.state_names) == meta["state_names"]
    assert np.allclose(ps.limits, meta["limits"], rtol=1e-13, atol=0)
    assert (ps._cfg.limit_mask, ps._cfg.squared_mask) == masks
    if cc.MATRIX[case_id].get("default_bits"):
        assert bytes(ps._cfg) == bytes(_make_from_meta(dict(meta, constraints="default"), 2, solver="euler", _defer_create=True).physical_system._cfg)
    c = cc.oracle_counts(run)
    const = [i for i in range(run["rows"].shape[2]) if (masks[0] >> i & 1) and (np.abs(run["rows"][:, :, i]) == 1.0).all()]
    moving = (masks[0] & ~sum(1 << i for i in const), masks[1])
    lim, sq = cc.term_values(meta, moving, run["rows"])
    near_moving = int((np.abs(np.maximum(lim, sq) - 1.0) < cc.DONE_BAND).sum())
    print(f"{case_id}: {c['terminations']} terminations, {c['lanes_without']} lanes without one, {c['lanes_repeated']} with two or more, fired {c['fired']}, "
          f"|value - 1| < 1e-5 on {c['near']} of {c['lane_steps']} lane-steps ({near_moving} without the constant columns {[meta['state_names'][i] for i in const]})")
    assert c["fired"] == c["want"], "a dead term proves nothing"
    assert near_moving <= 5
    assert c["lanes_without"] >= 1 and c["lanes_repeated"] >= 1


@pytest.mark.parametrize("case_id, default_differs", [("pmsm_sc_sq_idq_lim_omega", True), ("pmsm_dq_space_sq_iab_lim_isd", True),
                                                      ("pmsm_fin_dead_time_lim_ia_ib_ic", True), ("permexdc_all_states", False)])
def test_lane_comparison_helpers_judge_by_the_custom_set(case_id, default_differs):
    """Plumbing of the test helpers only -- no kernel is involved: `_lanes_against_oracle(masks=...)` and `_constraint_margin(masks=...)`
    (tests/test_gpu_parity.py) given the oracle's own rows rounded to fp32.  Under the set's masks every lane is compared over the whole
    run without a flip; a `done` flag that is wrong at one step clear of the boundary fails, also under "all_states", where the constant
    `u_sup` column must not put the margin to zero; and judged by the env's DEFAULT masks the same rows fail."""
    from test_gpu_parity import LANE_SAMPLE, _constraint_margin, _lanes_against_oracle

    run = cc.oracle_run(case_id)
    meta, masks, a_np = run["meta"], run["masks"], run["actions"]
    rows, done = run["rows"].astype(np.float32).astype(np.float64), run["done"]
    K = a_np.shape[0]
    sol, nd = ga.EulerSolver(), 2 if a_np.shape[2] > 1 else 1
    sample = list(LANE_SAMPLE)
    stats = []
    worst = _lanes_against_oracle(case_id, meta, a_np, rows, done, sample, sol, "float32", nd, masks=masks, stats=stats)
    assert worst < 1e-6 and [s["compared"] for s in stats] == [K] * len(sample) and not any(s["flip"] for s in stats)
    assert sum(s["terminations"] for s in stats) == int(done[:, sample].sum()) > 0
    # the margin is the issue's expression on the oracle's rows, over the columns that move
    names = meta["state_names"]
    moving = masks
    if "all_states" in case_id:
        assert (run["rows"][:, :, names.index("u_sup")] == 1.0).all()
        moving = (masks[0] & ~(1 << names.index("u_sup")), masks[1])
    margin = np.abs(np.maximum(*cc.term_values(meta, moving, run["rows"])) - 1.0)
    for j in sample:
        dj = dict(states=run["rows"][:, j], terminated=done[:, j], state_index=np.arange(K))
        assert np.array_equal(_constraint_margin(dict(meta, every=1), dj, masks=masks), margin[:, j])
    # one wrong flag at a step that neither violates nor is near the boundary
    lane = next(j for j in sample if ((margin[:, j] >= cc.DONE_BAND) & ~done[:, j]).any())
    k = int(np.argmax((margin[:, lane] >= cc.DONE_BAND) & ~done[:, lane]))
    wrong = done.copy()
    wrong[k, lane] = True
    with pytest.raises(AssertionError, match="done mask differs"):
        _lanes_against_oracle(case_id, meta, a_np, rows, wrong, [lane], sol, "float32", nd, masks=masks)
    # where the default set decides a sampled row the other way, the same rows fail under it (PermExDc under "all_states": on the
    # sampled lanes only the default's own `i` fires, so the two sets agree there -- stated in the parametrisation, not found out here)
    lim_d, sq_d = cc.term_values(meta, orc.default_masks(meta), run["rows"][:, sample])
    assert np.array_equal(done[:, sample], (lim_d > 1.0) | (sq_d > 1.0)) != default_differs
    if default_differs:
        with pytest.raises(AssertionError):
            _lanes_against_oracle(case_id, meta, a_np, rows, done, sample, sol, "float32", nd)


def test_ideal_supply_column_is_exactly_one_in_fp32():
    """The device forms the `u_sup` column as fl32(u_sup) * r, r the reciprocal limit.  With r = fl32(1 / u_sup) the product is exactly
    1.0f for every supply voltage of the 54 envs and of the fixtures and for every integer voltage, but ABOVE 1 for one in twenty arbitrary
    voltages (fl32(u_sup) may lie above u_sup): such an env under "all_states" would terminate at once where the reference, whose column
    is 1.0, never does.  gemx_capi.hip (fill_params) therefore steps r down while the product exceeds 1 -- restated here: one step
    always suffices, the column then is 1.0f or one ulp below, and the voltages in use keep r as it was."""
    import glob
    import json

    used = {float(json.loads(str(np.load(f)["meta"]))["u_nominal"]) for f in glob.glob(os.path.join(cc.GOLDEN, "*.npz")) + glob.glob(os.path.join(cc.FIXTURE_DIR, "*.npz"))
            if "meta" in np.load(f).files}
    assert {60.0, 300.0, 420.0} <= used
    assert np.float32(300.2) * np.float32(1.0 / 300.2) > np.float32(1.0)  # (the voltage of the matrix case `pmsm_all_states_300v2`)
    for u in sorted(used):
        assert np.float32(u) * np.float32(1.0 / u) == np.float32(1.0), u
        assert u * (1.0 / u) == 1.0, u
    rng = np.random.default_rng(0)
    ints, anyu = np.arange(1, 2001, dtype=np.float64), rng.uniform(1.0, 2000.0, 100000)
    assert (ints.astype(np.float32) * (1.0 / ints).astype(np.float32) <= np.float32(1.0)).all()
    uf, r = anyu.astype(np.float32), (1.0 / anyu).astype(np.float32)
    above = uf * r > np.float32(1.0)
    assert 0.01 < above.mean() < 0.2  # (the plain reciprocal is not good enough)
    r = np.where(above, np.nextafter(r, np.float32(0.0)), r)
    col = uf * r
    assert (col <= np.float32(1.0)).all() and (col >= np.float32(1.0) - np.float32(2.0 ** -23)).all()
