"""GPU tests of custom constraint sets (run with `-m gpu` on an MI355X): every kernel that decides `done` for a set that is not the
env's default -- constraint_done() in the single-wave kernel and in step_kernel, and the pipelined kernel's own copy of the expressions
-- against the fp64 oracle and against runs recorded from the live reference (tests/golden/constraints/).

Tolerances are the parity contract's (tests/parity_contract.py): fp32 within TOL_FP32 of the oracle, column-scaled
as compare_trajectory does; fp64 with the same integrator within 1e-7; the induction machines' dq columns by their conditioning; dead-time
lanes by SIGN_MARGIN.  A `done` flip is accepted only where the oracle's margin |max(max_i |x_i|, sum x_i^2) - 1| at that step is below
DONE_MARGIN; that lane's comparison ends there, and over all compared lanes of a case at most ONE lane may end so and at least 90 % of
the lane-steps must be compared.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import constraint_cases as cc  # noqa: E402
from parity_contract import DONE_MARGIN, TOL_FP32  # noqa: E402
from test_gpu_parity import LANE_SAMPLE, _lanes_against_oracle, _make_from_meta, _undefined_dq_steps_checked, compare_trajectory  # noqa: E402

TOL_FP64 = 1e-7       # the fp64 build against the oracle / the recording with the same integrator (as _lanes_against_oracle holds it)
MAX_FLIP_LANES = 1    # compared lanes of a case that may end at a done flip
MIN_COMPARED = 0.9    # share of the compared lanes' steps that must be compared

ROUTES = {
    # route: (GEMX_PIPE, dtype, kernel named by last_launch())
    "pipelined": ("1", "float32", "advance_pipe_kernel"),
    "single_wave": ("0", "float32", "advance_kernel"),
    "k_steps": ("1", "float32", "step_kernel"),        # K x simulate(): step_kernel's constraint_done() call
    "single_wave_fp64": (None, "float64", "advance_kernel"),
}


def _solver(ga, name):
    return {"euler": ga.EulerSolver, "rk4x3": lambda: ga.RK4Solver(nsteps=3), "scipy": ga.ScipyOdeSolver}[name]()


def _device_run(monkeypatch, meta, a_np, route, solver="euler", **extra):
    """The env of `meta` with a_np [K, N, A] through one route -> (obs [K, N, S] float64, done [K, N] bool, last_launch, solver object)."""
    import torch

    import gym_electric_motor_amd as ga

    pipe, dtype, kernel = ROUTES[route]
    if pipe is None:
        monkeypatch.delenv("GEMX_PIPE", raising=False)
    else:
        monkeypatch.setenv("GEMX_PIPE", pipe)
    K, n = a_np.shape[:2]
    env = _make_from_meta(meta, n, solver=_solver(ga, solver), dtype=dtype, auto_reset=True, **extra)
    ps = env.physical_system
    assert list(ps.state_names) == meta["state_names"] and np.allclose(ps.limits, meta["limits"], rtol=1e-13, atol=0)
    if ps._discrete:
        a = torch.as_tensor((a_np[:, :, 0] if a_np.shape[2] == 1 else a_np).astype(np.uint8)).cuda().contiguous()
    else:
        a = torch.as_tensor(a_np).to(ps._tdtype).cuda().contiguous()
    if route == "k_steps":
        rows, flags = [], []
        for k in range(K):
            rows.append(ps.simulate(a[k]).clone())
            flags.append(ps.done.clone())
        obs, done = torch.stack(rows), torch.stack(flags)
    else:
        obs, done = env.rollout(a)
    torch.cuda.synchronize()
    ll = ps.last_launch()
    sol_obj = ps._ode_solver
    obs, done = obs.double().cpu().numpy(), done.cpu().numpy().astype(bool)
    env.close()
    return obs, done, ll, sol_obj, kernel


def _caps(what, stats):
    flips = [s for s in stats if s["flip"]]
    compared, total = sum(s["compared"] for s in stats), sum(s["steps"] for s in stats)
    worst = max(stats, key=lambda s: s["rel"])
    print(f"{what}: worst rel err {worst['rel']:.2e} ({worst['col']}, lane {worst['lane']}); {len(flips)} lanes end at a flip"
          f"{[s['done'] for s in flips]}; {compared}/{total} lane-steps compared ({100.0 * compared / total:.1f} %)")
    assert len(flips) <= MAX_FLIP_LANES, (what, [s["done"] for s in flips])
    assert compared >= MIN_COMPARED * total, (what, compared, total)


# ------------------------------------------------------------------------------------------------------------------ recorded runs
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", cc.FIXTURES)
def test_recorded_custom_set_runs_through_every_kernel(name, route, monkeypatch):
    """A run recorded from the live reference under a custom set, on 70 envs: lanes 0, 64 and 69 carry the recorded actions, agree bit
    for bit and reproduce the recording episode by episode; the lanes of LANE_SAMPLE carry their own random streams and are held against
    the oracle under the same set.  Through the pipelined kernel, the single-wave kernel, K single steps (step_kernel) and the fp64 build."""
    import zlib

    from oracle import oracle as orc

    d, meta = cc.load_fixture(name)
    masks = orc.masks_from_spec(meta, meta["constraints"])
    acts = d["actions"]
    K, n = acts.shape[0], cc.N_ENVS
    a_np = np.repeat(acts.reshape(K, 1, -1), n, axis=1).astype(np.float64)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    recorded = [0, 64, n - 1]
    others = [j for j in range(n) if j not in recorded]
    nvec = cc.n_actions(meta)
    if nvec is not None:
        for c, nv in enumerate(nvec):
            a_np[:, others, c] = rng.integers(0, nv, (K, len(others)))
    else:
        a_np[:, others, :] = rng.uniform(-1.0, 1.0, (K, len(others), a_np.shape[2]))
    obs, done, ll, sol_obj, kernel = _device_run(monkeypatch, meta, a_np, route)
    dtype = ROUTES[route][1]
    assert kernel in ll and (kernel != "advance_kernel" or "advance_pipe_kernel" not in ll), ll
    for j in recorded[1:]:
        assert np.array_equal(obs[:, 0], obs[:, j]) and np.array_equal(done[:, 0], done[:, j]), j
    tol = TOL_FP32 if dtype == "float32" else TOL_FP64
    names = meta["state_names"]
    if meta["supply"] != "RCVoltageSupply" and masks[0] >> names.index("u_sup") & 1:
        assert (obs[:, :, names.index("u_sup")] == 1.0).all()  # ("all_states": the constant column is exactly 1.0 and excuses no flip)
    obs0 = obs[:, 0].copy()
    if meta["system"] == "DoublyFedInductionMotorSystem":
        obs0 = _undefined_dq_steps_checked(meta, d, obs0, masks=masks)
    info = {}
    rel, _, col, dmsg = compare_trajectory(meta, d, obs0, done[:, 0], masks=masks, info=info)
    assert rel < tol, (name, route, rel, col, dmsg)
    stats = [dict(lane=0, rel=rel, col=col, compared=info["compared"], flip=info["flip_step"] is not None, done=dmsg, steps=K)]
    lanes = [j for j in LANE_SAMPLE if j not in recorded]
    lane_stats = []
    worst = _lanes_against_oracle(name, meta, a_np, obs, done, lanes, sol_obj, dtype, acts.ndim, masks=masks, stats=lane_stats)
    assert worst is not None and len(lane_stats) == len(lanes)
    stats += [dict(s, steps=K) for s in lane_stats]
    print(f"{name} [{route}] {ll.split(' grid')[0]}: recording {dmsg}; oracle lanes {sum(s['terminations'] for s in lane_stats)} terminations")
    _caps(f"{name} [{route}]", stats)


# -------------------------------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("case_id", sorted(cc.MATRIX))
def test_matrix_of_sets_against_the_oracle(case_id, monkeypatch):
    """One set of tests/constraint_cases.py:MATRIX on per-lane random streams (N = 70, K = 300, random for 40 steps and then held, every
    third lane calm): the pipelined and the single-wave kernel agree bit for bit, the lanes of LANE_SAMPLE are held against the fp64 oracle
    under the same set, the run holds lanes that terminate repeatedly and lanes that never do, and every term of the set fires on the
    device at a step where the oracle -- in phase with that lane up to there -- fires it too."""
    case = cc.MATRIX[case_id]
    run = cc.oracle_run(case_id)
    meta, masks, a_np = run["meta"], run["masks"], run["actions"]
    K, n = a_np.shape[:2]
    solver = case.get("solver", "euler")
    obs, done, ll, sol_obj, _ = _device_run(monkeypatch, meta, a_np, "pipelined", solver=solver)
    obs1, done1, ll1, _, _ = _device_run(monkeypatch, meta, a_np, "single_wave", solver=solver)
    assert "advance_pipe_kernel" in ll, ll
    assert "advance_kernel" in ll1 and "advance_pipe_kernel" not in ll1, ll1
    assert np.array_equal(obs, obs1) and np.array_equal(done, done1)
    assert np.isfinite(obs).all()
    names = meta["state_names"]
    if case.get("default_bits"):  # the env's default written as objects: the bits of the same env built without naming a set
        obs2, done2, _, _, _ = _device_run(monkeypatch, dict(meta, constraints="default"), a_np, "pipelined", solver=solver)
        assert np.array_equal(obs, obs2) and np.array_equal(done, done2)
    if meta["supply"] != "RCVoltageSupply" and masks[0] >> names.index("u_sup") & 1:
        # an ideal supply's column is the constant 1.0 on the oracle; the device's must be exactly that, so it can never violate -- and
        # the margin that judges a flip leaves the constant column out (_constraint_margin): nothing is excused by it
        assert (obs[:, :, names.index("u_sup")] == 1.0).all()
    # both kinds of lane, on the device
    per_lane = done.sum(axis=0)
    assert (per_lane >= 2).any(), "no lane terminates repeatedly"
    assert (per_lane == 0).any(), "every lane terminated"
    # every term fired on the device where the oracle fires it
    lim, sq = cc.term_values(meta, masks, run["rows"])
    in_phase = np.cumsum(done != run["done"], axis=0) == 0  # (up to and including step k the two done masks of the lane agree)
    fired = {}
    for term, val, on in (("limit", lim, masks[0]), ("squared", sq, masks[1])):
        if on:
            fired[term] = int((in_phase & done & run["done"] & (val > 1.0)).sum())
            assert fired[term] > 0, (case_id, term, "never fired on the device in phase with the oracle: a dead term proves nothing")
    stats = []
    worst = _lanes_against_oracle(case_id, meta, a_np, obs, done, list(LANE_SAMPLE), sol_obj, "float32", 2 if a_np.shape[2] > 1 else 1, masks=masks, stats=stats)
    assert worst is not None and len(stats) == len(LANE_SAMPLE)
    print(f"{case_id} {ll.split(' grid')[0]} | {ll1.split(' grid')[0]}: {int(done.sum())} terminations (oracle {int(run['done'].sum())}), "
          f"{int((per_lane == 0).sum())} lanes without one, terms fired {fired}, all constraint terms fired")
    _caps(case_id, [dict(s, steps=K) for s in stats])
    print(f"{case_id}: within the caps")


def _own_rows_decide_done(meta, masks, obs, done):
    """`done` against the set's expression recomputed in fp64 from the device's OWN stored rows, outside a band of DONE_MARGIN around 1."""
    lim, sq = cc.term_values(meta, masks, obs)
    val = np.maximum(lim, sq)
    clear = np.abs(val - 1.0) >= DONE_MARGIN
    assert np.array_equal(done[clear], (val > 1.0)[clear]), int((done[clear] != (val > 1.0)[clear]).sum())
    return lim, sq, int((~clear).sum())


def test_custom_set_beside_random_initial_states(monkeypatch):
    """Random initial states (every env restarts from its own draw): no oracle run exists, so the device is held against itself -- the
    same bits with the pipelined kernel switched on and off, whichever kernel serves the launch -- and `done` against the set's
    expression on the device's own rows; both terms fire, lanes terminate repeatedly and lanes never do."""
    from oracle import oracle as orc

    meta = cc.case_meta("pmsm_sc_sq_idq_lim_omega")
    meta["overrides"] = dict(motor=dict(meta["overrides"]["motor"], motor_initializer=dict(random_init="uniform")))
    masks = orc.masks_from_spec(meta, meta["constraints"])
    a_np = cc.oracle_run("pmsm_sc_sq_idq_lim_omega")["actions"]
    obs, done, ll, _, _ = _device_run(monkeypatch, meta, a_np, "pipelined", seed=5)
    obs1, done1, ll1, _, _ = _device_run(monkeypatch, meta, a_np, "single_wave", seed=5)
    assert np.array_equal(obs, obs1) and np.array_equal(done, done1)
    assert np.isfinite(obs).all()
    lim, sq, n_band = _own_rows_decide_done(meta, masks, obs, done)
    per_lane = done.sum(axis=0)
    print(f"random initial states {ll.split(' grid')[0]} | {ll1.split(' grid')[0]}: {int(done.sum())} terminations, {int((per_lane == 0).sum())} lanes without one, "
          f"limit fired {int((done & (lim > 1)).sum())}, squared fired {int((done & (sq > 1)).sum())}, {n_band} lane-steps inside the band")
    assert (done & (lim > 1.0)).any() and (done & (sq > 1.0)).any()
    assert (per_lane >= 2).any() and (per_lane == 0).any()
    i_sd = meta["state_names"].index("i_sd")
    after = np.nonzero(done[:-1, 1])[0] + 1  # rows after a termination of lane 1: one step from a DRAWN state, not from zero current
    assert len(after) >= 2 and len({float(obs[k, 1, i_sd]) for k in after}) > 1


def test_empty_set_never_terminates(monkeypatch):
    meta = dict(cc.case_meta("pmsm_lim_ia_ib_torque"), constraints=[])
    a_np = cc.oracle_run("pmsm_lim_ia_ib_torque")["actions"]
    for route in ("pipelined", "single_wave", "k_steps"):
        obs, done, ll, _, kernel = _device_run(monkeypatch, meta, a_np[:60], route)
        assert kernel in ll, ll
        assert not done.any() and np.isfinite(obs).all()
    assert np.abs(obs[:, :, meta["state_names"].index("i_a")]).max() > 1.0  # (the run does leave the limits the other cases stop at)


# ------------------------------------------------------------------------------------------------------------- the complete env
def test_complete_env_rollout_equals_k_steps_under_a_mixed_custom_set():
    """rollout_complete(actions) == K x step() bit for bit -- state, references, reward, done -- under a mixed custom set: `terminated`
    drives the auto-reset, the reward's violation value and the reference generators' restarts there."""
    import torch

    import gym_electric_motor_amd as ga
    from oracle import oracle as orc
    from test_gpu_complete_rollout import SEED, _actions, _same, _steps

    env_id, n, K = "Cont-CC-PMSM-v0", 37, 64
    spec = [cc.S("i_sd", "i_sq"), cc.L("i_a", "torque")]

    def mk():
        return ga.make(env_id, n_envs=n, reference_generator="default", seed=SEED, constraints=cc.package_constraints(ga, spec))

    a, b = mk(), mk()
    assert isinstance(a, ga.CompleteBatchedElectricMotorEnv)
    a.reset(), b.reset()
    acts = _actions(a.physical_system, K, n)
    got = a.rollout_complete(acts)
    want = _steps(torch, b, acts)
    torch.cuda.synchronize()
    _same(torch, got, want, f"{env_id} mixed custom set N={n} K={K}")
    done = got[3].bool()
    assert bool(done[1:K - 1].any()), "no termination strictly inside the run"
    assert bool((~done.any(dim=0)).any()), "every env terminated"
    assert bool((got[2][done] == a.reward_config.violation_reward).all())
    meta = dict(state_names=list(a.physical_system.state_names))
    masks = orc.masks_from_spec(meta, spec)
    assert (a.physical_system._cfg.limit_mask, a.physical_system._cfg.squared_mask) == masks
    lim, sq, n_band = _own_rows_decide_done(meta, masks, got[0].double().cpu().numpy()[:, :, :len(meta["state_names"])], done.cpu().numpy())
    print(f"complete env {env_id} under {spec}: {int(done.sum())} terminations, {int((~done.any(dim=0)).sum())} envs without one, "
          f"limit above 1 on {int((lim > 1).sum())} rows, squared on {int((sq > 1).sum())}, {n_band} inside the band")
    a.close(), b.close()
