"""Per-env parameter tables (csrc/gemx_envparams.hip, gemx_set_env_params): every per-env kernel unit, every table field, every lane.

tests/test_gpu_env_parameters.py gives env e the parameter set e % 4 of seven envs.  That leaves four gaps, closed here with the cases,
families and conditions of tests/env_parameters_cases.py (N = 197, K = 48; the conditions are asserted from the fp64 oracle alone in
tests/test_env_parameters_cpu.py):

1. A table read at the wrong env index.  BLOCK = 64 is a multiple of 4, so with set = env % 4 a kernel that read the table by the lane within
   its block (threadIdx.x), or at an index off by any multiple of 4, would still hand every lane a column of ITS set, and the C ABI could
   write `tab[i * N + e]` at such an index as well: every bit-for-bit assertion of that module would hold.  Here every env is its own machine
   (family "lanes": no two envs share a value of any field that is overridden), and
     * the table is read back and compared, field by field and env by env with exact equality, with a float64 host restatement of
       derive_machine_params rounded once to fp32 -- the C ABI's indexing, no kernel in the loop;
     * every lane is compared with the fp64 oracle run with that lane's machine (rollout and step x K), and lanes 0, 63, 64, 65 and 196
       (block edges, the tail) bit for bit with uniform handles of n_envs = 197 built with their machine: a read by the lane within the block
       leaves only lanes 0 and 63 right, a read off by a constant leaves none.
2. Units never launched with a table.  One case per remaining unit; the launch string asserted names the unit (sys=, conv=):

       unit (system, converter unit)   case                                           test
       (1,2)  SYNC, continuous B6      Cont-SC-PMSM-v0, Cont-SC-SynRM-v0 (no psi_p)   test_lane_equals_its_uniform_handle
       (2,1)  SCIM, finite B6          Finite-SC-SCIM-v0                              "
       (0,3)  PermExDc, finite 4QC     Finite-CC-PermExDc-v0 (constant speed)         "
       (3,3)  SeriesDc, finite 4QC     Finite-SC-SeriesDc-v0                          "
       (4,0)  ShuntDc, continuous 4QC  Cont-SC-ShuntDc-v0                             "
       (4,3)  ShuntDc, finite 4QC      Finite-SC-ShuntDc-v0                           "
       (5,4)  ExtExDc, continuous      Cont-SC-ExtExDc-v0                             "
       (5,5)  ExtExDc, finite          Finite-CC-ExtExDc-v0 (constant speed)          "
       (6,7)  EESM, finite             Finite-SC-EESM-v0                              "
       (7,8)  DFIM, continuous         Cont-SC-DFIM-v0                                "
       (6,11) EESM, dq processor       dqproc-EESM  (DqToAbcActionProcessor('EESM'))  "
       (2,10) SCIM, dq space           dq-SCIM  (control_space='dq')                  "

   The other seven -- (0,0), (1,1), (2,2), (6,6), (7,9), (3,0), (1,10) -- are asserted by tests/test_gpu_env_parameters.py
   (test_unit_of_every_case_is_named_by_its_launch below repeats it for all of them).  No unit is out of reach: control_space='dq' of a SCIM
   rotates by the rotor-flux angle of the system's own state and needs no FluxObserver.
3. Fields that were constant across lanes.  Family "fields" varies a, b, c, psi_p / psi_e and j_rotor between the sets; its set 1 has a = 0,
   so lanes with and without a kink share every wave under the split-kink solver (test_lanes_with_and_without_a_kink_share_a_wave).
4. No independent check of the polynomial-load cases; two branches never run.  Every case and family is compared with the fp64 oracle at the
   parity contract's tolerance, done masks exact; obs_layout='soa' and auto_reset=False each run with a table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import env_parameters_cases as cases  # noqa: E402
from parity_contract import TOL_FP32  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import gym_electric_motor_amd as ga  # noqa: E402
from gym_electric_motor_amd import _lib  # noqa: E402
from test_gpu_env_parameters import run_rollout, run_steps, same_bits, with_common_limits  # noqa: E402

N, K = cases.N, cases.K
UNIT = [(c, f) for c in cases.UNIT_CASES for f in cases.families_of(c)]
UNIT_OF_OLD = {"Cont-CC-PermExDc-v0": (0, 0), "Finite-CC-PMSM-v0": (1, 1), "Cont-SC-SCIM-v0": (2, 2), "Cont-CC-EESM-v0": (6, 6), "Finite-TC-DFIM-v0": (7, 9),
               "Cont-SC-SeriesDc-v0": (3, 0), "dq-PMSM": (1, 10)}


def ids(params):
    return ["-".join(p) if isinstance(p, tuple) else p for p in params]


def unit_of(case):
    return UNIT_OF_OLD[case] if case in UNIT_OF_OLD else cases.UNIT_CASES[case]["unit"]


def names_unit(launch, case):
    return "<sys=%d,conv=%d," % unit_of(case) in launch


class no_linear_map:
    """GEMX_LINMAP=0 while a handle is created: the stage-by-stage solver for a constant-speed load, which is what the per-env kernels run."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("GEMX_LINMAP")
        if self.on:
            os.environ["GEMX_LINMAP"] = "0"

    def __exit__(self, *exc):
        if self.on:
            os.environ.pop("GEMX_LINMAP") if self.old is None else os.environ.__setitem__("GEMX_LINMAP", self.old)


def table_env(case, family, **extra):
    return ga.make(cases.env_id_of(case), n_envs=N, env_parameters=cases.env_parameters(case, family=family), **cases.make_kwargs(case), **extra)


def uniform_env(case, s, family, **extra):
    """The uniform env of set s with the COMMON limits; a constant-speed load without the one-step linear map."""
    with no_linear_map(not cases._case(case)["poly"]):
        return with_common_limits(ga.make(cases.env_id_of(case), n_envs=N, **dict(cases.uniform_kwargs(case, s, family), **extra)), case)


_table, _uniform = {}, {}


def table_runs(case, family, **extra):
    """The table env's rollout and step x K results (obs, done, final state, launch), computed once and shared."""
    key = (case, family) + tuple(sorted(extra.items()))
    if key not in _table:
        env = table_env(case, family, **extra)
        a = cases.actions(case, family=family)
        env.physical_system.reset()
        init = env.physical_system.get_state().cpu().numpy()
        _table[key] = dict(rollout=run_rollout(env.physical_system, a), steps=run_steps(env.physical_system, a), init=init)
        env.close()
    return _table[key]


def uniform_runs(case, family, sets, **extra):
    """set -> the uniform env's results like table_runs, computed once and shared."""
    key = (case, family) + tuple(sorted(extra.items()))
    runs = _uniform.setdefault(key, {})
    a = cases.actions(case, family=family)
    for s in sets:
        if s not in runs:
            env = uniform_env(case, s, family, **extra)
            runs[s] = dict(rollout=run_rollout(env.physical_system, a), steps=run_steps(env.physical_system, a))
            env.close()
    return runs


def assert_table_launches(tab, case):
    assert "envparams_rollout_kernel" in tab["rollout"][3] and "envparams_step_kernel" in tab["steps"][3], tab
    assert names_unit(tab["rollout"][3], case) and names_unit(tab["steps"][3], case), (tab["rollout"][3], unit_of(case))
    for i in range(3):
        assert same_bits(tab["rollout"][i], tab["steps"][i]), (case, i)


def compare_with_uniform(case, family, sets, lanes_of, **extra):
    """Rows, done bytes and final state of the lanes `lanes_of(s)` against the uniform handle of set s: step x K and rollout, bit for bit."""
    tab = table_runs(case, family, **extra)
    assert_table_launches(tab, case)
    assert tab["rollout"][1].any(), "no lane of the table env terminated: the done path went unexercised"
    uni = uniform_runs(case, family, sets, **extra)
    for s in sets:
        lanes = lanes_of(s)
        for how in ("rollout", "steps"):
            obs, done, state, launch = uni[s][how]
            assert "envparams" not in launch and "kernel" in launch, launch
            t_obs, t_done, t_state, _ = tab[how]
            assert same_bits(t_done[:, lanes], done[:, lanes]), (case, family, s, how)
            assert same_bits(t_obs[:, lanes], obs[:, lanes]), (case, family, s, how, float(np.abs(t_obs[:, lanes] - obs[:, lanes]).max()))
            assert same_bits(t_state[:, lanes], state[:, lanes]), (case, family, s, how)


def assert_conditions(case, family):
    """The oracle's verdict on the chosen sets and actions (tests/test_env_parameters_cpu.py asserts it without a GPU)."""
    assert cases.exercised(case, family) == (True, True), (case, family)
    assert cases.margin(case, family) >= cases.MARGIN, (case, family, cases.margin(case, family))


def oracle_error(case, family, got, got_done, auto_reset=True):
    ref, ref_done = cases.oracle_runs(case, family, auto_reset)
    names = list(cases.base_env(case).physical_system.state_names)
    return cases.oracle_error(names, got, got_done, ref, ref_done, cases.live_steps(ref_done, auto_reset))


@pytest.mark.parametrize("case, family", UNIT, ids=ids(UNIT))
def test_lane_equals_its_uniform_handle(case, family):
    """Gaps 2 and 3: rows, done bytes and final state of every lane, through step x K and through rollout; the launch names the unit."""
    assert_conditions(case, family)
    sets = cases.set_of_env(family)
    compare_with_uniform(case, family, range(cases.NSETS), lambda s: np.flatnonzero(sets == s))


@pytest.mark.parametrize("case, family", UNIT, ids=ids(UNIT))
def test_lanes_match_the_fp64_oracle(case, family):
    """Gap 4: every lane of every case -- the polynomial loads included -- against the fp64 oracle run once per set; done masks exact.
    A case beyond the tolerance while its lanes equal their uniform handles is a finding about the existing kernels at those parameters:
    the uniform handles' own error is printed beside it."""
    assert_conditions(case, family)
    obs, done, _, launch = table_runs(case, family)["rollout"]
    assert "envparams_rollout_kernel" in launch and names_unit(launch, case)
    worst = oracle_error(case, family, obs, done)
    print(f"ORACLE {case} {family}: worst relative error against the fp64 oracle {worst:.3e}")
    if not worst < TOL_FP32:
        uni = uniform_runs(case, family, range(cases.NSETS))
        sets = cases.set_of_env(family)
        own = np.stack([uni[sets[e]]["rollout"][0][:, e] for e in range(N)], axis=1)
        own_done = np.stack([uni[sets[e]]["rollout"][1][:, e] for e in range(N)], axis=1)
        print(f"ORACLE {case} {family}: the uniform handles' own worst relative error {oracle_error(case, family, own, own_done):.3e}")
    assert worst < TOL_FP32, (case, family, worst)


@pytest.mark.parametrize("case", list(UNIT_OF_OLD) + list(cases.UNIT_CASES))
def test_unit_of_every_case_is_named_by_its_launch(case):
    """All 19 per-env units, each by one step and one two-step rollout of a small table env: the launch string names kernel and unit."""
    env = ga.make(cases.env_id_of(case), n_envs=N, env_parameters=ga.EnvParameters(), **cases.make_kwargs(case))
    ps = env.physical_system
    a = cases.actions(case)[:2]
    step, roll = run_steps(ps, a[:1])[3], run_rollout(ps, a)[3]
    env.close()
    assert "envparams_step_kernel" in step and names_unit(step, case), (step, unit_of(case))
    assert "envparams_rollout_kernel" in roll and names_unit(roll, case), (roll, unit_of(case))
    assert len({unit_of(c) for c in list(UNIT_OF_OLD) + list(cases.UNIT_CASES)}) == 19


# ---------------------------------------------------------------------------------------------------------------------------------------
# Every lane its own machine (gap 1)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.LANE_CASES)
def test_every_lane_matches_the_oracle_of_its_own_machine(case):
    """Rollout and step x K against the fp64 oracle run per lane with that lane's machine; done masks exact."""
    assert_conditions(case, "lanes")
    tab = table_runs(case, "lanes")
    assert_table_launches(tab, case)
    for how in ("rollout", "steps"):
        worst = oracle_error(case, "lanes", tab[how][0], tab[how][1])
        print(f"ORACLE {case} lanes ({how}): worst relative error against the fp64 oracle {worst:.3e}")
        assert worst < TOL_FP32, (case, how, worst)


@pytest.mark.parametrize("case", cases.LANE_CASES)
def test_block_edges_and_the_tail_equal_uniform_handles_of_their_machines(case):
    """Lanes 0, 63, 64, 65 and 196 against uniform handles of the same n_envs built with the lane's machine, bit for bit."""
    compare_with_uniform(case, "lanes", cases.EDGE_LANES, lambda e: np.array([e]))


@pytest.mark.parametrize("case", cases.LANE_CASES)
def test_the_table_on_the_device_equals_the_host_restatement(case):
    """`get_env_parameter_table()` against derive_machine_params restated in float64 numpy and rounded once to fp32: per field and per env,
    exact.  Every pair of envs differs in some field, so a column written or read at another env's index cannot go unnoticed."""
    env = table_env(case, "lanes")
    ps = env.physical_system
    got = ps.get_env_parameter_table().cpu().numpy()
    want, names = cases.restated_table(ps, ps._env_parameter_arrays, _lib.MODEL_COLS)
    env.close()
    assert got.shape == want.shape == (len(names), N)
    for f, name in enumerate(names):
        bad = np.flatnonzero(got[f].view(np.uint32) != want[f].view(np.uint32))
        assert bad.size == 0, (case, name, bad[:8], got[f][bad[:8]], want[f][bad[:8]])
    assert max(len(np.unique(want[f])) for f in range(len(names))) == N  # (one field alone tells every env from every other)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Branches (gaps 3 and 4)
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_soa_rows_equal_the_aos_rows():
    """The GEMX_OBS_SOA branch of ep_store_row: rollout rows [K][S_out][N] and step rows [S_out][N], transposed, equal the AoS run."""
    case, family = cases.SOA_CASE, "fields"
    aos = table_runs(case, family)
    soa = table_runs(case, family, obs_layout="soa")
    assert_table_launches(soa, case)
    s_out = aos["rollout"][0].shape[-1]
    for how in ("rollout", "steps"):
        assert soa[how][0].shape == (K, s_out, N), soa[how][0].shape
        assert same_bits(soa[how][0].transpose(0, 2, 1), aos[how][0]), how
        assert same_bits(soa[how][1], aos[how][1]) and same_bits(soa[how][2], aos[how][2]), how


def test_without_auto_reset_a_done_lane_keeps_its_state():
    """`if (done && P.auto_reset)` not taken: bit for bit against uniform handles built with auto_reset=False, against the oracle's
    rollout(auto_reset=False) up to and including each lane's first done step, and some done lane's state is not the initial state."""
    case, family = cases.NO_RESET_CASE, "factors"
    assert_conditions(case, family)
    sets = cases.set_of_env(family)
    compare_with_uniform(case, family, range(cases.NSETS), lambda s: np.flatnonzero(sets == s), auto_reset=False)
    tab = table_runs(case, family, auto_reset=False)
    for how in ("rollout", "steps"):
        worst = oracle_error(case, family, tab[how][0], tab[how][1], auto_reset=False)
        print(f"ORACLE {case} {family} auto_reset=False ({how}): worst relative error against the fp64 oracle {worst:.3e}")
        assert worst < TOL_FP32, (how, worst)
    obs, done, state, _ = tab["rollout"]
    lanes = np.flatnonzero(done[-1])  # done at the last step: with auto-reset the final state would be the initial state, here it is not
    assert lanes.size > 0 and done.astype(bool).any(0).sum() < N
    assert np.all(np.any(state[:, lanes] != tab["init"][:, lanes], axis=0)), (case, lanes)
    reset = table_runs(case, family)
    again = np.flatnonzero(reset["rollout"][1][-1])  # (the run WITH auto-reset: such a lane ends in the initial state)
    assert same_bits(reset["rollout"][2][:, again], reset["init"][:, again])


def test_lanes_with_and_without_a_kink_share_a_wave():
    """ep_apply's per-lane `kink_split = flag && omega_lim > 0` under make()'s default solver (RK4 that splits at the kink): by the oracle,
    lanes with a > 0 leave |omega| < omega_lim within K while lanes with a = 0 (plain RK4) sit in the same wave; then bit for bit against
    the uniform handles and against the oracle."""
    case, family = cases.MIXED_KINK_CASE, "fields"
    assert getattr(cases.base_env(case).physical_system._ode_solver, "_split_kinks", False)
    crossing, without = cases.kink_crossings(case, family)
    assert crossing.size > 0 and without.size > 0 and np.intersect1d(crossing // 64, without // 64).size > 0
    assert {cases.oracle_solver(case, s, family) for s in range(cases.NSETS)} == {"rk4", "rk4_kink"}
    sets = cases.set_of_env(family)
    compare_with_uniform(case, family, range(cases.NSETS), lambda s: np.flatnonzero(sets == s))
    for how in ("rollout", "steps"):
        obs, done = table_runs(case, family)[how][:2]
        worst = oracle_error(case, family, obs, done)
        print(f"ORACLE {case} {family} mixed kink ({how}): worst relative error against the fp64 oracle {worst:.3e}")
        assert worst < TOL_FP32, (how, worst)
