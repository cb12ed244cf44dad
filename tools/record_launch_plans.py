"""Every branch of the rollout launch planner (csrc/gemx_launch_plan.hpp), one short launch per row: prints gemx_last_launch() of each.

    GEMX_PACE_CAL=0 python tools/record_launch_plans.py [--plans FILE]

Two checkouts whose planners decide alike print the same lines (the calibration is off, so no timing enters; the one closed-loop row is a
handle's FIRST launch, which always runs the built-in target).  --plans FILE additionally makes every planned launch append the pure
layer's inputs and outputs to FILE (GEMX_PLAN_RECORD): tests/golden/launch_plans.txt is such a file, replayed without a GPU by
tests/test_launch_plan_cpu.py.  The sizes come from the planner's own thresholds -- workgroups per CU, the limiter's K >= 64, deep rounds
from 400 steps, the long launches from 1200 -- not from the benchmark.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--plans", default=None)
args = ap.parse_args()
os.environ["GEMX_PACE_CAL"] = "0"
os.environ["GEMX_QUIET"] = "1"
if args.plans:
    if os.path.exists(args.plans):
        os.remove(args.plans)
    os.environ["GEMX_PLAN_RECORD"] = os.path.abspath(args.plans)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gym_electric_motor_amd as ga  # noqa: E402

CU = torch.cuda.get_device_properties(0).multi_processor_count
WG = 64
ONE, ABOVE, TWO, FOUR = CU * WG, CU * WG + WG, 2 * CU * WG, 4 * CU * WG
PARTIAL, ODD = CU * WG + 32, 20005  # a partial last workgroup; N % 16 != 0
K_ALL = (1, 2, 63, 64, 399, 400, 1199, 1200)


def const_speed():
    return ga.ConstantSpeedLoad(omega_fixed=60.0)


def launch(tag, env, K, how="plain"):
    ps = env.physical_system
    n = ps._n_envs
    try:
        if how == "synth":
            ps.rollout_synthetic(K, seed=1, step0=0)
        else:
            acts = torch.zeros((K, n) if ps._discrete else (K, n, ps._n_act), device="cuda", dtype=torch.uint8 if ps._discrete else ps._tdtype)
            if how == "half":
                ps.rollout(acts.half())
            elif how == "reward":
                refs = torch.zeros((K, n, int(ps._reward_cfg.n_ref)), device="cuda", dtype=ps._tdtype)
                ps.rollout(acts, references=refs)
            elif K == 1:
                ps.simulate(acts[0])
            else:
                ps.rollout(acts)
        torch.cuda.synchronize()
        print(f"{tag} N={n} K={K} {how}: {ps.last_launch()}", flush=True)
    except Exception as e:  # a refusal is a decision as well: both checkouts must word it alike
        print(f"{tag} N={n} K={K} {how}: {type(e).__name__}: {e}", flush=True)


def rows(tag, env_id, sizes, ks=(64,), how="plain", limiter=None, setup=None, **kw):
    for n in sizes:
        try:
            env = ga.make(env_id, n_envs=n, **kw)
            if setup is not None:
                setup(env.physical_system)
            if limiter is not None:
                env.physical_system.set_rate_limiter(*limiter)
            env.reset()
        except Exception as e:
            print(f"{tag} N={n}: {type(e).__name__}: {e}", flush=True)
            continue
        for K in ks:
            launch(tag if limiter is None else f"{tag} limiter={limiter}", env, K, how)
        env.close()
        del env
        torch.cuda.empty_cache()


# PMSM finite behind a constant-speed load: COMPACT rows, the deep shapes, deep rounds, the long launches at one workgroup per CU
pmsm_c = dict(load=const_speed())
rows("pmsm-finite-constspeed", "Finite-CC-PMSM-v0", (ONE,), K_ALL, **pmsm_c)
rows("pmsm-finite-constspeed", "Finite-CC-PMSM-v0", (ABOVE, TWO, FOUR, PARTIAL, ODD), (2, 63, 64), **pmsm_c)
rows("pmsm-finite-constspeed", "Finite-CC-PMSM-v0", (ONE, TWO, 3 * CU * WG, FOUR), (63, 64, 399, 400), limiter=("off",), **pmsm_c)
rows("pmsm-finite-constspeed", "Finite-CC-PMSM-v0", (ONE, TWO, FOUR + WG), (63, 64), limiter=("open", 5000.0), **pmsm_c)
rows("pmsm-finite-constspeed", "Finite-CC-PMSM-v0", (TWO,), (64,), limiter=("closed",), **pmsm_c)
rows("pmsm-finite-constspeed", "Finite-CC-PMSM-v0", (ONE,), (1199, 1200), limiter=("open",), **pmsm_c)
# ... and behind its default load (no one-step map: no COMPACT rows)
rows("pmsm-finite", "Finite-CC-PMSM-v0", (ONE, ABOVE, TWO, FOUR, 8 * CU * WG), (2, 64))
# PMSM continuous: reads >= 8 bytes per env-step; half and synthetic actions; the fused reward
rows("pmsm-cont", "Cont-CC-PMSM-v0", (ONE, TWO, FOUR, 5 * CU * WG, 8 * CU * WG), (2, 64))
rows("pmsm-cont", "Cont-CC-PMSM-v0", (ONE, TWO, FOUR, 8 * CU * WG), (2, 64), how="half")
rows("pmsm-cont", "Cont-CC-PMSM-v0", (ONE, TWO, FOUR, 8 * CU * WG), (2, 64), how="synth")
with_reward = lambda ps: ps.set_reward(referenced_states=("i_sd", "i_sq"))  # noqa: E731
rows("pmsm-cont-reward", "Cont-CC-PMSM-v0", (ONE, TWO, FOUR, 5 * CU * WG), (2, 64, 400), how="reward", setup=with_reward)
rows("pmsm-finite-constspeed-reward", "Finite-CC-PMSM-v0", (ONE, TWO), (64, 400), how="reward", setup=with_reward, **pmsm_c)
# SCIM: the <2, 2> rule (one round of <2, 2> where <4, 2> runs a round and a short tail)
rows("scim-finite", "Finite-CC-SCIM-v0", (ONE, 3 * CU * WG, 3 * CU * WG + WG, FOUR, FOUR + WG, 5 * CU * WG, 6 * CU * WG, 6 * CU * WG + WG, 8 * CU * WG), (64,))
rows("scim-finite", "Finite-CC-SCIM-v0", (FOUR,), (64,), limiter=("off",))
# DFIM: no deep shape
rows("dfim-finite", "Finite-CC-DFIM-v0", (ONE, TWO, FOUR), (2, 64))
# DC machines: dc_stream (32 and 64 envs per workgroup, up to one workgroup per two CUs), and the "one slot less" band of the limiter
dc = dict(load=const_speed())
rows("permexdc-cont-constspeed", "Cont-CC-PermExDc-v0", (CU * WG // 8, CU * WG // 4, CU * WG // 4 + WG, CU * WG // 2, CU * WG // 2 + WG, ONE, TWO), (2, 64), **dc)
for per_cu in (5, 6, 7, 8):
    rows("shuntdc-finite", "Finite-CC-ShuntDc-v0", (per_cu * CU * WG - WG, per_cu * CU * WG, per_cu * CU * WG + WG), (64,))
# PMSM with each of the things that pick another instantiation or refuse
pmsm = ("Finite-CC-PMSM-v0", (ONE, FOUR), (2, 64))
rows("pmsm-rc-supply", *pmsm, supply=ga.RCVoltageSupply(supply_parameter=dict(R=0.05, C=2e-3)))
rows("pmsm-rinit", *pmsm, motor=dict(motor_initializer=dict(random_init="uniform")), seed=3)
rows("pmsm-substeps", *pmsm, ode_solver=ga.RK4Solver(nsteps=2))
rows("pmsm-substeps-rinit", *pmsm, ode_solver=ga.RK4Solver(nsteps=2), motor=dict(motor_initializer=dict(random_init="uniform")), seed=3)
rows("pmsm-deadtime", *pmsm, physical_system_wrappers=(ga.DeadTimeProcessor(steps=1),))
rows("pmsm-deadtime-constspeed", "Finite-CC-PMSM-v0", (TWO,), (400,), limiter=("off",), physical_system_wrappers=(ga.DeadTimeProcessor(steps=1),), **pmsm_c)
rows("pmsm-cont-dq-deadtime", "Cont-CC-PMSM-v0", (ONE, FOUR), (64,), physical_system_wrappers=(ga.DeadTimeProcessor(steps=2), ga.DqToAbcActionProcessor()))
for n in (ONE, FOUR):
    table = ga.EnvParameters(motor=dict(r_s=np.linspace(17e-3, 19e-3, n)))
    rows("pmsm-env-parameters", "Finite-CC-PMSM-v0", (n,), (1, 2, 64), env_parameters=table)
    rows("pmsm-cont-env-parameters", "Cont-CC-PMSM-v0", (n,), (64,), how="half", env_parameters=table)
    rows("pmsm-cont-env-parameters", "Cont-CC-PMSM-v0", (n,), (64,), how="synth", env_parameters=table)
rows("pmsm-fp64", "Cont-CC-PMSM-v0", (ONE, FOUR), (1, 2, 64), dtype="float64")
for shape in (0, 1, 2, 3):  # the forced test shapes
    os.environ["GEMX_PIPE_SHAPE"] = str(shape)
    rows(f"pmsm-finite-constspeed-forced{shape}", "Finite-CC-PMSM-v0", (TWO,), (64,), **pmsm_c)
    rows(f"dfim-finite-forced{shape}", "Finite-CC-DFIM-v0", (WG * 3,), (26,))
del os.environ["GEMX_PIPE_SHAPE"]
