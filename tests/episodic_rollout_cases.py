"""Inputs of the episodic rollout's comparison with the float64 host shell (tests/env_shell_restatement.py), as data that needs no device:
tests/test_episodic_rollout_cpu.py runs the shell alone on them and asserts what they must show, tests/test_gpu_episodic_rollout.py
compares `rollout_complete_episodic` with the shell on the same inputs.  The env is case E of tests/env_shell_cases.py (Cont-CC-PMSM-v0, step
and sinusoidal references, CosSin flat observation, no noise) at the episodic tests' shape, N = 197 and K = 48, with its actions: every third
lane holds the action that passes the current limit in the eighth step, the lanes behind them hold it for the first half of the run, the
others stay near zero.  M = 7 lies below that episode length -- every episode is cut by the time limit --, M = 10 above it: terminations and
truncations meet in one lane."""
import env_shell_cases as cases

N, K = 197, 48
LIMITS = (7, 10)


def spec(M):
    return dict(cases.CASES["E"], N=N, K=K, M=M)
