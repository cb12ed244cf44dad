"""A float64 numpy restatement of the returns pass's row function (csrc/gemx_returns.hip: returns_row), for the tests: operation for
operation in the kernel's order, each product and sum a numpy float64 operation of its own (numpy forms no fused multiply-add), vectorised
over the envs and sequential over the rows, k = K-1 ... 0.  Inputs are widened to float64 first (exact for float32 and float64).  It
shares no code with the package.  An fp32 device output is this float64 result cast to float32 (round to nearest)."""
import numpy as np


def _f64(x):
    return None if x is None else np.asarray(x).astype(np.float64)


def gae(reward, value, terminated, gamma, lam, last_value=None, ended=None, final_value=None, carry_in=None):
    """reward, value [K, N]; terminated, ended [K, N] (nonzero: set) -> (advantage [K, N], returns [K, N], carry_out [N]), all float64."""
    reward, value, final_value = _f64(reward), _f64(value), _f64(final_value)
    K, N = reward.shape
    gamma, lam = np.float64(gamma), np.float64(lam)
    A = np.zeros(N, np.float64) if carry_in is None else _f64(carry_in).copy()
    v_above = np.zeros(N, np.float64) if last_value is None else _f64(last_value).copy()
    adv, ret = np.empty((K, N), np.float64), np.empty((K, N), np.float64)
    for k in range(K - 1, -1, -1):
        term = np.asarray(terminated[k]) != 0
        end = term if ended is None else np.asarray(ended[k]) != 0
        trunc = end & ~term
        v = value[k]
        v_next = v_above
        at_end = np.where(trunc, final_value[k], 0.0) if final_value is not None else np.zeros(N, np.float64)
        v_next = np.where(end, at_end, v_next)
        t1 = gamma * v_next
        delta = (reward[k] + t1) - v
        t2 = gamma * lam
        t3 = t2 * A
        A = np.where(end, delta, delta + t3)
        adv[k] = A
        ret[k] = A + v
        v_above = v
    return adv, ret, A


def discounted(reward, terminated, gamma, last_value=None, ended=None, carry_in=None):
    """The pass without a critic: v = 0 and v_next = 0 in every row, lam = 1; the accumulator starts as carry_in if given, else as
    last_value if given, else as 0 -> (returns [K, N], carry_out [N]), float64."""
    assert last_value is None or carry_in is None
    reward = _f64(reward)
    seed = carry_in if carry_in is not None else last_value
    _, ret, A = gae(reward, np.zeros_like(reward), terminated, gamma, 1.0, last_value=None, ended=ended, final_value=None, carry_in=seed)
    return ret, A
