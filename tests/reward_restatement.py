"""Plain numpy restatement, in float64, of the reference's WeightedSumOfErrors reward (reward_functions/weighted_sum_of_errors.py:
125-129, with the env shell's choice between it and the violation reward, core.py:346-350):

    r = bias - sum_i w_i * (|s_i - ref_i| / len_i) ** n_i        r = violation_reward where terminated

over ALL states i, with ref_i = 0 for the states no generator references.  It takes the full-length arrays exactly as the reference's
reward function holds them (`_reward_weights`, `_n`, `_state_length`, one entry per state) and imports neither the reference nor the
product: tests compare the two with it (tests/test_reward_restatement_cpu.py pins it to the reference's recorded rewards).
"""
import numpy as np


def full_references(references, ref_columns, n_states):
    """references [..., n_ref] of the referenced states (columns `ref_columns`, ascending) -> [..., n_states] with 0 elsewhere."""
    references = np.asarray(references, dtype=np.float64)
    out = np.zeros(references.shape[:-1] + (n_states,))
    for j, c in enumerate(ref_columns):
        out[..., c] = references[..., j]
    return out


def error_terms(states, references, weights, powers, state_length):
    """-> [..., n_states]: w_i * (|s_i - ref_i| / len_i) ** n_i per state (0 where the weight is 0, whatever the state holds)."""
    s, r = np.asarray(states, dtype=np.float64), np.asarray(references, dtype=np.float64)
    w, n, length = (np.asarray(x, dtype=np.float64) for x in (weights, powers, state_length))
    assert s.shape == r.shape and w.shape == n.shape == length.shape == (s.shape[-1],)
    used = w != 0
    out = np.zeros(s.shape)
    out[..., used] = w[used] * (np.abs(s[..., used] - r[..., used]) / length[used]) ** n[used]
    return out


def reward(states, references, terminated, weights, powers, state_length, bias, violation_reward):
    """states, references [..., n_states] (normalised, references 0 where un-referenced), terminated [...] -> rewards [...]."""
    wse = float(bias) - error_terms(states, references, weights, powers, state_length).sum(axis=-1)
    return np.where(np.asarray(terminated, dtype=bool), float(violation_reward), wse)
