"""The selection rule of the lookahead rollout (csrc/gemx_lookahead.hip), restated in numpy: the lowest index among the maxima,
    best = 0;  for a in 1 .. NA-1:  if s[a] > s[best]: best = a
on `s = scores + noise` added in float32, as the kernel adds them.  A NaN never wins a comparison and never loses one it holds."""
import numpy as np


def noisy(scores, noise=None):
    """scores [..., NA] float32 (+ noise [..., NA] float32) -> what the kernel compares, in float32"""
    s = np.asarray(scores, dtype=np.float32)
    if noise is None:
        return s + np.float32(0.0)
    with np.errstate(invalid="ignore"):
        return s + np.asarray(noise, dtype=np.float32)


def select(s):
    """s [..., NA] -> the chosen index [...] uint8, by the rule's own loop (vectorised over the leading axes)"""
    s = np.asarray(s)
    best = np.zeros(s.shape[:-1], dtype=np.int64)
    best_value = s[..., 0].copy()
    for a in range(1, s.shape[-1]):
        with np.errstate(invalid="ignore"):
            take = s[..., a] > best_value
        best = np.where(take, a, best)
        best_value = np.where(take, s[..., a], best_value)
    return best.astype(np.uint8)
