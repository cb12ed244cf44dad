"""A numpy restatement of the episode stage's row function (csrc/gemx_episode.hip: episode_row), for the tests: one call of `step` is one
control step of N envs, in the kernel's order of operations; the return is a sequential float64 sum (the reward is widened to float64
first -- exact for float32 and float64 -- so a float64 `+=` per step IS the kernel's add)."""
import numpy as np


class Episodes:
    def __init__(self, n_envs, max_steps=0, auto_reset_in_kernel=False):
        n = int(n_envs)
        self.max_steps, self.in_kernel = int(max_steps), bool(auto_reset_in_kernel)
        self.length, self.last_length = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.ret, self.last_ret = np.zeros(n, np.float64), np.zeros(n, np.float64)
        self.n_finished = np.zeros(n, np.int64)

    def step(self, done, reward=None):
        """done [N] (nonzero: terminated), reward [N] | None -> (truncated, ended, reset_mask) uint8 [N]."""
        done = np.asarray(done) != 0
        self.length = self.length + np.int32(1)
        if reward is not None:
            self.ret = self.ret + np.asarray(reward).astype(np.float64)
        truncated = (self.length >= self.max_steps) & ~done if self.max_steps > 0 else np.zeros_like(done)
        ended = done | truncated
        self.last_length = np.where(ended, self.length, self.last_length)
        self.last_ret = np.where(ended, self.ret, self.last_ret)
        self.n_finished = self.n_finished + ended
        self.length = np.where(ended, np.int32(0), self.length)
        self.ret = np.where(ended, 0.0, self.ret)
        reset = truncated if self.in_kernel else ended
        return truncated.astype(np.uint8), ended.astype(np.uint8), reset.astype(np.uint8)

    def rows(self, done, reward=None):
        """done [K, N], reward [K, N] | None -> dict(truncated, ended, reset_mask, finished_return, finished_length), each [K, N]."""
        out = dict(truncated=[], ended=[], reset_mask=[], finished_return=[], finished_length=[])
        for k in range(len(done)):
            t, e, m = self.step(done[k], None if reward is None else reward[k])
            out["truncated"].append(t), out["ended"].append(e), out["reset_mask"].append(m)
            out["finished_return"].append(np.where(e != 0, self.last_ret, 0.0))
            out["finished_length"].append(np.where(e != 0, self.last_length, 0).astype(np.int32))
        return {k: np.stack(v) for k, v in out.items()}

    def fields(self):
        return dict(length=self.length, ret=self.ret, last_length=self.last_length, last_ret=self.last_ret, n_finished=self.n_finished)
