"""The profile references (csrc/gemx_refprofile.hip) restated on the host in float64 -- the one definition the CPU and GPU tests of
ProfileReferenceGenerator check against.  Per env: k (steps shown since the episode began), s (its start row), e (episodes begun).

    p = s + k * ratio          float64 from the integers every time: one product, one sum (numpy rounds each once, as the device does)
    i = floor(p), w = p - i    end 'hold': p >= T - 1 shows row T - 1;  end 'wrap': rows modulo T, the partner of row T - 1 is row 0
    value                      w == 0 or interpolation 'hold': the table entry itself;  'linear': a + w (b - a), evaluated in extended
                               precision and rounded once to float64 (the device: one fma in its working dtype)

A restart sets k = 0, e += 1 and s = the start row the caller hands in (0 by default): random start rows are device draws that the tests
check by property and feed back here, they are not restated."""
import numpy as np


class Profiles:
    def __init__(self, table, n_envs, ratio=1.0, interpolation="linear", end="hold"):
        self.table = np.asarray(table, dtype=np.float64)  # [T, n_ref] or [T, N, n_ref]: the values the device table holds
        assert self.table.ndim in (2, 3) and interpolation in ("linear", "hold") and end in ("hold", "wrap")
        self.per_env = self.table.ndim == 3
        self.T, self.n_ref, self.n = self.table.shape[0], self.table.shape[-1], int(n_envs)
        assert not self.per_env or self.table.shape[1] == self.n
        self.ratio, self.linear, self.wrap = np.float64(ratio), interpolation == "linear", end == "wrap"
        self.k = np.zeros(self.n, np.int64)
        self.s = np.zeros(self.n, np.int64)
        self.e = np.zeros(self.n, np.int64)

    def reset(self, mask=None, start=None):
        m = np.ones(self.n, bool) if mask is None else np.asarray(mask).astype(bool)
        self.k[m] = 0
        self.e[m] += 1
        self.s[m] = 0 if start is None else np.asarray(start, np.int64)[m]

    def rows(self):
        """-> (ia, ib, w) of every env's position"""
        p = self.s.astype(np.float64) + self.k.astype(np.float64) * self.ratio
        i = np.floor(p)
        w = p - i
        i = i.astype(np.int64)
        if self.wrap:
            ia = i % self.T
            ib = (ia + 1) % self.T
        else:
            past = p >= self.T - 1
            ia = np.where(past, self.T - 1, i)
            ib = np.where(past, self.T - 1, i + 1)
            w = np.where(past, 0.0, w)
        return ia, ib, w

    def show(self):
        """the [N, n_ref] values at the current positions; k advances"""
        ia, ib, w = self.rows()
        env = np.arange(self.n)
        a = self.table[ia, env] if self.per_env else self.table[ia]
        b = self.table[ib, env] if self.per_env else self.table[ib]
        out = a.copy()
        lerp = (w != 0.0) & self.linear
        if lerp.any():
            al, bl, wl = a[lerp].astype(np.longdouble), b[lerp].astype(np.longdouble), w[lerp].astype(np.longdouble)[:, None]
            out[lerp] = (al + wl * (bl - al)).astype(np.float64)
        self.k += 1
        return out

    def step(self, done=None, start=None):
        """restart the done envs first, then show and advance (the env shell's order)"""
        if done is not None:
            self.reset(done, start)
        return self.show()

    def rollout_shell(self, K, done=None, start=None):
        """[K, N, n_ref]: K x step(done[k])"""
        return np.stack([self.step(None if done is None else done[k], start) for k in range(K)])

    def rollout(self, K, done=None, start=None):
        """[K, N, n_ref]: row k is shown, THEN the envs with done[k] restart"""
        out = []
        for k in range(K):
            out.append(self.show())
            if done is not None:
                self.reset(done[k], start)
        return np.stack(out)

    def state(self):
        return dict(k=self.k.copy(), s=self.s.copy(), e=self.e.copy())
