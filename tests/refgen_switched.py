"""The SwitchedReferenceGenerator's state machine, restated on the host for a batch of lanes (numpy) -- the yardstick of
tests/test_refgen_switched_cpu.py (fed the draws the live reference made, tests/golden/refgen/refgen_switched.npz) and of
tests/test_gpu_refgen_switched.py (fed the draws the device made).  Waveform values come from tests/refgen_waveforms.py.  Paths
relative to the reference's reference_generators/:

    reset()                      switched ... :65-68   a new super-episode (length, alternative), sk = 0; the alternative is reset WITHOUT an
                                                       initial reference (Wiener draws its initial value, the others restart from 0) and shows
                                                       its own first value at once (core.py:485-505): not counted in sk, not tested against slen
    get_reference_observation()  switched ... :74-81   sk >= slen: a new super-episode, sk = 0, the chosen alternative is reset WITH the value
                                                       shown last and shows the first value of a new sub-episode; else the current alternative
                                                       advances (subepisoded ... :93-100: k >= L starts a new sub-episode); sk += 1

so the super-episode after a reset shows slen + 1 values and every later one slen.  This module draws nothing: every random quantity is
asked of a `draws` object --

    draws.super_episode(mask) -> (slen, alternative)      arrays over all lanes, read where mask
    draws.sub_episode(mask, kind) -> dict of arrays       length, amplitude, frequency, offset, phase, width, roll, sigma
    draws.initial(mask) -> array                          Wiener's initial value
    draws.walk(mask, before, sigma, lo, hi) -> array      the next value of a Wiener / Laplace walk

and asserts nothing itself; it returns what the reference would show and the state it would be in.
"""
import numpy as np

import refgen_waveforms as rw

KINDS = ("wiener", "laplace", "sinusoidal", "step", "triangular", "sawtooth", "const")  # indexed by GEMX_REF_*
WALKS, WAVES, CONST = (0, 1), (2, 3, 4, 5), 6
PARAMS = ("amplitude", "frequency", "offset", "phase", "width", "roll")


class Switched:
    """n lanes of one switched column.  alternatives: list of dicts -- kind (index into KINDS), margin (lo, hi), value (const)."""

    def __init__(self, alternatives, tau, n, draws):
        self.alts, self.tau, self.n, self.draws = alternatives, float(tau), int(n), draws
        self.kind_of = np.array([a["kind"] for a in alternatives])
        self.m_lo = np.array([a.get("margin", (0.0, 0.0))[0] for a in alternatives], dtype=float)
        self.m_hi = np.array([a.get("margin", (0.0, 0.0))[1] for a in alternatives], dtype=float)
        self.const = np.array([a.get("value", 0.0) for a in alternatives], dtype=float)
        z = lambda dt=float: np.zeros(self.n, dtype=dt)  # noqa: E731
        self.alt, self.sk, self.slen = z(int), z(int), z(int)
        self.k, self.L = z(int), z(int)  # samples shown of the current sub-episode, its length
        self.value, self.sigma = z(), z()
        self.par = {p: z() for p in PARAMS}
        self.fresh = np.zeros(self.n, dtype=bool)  # reset, its first value not shown yet

    kind = property(lambda self: self.kind_of[self.alt])

    def _new_super(self, mask):
        slen, alt = self.draws.super_episode(mask)
        self.slen = np.where(mask, slen, self.slen)
        self.alt = np.where(mask, alt, self.alt)

    def reset(self, mask=None):
        """reset() up to the point where the alternative shows its first value; `show` does that."""
        mask = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        if not mask.any():
            return
        self._new_super(mask)
        self.sk = np.where(mask, 0, self.sk)
        wiener = mask & (self.kind == 0)
        self.value = np.where(mask, 0.0, self.value)
        if wiener.any():
            self.value = np.where(wiener, self.draws.initial(wiener), self.value)
        self.k = np.where(mask, 0, self.k)
        self.L = np.where(mask, -1, self.L)  # `_current_episode_length = -1`: the next sample starts a sub-episode
        self.fresh |= mask

    def show(self):
        """The next reference of every lane -> (values, on_jump, tolerance, switched): what reset() returns for the lanes just reset,
        get_reference_observation() for the others.  switched: the lanes that started a super-episode in this call."""
        switch = ~self.fresh & (self.sk >= self.slen)
        if switch.any():
            self._new_super(switch)
            self.sk = np.where(switch, 0, self.sk)
            self.k = np.where(switch, 0, self.k)  # sub-generator reset(initial_reference = the value shown last): the value is kept
            self.L = np.where(switch, -1, self.L)
        kind = self.kind
        sub = (kind != CONST) & (self.k >= self.L)
        if sub.any():
            d = self.draws.sub_episode(sub, kind)
            self.L = np.where(sub, d["length"], self.L)
            self.k = np.where(sub, 0, self.k)
            self.sigma = np.where(sub & np.isin(kind, WALKS), d["sigma"], self.sigma)
            for p in PARAMS:
                self.par[p] = np.where(sub & np.isin(kind, WAVES), d[p], self.par[p])
        out, on_jump, tol = np.zeros(self.n), np.zeros(self.n, dtype=bool), np.zeros(self.n)
        lo, hi = self.m_lo[self.alt], self.m_hi[self.alt]
        for kd in WAVES:
            m = kind == kd
            if m.any():
                v, j, t = rw.evaluate(KINDS[kd], self.k[m], self.L[m], self.tau, self.par["amplitude"][m], self.par["frequency"][m], self.par["offset"][m],
                                      (lo[m], hi[m]), phase=self.par["phase"][m], width=self.par["width"][m], roll=self.par["roll"][m])
                out[m], on_jump[m], tol[m] = v, j, t
        walk = np.isin(kind, WALKS)
        if walk.any():
            out[walk] = np.asarray(self.draws.walk(walk, self.value, self.sigma, lo, hi))[walk]
        c = kind == CONST
        out[c] = self.const[self.alt][c]
        self.value = out.copy()
        self.k = np.where(c, self.k, self.k + 1)
        self.sk = np.where(self.fresh, self.sk, self.sk + 1)  # (the first value after a reset is not counted)
        self.fresh[:] = False
        return out, on_jump, tol, switch


def clipped_walk(before, increment, lo, hi):
    """wiener_process_reference_generator.py:35-41 (laplace ... alike): value += increment, cut to the margin -- upper bound first."""
    v = before + increment
    v = np.where(v > hi, hi, v)
    return np.where(v < lo, lo, v)
