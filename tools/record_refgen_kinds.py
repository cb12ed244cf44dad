#!/usr/bin/env python3
"""Record what the reference's sinusoidal, step, triangular, sawtooth and Laplace generators produce, as data:
tests/golden/refgen/refgen_kinds.npz.

TEST INFRASTRUCTURE ONLY -- never imported by the product package.  Imports the unmodified reference the way oracle/make_golden.py
does (oracle/gymnasium_standin and $GEM_REFERENCE/src on sys.path), instantiates its generator classes against the physical systems of
`gem.make(env_id)` and writes

  * waveform cases (CASES x the four waveform kinds, a few sub-episodes each): the margins, tau and the amplitude / offset ranges after
    `set_modules`; per sub-episode the drawn length, amplitude, frequency, offset, the extra uniform / triangular draws (seen by a
    recording proxy around the generator's `random_generator`) and the `_reference` array the generator tabulated;
  * samples for distribution tests (SAMPLE_CASES): the parameter draws of a few thousand sub-episodes per kind; for the Laplace
    process the sub-episodes' scales and increments divided by the scale.

    MPLBACKEND=Agg python tools/record_refgen_kinds.py [--out tests/golden/refgen/refgen_kinds.npz]

tests/refgen_waveforms.py restates the waveforms in closed form; tests/test_refgen_kinds_cpu.py holds it against this file, and
tests/test_gpu_refgen_kinds.py holds the device generators against both.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVEFORMS = ("Sinusoidal", "Step", "Triangular", "Sawtooth")
# name -> env id, referenced state, generator keywords, sub-episodes recorded, seed
CASES = {
    "sc_pmsm_omega": ("Cont-SC-PMSM-v0", "omega", dict(), 3, 11),
    "cc_pmsm_i_sq": ("Cont-CC-PMSM-v0", "i_sq", dict(frequency_range=(20, 200), episode_lengths=(300, 900), amplitude_range=(0.1, 0.5), offset_range=(-0.2, 0.3)), 4, 12),
    "tc_shunt_torque": ("Cont-TC-ShuntDc-v0", "torque", dict(limit_margin=(0, 0.8), episode_lengths=(300, 900), frequency_range=(5, 60)), 4, 13),
    "cc_eesm_i_e": ("Cont-CC-EESM-v0", "i_e", dict(limit_margin=(0, 1), episode_lengths=(300, 900), frequency_range=15), 3, 14),
}
# name -> env id, state, keywords, kinds, sub-episodes
SAMPLE_CASES = {
    "sc_pmsm_omega": ("Cont-SC-PMSM-v0", "omega", dict(), WAVEFORMS + ("LaplaceProcess",), 2500),
    "tc_shunt_torque": ("Cont-TC-ShuntDc-v0", "torque", dict(limit_margin=(0, 0.8)), ("Sinusoidal", "Step"), 1500),
}


def _import_reference():
    sys.path.insert(0, REPO)
    from oracle import make_golden  # puts the gymnasium stand-in and the reference on sys.path, imports it

    return make_golden.gem


class _Spy:
    """Passes every call on to the generator's numpy Generator and keeps (method, value) of the scalar draws."""

    def __init__(self, rng):
        self._rng, self.log = rng, []

    def __getattr__(self, name):
        fn = getattr(self._rng, name)

        def call(*a, **k):
            v = fn(*a, **k)
            if np.ndim(v) == 0:
                self.log.append((name, float(v)))
            return v

        return call


def _generator(gem, kind, ps, state, kw, seed):
    cls = getattr(gem.reference_generators, kind + "ReferenceGenerator")
    gen = cls(reference_state=state, **kw)
    gen.set_modules(ps)
    gen.seed(np.random.SeedSequence(seed))
    gen.reset()  # (draws the first sub-episode and shows its first value, core.py ReferenceGenerator.reset)
    for _ in range(int(gen._current_episode_length) - int(gen._k)):  # that sub-episode is not recorded: the proxy was not there yet
        gen.get_reference_observation()
    spy = _Spy(gen._random_generator)
    gen._random_generator = spy
    return gen, spy


N_EXTRA = dict(Sinusoidal=1, Sawtooth=1, Step=2, Triangular=2, LaplaceProcess=0)


def _subepisodes(gen, spy, kind, n_sub):
    """Steps the generator through n_sub sub-episodes -> per sub-episode a dict: length, the drawn amplitude / frequency / offset (or the
    Laplace scale), the extra draws as the random generator returned them (sinusoidal, sawtooth: the phase's uniform; step: the
    triangular ratio, the roll's uniform; triangular: the phase's uniform, the width), the tabulated array, the carried value the
    sub-episode started from."""
    out = []
    while len(out) < n_sub:
        spy.log.clear()
        before = float(gen._reference_value)
        gen.get_reference_observation()
        assert gen._k == 1  # (a fresh sub-episode)
        L = int(gen._current_episode_length)
        extra = spy.log[len(spy.log) - N_EXTRA[kind]:] if N_EXTRA[kind] else []
        assert [m for m, _ in extra] == dict(Step=["triangular", "uniform"]).get(kind, ["uniform"] * N_EXTRA[kind])
        out.append(dict(length=L, amplitude=float(getattr(gen, "_amplitude", 0.0)), frequency=float(getattr(gen, "_frequency", 0.0)),
                        offset=float(getattr(gen, "_offset", 0.0)), scale=float(getattr(gen, "_current_sigma", 0.0)),
                        extra=([v for _, v in extra] + [0.0, 0.0])[:2], reference=np.array(gen._reference, dtype=np.float64), before=before))
        for _ in range(L - 1):
            gen.get_reference_observation()
    return out


def _rows(subs):
    """length, amplitude, frequency, offset, first extra draw, second extra draw"""
    return [[e["length"], e["amplitude"], e["frequency"], e["offset"]] + e["extra"] for e in subs]


def record(out_path):
    gem = _import_reference()
    arrays, meta = {}, dict(cases={}, samples={})
    systems = {}

    def system(env_id):
        if env_id not in systems:
            env = gem.make(env_id)
            systems[env_id] = getattr(env, "unwrapped", env).physical_system
        return systems[env_id]

    for name, (env_id, state, kw, n_sub, seed) in CASES.items():
        ps = system(env_id)
        for i, kind in enumerate(WAVEFORMS):
            gen, spy = _generator(gem, kind, ps, state, kw, seed * 100 + i)
            key = f"case/{name}/{kind}"
            subs = _subepisodes(gen, spy, kind, n_sub)
            meta["cases"][key] = dict(env_id=env_id, state=state, kind=kind, keywords={k: v for k, v in kw.items()}, tau=float(ps.tau),
                                      margin=[float(x) for x in gen._limit_margin], amplitude_range=[float(x) for x in np.atleast_1d(gen._amplitude_range)],
                                      offset_range=[float(x) for x in np.atleast_1d(gen._offset_range)], n_sub=n_sub)
            arrays[key + "/params"] = np.array(_rows(subs), dtype=np.float64)
            arrays[key + "/reference"] = np.concatenate([e["reference"] for e in subs])
    for name, (env_id, state, kw, kinds, n_sub) in SAMPLE_CASES.items():
        ps = system(env_id)
        for i, kind in enumerate(kinds):
            gen, spy = _generator(gem, kind, ps, state, kw, 7000 + 10 * len(name) + i)
            key = f"samples/{name}/{kind}"
            subs = _subepisodes(gen, spy, kind, n_sub)
            meta["samples"][key] = dict(env_id=env_id, state=state, kind=kind, keywords={k: v for k, v in kw.items()}, tau=float(ps.tau),
                                        margin=[float(x) for x in gen._limit_margin], n_sub=n_sub)
            if kind == "LaplaceProcess":
                z = []
                lo, hi = gen._limit_margin
                for e in subs:
                    seq = np.concatenate([[e["before"]], e["reference"]])
                    ok = (seq[1:] > lo + 1e-9) & (seq[1:] < hi - 1e-9) & (seq[:-1] > lo + 1e-9) & (seq[:-1] < hi - 1e-9)  # (not clipped)
                    z.append((np.diff(seq) / e["scale"])[ok][:12])
                arrays[key + "/length"] = np.array([e["length"] for e in subs], dtype=np.int32)
                arrays[key + "/scale"] = np.array([e["scale"] for e in subs], dtype=np.float32)
                arrays[key + "/z"] = np.concatenate(z).astype(np.float32)
            else:
                arrays[key + "/params"] = np.array(_rows(subs), dtype=np.float32)
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(out_path, **arrays)
    return out_path


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "refgen", "refgen_kinds.npz"))
    a = ap.parse_args()
    print(record(a.out), os.path.getsize(a.out), "bytes")
