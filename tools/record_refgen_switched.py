#!/usr/bin/env python3
"""Record what the reference's SwitchedReferenceGenerator produces, as data: tests/golden/refgen/refgen_switched.npz.

TEST INFRASTRUCTURE ONLY -- never imported by the product package.  Imports the unmodified reference the way tools/record_refgen_kinds.py
does, builds a SwitchedReferenceGenerator over the physical system of `gem.make(env_id)` and drives it in the env's order (core.py:300-371:
`reset(state)`, then per step `get_reference(state)` and `get_reference_observation(state)`), with a few resets placed inside a
super-episode.  Written per case

  * per step: the observation shown, `get_reference` before it, whether the row came from a reset;
  * per super-episode: the drawn length and the index of the chosen alternative;
  * per sub-episode: alternative index, length, amplitude, frequency, offset, the two extra draws (the columns of refgen_kinds.npz), sigma;
  * Wiener alternatives: the initial values drawn at resets and the normal increments (already scaled by sigma) of every sub-episode;
  * per alternative (meta): kind, keywords, the margin and the clipped amplitude / offset ranges after `set_modules`;

and 20000 samples of the super-episode draw (length, choice) for the distribution tests.  Every draw is seen by a recording proxy
around the generators' numpy Generators (`next_generator` is overridden per INSTANCE so that the proxy survives the resets).

A ConstReferenceGenerator keeps its `reference_names` as a plain string while the sub-episoded generators keep a list, so the switched
generator's own assertion would refuse the mix: the recorder sets the constant instance's attribute to the list form first.

    MPLBACKEND=Agg python tools/record_refgen_switched.py [--out tests/golden/refgen/refgen_switched.npz]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = dict(episode_lengths=(3, 8))
SUPER = (2, 6)


def _five(state, **kw):
    """step, sinusoidal, triangular, sawtooth and constant alternatives for one state"""
    return [("Step", dict(reference_state=state, **SUB, **kw)), ("Sinusoidal", dict(reference_state=state, **SUB, **kw)),
            ("Triangular", dict(reference_state=state, **SUB, **kw)), ("Sawtooth", dict(reference_state=state, **SUB, **kw)),
            ("Const", dict(reference_state=state, reference_value=0.25))]


# name -> env id, state, alternatives (kind, keywords), p, steps, seed
CASES = {
    "sc_pmsm_omega": ("Cont-SC-PMSM-v0", "omega", _five("omega", frequency_range=(500, 3000)), [0.3, 0.2, 0.2, 0.2, 0.1], 260, 21),
    "cc_pmsm_i_sq": ("Cont-CC-PMSM-v0", "i_sq", _five("i_sq", frequency_range=(800, 4000), amplitude_range=(0.1, 0.5), offset_range=(-0.2, 0.3)),
                     [0.1, 0.3, 0.2, 0.3, 0.1], 260, 22),
    "tc_shunt_torque": ("Cont-TC-ShuntDc-v0", "torque", _five("torque", limit_margin=(0, 0.8), frequency_range=(500, 3000)), [0.25, 0.25, 0.2, 0.2, 0.1], 260, 23),
    "sc_pmsm_omega_wiener": ("Cont-SC-PMSM-v0", "omega", [("WienerProcess", dict(reference_state="omega", sigma_range=(1e-2, 1e-1), **SUB)),
                                                          ("Sinusoidal", dict(reference_state="omega", frequency_range=(500, 3000), limit_margin=0.5, **SUB)),
                                                          ("Const", dict(reference_state="omega", reference_value=-0.125))], [0.5, 0.3, 0.2], 260, 24),
}
N_EXTRA = dict(Sinusoidal=1, Sawtooth=1, Step=2, Triangular=2, WienerProcess=0, Const=0)
N_SAMPLES = 20000


def _import_reference():
    sys.path.insert(0, REPO)
    from oracle import make_golden  # puts the gymnasium stand-in and the reference on sys.path, imports it

    return make_golden.gem


class _Spy:
    """Passes every call on to a numpy Generator and keeps (method, value) of every draw in `log`."""

    def __init__(self, rng, log):
        self._rng, self.log = rng, log

    def __getattr__(self, name):
        fn = getattr(self._rng, name)

        def call(*a, **k):
            v = fn(*a, **k)
            self.log.append((name, v))
            return v

        return call


def _watch(component):
    """The component's draws end up in the returned list, across its `next_generator` calls."""
    log = []

    def next_generator():
        component._random_generator = _Spy(np.random.default_rng(component._seed_sequence.spawn(1)[0]), log)

    component.next_generator = next_generator
    component._random_generator = _Spy(component._random_generator, log)
    return log


def _build(gem, ps, alternatives, p, seed):
    rg = gem.reference_generators
    subs = []
    for kind, kw in alternatives:
        g = getattr(rg, kind + "ReferenceGenerator")(**kw)
        if kind == "Const":
            g._reference_names = [g._reference_state]  # (see the module docstring)
        subs.append(g)
    sw = rg.SwitchedReferenceGenerator(subs, p=list(p), super_episode_length=SUPER)
    sw.set_modules(ps)
    sw.seed(np.random.SeedSequence(seed))
    return sw, subs


def _record_case(gem, ps, state_name, alternatives, p, n_steps, seed):
    sw, subs = _build(gem, ps, alternatives, p, seed)
    top = _watch(sw)
    logs = [_watch(g) if hasattr(g, "_random_generator") else [] for g in subs]
    state = np.zeros(len(ps.state_names))
    col = list(ps.state_names).index(state_name)
    obs, ref, is_reset, supers, sub_rows, initial, increments = [], [], [], [], [], [], []

    def harvest():
        """what the call just made drew: super-episodes from the switched generator's log, a sub-episode from the current alternative's"""
        drawn = [v for _, v in top]
        for i in range(0, len(drawn), 2):  # integers(lo, hi), then choice(sub_generators, p)
            supers.append((int(drawn[i]), subs.index(drawn[i + 1])))
        top.clear()
        a = subs.index(sw._current_ref_generator)
        g, kind, log = subs[a], alternatives[a][0], logs[a]
        if kind == "Const":
            return
        started = int(g._k) == 1
        if kind == "WienerProcess":
            for name, v in log:
                if name == "normal":
                    increments.append(np.asarray(v, dtype=np.float64))
                elif name == "uniform" and np.ndim(v) == 1:  # uniform(lo, hi, 1): the initial value of a reset
                    initial.append(float(v[0]))
        if started:
            scalars = [float(v) for _, v in log if np.ndim(v) == 0]
            extra = (scalars[len(scalars) - N_EXTRA[kind]:] if N_EXTRA[kind] else []) + [0.0, 0.0]
            sub_rows.append([a, int(g._current_episode_length), float(getattr(g, "_amplitude", 0.0)), float(getattr(g, "_frequency", 0.0)),
                             float(getattr(g, "_offset", 0.0)), extra[0], extra[1], float(getattr(g, "_current_sigma", 0.0))])
        for lg in logs:
            lg.clear()

    def do_reset():
        r, o, _ = sw.reset(state)
        harvest()
        obs.append(float(o[0])); ref.append(float(r[col])); is_reset.append(True)

    do_reset()
    resets_at = {60, 130, 200}
    pending = False
    for k in range(n_steps):
        pending |= k in resets_at
        if pending and 1 <= sw._k < sw._current_episode_length - 1:  # inside a super-episode: neither its first nor its last step
            do_reset()
            pending = False
            continue
        r = sw.get_reference(state)
        o = sw.get_reference_observation(state)
        harvest()
        obs.append(float(o[0])); ref.append(float(r[col])); is_reset.append(False)
    assert not pending
    meta_alts = []
    for (kind, kw), g in zip(alternatives, subs):
        m = dict(kind=kind, keywords={k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()})
        if kind == "Const":
            m["value"] = float(g._reference_value)
        else:
            m["margin"] = [float(x) for x in g._limit_margin]
            if kind == "WienerProcess":
                m["initial_range"] = [float(x) for x in g._initial_range]
            else:
                m["amplitude_range"] = [float(x) for x in np.atleast_1d(g._amplitude_range)]
                m["offset_range"] = [float(x) for x in np.atleast_1d(g._offset_range)]
        meta_alts.append(m)
    arrays = dict(obs=np.array(obs), ref=np.array(ref), is_reset=np.array(is_reset), super=np.array(supers, dtype=np.int32),
                  sub=np.array(sub_rows, dtype=np.float64), initial=np.array(initial, dtype=np.float64),
                  increments=np.concatenate(increments) if increments else np.zeros(0))
    meta = dict(alternatives=meta_alts, p=list(p), super_episode_length=list(SUPER), tau=float(ps.tau), state=state_name,
                reference_space=[float(sw.reference_space.low[0]), float(sw.reference_space.high[0])], n_super=len(supers), n_resets=int(sum(is_reset)))
    return arrays, meta


def record(out_path):
    gem = _import_reference()
    arrays, meta = {}, dict(cases={}, samples={})
    for name, (env_id, state, alternatives, p, n_steps, seed) in CASES.items():
        env = gem.make(env_id)
        ps = getattr(env, "unwrapped", env).physical_system
        a, m = _record_case(gem, ps, state, alternatives, p, n_steps, seed)
        m["env_id"] = env_id
        meta["cases"][name] = m
        for k, v in a.items():
            arrays[f"case/{name}/{k}"] = v
        if name == "sc_pmsm_omega":  # the super-episode draw on its own
            sw, subs = _build(gem, ps, alternatives, p, 99)
            lengths, choices = np.empty(N_SAMPLES, dtype=np.int8), np.empty(N_SAMPLES, dtype=np.int8)
            for i in range(N_SAMPLES):
                sw._reset_reference()
                lengths[i], choices[i] = sw._current_episode_length, subs.index(sw._current_ref_generator)
            arrays["samples/length"], arrays["samples/choice"] = lengths, choices
            meta["samples"] = dict(p=list(p), super_episode_length=list(SUPER), n=N_SAMPLES)
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(out_path, **arrays)
    return out_path


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "refgen", "refgen_switched.npz"))
    a = ap.parse_args()
    print(record(a.out), os.path.getsize(a.out), "bytes")
