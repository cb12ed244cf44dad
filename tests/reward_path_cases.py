"""The cases of tests/test_gpu_reward_paths.py as data, and the deliberately WRONG restatements ("mutants") each case must tell from the
right one.  Plain numpy and json: it imports neither the reference nor the product, and nothing here comes from the reward description
the product derives -- weights and powers are the literals below, lengths are the reference's recorded `_state_length`
(tests/golden/env_defaults.json, by state name).

The device orders the terms of the sum as: the referenced states in column order (term t < n_ref is compared with reference column t),
then the other weighted states in column order (compared with 0).  The first four terms are evaluated from registers, the others in
a loop through memory; one power other than 1 or 2 sends EVERY term through that loop.  The mutants restate the ways this can go wrong.
"""
import json
import os

import numpy as np

from reward_restatement import error_terms, full_references

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "env_defaults.json")) as _f:
    DEFAULTS = json.load(_f)

HOT = 4  # terms the device keeps in registers

SYSTEMS = {"series": "Cont-SC-SeriesDc-v0", "shunt": "Cont-CC-ShuntDc-v0", "eesm": "Cont-CC-EESM-v0", "dfim": "Finite-CC-DFIM-v0"}  # 5, 6, 16, 24 columns

_EESM = DEFAULTS[SYSTEMS["eesm"]]["state_names"]
_DFIM = DEFAULTS[SYSTEMS["dfim"]]["state_names"]

# name: (system, referenced states, weights by state, powers by state (default 1), bias)
SHAPES = {
    # the series machine's speed has length 1: the default reward of the speed-control ids
    "series_default": ("series", ("omega",), dict(omega=1.0), {}, 0.0),
    # no reference at all, every column weighted: the fifth term (u_sup, length 1) is beyond the register terms
    "series_nref0_all5": ("series", (), dict(omega=0.2, torque=0.2, i=0.2, u=0.2, u_sup=0.2), dict(u=2), "positive"),
    # four references (the most the device takes), one of them with weight 0; the un-referenced u_sup is term 4
    "series_nref4_weight0": ("series", ("omega", "torque", "i", "u"), dict(omega=0.3, torque=0.2, i=0.3, u=0.0, u_sup=0.2), dict(torque=2, i=2), 0.0),
    # un-referenced weighted states before (omega, length 1) and after (u, u_sup) the referenced one in column order: four terms
    "shunt_before_after_4": ("shunt", ("i_a",), dict(omega=0.3, i_a=0.3, u=0.2, u_sup=0.2), dict(omega=2, u_sup=2), "positive"),
    # five terms, one power 0.5: the general path with a term beyond the register terms
    "shunt_5_half": ("shunt", ("i_a",), dict(omega=0.2, torque=0.2, i_a=0.3, i_e=0.1, u=0.2), dict(torque=0.5), 0.0),
    # every column; the power 3 sits on term 4 (u): terms are i_e, omega, torque, i_a, u, u_sup
    "shunt_all6_p3_beyond": ("shunt", ("i_e",), dict(omega=0.2, torque=0.1, i_a=0.2, i_e=0.2, u=0.2, u_sup=0.1), dict(torque=2, i_e=2, u=3), "positive"),
    "eesm_nref4_5": ("eesm", ("omega", "i_sd", "i_sq", "i_e"), dict(omega=0.2, i_sd=0.2, i_sq=0.2, i_e=0.2, u_sup=0.2), dict(i_sd=2, i_e=2), 0.0),
    "eesm_all16_ones": ("eesm", ("i_sq",), {n: 0.06 for n in _EESM}, {}, "positive"),
    "eesm_all16_general": ("eesm", ("omega", "i_sd", "i_sq", "i_e"), {n: 0.06 for n in _EESM},
                           dict({n: 1 + (i % 2) for i, n in enumerate(_EESM)}, i_sq=3, u_sq=0.5), 0.0),
    "dfim_nref4_all24": ("dfim", ("i_sd", "i_sq", "i_rd", "i_rq"), {n: 0.05 for n in _DFIM}, {n: 1 + (i % 2) for i, n in enumerate(_DFIM)}, 0.0),
    "dfim_nref0_4": ("dfim", (), dict(omega=0.25, i_sd=0.25, u_sd=0.25, u_sup=0.25), {}, "positive"),
    "dfim_nref1_p3": ("dfim", ("i_sq",), dict(omega=0.2, i_sq=0.4, u_sq=0.2, u_sup=0.2), dict(i_sq=3), 0.0),
}

# Runs in which the test ALSO asserts that terminations occurred and that other samples went on (the violation reward is asserted
# exact wherever `done` is set in every run): random armature voltages take the shunt machine's armature current past its limit
# within a few steps (a third of all samples in the fp64 CPU oracle), the EESM's within 37.
def must_terminate(shape, K):
    return K == 37 and (SHAPES[shape][0] == "shunt" or shape == "eesm_all16_ones")


K_VALUES = (1, 3, 4, 5, 7, 8, 9, 37)  # every remainder of the single-wave kernel's groups of four rows and of its double buffer of eight


def pruned_runs():
    """(shape, dtype, K, pipelined, n_envs): float32 -- every K through both kernels, with three shapes each, every shape
    through both kernels at two K each; float64 (which always takes the single-wave kernel) -- every shape at one K, every K used."""
    runs = []
    for j, shape in enumerate(SHAPES):
        for ki, K in enumerate(K_VALUES):
            for p in (0, 1):
                if (ki + 2 * p + j) % 4 == 0:
                    runs.append((shape, "float32", K, bool(p), (70, 128)[(ki + j) % 2]))
        runs.append((shape, "float64", K_VALUES[(5 * j + 3) % len(K_VALUES)], False, (70, 128)[j % 2]))
    return runs


class Case:
    """One reward shape on one system, with everything the restatement needs taken from the literals above and the recorded defaults."""

    def __init__(self, shape):
        system, refs, weights, powers, bias = SHAPES[shape]
        self.shape, self.env_id = shape, SYSTEMS[system]
        rec = DEFAULTS[self.env_id]
        # ('i_sum', which a wrapper of the reference's shunt envs appends, is not a column of the physical system)
        self.names = [n for n in rec["state_names"] if n != "i_sum"]
        n = len(self.names)
        length_of = dict(zip(rec["state_names"], rec["reward"]["_state_length"]))
        low, high = (dict(zip(rec["state_names"], rec["state_space"][k])) for k in ("low", "high"))
        assert all(length_of[s] == high[s] - low[s] for s in self.names)
        self.length = np.array([length_of[s] for s in self.names])
        self.weights = np.array([float(weights.get(s, 0.0)) for s in self.names])
        self.powers = np.array([float(powers.get(s, 1)) for s in self.names])
        assert set(weights) <= set(self.names) and set(powers) <= set(self.names) and set(refs) <= set(self.names)
        assert all(w == 0.0 or w >= 0.05 for w in self.weights)
        self.ref_names = [s for s in self.names if s in refs]  # column order
        self.ref_cols = [self.names.index(s) for s in self.ref_names]
        self.bias_arg = bias
        self.bias = float(self.weights.sum()) if bias == "positive" else float(bias)
        self.violation_reward = -3.5  # (a value that is exact in float32)
        self.set_reward_kwargs = dict(reward_weights={s: float(weights[s]) for s in weights}, reward_power={s: powers.get(s, 1) for s in self.names},
                                      bias=bias, violation_reward=self.violation_reward)
        # the device's term order
        self.term_cols = self.ref_cols + [i for i in range(n) if i not in self.ref_cols and self.weights[i] != 0.0]
        self.general = any(self.powers[c] not in (1.0, 2.0) for c in self.term_cols)
        self.paths = {
            "hot": not self.general,
            "beyond-hot": not self.general and len(self.term_cols) > HOT,
            "general": self.general,
            "general beyond-hot": self.general and any(self.powers[c] not in (1.0, 2.0) for c in self.term_cols[HOT:]),
            "n_ref 0": len(self.ref_cols) == 0,
            "n_ref 4": len(self.ref_cols) == 4,
            "length 1": any(self.length[c] == 1.0 and self.weights[c] != 0.0 for c in self.term_cols),
        }

    # ---------------------------------------------------------------- the right answer
    def terms(self, states, refs):
        """[..., n_states]: every state's share of the sum; states [..., n] float64, refs [..., n_ref] float64."""
        return error_terms(states, full_references(refs, self.ref_cols, len(self.names)), self.weights, self.powers, self.length)

    def reward(self, states, refs, done):
        return np.where(done, self.violation_reward, self.bias - self.terms(states, refs).sum(axis=-1))

    def scale(self, states, refs):
        """|bias| + sum_i w_i d_i ** n_i per sample: what the rounding errors of the sum are proportional to."""
        return abs(self.bias) + self.terms(states, refs).sum(axis=-1)

    # ---------------------------------------------------------------- the wrong answers
    def _by_term(self, states, refs, length=None, powers=None, keep=None, ref_of=None):
        """The sum written term by term in the device's order, with the pieces a mutant replaces: length / powers [n_term] per TERM,
        keep: number of terms summed, ref_of(t) -> reference column of term t or None."""
        cols = self.term_cols
        length = [self.length[c] for c in cols] if length is None else length
        powers = [self.powers[c] for c in cols] if powers is None else powers
        ref_of = (lambda t: t if t < len(self.ref_cols) else None) if ref_of is None else ref_of
        acc = np.zeros(states.shape[:-1])
        for t, c in enumerate(cols[:len(cols) if keep is None else keep]):
            j = ref_of(t)
            r = refs[..., j] if j is not None else 0.0
            acc = acc + self.weights[c] * (np.abs(states[..., c] - r) / length[t]) ** powers[t]
        return self.bias - acc

    def mutants(self):
        """name -> f(states, refs) of every mutation that changes this case's formula at all (decided from the case's structure, never
        from what the device returns).  A mutation that leaves the formula as it is (swapped powers where all powers are equal, dropped
        terms where there are four at most, ...) says nothing about the case and is left out; test_every_mutant_is_covered keeps count."""
        cols, n_ref = self.term_cols, len(self.ref_cols)
        w = [self.weights[c] for c in cols]
        out = {}
        if any(self.length[c] != 2.0 and w[t] for t, c in enumerate(cols)):
            out["all lengths 2"] = lambda s, r: self._by_term(s, r, length=[2.0] * len(cols))
        if any(self.length[t] != self.length[c] and w[t] for t, c in enumerate(cols)):
            out["len[t] for len[col]"] = lambda s, r: self._by_term(s, r, length=[self.length[t] for t in range(len(cols))])
        if any(w[t] for t in range(HOT, len(cols))):
            out["terms t >= 4 dropped"] = lambda s, r: self._by_term(s, r, keep=HOT)
        pair = next(((a, b) for a in range(len(cols)) for b in range(a + 1, len(cols))
                     if w[a] and w[b] and self.powers[cols[a]] != self.powers[cols[b]]), None)
        if pair is not None:
            p = [self.powers[c] for c in cols]
            p[pair[0]], p[pair[1]] = p[pair[1]], p[pair[0]]
            out["two powers swapped"] = lambda s, r: self._by_term(s, r, powers=p)
        if n_ref and any(w[t] for t in range(n_ref, len(cols))):
            out["un-referenced term against a reference"] = lambda s, r: self._by_term(s, r, ref_of=lambda t: t % n_ref)
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Tolerance.  MEASURED: the largest |device - restatement| / (|bias| + sum_i w_i d_i ** n_i) over every non-terminated sample of every
# run of pruned_runs() on an MI355X (profiles/reward_paths.md), by number format and by whether the case has a power other than 1 or 2.
# The tests assert FOUR times that (headroom for other seeds), and never more than the project's contract for the fused reward:
# 1e-4 x reward scale in float32, 1e-9 in float64 (tests/test_gpu_parity.py).
MEASURED = {("float32", False): 2.005e-07, ("float32", True): 1.630e-07, ("float64", False): 5.019e-16, ("float64", True): 3.742e-16}
CAP = {"float32": 1e-4, "float64": 1e-9}
HEADROOM = 4.0
MUTANT_FACTOR = 100.0  # a mutant differs from the right answer by at least this many tolerances on more than half of the samples


def bound(case, dtype, states, refs, reward_scale):
    """Per-sample bound on |device - restatement|."""
    return np.minimum(HEADROOM * MEASURED[(dtype, case.general)] * case.scale(states, refs), CAP[dtype] * reward_scale)
