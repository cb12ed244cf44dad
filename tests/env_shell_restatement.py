"""A host restatement of the COMPLETE env's step and reset with every stage on at once, in plain numpy and float64: the yardstick of
tests/test_env_shell_cpu.py (against recorded runs of the reference, tests/golden/env_shell/*.npz) and tests/test_gpu_env_shell.py
(against `ga.make(...)` envs on the device).

It shares no code with the package's env shells (envs.py, observation.py, episodes.py): it COMPOSES the restatements the suite already
has, in the order the reference's env shell prescribes (core.py `reset` / `step`, physical_system_wrappers/state_noise_processor.py:62-92,
gymnasium's TimeLimit and RecordEpisodeStatistics as episode_restatement.py restates them), per control step:

    1. the envs whose last step ENDED (terminated | truncated) restart: `if terminated or truncated: env.reset()`           physics
    2. one step of the fp64 C oracle per env (oracle.OracleEnv, no constraints inside: the shell decides)                      physics
    3. the noise draws of this stream position added to the named columns                                        StateNoiseProcessor
    4. `terminated` and the reward on the NOISY row, against the references the previous observation showed        core.py:344-349
    5. Episodes.step -> truncated, ended, the counters; a step that terminates and reaches the limit counts as terminated
    6. the flux observer on the noisy row (flux_observer.py:85-102), cleared where the episode ended
    7. the generators of the ended envs restart, every generator advances (core.py:351; a reset shows a fresh sub-episode's first value)
    8. the observation-side wrappers, the state filter and the flat observation (obs_stage_restatement.simulate_chain)

TWO inputs are random streams that no host code restates; they are handed in, not computed here:
  * the noise, `draws[k, env, slot]`: on the device from `StateNoiseStage.draws(step0, K)`, in the CPU test the reference's own rows;
  * each sub-episode's waveform parameters, `param_sets[column][env]`: a list of dicts(length, amplitude, frequency, offset, phase, width,
    roll) in the order drawn -- on the device read through `reference_generator.state()`, in the CPU test recorded from the reference.
What the shell decides by itself is WHEN and FOR WHOM each stream position and each parameter set applies: it keeps its own stream
position, its own step index inside every sub-episode, and takes the next parameter set whenever ITS rules start a sub-episode.

From the package it takes only the flux observer's float64 host restatement (an object handed in: `host_reset`, `evaluate`,
`host_actions`).  The shell also reports the constraint margin of every lane and step, |max expression - 1| (the expressions: |x| of a
limited column, the sum of squares of the squared set), and `terminated` of the clean row.
"""
import numpy as np

import obs_stage_restatement as osr
import refgen_waveforms as rw
import reward_restatement as rr
from episode_restatement import Episodes

PARAM_KEYS = ("length", "amplitude", "frequency", "offset", "phase", "width", "roll")


def reward_description(state_names, state_space_low, state_space_high, referenced_states, gamma=0.9):
    """The arrays WeightedSumOfErrors.set_modules derives for the env ids' default reward (weighted_sum_of_errors.py:97-123): equal
    weights over the referenced states, power 1, no bias, violation reward min(-sum(w) / (1 - gamma), 0)."""
    n = len(state_names)
    w = np.zeros(n)
    for s in referenced_states:
        w[list(state_names).index(s)] = 1.0 / len(referenced_states)
    length = np.asarray(state_space_high, dtype=np.float64)[:n] - np.asarray(state_space_low, dtype=np.float64)[:n]
    return dict(weights=w, powers=np.ones(n), state_length=length, bias=0.0, violation_reward=min(-float(w.sum()) / (1.0 - gamma), 0.0))


def mask_columns(mask):
    return [i for i in range(64) if mask >> i & 1]


class EnvShell:
    """oracle_params: OrcParams WITHOUT constraints (episodic=False); n_envs; state_names of the base system;
    limit_columns / squared_columns: the constraint set; noise_columns: None | the noisy columns in slot order;
    reward: dict(weights, powers, state_length, bias, violation_reward) over the base system's states; generators: per reference column
    (ascending state order) dict(kind, state, margin); param_sets: see the module docstring; tau;
    max_steps: 0 | the time limit; restart: whether an ended env restarts (False: nobody resets it);
    observer: None | the flux observer's host restatement; dq_actions: actions are (u_d, u_q) pairs in its frame;
    chain / observed_states / flatten: the observation side (obs_stage_restatement specs over the wrapped names)."""

    def __init__(self, oracle_params, n_envs, state_names, limit_columns=(), squared_columns=(), noise_columns=None, reward=None, generators=(),
                 param_sets=None, tau=1e-4, max_steps=0, restart=True, observer=None, dq_actions=False, chain=(), observed_states=None, flatten=False):
        from oracle import oracle as orc

        self.n = int(n_envs)
        self.names = list(state_names)
        self.envs = [orc.OracleEnv(oracle_params) for _ in range(self.n)]
        self.limit_columns, self.squared_columns = list(limit_columns), list(squared_columns)
        self.noise_columns = None if noise_columns is None else list(noise_columns)
        self.reward_cfg = reward
        self.generators = list(generators)
        self.ref_columns = [self.names.index(g["state"]) for g in self.generators]
        assert self.ref_columns == sorted(self.ref_columns)
        self.param_sets, self.tau = param_sets, float(tau)
        self.max_steps, self.restart = int(max_steps), bool(restart)
        self.observer, self.dq_actions = observer, bool(dq_actions)
        self.wrapped = self.names + (["psi_abs", "psi_angle"] if observer is not None else [])
        self.chain = list(chain)
        out_names = osr.wrapped_names(self.wrapped, self.chain)
        self.state_filter = None if observed_states is None else [out_names.index(s) for s in observed_states]
        self.flatten = bool(flatten)

    # ------------------------------------------------------------------ the pieces
    def _expressions(self, row):
        e = [abs(row[c]) for c in self.limit_columns]
        if self.squared_columns:
            e.append(float(np.sum(row[self.squared_columns] ** 2)))
        return max(e) if e else 0.0

    def _noisy(self, rows):
        out = rows.copy()
        if self.noise_columns is not None:
            out[:, self.noise_columns] += np.asarray(self.draws[self.position], dtype=np.float64)
            self.position += 1
        return out

    def _advance_generators(self, restart):
        """The generators of the `restart` envs begin a fresh sub-episode, so does every one whose sub-episode is over
        (subepisoded_reference_generator.py:85-102); then every generator shows its next value."""
        for c, g in enumerate(self.generators):
            for j in range(self.n):
                if restart[j] or self._index[c][j] >= self._params[c]["length"][j]:
                    sets = self.param_sets[c][j]
                    if self._taken[c][j] >= len(sets):
                        raise IndexError(f"reference column {c}, env {j}: the shell starts sub-episode {self._taken[c][j]}, only {len(sets)} parameter sets were drawn")
                    for key in PARAM_KEYS:
                        self._params[c][key][j] = sets[self._taken[c][j]][key]
                    self._taken[c][j] += 1
                    self._index[c][j] = 0
            p = self._params[c]
            value, on_jump, _ = rw.evaluate(g["kind"], self._index[c], p["length"], self.tau, p["amplitude"], p["frequency"], p["offset"], tuple(g["margin"]),
                                            phase=p["phase"], width=p["width"], roll=p["roll"])
            self.refs[:, c], self.ref_on_jump[:, c] = value, on_jump
            self._index[c] += 1

    def _observation(self, rows):
        state = osr.simulate_chain(rows, self.wrapped, self.chain, self.state_filter)
        return np.concatenate((state, self.refs), axis=-1) if self.flatten else state

    # ------------------------------------------------------------------ reset / step
    def reset(self, draws=None, position=0):
        """`env.reset()`: -> dict(state, refs, obs).  draws [.., N, n_noisy]: the stream; position: the row the reset state takes."""
        n = self.n
        self.draws, self.position = draws, int(position)
        rows = np.stack([e.reset() for e in self.envs])
        self.reset_row = rows[0].copy()
        self.state = self._noisy(rows)
        self.pending = np.zeros(n, dtype=bool)
        self.episodes = Episodes(n, self.max_steps)
        self.refs, self.ref_on_jump = np.zeros((n, len(self.generators))), np.zeros((n, len(self.generators)), dtype=bool)
        self._index = [np.zeros(n, dtype=np.int64) for _ in self.generators]
        self._taken = [np.zeros(n, dtype=np.int64) for _ in self.generators]
        self._params = [{k: np.zeros(n) for k in PARAM_KEYS} for _ in self.generators]
        self._advance_generators(np.ones(n, dtype=bool))
        self.rows = self.state
        if self.observer is not None:
            self.observer.auto_reset = True  # (the shell hands over its own mask)
            self.observer.set_reset_observation(self.reset_row)
            self.observer.host_reset(n)
            self.rows = np.concatenate((self.state, np.zeros((n, 2))), axis=-1)
        return dict(state=self.rows.copy(), refs=self.refs.copy(), obs=self._observation(self.rows))

    def step(self, actions):
        """actions [N, A] | [N] -> dict of this step's arrays (see the keys below)."""
        n = self.n
        a = np.asarray(actions, dtype=np.float64).reshape(n, -1)
        if self.dq_actions:  # rotated by the frame the last observation (or the reset) left
            a = self.observer.host_actions(a)
        clean = np.empty((n, len(self.names)))
        psi_r = np.zeros(n)
        for j, e in enumerate(self.envs):
            if self.pending[j]:
                e.reset()
            if self.observer is not None:
                psi_r[j] = np.hypot(e.y[3], e.y[4])  # |psi_r| at the START of the step: the conditioning of the field-oriented columns
            clean[j] = e.step(a[j])
        noisy = self._noisy(clean)
        expr = np.array([self._expressions(r) for r in noisy])
        terminated = expr > 1.0
        clean_terminated = np.array([self._expressions(r) for r in clean]) > 1.0
        reward = None
        if self.reward_cfg is not None:
            c = self.reward_cfg
            full = rr.full_references(self.refs, self.ref_columns, len(self.names))
            reward = rr.reward(noisy, full, terminated, c["weights"], c["powers"], c["state_length"], c["bias"], c["violation_reward"])
        truncated, ended, _ = (x.astype(bool) for x in self.episodes.step(terminated, reward))
        rows = noisy
        if self.observer is not None:
            rows = self.observer.evaluate(noisy[None], done=(ended if self.restart else np.zeros(n, dtype=bool))[None])[0]
        self._advance_generators(ended)
        self.pending = ended if self.restart else np.zeros(n, dtype=bool)
        self.state, self.rows = noisy, rows
        return dict(state=rows.copy(), clean=clean, refs=self.refs.copy(), ref_on_jump=self.ref_on_jump.copy(), reward=reward, terminated=terminated,
                    clean_terminated=clean_terminated, truncated=truncated, ended=ended, margin=np.abs(expr - 1.0), psi_r=psi_r,
                    obs=self._observation(rows), statistics={k: v.copy() for k, v in self.episodes.fields().items()})

    def run(self, actions, draws=None, position=0):
        """reset + K steps -> (the reset's dict, dict of the steps' arrays stacked on a leading axis [K, ...])."""
        first = self.reset(draws, position)
        steps = [self.step(a) for a in actions]
        out = {}
        for k in steps[0]:
            if k == "statistics":
                out[k] = {f: np.stack([s[k][f] for s in steps]) for f in steps[0][k]}
            elif steps[0][k] is not None:
                out[k] = np.stack([s[k] for s in steps])
        return first, out


def first_close_call(margin, done_margin):
    """margin [K, N] -> [N]: the first step whose margin is below `done_margin` (K: none).  A lane is compared BEFORE that step only,
    values, masks and counters alike: the step itself and everything behind it count as left out."""
    close = np.asarray(margin) < done_margin
    return np.where(close.any(axis=0), close.argmax(axis=0), close.shape[0])
