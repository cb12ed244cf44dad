"""Device-side observation stage: what the reference's observation-side physical-system wrappers, the env shell's `state_filter`
and gymnasium's FlattenObservation do to a state, as ONE kernel launch over the state rows the stepping kernels wrote
(csrc/gemx_obsproc.hip, include/gemx.h: gemx_obsproc_*).

`ObservationStage(physical_system, chain, observed_states=None, flatten=False, n_ref=0)` resolves the chain the way the reference's
`set_physical_system` calls do -- innermost first, every processor seeing the state names of what is beneath it -- into

* the metadata the WRAPPED system shows: `state_names`, `state_positions`, `limits`, `nominal_state`, `state_space`
  (current_sum_processor.py:24-44, cos_sin_processor.py:33-50), plus `state_filter` (core.py:273-277: indices into those names) and
  `observation_names` / `observation_space` (the filtered state the observation carries);
* a flat COLUMN PROGRAM over the base system's columns, one entry `(op, src, mask)` per observed column: COPY a column, SUM the columns
  of a bit mask, cos / sin of pi times a column.  The program is one level deep: a processor whose source is itself a derived column
  (`CosSinProcessor(angle='i_sum')`, a current sum over another `i_sum`) is refused by name.

A `FluxObserver` in the chain (`('flux', wrapper)`; induction machines) is a stage of its own IN FRONT of the program (flux_observer.py,
csrc/gemx_fluxobs.hip): it extends the system's row by `psi_abs` and `psi_angle`, and the program then runs over that extended row of
`n_in = n_base + 2` columns -- `CosSinProcessor(angle='psi_angle')`, `observed_states=` and `flatten` work as for any other column, at any
position of the chain.  The observer's own sources (its three currents) must be columns of the base system.  `stage.flux` is the
`FluxObserverStage`; `evaluate(state [K, (N,) n_base], done=...)` runs its float64 recursion first (stateful over the trajectory).

`remove_angle=True`: the reference's CosSinProcessor deletes the angle in `simulate()` but forgets to in `reset()`
(cos_sin_processor.py:52-55 against 57-62), so its reset state is one column longer than its step state and than its own state space.
A batched tensor has one shape: the stage uses `simulate()`'s -- the shape the wrapper's `state_space`, `state_names` and `limits`
describe -- everywhere, reset included.

`apply(state [..., n_in], refs=None, out=None)` runs the program on any contiguous trajectory; `evaluate(state)` is the same program on
the host in numpy (float64 unless told otherwise), for tests and for data that never was on a device.
"""
import ctypes as C

import numpy as np

from . import _lib
from .spaces import Box

_OPS = {"copy": _lib.OBS_COPY, "sum": _lib.OBS_SUM, "cospi": _lib.OBS_COSPI, "sinpi": _lib.OBS_SINPI}


class _Column:
    __slots__ = ("name", "op", "src", "mask", "limit", "nominal", "low", "high")

    def __init__(self, name, op, src, mask, limit, nominal, low, high):
        self.name, self.op, self.src, self.mask = name, op, src, mask
        self.limit, self.nominal, self.low, self.high = float(limit), float(nominal), float(low), float(high)


def _source(col, what):
    if col.op != "copy":
        raise ValueError(f"{what}: its source {col.name!r} is itself a derived column; the device-side column program is one level deep "
                         "(sources must be states of the base physical system)")
    return col.src


class ObservationStage:
    """The resolved observation stage of one physical system (see the module docstring)."""

    def __init__(self, physical_system, chain=(), observed_states=None, flatten=False, n_ref=0, flux_action=None):
        ps = physical_system
        names = [str(n) for n in ps.state_names]
        self.n_in = self.n_base = len(names)
        self.flux = None
        self.n_ref = int(n_ref)
        self.flatten = bool(flatten)
        if not 0 <= self.n_ref <= _lib.MAX_REF:
            raise ValueError(f"n_ref must be in [0, {_lib.MAX_REF}]")
        low, high = np.asarray(ps.state_space.low, dtype=float), np.asarray(ps.state_space.high, dtype=float)
        cols = [_Column(n, "copy", j, 0, ps.limits[j], ps.nominal_state[j], low[j], high[j]) for j, n in enumerate(names)]
        positions = {n: j for j, n in enumerate(names)}
        self.chain = tuple(chain)
        for spec in self.chain:
            if spec[0] == "sum":
                _, currents, limit = spec
                idx = [positions[c] for c in currents]  # (KeyError for an unknown name, as current_sum_processor.py:27)
                if len(set(idx)) != len(idx) or not idx:
                    raise ValueError(f"CurrentSumProcessor({list(currents)}): the currents must be distinct and at least one")
                mask = 0
                for i in idx:
                    mask |= 1 << _source(cols[i], f"CurrentSumProcessor({list(currents)})")
                f = max if limit == "max" else np.sum
                cols.append(_Column("i_sum", "sum", 0, mask, f(np.array([cols[i].limit for i in idx])), f(np.array([cols[i].nominal for i in idx])), -1.0, 1.0))
                positions = dict(positions)
                positions["i_sum"] = [c.name for c in cols].index("i_sum")
            elif spec[0] == "cossin":
                _, angle, remove = spec
                i = positions[angle]  # (KeyError for an unknown name, as cos_sin_processor.py:36)
                src = _source(cols[i], f"CosSinProcessor({angle!r})")
                if remove:
                    del cols[i]
                cols.append(_Column(f"cos({angle})", "cospi", src, 0, 1.0, 1.0, -1.0, 1.0))
                cols.append(_Column(f"sin({angle})", "sinpi", src, 0, 1.0, 1.0, -1.0, 1.0))
                positions = {c.name: j for j, c in enumerate(cols)}
            elif spec[0] == "flux":
                from .flux_observer import FluxObserverStage

                probe = FluxObserverStage(ps, action_mode=flux_action)  # (the motor check: before any attribute of the wrapper is read)
                currents = tuple(getattr(spec[1], "_current_names", ("i_sa", "i_sb", "i_sc")))
                idx = []
                for c in currents:
                    src = _source(cols[positions[c]], f"FluxObserver({list(currents)})")  # (KeyError for an unknown name, as flux_observer.py:70)
                    if src >= self.n_base:
                        raise ValueError(f"FluxObserver({list(currents)}): its source {c!r} is not a state of the base physical system")
                    idx.append(src)
                self.flux = FluxObserverStage(ps, currents, action_mode=flux_action, current_indices=idx)
                del probe
                for j, (name, limit, nominal, lo, hi) in enumerate(self.flux.columns):
                    cols.append(_Column(name, "copy", self.n_base + j, 0, limit, nominal, lo, hi))
                self.n_in = self.n_base + 2
                positions = {c.name: j for j, c in enumerate(cols)}
            else:
                raise ValueError(f"unknown observation-stage spec {spec!r}")
        if flux_action and self.flux is None:
            raise ValueError("the flux-oriented dq action processor needs a FluxObserver in the chain")
        # the wrapped system's metadata
        self.state_names = [c.name for c in cols]
        self.state_positions = positions
        self.limits = np.array([c.limit for c in cols])
        self.nominal_state = np.array([c.nominal for c in cols])
        self.state_space = Box(np.array([c.low for c in cols]), np.array([c.high for c in cols]), dtype=np.float64)
        # the env shell's state_filter, applied last (core.py:273-277)
        observed = list(observed_states) if observed_states is not None else list(self.state_names)
        self.state_filter = [self.state_names.index(s) for s in observed]
        if not self.state_filter:
            raise ValueError("observed_states selects no state")
        self._cols = [cols[i] for i in self.state_filter]
        self.observation_names = [c.name for c in self._cols]
        self.observation_space = Box(self.state_space.low[self.state_filter], self.state_space.high[self.state_filter], dtype=np.float64)
        self.n_post = len(self._cols)
        if self.n_post > _lib.OBS_MAX_POST:
            raise ValueError(f"the observation has {self.n_post} columns, the device-side stage at most {_lib.OBS_MAX_POST}")
        if self.n_base > _lib.MAX_OUT:
            raise ValueError(f"the physical system has {self.n_base} states, the device-side stage reads at most {_lib.MAX_OUT}")
        self.n_out = self.n_post + (self.n_ref if self.flatten else 0)
        if self.n_in > _lib.MAX_OUT and not (not self.flatten and self.n_post == self.n_in and all(c.op == "copy" and c.src == j for j, c in enumerate(self._cols))):
            raise NotImplementedError(f"the column program reads rows of at most {_lib.MAX_OUT} columns (gemx_obsproc_create); the flux observer's extended "
                                      f"row of this system has {self.n_in}: it can be handed out as it is, but not processed further (CosSinProcessor, "
                                      "observed_states, flatten_observation)")
        self.program = [(c.op, c.src, c.mask) for c in self._cols]
        self._cfg = self._build_config()
        self._handle = None

    @property
    def is_identity(self):
        return not self.flatten and self.n_post == self.n_in and all(op == "copy" and src == j for j, (op, src, _) in enumerate(self.program))

    def _build_config(self):
        cfg = _lib.GemxObsprocConfig()
        cfg.struct_size = C.sizeof(_lib.GemxObsprocConfig)
        cfg.n_in, cfg.n_post, cfg.n_ref, cfg.flat = self.n_in, self.n_post, self.n_ref, int(self.flatten)
        for c, (op, src, mask) in enumerate(self.program):
            cfg.entries[c].op, cfg.entries[c].src, cfg.entries[c].mask = _OPS[op], src, mask
        return cfg

    # ------------------------------------------------------------------ host-side evaluator
    def evaluate(self, state, refs=None, dtype=np.float64, done=None):
        """The program in numpy on `state [..., n_in]` (computed in `dtype`; sums sequentially in ascending column order, as the kernel
        adds them) -> [..., n_post], or with `flatten` [..., n_post + n_ref].  With a FluxObserver, rows of the BASE system
        `[K, (N,) n_base]` first go through its float64 recursion (`done [K, (N)]`: the lanes reset after that row)."""
        if self.flux is not None and np.shape(state)[-1] == self.n_base:
            state = self.flux.evaluate(state, done)
        s = np.asarray(state, dtype=dtype)
        if s.shape[-1] != self.n_in:
            raise ValueError(f"state has {s.shape[-1]} columns, the stage reads {self.n_in}")
        out = np.empty(s.shape[:-1] + (self.n_out,), dtype=dtype)
        for c, (op, src, mask) in enumerate(self.program):
            if op == "copy":
                out[..., c] = s[..., src]
            elif op == "sum":
                js = [j for j in range(self.n_in) if mask >> j & 1]
                acc = s[..., js[0]].copy()
                for j in js[1:]:
                    acc = acc + s[..., j]
                out[..., c] = acc
            else:
                x = s[..., src].astype(np.float64) * np.pi
                out[..., c] = (np.cos(x) if op == "cospi" else np.sin(x)).astype(dtype)
        if self.flatten and self.n_ref:
            out[..., self.n_post:] = np.asarray(refs, dtype=dtype).reshape(s.shape[:-1] + (self.n_ref,))
        return out

    # ------------------------------------------------------------------ device side
    def create(self, device, dtype_name="float32"):
        """Create the device handle (no CPU fallback: without a HIP device this raises)."""
        import torch

        L = _lib.load()
        h = C.c_void_p()
        _lib.check(L.gemx_obsproc_create(C.byref(self._cfg), _lib.F64 if dtype_name == "float64" else _lib.F32, int(device), C.byref(h)))
        self._handle, self._L = h, L
        self._tdev = torch.device("cuda", int(device))
        self._tdtype = torch.float64 if dtype_name == "float64" else torch.float32
        return self

    def close(self):
        if getattr(self, "_handle", None) is not None:
            self._L.gemx_obsproc_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, t, cols, what):
        import torch

        if not (torch.is_tensor(t) and t.device == self._tdev and t.dtype == self._tdtype and t.is_contiguous() and t.dim() >= 1 and t.shape[-1] == cols):
            raise ValueError(f"{what} must be a contiguous {self._tdtype} tensor [..., {cols}] on {self._tdev}")

    def apply(self, state, refs=None, out=None, stream=None):
        """state [..., n_in] (contiguous device tensor) -> out [..., n_post] (or [..., n_post + n_ref] with `flatten`, reading refs
        [..., n_ref]).  One kernel launch on `stream` (default: the current one); `out` is allocated unless given and must not alias
        the inputs."""
        return self.bind_apply(state, refs, out, stream)()

    def bind_apply(self, state, refs, out, stream=None):
        """-> zero-argument launch() of `apply` on fixed tensors, returning `out`: everything is checked and resolved here, once (`out`
        None: allocated here; `stream` None: the one current now)."""
        import torch

        if self._handle is None:
            raise _lib.GemxError("the observation stage has no device handle (built with _defer_create, or closed)")
        self._check(state, self.n_in, "state")
        lead = tuple(state.shape[:-1])
        need_refs = self.flatten and self.n_ref > 0
        if need_refs:
            if refs is None:
                raise ValueError(f"a flat observation needs refs [..., {self.n_ref}]")
            self._check(refs, self.n_ref, "refs")
            if tuple(refs.shape[:-1]) != lead:
                raise ValueError(f"refs {tuple(refs.shape)} do not match state {tuple(state.shape)}")
        if out is None:
            out = torch.empty(lead + (self.n_out,), dtype=self._tdtype, device=self._tdev)
        else:
            self._check(out, self.n_out, "out")
            if tuple(out.shape[:-1]) != lead:
                raise ValueError(f"out {tuple(out.shape)} does not match state {tuple(state.shape)}")
        stream = stream if stream is not None else torch.cuda.current_stream(self._tdev)
        args = (C.c_void_p(state.data_ptr()), C.c_void_p(refs.data_ptr()) if need_refs else None, state.numel() // self.n_in, C.c_void_p(out.data_ptr()),
                C.c_void_p(stream.cuda_stream))
        return _lib.bound_call(self._L.gemx_obsproc_apply, self, args, (state, refs, out, stream), out)


class ObservationPipeline:
    """Everything between a physical system's raw state rows and the state an env hands out, for BOTH env shells, and the one place
    where the order of the launches around the physics lives:

        the masked reset of the envs the last NOISY row terminated, IN FRONT of the physics    (with a StateNoiseProcessor: `noise`;
                                                             with a time limit: of the envs in the episode stage's `reset_mask`)
        the noise on the raw rows, done and reward on the noisy row -> `noisy` [N, n_base]    (with a StateNoiseProcessor)
        the episode stage on that step's done byte and reward -> truncated, ended, reset_mask  (with a time limit / episode statistics)
        the flux observer on the raw (noisy) rows -> `rows` [.., n_base + 2]      (when the chain holds a FluxObserver)
        the column program on those rows, reading the references when the observation is flat -> `state`   (unless it is the identity)

    `observation`: None (no stage: `state` is the system's own buffer and nothing is launched) or dict(chain=, observed_states=,
    flatten=); `n_ref`: the reference columns a flat observation carries; `flux_action`: None | 'SCIM' | 'DFIM', the flux-oriented dq
    action processor.  Owns the stage, the observer, `rows`, the dq processor's `abc` scratch, the `state` buffer and the raw and
    extended scratch trajectories of the K-step rollouts; every refusal of a combination is raised here.
    `noise`: None or the StateNoiseProcessor's spec (state_noise.py) with the constraint masks and the auto-reset the user asked for -- the
    system itself then has neither; `reward_config`: the reward the noise stage evaluates on the noisy row (the complete env's).  The
    system's own `done` buffer carries the NOISY done mask: the physics clears it, the noise stage behind it writes it, and the reset in
    front of the next physics reads it.
    `episode`: None or dict(max_steps=, statistics=) -- the episode stage (episodes.py) directly behind the launch that produces reward and
    done; `episode_reward`: whether it reads a reward (the complete env's).  With the stage, `ended` = done | truncated replaces `done` as the
    byte the generators restart on and the observer resets on (`restart_mask`), and with a time limit `reset_mask` is the mask of the reset
    in front of the next physics: a truncated env is `env.reset()` in the reference."""

    AFTER_STEP = ("noise", "episode", "observer", "generators", "program")  # THE order of the launches behind a step's physics

    def __init__(self, physical_system, observation=None, n_ref=0, flux_action=None, defer_create=False, noise=None, reward_config=None, episode=None,
                 episode_reward=False):
        ps = self.physical_system = physical_system
        self.stage = self.flux = self.flux_action = self.raw_scratch = self.ext_scratch = self.noise = self.episode = None
        self.ended_scratch = self.finished_return_scratch = self.finished_length_scratch = None
        self.truncated = False  # (what `step()` hands out in the fourth slot; with a time limit: the bool view of the stage's bytes)
        self.flux_only = self.has_program = False
        self.action_space = ps.action_space
        if noise is not None:
            from .state_noise import REFUSAL, StateNoiseStage

            if getattr(ps, "_obs_layout", "aos") != "aos":
                raise NotImplementedError(REFUSAL + "obs_layout='soa' was asked for")
            self.noise = StateNoiseStage(ps, noise, reward_config)
        if observation is None:
            if flux_action:
                raise ValueError("the flux-oriented dq action processor needs a FluxObserver")
        else:
            if getattr(ps, "_obs_layout", "aos") != "aos":
                raise ValueError("the observation stage reads state rows: it needs obs_layout='aos', not 'soa'")
            stage = self.stage = ObservationStage(ps, observation.get("chain", ()), observation.get("observed_states"), observation.get("flatten", False),
                                                  n_ref=n_ref, flux_action=flux_action)
            self.flux, self.flux_action = stage.flux, flux_action
            if self.flux is not None and self.noise is not None:
                self.flux.auto_reset = self.noise.auto_reset  # (the system itself runs without auto-reset: the observer follows the env's)
            self.flux_only = self.flux is not None and stage.is_identity  # (the extended row IS the observation: no column program to run)
            self.has_program = not self.flux_only
            if flux_action:
                if ps._cfg.init_kind != _lib.INIT_CONST:
                    raise NotImplementedError("random initial states together with the flux-oriented dq action processor are not on the accelerated path: "
                                              "the frame of the first action after a reset comes from the reset observation, which would not be a constant")
                self.action_space = Box(-1, 1, shape=(self.flux.n_action,), dtype=np.float64)
        if episode is not None:
            from .episodes import EpisodeStage

            # (under a StateNoiseProcessor the system is built without auto-reset: the stepping kernel restarts nothing)
            in_kernel = bool(getattr(ps, "_auto_reset", False)) and self.noise is None
            self.episode = EpisodeStage(episode.get("max_steps"), episode.get("statistics", False), in_kernel, has_reward=episode_reward)
            if self.flux is not None and self.episode.max_steps:
                self.flux.auto_reset = True  # (every env in `ended` restarts, by the kernel or by the masked reset: the observer follows)
        if defer_create:
            return
        import torch

        new = lambda *shape: torch.zeros(shape, dtype=ps._tdtype, device=ps._tdev)  # noqa: E731
        self.rows = self.state = ps._obs
        if self.noise is not None:
            self.noise.create(ps.n_envs, ps._device, ps._dtype_name)
            self.noisy = self.rows = self.state = new(ps.n_envs, self.noise.n_in)
            self._reset_done = torch.zeros(ps.n_envs, dtype=torch.uint8, device=ps._tdev)  # (a reset row is noised, never checked: core.py:312)
        if self.flux is not None:
            self.flux.set_reset_observation(ps.reset_observation)
            self.flux.create(ps.n_envs, ps._device, ps._dtype_name)
            self.rows = self.state = new(ps.n_envs, self.flux.n_in + 2)
            if flux_action:
                self.abc = new(ps.n_envs, self.flux.n_action * 3 // 2)
        if self.has_program:
            self.stage.create(ps._device, ps._dtype_name)
            self.state = new(ps.n_envs, self.stage.n_out)
        if self.episode is not None:
            self.episode.create(ps.n_envs, ps._device, ps._dtype_name)
            if self.episode.max_steps:
                self.truncated = self.episode.truncated.view(torch.bool)

    @property
    def restart_mask(self):
        """[N] uint8: the envs that restart after this step -- `ended` with an episode stage, else the system's `done`."""
        return self.physical_system._done if self.episode is None else self.episode.ended

    def _reset_source(self):
        """Whose mask the reset in front of the physics reads: None (no such launch), 'episode' or 'noise'."""
        if self.episode is not None and self.episode.max_steps:
            return "episode"
        return "noise" if self.noise is not None and self.noise.auto_reset else None

    def launch_order(self, generators=False):
        """The names of a step's launches, in order, as `bind_before_step` / `bind_after_step` resolve them (needs no device)."""
        present = dict(noise=self.noise is not None, episode=self.episode is not None, observer=self.flux is not None, generators=bool(generators),
                       program=self.has_program)
        return (["actions"] if self.flux_action else []) + (["reset"] if self._reset_source() else []) + ["physics"] + [n for n in self.AFTER_STEP if present[n]]

    def refuse_rollout(self):
        if self.episode is not None and self.episode.max_steps:
            from .episodes import ROLLOUT_REFUSAL as EPISODE_ROLLOUT_REFUSAL

            raise NotImplementedError(EPISODE_ROLLOUT_REFUSAL)
        if self.noise is not None:
            from .state_noise import ROLLOUT_REFUSAL as NOISE_ROLLOUT_REFUSAL

            raise NotImplementedError(NOISE_ROLLOUT_REFUSAL)
        if self.flux_action:
            from .flux_observer import ROLLOUT_REFUSAL

            raise NotImplementedError(ROLLOUT_REFUSAL)

    def need_episodic(self):
        """What the episodic rollouts (the time limit inside the fused launch) need of this env, checked before anything is launched and
        without a device: a time limit (ValueError without one), no stage whose mask another launch decides, and a physical system the
        episodic kernel serves (NotImplementedError, one message each: episodes.episodic_refusal)."""
        from .episodes import EPISODIC_REFUSAL, NO_TIME_LIMIT, episodic_refusal

        if self.episode is None or not self.episode.max_steps:
            raise ValueError(NO_TIME_LIMIT)
        if self.noise is not None:
            raise NotImplementedError(EPISODIC_REFUSAL + "a StateNoiseProcessor: its done mask is decided on the noisy row by another launch, which a "
                                      "fused launch has not seen")
        if self.flux_action:
            raise NotImplementedError(EPISODIC_REFUSAL + "a FluxOrientedDqToAbcActionProcessor: each step's action frame comes from the previous step's "
                                      "observation")
        why = episodic_refusal(self.physical_system)
        if why is not None:
            raise NotImplementedError(why)

    def _scratch(self, name, shape, dtype=None):
        ps, buf = self.physical_system, getattr(self, name)
        if buf is None or tuple(buf.shape) != shape:
            import torch

            buf = torch.empty(shape, dtype=dtype or ps._tdtype, device=ps._tdev)
            setattr(self, name, buf)
        return buf

    def raw_rows(self, K, out, last_only=False):
        """Where the physics of a K-step rollout writes: `out` itself without a stage, else the raw scratch trajectory."""
        if self.stage is None:
            return out
        shape = tuple(self.physical_system._obs.shape)
        return self._scratch("raw_scratch", shape if last_only else (K,) + shape)

    # ------------------------------------------------------------------ the launches around the physics
    def bind_before_step(self, stream=None):
        """-> zero-argument launch() of what precedes a step's physics, or None: with a StateNoiseProcessor (and auto-reset) the masked
        `gemx_reset` of the envs whose last noisy row terminated -- one asynchronous launch, no observation written, no host state.  With
        a time limit the mask is the episode stage's `reset_mask` instead (the truncated envs; behind a StateNoiseProcessor or with
        auto_reset=False every ended env): still one launch."""
        source = self._reset_source()
        if source is None:
            return None
        import torch

        ps = self.physical_system
        mask = self.episode.reset_mask if source == "episode" else ps._done
        stream = stream if stream is not None else torch.cuda.current_stream(ps._tdev)
        args = (C.c_void_p(mask.data_ptr()), None, C.c_void_p(stream.cuda_stream))
        return _lib.bound_call(ps._L.gemx_reset, ps, args, (mask, stream))

    def before_step(self):
        """`bind_before_step` on the current stream, run once."""
        launch = self.bind_before_step()
        if launch is not None:
            launch()

    def bind_after_step(self, refs=None, stream=None, generators=None, reward=None, returns=None):
        """-> zero-argument launch() of what follows a step's physics, or None when there is nothing to run, in the order AFTER_STEP: the
        noise stage on the system's fresh rows (noisy rows, the done mask and -- `reward` [N] given -- the reward against `refs` as they
        stand, i.e. as the previous observation showed them), the episode stage on the done mask and `returns` (the [N] reward of this step,
        whichever launch wrote it), the observer on the (noisy) rows and `restart_mask`, then `generators` (the complete env's reference
        step, bound on `restart_mask`: a flat observation carries what it writes into `refs` [N, n_ref]), then the column program into `state`."""
        ps = self.physical_system
        bound, src = dict(generators=generators), ps._obs
        if self.noise is not None:
            bound["noise"], src = self.noise.bind_step(ps._obs, refs, self.noisy, ps._done, reward, stream), self.noisy
        if self.episode is not None:
            bound["episode"] = self.episode.bind_step(ps._done, returns if self.episode.has_reward else None, stream=stream)
        if self.flux is not None:
            bound["observer"] = self.flux.bind_step(src, self.restart_mask, self.rows, stream)
        if self.has_program:
            bound["program"] = self.stage.bind_apply(self.rows, refs, self.state, stream)
        return _lib.sequence(*(bound.get(name) for name in self.AFTER_STEP))

    def after_step(self, refs=None):
        """`bind_after_step` on the current stream, run once -> `state`."""
        launch = self.bind_after_step(refs)
        if launch is not None:
            launch()
        return self.state

    def bind_after_rollout(self, raw, done, refs, out, stream=None):
        """-> zero-argument launch() of what follows a K-step rollout's physics, returning `out` (None: allocated here), or None without a
        stage (`raw` is the result): ONE pass of the observer over the stored rows `raw` [K, N, n_base] and `done` [K, N], then the column
        program, reading `refs` [K, N, n_ref] when the observation is flat."""
        if self.stage is None:
            return None
        lead = tuple(raw.shape[:-1])
        if out is None:
            import torch

            out = torch.empty(lead + (self.stage.n_out,), dtype=raw.dtype, device=raw.device)
        observer, src = None, raw
        if self.flux is not None:
            if raw.dim() != 3:
                raise NotImplementedError("last_only rollouts cannot carry a FluxObserver: its recursion needs every row")
            src = out if self.flux_only else self._scratch("ext_scratch", lead + (self.flux.n_in + 2,))
            observer = self.flux.bind_rows(raw, done, src, stream)
        return _lib.sequence(observer, self.stage.bind_apply(src, refs, out, stream) if self.has_program else None, result=out)

    def bind_episode_rows(self, done, reward=None, outputs=None, stream=None):
        """-> (launch | None, outputs | None): the episode stage's pass over the stored `done` [K, N] and `reward` [K, N] rows of a K-step
        rollout.  With a stage the pass always runs (the counters follow the rollout).  `outputs`: None / False (nothing handed out: `ended`
        goes to scratch), True (ended, finished_return, finished_length in the pipeline's scratch, overwritten by the next rollout) or a
        dict of the caller's tensors under those names (`ended` at least): what a bound launch takes, since it allocates nothing."""
        if self.episode is None:
            if outputs:
                raise ValueError("episode_statistics= outputs need an env built with make(..., episode_statistics=True)")
            return None, None
        import torch

        if done.dim() != 2:
            raise NotImplementedError("last_only rollouts cannot carry the episode stage: its counters need every row")
        shape = tuple(done.shape)
        if isinstance(outputs, dict):
            unknown = sorted(set(outputs) - {"ended", "finished_return", "finished_length"})
            if unknown or outputs.get("ended") is None:
                raise ValueError(f"episode_statistics: a dict of tensors under 'ended' (needed), 'finished_return', 'finished_length'; got {sorted(outputs)}")
            outs = {k: v for k, v in outputs.items() if v is not None}
        else:
            outs = dict(ended=self._scratch("ended_scratch", shape, torch.uint8))
            if outputs:
                outs.update(finished_return=self._scratch("finished_return_scratch", shape, torch.float64),
                            finished_length=self._scratch("finished_length_scratch", shape, torch.int32))
        launch = self.episode.bind_rows(done, reward if self.episode.has_reward else None, outs["ended"], outs.get("finished_return"),
                                        outs.get("finished_length"), stream)
        return launch, (outs if outputs else None)

    def reset(self, refs=None):
        """After the system's reset: the observer's, the extended reset rows -- the system's, then [0, 0] (flux_observer.py:80-83) --
        and the column program -> `state`.  With a StateNoiseProcessor the reset rows are noised first (state_noise_processor.py:70-74: one
        stream position), and no env is left waiting for a restart."""
        src = self.physical_system._obs
        if self.episode is not None:
            self.episode.restart()
        if self.noise is not None:
            self.physical_system._done.zero_()
            self.noise.step(src, None, self.noisy, self._reset_done)
            src = self.noisy
        if self.flux is not None:
            self.flux.reset()
            nb = self.flux.n_in
            self.rows[:, :nb].copy_(src)
            self.rows[:, nb:].zero_()
        if self.has_program:
            self.stage.apply(self.rows, refs, out=self.state)
        return self.state

    # ------------------------------------------------------------------ flux-oriented dq actions
    def dq_to_device(self, actions):
        """-> contiguous device tensor [N, 2 | 4] of the dq actions."""
        import torch

        ps = self.physical_system
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions, dtype=np.float64))
        return actions.to(device=ps._tdev, dtype=ps._tdtype).reshape(ps.n_envs, self.flux.n_action).contiguous()

    def bind_actions(self, dq, stream=None):
        """-> zero-argument launch(): the dq actions [N, 2 | 4] rotated into the frame the last observation left -> `abc` [N, 3 | 6]."""
        return self.flux.bind_actions(dq, self.abc, stream)

    def close(self):
        if self.noise is not None:
            self.noise.close()
        if self.episode is not None:
            self.episode.close()
        if self.stage is not None:
            self.stage.close()
        if self.flux is not None:
            self.flux.close()
