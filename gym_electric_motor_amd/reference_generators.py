"""Device-side reference generation: the batched counterpart of
`MultipleReferenceGenerator([WienerProcessReferenceGenerator(reference_state=s, ...) for s in reference_states])`
(reference_generators/wiener_process_reference_generator.py:9-49, subepisoded_reference_generator.py:11-119,
multiple_reference_generator.py:9-92) for N envs.  All generation runs in HIP kernels (csrc/gemx_refgen.hip); this class only
derives the margins the way the reference's `set_modules` does and owns the tensors.

    gen = ga.BatchedWienerProcessReferenceGenerator(reference_states=("i_sd", "i_sq"), seed=3).set_modules(env.physical_system)
    ps.set_reward(reward_weights=dict(i_sd=0.5, i_sq=0.5), referenced_states=gen.reference_names)
    gen.reset()
    refs = gen.rollout(K)                                  # [K, N, n_ref]: reference of each of the next K steps
    obs, done, reward = env.rollout(actions, references=refs)
    gen.apply_done(done)   # envs that terminated get a fresh generator state, as `if terminated: env.reset()` does

Closed loop, one launch per control step (what `ga.make(env_id, reference_generator="default")` drives): `gen.reset(); ref = gen.step()`,
then per control step `ref = gen.step(done)` -- terminated envs restart their generators, every generator advances, `ref [N, n_ref]` is
rewritten in place.  K x `step(done[k-1])` equals `rollout(K, done)` bit for bit, and the two can be mixed.
`rollout_shell(K, done)` is K such steps in one call -- row k is `step(done[k])`: restart first, then advance (what the complete env's
`rollout_complete` runs on the physics rollout's done mask); `rollout` resets AFTER row k.

The reference's other generator kinds -- sinusoidal, step, triangular, sawtooth, Laplace process, constant -- are parameter holders named
after the reference's classes, mixed per state by `BatchedMultipleReferenceGenerator` (MultipleReferenceGenerator's counterpart), on the
same kernels' handle and with the same surface and invariants; `SwitchedReferenceGenerator(holders, p=..., super_episode_length=...)`
is a holder too: its column runs one of its alternatives per super-episode, the choice being per-env device state:

    gen = ga.BatchedMultipleReferenceGenerator([ga.SinusoidalReferenceGenerator(reference_state="i_sd", frequency_range=(5, 50)),
                                                ga.StepReferenceGenerator(reference_state="i_sq", amplitude_range=(0.1, 0.4))], seed=3)
    env = ga.make("Cont-CC-PMSM-v0", n_envs=4096, reference_generator=gen)

The numpy PCG64 streams of the reference cannot be reproduced on a device; the generated process is the same in distribution
(tests/test_gpu_parity.py), chunked generation equals one-shot generation bit for bit (counter-based Philox).
"""
import ctypes as C

import numpy as np

from . import _lib


def _limit_margins(ps, name, limit_margin):
    """subepisoded_reference_generator.py:45-64 (set_modules): None (nominal / limit) | number | (lower, upper), factors of the state
    space's bounds."""
    i = ps.state_positions[name]
    low, high = ps.state_space.low[i], ps.state_space.high[i]
    if limit_margin is None:
        f = ps.nominal_state[i] / ps.limits[i]
        return f * low, f * high
    if isinstance(limit_margin, (float, int)):
        return limit_margin * low, limit_margin * high
    if isinstance(limit_margin, tuple):
        return limit_margin[0] * low, limit_margin[1] * high
    raise Exception("Unknown type for the limit margin.")


class _DeviceGenerators:
    """What every generator that owns a gemx_refgen handle offers the env shell; the subclasses derive the handle's config."""

    reference_names = property(lambda self: self._ordered)
    n_envs = property(lambda self: self._n_envs)
    is_set = property(lambda self: hasattr(self, "_cfg"), doc="set_modules has run")
    # the entry points behind the surface below (a generator on a handle of another kind names its own: ProfileReferences)
    _ABI = dict(reset="gemx_refgen_reset", step="gemx_refgen_step", rollout="gemx_refgen_rollout", rollout_shell="gemx_refgen_rollout_shell",
                state_bytes="gemx_refgen_state_bytes", get_blob="gemx_refgen_get_blob", set_blob="gemx_refgen_set_blob", destroy="gemx_refgen_destroy")

    def _create(self, ps, create, cfg):
        import torch

        self._L = _lib.load()
        self._tdev = ps._tdev
        self._tdtype = ps._tdtype
        h = C.c_void_p()
        _lib.check(getattr(self._L, create)(C.byref(cfg), self._n_envs, ps.device, _lib.F64 if self._tdtype == torch.float64 else _lib.F32, C.byref(h)))
        self._handle = h
        self._refs = torch.zeros((self._n_envs, int(cfg.n_ref)), dtype=self._tdtype, device=self._tdev)  # step()'s own buffer
        return self

    @property
    def references(self):
        """[N, n_ref] device tensor `step()` writes (without `out=`): the references shown last."""
        return self._refs

    def _stream(self):
        import torch

        return C.c_void_p(torch.cuda.current_stream(self._tdev).cuda_stream)

    def reset(self, mask=None):
        """reference_generator.reset() for the masked envs (all by default)."""
        import torch

        m = None if mask is None else torch.as_tensor(mask).to(device=self._tdev, dtype=torch.uint8).contiguous()
        _lib.check(getattr(self._L, self._ABI["reset"])(self._handle, C.c_void_p(m.data_ptr()) if m is not None else None, self._stream()))

    def rollout(self, K, done=None, out=None):
        """References of the next K control steps, [K, N, n_ref].  done [K, N] (optional): terminations of those steps known in
        advance (e.g. a recorded rollout): generators restart after a terminating step."""
        import torch

        if out is None:
            out = torch.empty((int(K), self._n_envs, int(self._cfg.n_ref)), dtype=self._tdtype, device=self._tdev)
        d = None if done is None else done.to(device=self._tdev, dtype=torch.uint8).contiguous()
        _lib.check(getattr(self._L, self._ABI["rollout"])(self._handle, C.c_void_p(d.data_ptr()) if d is not None else None, int(K),
                                               C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def _check_shell(self, K, done, out, what):
        """Validation of rollout_shell / bind_rollout_shell, without a device: K >= 1, done [K, N] uint8, out [K, N, n_ref]."""
        import torch

        K = int(K)
        if K < 1:
            raise ValueError(f"{what}: K must be >= 1, not {K}")
        if done is not None and not (torch.is_tensor(done) and done.dtype == torch.uint8 and tuple(done.shape) == (K, self._n_envs) and done.is_contiguous()
                                     and done.device == getattr(self, "_tdev", done.device)):
            raise ValueError(f"{what}: done must be a contiguous uint8 tensor of shape {(K, self._n_envs)} on the generator's device")
        oshape = (K, self._n_envs, int(self._cfg.n_ref))
        if out is not None and not (torch.is_tensor(out) and tuple(out.shape) == oshape and out.is_contiguous() and out.dtype == getattr(self, "_tdtype", out.dtype)
                                    and out.device == getattr(self, "_tdev", out.device)):
            raise ValueError(f"{what}: out must be a contiguous tensor of shape {oshape} of the generator's dtype on its device")
        return K

    def rollout_shell(self, K, done=None, out=None):
        """K env-shell steps in the SHELL's order (gemx_refgen_rollout_shell): row k of the returned [K, N, n_ref] tensor is what
        `step(done[k])` returns -- the generators of the envs with done[k, env] != 0 restart first, then every generator advances.  (`rollout`
        resets AFTER row k.)  done: [K, N] uint8 device tensor, e.g. a physics rollout's done mask, or None.  `references` is not
        touched; may be mixed freely with `step` and `rollout`."""
        return self._bind_shell(K, done, out, None, "rollout_shell")()

    def bind_rollout_shell(self, done, out, stream=None):
        """-> zero-argument launch(): `gemx_refgen_rollout_shell(done) -> out` with the handle, both pointers and the stream resolved once."""
        import torch

        if done is None or out is None:
            raise ValueError("bind_rollout_shell needs the done [K, N] and out [K, N, n_ref] tensors")
        return self._bind_shell(done.shape[0] if torch.is_tensor(done) and done.dim() == 2 else 0, done, out, stream, "bind_rollout_shell")

    def _bind_shell(self, K, done, out, stream, what):
        """The one validation and the one launcher behind `rollout_shell` (out None: allocated here, once) and `bind_rollout_shell`."""
        import torch

        K = self._check_shell(K, done, out, what)
        if out is None:
            out = torch.empty((K, self._n_envs, int(self._cfg.n_ref)), dtype=self._tdtype, device=self._tdev)
        stream = stream if stream is not None else torch.cuda.current_stream(self._tdev)
        args = (C.c_void_p(done.data_ptr()) if done is not None else None, K, C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream))
        return _lib.bound_call(getattr(self._L, self._ABI["rollout_shell"]), self, args, (done, out, stream), out)

    def step(self, done=None, out=None):
        """One env-shell step in ONE launch (gemx_refgen_step): the generators of the envs with done[env] != 0 restart, then every
        generator advances by one step.  Returns the references [N, n_ref] -- the buffer this generator owns (rewritten by every call)
        unless `out` is given.  `done` [N] uint8 device tensor, e.g. the physical system's `done`."""
        import torch

        if out is None:
            out = self._refs
        elif not (torch.is_tensor(out) and tuple(out.shape) == tuple(self._refs.shape) and out.dtype == self._tdtype and out.device == self._tdev and out.is_contiguous()):
            raise ValueError(f"step: out must be a contiguous {self._tdtype} tensor of shape {tuple(self._refs.shape)} on {self._tdev}")
        if done is not None:
            if not (done.dtype == torch.uint8 and done.device == self._tdev and done.is_contiguous()):
                done = done.to(device=self._tdev, dtype=torch.uint8).contiguous()
            if done.numel() != self._n_envs:
                raise ValueError(f"step: done must have {self._n_envs} elements")
        return self._bind_step(done, out, None)()

    def bind_step(self, done, stream=None):
        """-> zero-argument step(): `gemx_refgen_step(done) -> references` with the handle, both pointers and the stream resolved once."""
        import torch

        if not (torch.is_tensor(done) and done.dtype == torch.uint8 and done.device == self._tdev and done.is_contiguous() and done.numel() == self._n_envs):
            raise ValueError(f"bind_step needs a contiguous uint8 tensor of {self._n_envs} elements on {self._tdev}")
        return self._bind_step(done, self._refs, stream)

    def _bind_step(self, done, out, stream):
        import torch

        stream = stream if stream is not None else torch.cuda.current_stream(self._tdev)
        args = (C.c_void_p(done.data_ptr()) if done is not None else None, C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream))
        return _lib.bound_call(getattr(self._L, self._ABI["step"]), self, args, (done, out, stream), out)

    def apply_done(self, done):
        """After a rollout: envs with any termination in `done` ([K, N] or [N]) restart their generators (closed-loop use)."""
        import torch

        d = done if done.dim() == 1 else done.any(dim=0)
        self.reset(mask=d.to(torch.uint8))

    # ------------------------------------------------------------------ checkpoint
    def state_bytes(self):
        """Bytes of the handle's checkpoint blob (`gemx_refgen_state_bytes`)."""
        return int(getattr(self._L, self._ABI["state_bytes"])(self._handle))

    def get_state(self):
        """-> dict(blob, references) of new device tensors, for a checkpoint: the handle's whole per-(column, env) state as one opaque uint8
        blob (`gemx_refgen_get_blob`: values, sigmas, sub-episode counters, the stream indices, the waveform parameters, the super-episode
        state) and a clone of `references` -- the values shown last, which the reward of the next step reads."""
        import torch

        blob = torch.empty(self.state_bytes(), dtype=torch.uint8, device=self._tdev)
        _lib.check(getattr(self._L, self._ABI["get_blob"])(self._handle, C.c_void_p(blob.data_ptr()), self._stream()))
        return dict(blob=blob, references=self._refs.clone())

    def check_state(self, state):
        """What can be checked of `get_state()`'s dict without touching the device -> (blob, references), on this generator's device.
        ValueError names the mismatch."""
        import torch

        if not isinstance(state, dict) or "blob" not in state or "references" not in state:
            raise ValueError("a reference generator's checkpoint is the dict(blob=, references=) of its get_state()")
        blob, refs = state["blob"], state["references"]
        if not (torch.is_tensor(blob) and blob.dtype == torch.uint8 and blob.dim() == 1):
            raise ValueError("reference generator checkpoint: blob must be a one-dimensional uint8 tensor")
        if blob.numel() != self.state_bytes():
            raise ValueError(f"reference generator checkpoint: the blob has {blob.numel()} bytes, this generator's has {self.state_bytes()}: it is "
                             "truncated, or was taken from a generator of another configuration (n_envs, columns, kinds)")
        if not (torch.is_tensor(refs) and tuple(refs.shape) == tuple(self._refs.shape) and refs.dtype == self._tdtype):
            raise ValueError(f"reference generator checkpoint: references must be a {self._tdtype} tensor of shape {tuple(self._refs.shape)}, not "
                             f"{getattr(refs, 'dtype', type(refs).__name__)} {tuple(getattr(refs, 'shape', ()))}")
        return blob.to(self._tdev).contiguous(), refs.to(self._tdev)

    def set_state(self, state):
        """Restore `get_state()` of a generator of the same configuration: `step`, `rollout` and `rollout_shell` continue bit for bit.
        Checked before anything is enqueued (sizes and types here, the blob's header -- n_envs, columns, kinds, shard -- by
        `gemx_refgen_set_blob`, which synchronises the stream for it); ValueError names the mismatch and the generator is untouched.
        The references are copied INTO the buffer this generator owns: bound launchers and captured graphs keep pointing at it."""
        blob, refs = self.check_state(state)
        _lib.check(getattr(self._L, self._ABI["set_blob"])(self._handle, C.c_void_p(blob.data_ptr()), self._stream()))
        self._refs.copy_(refs)

    def close(self):
        if self._handle is not None:
            getattr(self._L, self._ABI["destroy"])(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchedWienerProcessReferenceGenerator(_DeviceGenerators):
    def __init__(self, reference_states=("omega",), sigma_range=(1e-3, 1e-1), episode_lengths=(500, 2000), limit_margin=None,
                 initial_range=None, seed=0, env_base=None):
        self._reference_states = tuple(s.lower() for s in ([reference_states] if isinstance(reference_states, str) else reference_states))
        if not 1 <= len(self._reference_states) <= _lib.MAX_REF:
            raise ValueError(f"1..{_lib.MAX_REF} reference states")
        self._sigma_range = sigma_range
        self._episode_lengths = (int(episode_lengths), int(episode_lengths)) if np.ndim(episode_lengths) == 0 else tuple(int(x) for x in episode_lengths)
        self._limit_margin = limit_margin
        self._initial_range = initial_range
        self._seed = int(seed) & (2**64 - 1)
        self._env_base = None if env_base is None else int(env_base)  # None: the physical system's (a shard's generators follow its envs)
        self._handle = None
        self._refs = None
        for what, v in (("limit_margin", limit_margin), ("sigma_range", sigma_range), ("initial_range", initial_range)):
            if isinstance(v, dict):  # per generator, by state name; states not named take the default
                unknown = sorted(set(k.lower() for k in v) - set(self._reference_states))
                if unknown:
                    raise ValueError(f"{what} names {unknown}, which are not among the reference states {list(self._reference_states)}")

    @staticmethod
    def _for_state(value, name, default):
        """A setting given for all generators, or as a dict by state name (states not named: the default)."""
        if isinstance(value, dict):
            return {k.lower(): v for k, v in value.items()}.get(name, default)
        return value

    def _margins(self, ps, name):
        return _limit_margins(ps, name, self._for_state(self._limit_margin, name, None))

    def set_modules(self, physical_system, _defer_create=False):
        ps = physical_system
        # the fused reward's reference tensor follows the state order of the physical system
        self._ordered = tuple(sorted(self._reference_states, key=lambda n: ps.state_positions[n]))
        self._n_envs = ps.n_envs
        cfg = _lib.GemxRefgenConfig()
        cfg.struct_size = C.sizeof(_lib.GemxRefgenConfig)
        cfg.n_ref = len(self._ordered)
        cfg.seed = self._seed
        cfg.env_base = self._env_base if self._env_base is not None else int(getattr(ps, "env_base", 0))
        cfg.episode_len_lo, cfg.episode_len_hi = self._episode_lengths
        for j, name in enumerate(self._ordered):
            lo, hi = self._margins(ps, name)
            cfg.margin_lo[j], cfg.margin_hi[j] = float(lo), float(hi)
            ir = self._for_state(self._initial_range, name, None)
            ir = ir if ir is not None else (lo, hi)  # wiener_process_reference_generator.py:25-28
            cfg.initial_lo[j], cfg.initial_hi[j] = float(ir[0]), float(ir[1])
            sr = self._for_state(self._sigma_range, name, (1e-3, 1e-1))
            cfg.sigma_lo[j], cfg.sigma_hi[j] = (float(sr), float(sr)) if np.ndim(sr) == 0 else (float(sr[0]), float(sr[1]))
        self._cfg = cfg
        if _defer_create:
            return self
        return self._create(ps, "gemx_refgen_create", cfg)

    @property
    def reference_space(self):
        """(low, high) arrays [n_ref]: the generators' limit margins (MultipleReferenceGenerator.reference_space)."""
        n = int(self._cfg.n_ref)
        return np.array(self._cfg.margin_lo[:n], dtype=float), np.array(self._cfg.margin_hi[:n], dtype=float)

    def state(self):
        """(value, sigma, steps_left) per (generator, env), for tests / inspection."""
        import torch

        n = (int(self._cfg.n_ref), self._n_envs)
        v = torch.empty(n, dtype=torch.float64, device=self._tdev)
        s = torch.empty(n, dtype=torch.float64, device=self._tdev)
        l_ = torch.empty(n, dtype=torch.int32, device=self._tdev)
        _lib.check(self._L.gemx_refgen_get_state(self._handle, C.c_void_p(v.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(l_.data_ptr()), self._stream()))
        torch.cuda.current_stream(self._tdev).synchronize()
        return v, s, l_


def _pair(value, what):
    """A range as (lo, hi); a plain number is that number (`_get_current_value`, subepisoded_reference_generator.py:109-119)."""
    if np.ndim(value) == 0:
        return float(value), float(value)
    if len(value) != 2:
        raise ValueError(f"{what}: a number or (low, high), not {value!r}")
    return float(value[0]), float(value[1])


class _SubGenerator:
    """Parameter holder of one sub-generator: the keyword arguments and defaults of the reference's class of the same name.  Holders
    generate nothing; a BatchedMultipleReferenceGenerator turns them into the columns of one device handle."""

    kind = None
    keywords = ("reference_state", "episode_lengths", "limit_margin")

    def __init__(self, reference_state="omega", episode_lengths=(500, 2000), limit_margin=None):
        self.reference_state = str(reference_state).lower()
        self.episode_lengths = tuple(int(x) for x in _pair(episode_lengths, "episode_lengths"))
        if isinstance(limit_margin, list):
            limit_margin = tuple(limit_margin)
        if isinstance(limit_margin, dict):  # by state name, as the env ids' defaults are kept: this holder's own state, else None
            limit_margin = {k.lower(): v for k, v in limit_margin.items()}.get(self.reference_state)
        self.limit_margin = limit_margin

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in vars(self).items())})"


class WienerProcessReferenceGenerator(_SubGenerator):
    """wiener_process_reference_generator.py:11-23."""

    kind = _lib.REF_WIENER
    keywords = _SubGenerator.keywords + ("sigma_range", "initial_range")

    def __init__(self, sigma_range=(1e-3, 1e-1), initial_range=None, **kwargs):
        super().__init__(**kwargs)
        self.sigma_range = _pair(sigma_range, "sigma_range")
        self.initial_range = None if initial_range is None else _pair(initial_range, "initial_range")


class LaplaceProcessReferenceGenerator(_SubGenerator):
    """laplace_process_reference_generator.py:15-22."""

    kind = _lib.REF_LAPLACE
    keywords = _SubGenerator.keywords + ("sigma_range",)

    def __init__(self, sigma_range=(1e-3, 1e-1), **kwargs):
        super().__init__(**kwargs)
        self.sigma_range = _pair(sigma_range, "sigma_range")


class _WaveformGenerator(_SubGenerator):
    keywords = _SubGenerator.keywords + ("amplitude_range", "frequency_range", "offset_range")

    def __init__(self, amplitude_range=None, frequency_range=(1, 10), offset_range=None, **kwargs):
        super().__init__(**kwargs)
        # `amplitude_range or (0, np.inf)`, `offset_range or (-np.inf, np.inf)` (e.g. sinusoidal_reference_generator.py:36-38): cut to the
        # limit margin in set_modules
        self.amplitude_range = _pair(amplitude_range if amplitude_range is not None else (0.0, np.inf), "amplitude_range")
        self.frequency_range = _pair(frequency_range, "frequency_range")
        self.offset_range = _pair(offset_range if offset_range is not None else (-np.inf, np.inf), "offset_range")


class SinusoidalReferenceGenerator(_WaveformGenerator):
    """sinusoidal_reference_generator.py:16-38."""

    kind = _lib.REF_SINUS


class StepReferenceGenerator(_WaveformGenerator):
    """step_reference_generator.py:15-26."""

    kind = _lib.REF_STEP


class TriangularReferenceGenerator(_WaveformGenerator):
    """triangle_reference_generator.py:14-37."""

    kind = _lib.REF_TRIANGULAR


class SawtoothReferenceGenerator(_WaveformGenerator):
    """sawtooth_reference_generator.py:17-29."""

    kind = _lib.REF_SAWTOOTH


class ConstReferenceGenerator(_SubGenerator):
    """const_reference_generator.py:11-22: always `reference_value`; no sub-episodes, no margin."""

    kind = _lib.REF_CONST
    keywords = ("reference_state", "reference_value")

    def __init__(self, reference_state="omega", reference_value=0.5):
        super().__init__(reference_state=reference_state)
        self.reference_value = float(reference_value)


class SwitchedReferenceGenerator(_SubGenerator):
    """switched_reference_generator.py:11-37: per super-episode of `super_episode_length` steps (a number n: (n, n + 1)) ONE of the
    alternatives, drawn by `p` (default: uniform), generates the references of its state; the next super-episode's alternative restarts
    from the value shown last.  sub_generators: holders of the kinds above or the reference's own sub-generator instances as constructed
    (read as `as_sub_generators` reads them), all for the same state, at most `_lib.MAX_ALT` of them."""

    keywords = ("sub_generators", "p", "super_episode_length")

    def __init__(self, sub_generators, p=None, super_episode_length=(100, 10000)):
        subs = as_sub_generators(list(sub_generators) if isinstance(sub_generators, (list, tuple)) else [sub_generators])
        if not subs:
            raise ValueError("No sub generator was passed.")
        if any(isinstance(h, SwitchedReferenceGenerator) for h in subs):
            raise ValueError("the alternatives of a SwitchedReferenceGenerator are generators of the other kinds, not switched ones")
        states = sorted({h.reference_state for h in subs})
        if len(states) != 1:  # (the reference asserts it, switched_reference_generator.py:28-30)
            raise ValueError(f"The passed sub generators have different referenced states: {states}")
        if len(subs) > _lib.MAX_ALT:
            raise ValueError(f"at most {_lib.MAX_ALT} alternatives per switched column, not {len(subs)}")
        self.reference_state = states[0]
        self.sub_generators = tuple(subs)
        self.p = tuple(float(x) for x in p) if p is not None and len(p) else (1.0 / len(subs),) * len(subs)
        if len(self.p) != len(subs):
            raise ValueError(f"p: one probability per sub generator ({len(subs)}), not {len(self.p)}")
        if min(self.p) < 0 or abs(sum(self.p) - 1.0) > 1e-9:
            raise ValueError(f"p: probabilities >= 0 that sum to 1, not {self.p}")
        if np.ndim(super_episode_length) == 0:
            super_episode_length = (super_episode_length, super_episode_length + 1)
        self.super_episode_length = tuple(int(x) for x in _pair(super_episode_length, "super_episode_length"))
        if self.super_episode_length[0] < 1 or self.super_episode_length[1] <= self.super_episode_length[0]:
            raise ValueError(f"super_episode_length: 1 <= low < high (the upper bound is excluded), not {self.super_episode_length}")


_HOLDERS = {c.__name__: c for c in (WienerProcessReferenceGenerator, LaplaceProcessReferenceGenerator, SinusoidalReferenceGenerator,
                                    StepReferenceGenerator, TriangularReferenceGenerator, SawtoothReferenceGenerator, ConstReferenceGenerator)}
# the private attributes the reference's instances keep their constructor arguments in -> the holders' keywords
_REFERENCE_ATTRIBUTES = dict(_reference_state="reference_state", _episode_len_range="episode_lengths", _limit_margin="limit_margin",
                             _sigma_range="sigma_range", _initial_range="initial_range", _amplitude_range="amplitude_range",
                             _frequency_range="frequency_range", _offset_range="offset_range", _reference_value="reference_value")
SWITCHED_REFUSAL = ("SwitchedReferenceGenerator is outside the accelerated path as an instance of the reference: pass the holder "
                    "ga.SwitchedReferenceGenerator(sub_generators, p=..., super_episode_length=...) with the same arguments instead.")


def as_sub_generators(generator):
    """-> list of holders.  A holder, a list / tuple of them, or the reference's own generator instances as constructed, recognised by
    class name with the settings read from the instance -- the way `fold_wrappers` treats the reference's wrapper instances; a
    MultipleReferenceGenerator instance contributes its sub-generators.  An instance that has been through its own `set_modules` is
    refused: its margins and ranges are no longer the constructor's.  Nothing of the reference is imported."""
    if isinstance(generator, (list, tuple)):
        return [h for g in generator for h in as_sub_generators(g)]
    if isinstance(generator, _SubGenerator):
        return [generator]
    if isinstance(generator, ProfileReferenceGenerator):
        raise ValueError("sub_generators: " + PROFILE_MIXED_REFUSAL)
    name = type(generator).__name__
    if name == "SwitchedReferenceGenerator":
        raise NotImplementedError(SWITCHED_REFUSAL)
    if name == "MultipleReferenceGenerator" and hasattr(generator, "_sub_generators"):
        return as_sub_generators(list(generator._sub_generators))
    if name not in _HOLDERS or not hasattr(generator, "_reference_state"):
        raise TypeError(f"{name} is not a reference generator of the accelerated path; known kinds: {sorted(_HOLDERS)}")
    if getattr(generator, "_physical_system", None) is not None or getattr(generator, "_referenced_states", None) is not None:
        # (both None as constructed, core.py:425-429.)  Its set_modules has run: `_limit_margin` now holds absolute margins and the
        # amplitude / offset ranges are already cut to them (subepisoded_reference_generator.py:45-64, e.g.
        # sinusoidal_reference_generator.py:40-48), which would be read here as factors and constructor arguments
        raise ValueError(f"this {name} has already been through set_modules; pass an instance as constructed, or a holder with its keyword arguments")
    holder = _HOLDERS[name]
    kw = {key: getattr(generator, attr) for attr, key in _REFERENCE_ATTRIBUTES.items() if key in holder.keywords and hasattr(generator, attr)}
    for key in ("amplitude_range", "offset_range", "sigma_range", "episode_lengths", "initial_range"):  # (numpy arrays -> tuples)
        if key in kw and kw[key] is not None and np.ndim(kw[key]) == 1:
            kw[key] = tuple(float(x) for x in kw[key])
    return [holder(**kw)]


class BatchedMultipleReferenceGenerator(_DeviceGenerators):
    """The batched MultipleReferenceGenerator (multiple_reference_generator.py:9-92) over the reference's sub-episoded and constant
    generator kinds: one holder per referenced state, any mix of kinds, ONE device handle (gemx_refgen_create_kinds; with a
    SwitchedReferenceGenerator holder among them gemx_refgen_create_switched, whose plain columns keep their bits).  The columns follow
    the state order of the physical system.  Surface and invariants are the Wiener generator's: `reset`, `step`, `rollout`, `bind_step`
    (graph-capturable), `apply_done`; K x step == rollout(K), chunked == one-shot, shards by `env_base`.  A Wiener column draws exactly
    what the same column of a BatchedWienerProcessReferenceGenerator with the same seed draws."""

    def __init__(self, sub_generators, seed=0, env_base=None):
        self._subs = as_sub_generators(sub_generators)
        if not 1 <= len(self._subs) <= _lib.MAX_REF:
            raise ValueError(f"1..{_lib.MAX_REF} sub-generators (columns of the reference tensor), not {len(self._subs)}")
        states = [h.reference_state for h in self._subs]
        if len(set(states)) != len(states):  # multiple_reference_generator.py:54-56
            raise ValueError(f"every state is referenced by at most one sub-generator: {states}")
        self._seed = int(seed) & (2**64 - 1)
        self._env_base = None if env_base is None else int(env_base)
        self._handle = None
        self._refs = None

    sub_generators = property(lambda self: tuple(self._subs), doc="the holders, in the order given")

    def set_modules(self, physical_system, _defer_create=False):
        ps = physical_system
        missing = [h.reference_state for h in self._subs if h.reference_state not in ps.state_positions]
        if missing:
            raise ValueError(f"reference states {missing} are not states of the physical system {list(ps.state_names)}")
        subs = sorted(self._subs, key=lambda h: ps.state_positions[h.reference_state])
        self._ordered = tuple(h.reference_state for h in subs)
        self._columns = tuple(subs)
        self._n_envs = ps.n_envs
        switched = any(isinstance(h, SwitchedReferenceGenerator) for h in subs)
        cfg = _lib.GemxRefgenSwitchedConfig() if switched else _lib.GemxRefgenKindsConfig()
        cfg.struct_size = C.sizeof(cfg)
        cfg.n_ref = len(subs)
        cfg.seed = self._seed
        cfg.env_base = self._env_base if self._env_base is not None else int(getattr(ps, "env_base", 0))
        cfg.tau = float(ps.tau)
        space_lo, space_hi = [], []
        for j, h in enumerate(subs):
            if not switched:
                lo, hi = self._describe(cfg, j, h, ps)
            elif not isinstance(h, SwitchedReferenceGenerator):  # a plain column of a switched handle: alternative 0, n_alt = 0
                lo, hi = self._describe(cfg, j * _lib.MAX_ALT, h, ps)
            else:  # reference space: the alternatives' lowest low and highest high (switched_reference_generator.py:47-55)
                cfg.n_alt[j] = len(h.sub_generators)
                cfg.super_len_lo[j], cfg.super_len_hi[j] = h.super_episode_length
                spaces = []
                for a, (alt, prob) in enumerate(zip(h.sub_generators, h.p)):
                    cfg.p[j * _lib.MAX_ALT + a] = prob
                    spaces.append(self._describe(cfg, j * _lib.MAX_ALT + a, alt, ps))
                lo, hi = min(x[0] for x in spaces), max(x[1] for x in spaces)
            space_lo.append(lo)
            space_hi.append(hi)
        self._cfg = cfg
        self._switched = switched
        self._space = (np.array(space_lo, dtype=float), np.array(space_hi, dtype=float))
        if _defer_create:
            return self
        return self._create(ps, "gemx_refgen_create_switched" if switched else "gemx_refgen_create_kinds", cfg)

    @staticmethod
    def _describe(cfg, j, h, ps):
        """Slot j of the config's per-description arrays from the holder h -> its reference space (low, high)."""
        cfg.kind[j] = h.kind
        if h.kind == _lib.REF_CONST:  # its reference space is the single point (const_reference_generator.py:20)
            cfg.reference_value[j] = h.reference_value
            return h.reference_value, h.reference_value
        cfg.episode_len_lo[j], cfg.episode_len_hi[j] = h.episode_lengths
        lo, hi = (float(x) for x in _limit_margins(ps, h.reference_state, h.limit_margin))
        cfg.margin_lo[j], cfg.margin_hi[j] = lo, hi
        if h.kind in (_lib.REF_WIENER, _lib.REF_LAPLACE):
            cfg.sigma_lo[j], cfg.sigma_hi[j] = h.sigma_range
            ir = getattr(h, "initial_range", None)
            cfg.initial_lo[j], cfg.initial_hi[j] = ir if ir is not None else (lo, hi)  # wiener_process_reference_generator.py:25-28
        else:  # e.g. sinusoidal_reference_generator.py:40-48: amplitudes within half the margin's width, offsets within the margin
            cfg.amplitude_lo[j], cfg.amplitude_hi[j] = (float(x) for x in np.clip(h.amplitude_range, 0, (hi - lo) / 2))
            cfg.offset_lo[j], cfg.offset_hi[j] = (float(x) for x in np.clip(h.offset_range, lo, hi))
            cfg.frequency_lo[j], cfg.frequency_hi[j] = h.frequency_range
        return lo, hi

    reference_space = property(lambda self: self._space, doc="(low, high) arrays [n_ref]: the limit margins; a constant column: its value")

    def state(self):
        """dict of [n_ref, N] tensors, for tests / inspection: value, sigma, left (steps left in the sub-episode), kind, index (step index
        inside the sub-episode), length, amplitude, frequency, offset, phase, width (a step column: its high / low ratio), roll."""
        import torch

        n = (int(self._cfg.n_ref), self._n_envs)
        v = torch.empty(n, dtype=torch.float64, device=self._tdev)
        s = torch.empty(n, dtype=torch.float64, device=self._tdev)
        l_ = torch.empty(n, dtype=torch.int32, device=self._tdev)
        kil = torch.empty((3,) + n, dtype=torch.int32, device=self._tdev)
        par = torch.empty((6,) + n, dtype=torch.float64, device=self._tdev)
        _lib.check(self._L.gemx_refgen_get_state(self._handle, C.c_void_p(v.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(l_.data_ptr()), self._stream()))
        _lib.check(self._L.gemx_refgen_get_params(self._handle, C.c_void_p(kil.data_ptr()), C.c_void_p(par.data_ptr()), self._stream()))
        torch.cuda.current_stream(self._tdev).synchronize()
        out = dict(value=v, sigma=s, left=l_, kind=kil[0], index=kil[1], length=kil[2])
        out.update(zip(("amplitude", "frequency", "offset", "phase", "width", "roll"), par))
        if self._switched:  # alternative (its kind is `kind`), super-episode step counter and length, super-episodes drawn so far
            sw = torch.empty((4,) + n, dtype=torch.int32, device=self._tdev)
            _lib.check(self._L.gemx_refgen_get_switch_state(self._handle, C.c_void_p(sw.data_ptr()), self._stream()))
            torch.cuda.current_stream(self._tdev).synchronize()
            out.update(zip(("alternative", "super_index", "super_length", "n_super"), sw))
        return out


class ReplayReferenceGenerator:
    """Fixed reference profiles behind the complete env (`ga.make(env_id, reference_generator=ReplayReferenceGenerator(refs))`):
    `references` [K, n_ref] (every env sees the same profile) or [K, N, n_ref]; `reset()` shows row 0, every `step` shows the next row,
    `done` is ignored.  For evaluation on given profiles and for comparing the shell with recorded runs of the reference; a tensor copy
    per step, not a hot path, and -- unlike the Wiener generators -- not capturable in a HIP graph: the row index is host state, so
    stepping while a stream is capturing is refused.  reference_states: the state each column of `references` refers to, in the
    columns' order (default: the env id's referenced states, `default_env_modules`, in the state order of the physical system); the
    env shows the columns in the state order of the physical system, as the fused reward reads them."""

    def __init__(self, references, reference_states=None):
        self._src = references
        if np.ndim(references) not in (2, 3):
            raise ValueError("references must be [K, n_ref] or [K, N, n_ref]")
        self._reference_states = None if reference_states is None else tuple(s.lower() for s in ([reference_states] if isinstance(reference_states, str) else reference_states))
        self._k = 0
        self._refs = None

    reference_names = property(lambda self: self._ordered)
    references = property(lambda self: self._refs)
    n_envs = property(lambda self: self._n_envs)

    def set_modules(self, physical_system, _defer_create=False, default_states=None):
        ps = physical_system
        states = self._reference_states if self._reference_states is not None else tuple(default_states or ())
        n_ref = int(np.shape(self._src)[-1])
        if len(states) != n_ref:
            raise ValueError(f"references carry {n_ref} columns for the {len(states)} referenced states {list(states)}")
        if len(set(states)) != len(states):
            raise ValueError(f"reference_states names a state twice: {list(states)}")
        order = sorted(range(n_ref), key=lambda j: ps.state_positions[states[j]])  # the caller's columns -> state order
        self._ordered = tuple(states[j] for j in order)
        self._n_envs = ps.n_envs
        if np.ndim(self._src) == 3 and int(np.shape(self._src)[1]) != ps.n_envs:
            raise ValueError(f"references are for {np.shape(self._src)[1]} envs, the system has {ps.n_envs}")
        idx = [ps.state_positions[n] for n in self._ordered]
        self._space = (np.asarray(ps.state_space.low, dtype=float)[idx], np.asarray(ps.state_space.high, dtype=float)[idx])
        if _defer_create:
            return self
        import torch

        self._rows = torch.as_tensor(self._src).to(device=ps._tdev, dtype=ps._tdtype)[..., order].contiguous()
        self._refs = torch.zeros((ps.n_envs, n_ref), dtype=ps._tdtype, device=ps._tdev)
        return self

    reference_space = property(lambda self: self._space)

    def _show(self):
        import torch

        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a ReplayReferenceGenerator cannot be captured in a graph: its row index lives on the host")
        if self._k >= self._rows.shape[0]:
            raise IndexError(f"the replayed profile has {self._rows.shape[0]} rows")
        self._refs.copy_(self._rows[self._k])  # ([n_ref] rows broadcast over the envs)
        self._k += 1
        return self._refs

    def reset(self, mask=None):
        self._k = 0

    def step(self, done=None, out=None):
        return self._show()

    def bind_step(self, done, stream=None):
        return self._show

    def rollout_shell(self, K, done=None, out=None):
        """The next K rows of the profile, [K, N, n_ref] (`done` is ignored); the host row index advances by K.  Eager only."""
        import torch

        K = int(K)
        if K < 1:
            raise ValueError(f"rollout_shell: K must be >= 1, not {K}")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a ReplayReferenceGenerator cannot be captured in a graph: its row index lives on the host")
        if self._k + K > self._rows.shape[0]:
            raise IndexError(f"the replayed profile has {self._rows.shape[0]} rows")
        rows = self._rows[self._k:self._k + K]
        if rows.dim() == 2:  # ([K, n_ref] profiles: every env sees the same row)
            rows = rows[:, None, :].expand(K, self._n_envs, rows.shape[-1])
        if out is None:
            out = rows.contiguous()
        else:
            if tuple(out.shape) != (K, self._n_envs, int(self._rows.shape[-1])):
                raise ValueError(f"rollout_shell: out must have shape {(K, self._n_envs, int(self._rows.shape[-1]))}")
            out.copy_(rows)
        self._k += K
        return out

    def bind_rollout_shell(self, done, out, stream=None):
        raise RuntimeError("a ReplayReferenceGenerator cannot be captured in a graph: its row index lives on the host, so a bound rollout "
                           "would replay the rows of its first launch")

    def get_state(self):
        """-> dict(row, references), for a checkpoint: the host row index and a clone of the references shown last."""
        return dict(row=int(self._k), references=self._refs.clone())

    def check_state(self, state):
        """`get_state()`'s dict, checked without touching the device -> (row, references); ValueError names the mismatch."""
        import torch

        if not isinstance(state, dict) or "row" not in state or "references" not in state:
            raise ValueError("a ReplayReferenceGenerator's checkpoint is the dict(row=, references=) of its get_state()")
        row, refs = state["row"], state["references"]
        if isinstance(row, bool) or not isinstance(row, (int, np.integer)) or not 0 <= int(row) <= int(self._rows.shape[0]):
            raise ValueError(f"ReplayReferenceGenerator checkpoint: row must be an index into the profile's {int(self._rows.shape[0])} rows, not {row!r}")
        if not (torch.is_tensor(refs) and tuple(refs.shape) == tuple(self._refs.shape) and refs.dtype == self._refs.dtype):
            raise ValueError(f"ReplayReferenceGenerator checkpoint: references must be a {self._refs.dtype} tensor of shape {tuple(self._refs.shape)}")
        return int(row), refs

    def set_state(self, state):
        """Restore `get_state()`: the next `step` shows the row the checkpointed generator would have shown."""
        row, refs = self.check_state(state)
        self._k = row
        self._refs.copy_(refs)

    def close(self):
        pass


PROFILE_MIXED_REFUSAL = ("a ProfileReferenceGenerator serves all referenced columns of its env: it cannot be mixed with other generator holders in "
                         "one list (give the other states' set points as further columns of the profile)")
_PROFILE_CHOICES = dict(interpolation=dict(hold=_lib.PROFILE_INTERP_HOLD, linear=_lib.PROFILE_INTERP_LINEAR),
                        end=dict(hold=_lib.PROFILE_END_HOLD, wrap=_lib.PROFILE_END_WRAP),
                        start=dict(zero=_lib.PROFILE_START_ZERO, random=_lib.PROFILE_START_RANDOM))


class ProfileReferenceGenerator:
    """Given reference trajectories -- drive cycles, recorded set-point profiles, a benchmark suite of steps -- on the device, per env:
    the holder `ga.make(env_id, reference_generator=ProfileReferenceGenerator(profiles, ...))` takes wherever it takes the other device
    generators.  Unlike a ReplayReferenceGenerator the position lives in device memory: an env that terminates (or is truncated)
    restarts its profile, a step is one kernel launch that can be captured in a HIP graph, `rollout_complete` replays the resets, and
    the position travels in the checkpoint.

    profiles: [T, n_ref] (every env follows the same profile) or [T, N, n_ref] (one per env), normalised units, numpy or torch.
    reference_states: the state each column refers to (default: the env id's referenced states); the env shows the columns in the state
    order of the physical system.  profile_tau: sampling time of the rows (None: the system's tau, one row per control step);
    interpolation 'linear' | 'hold' between rows when it differs.  end: 'hold' (stay on the last row) | 'wrap' (periodic).  start:
    'zero' | 'random' -- a start row per (env, episode), uniform in [0, T - 1], a function of (seed, global env index, episode number).
    An env at step k of its episode, started at row s, stands at position s + k * tau / profile_tau (csrc/gemx_refprofile.hip)."""

    def __init__(self, profiles, reference_states=None, profile_tau=None, interpolation="linear", end="hold", start="zero", seed=None):
        if np.ndim(profiles) not in (2, 3):
            raise ValueError(f"profiles must be [T, n_ref] or [T, N, n_ref], not {np.ndim(profiles)}-dimensional")
        shape = tuple(int(x) for x in np.shape(profiles))
        if shape[0] < 1:
            raise ValueError("profiles: T, the number of rows, must be >= 1")
        if not 1 <= shape[-1] <= _lib.MAX_REF:
            raise ValueError(f"profiles carry {shape[-1]} columns: 1..{_lib.MAX_REF} referenced states (_lib.MAX_REF)")
        for what, value in (("interpolation", interpolation), ("end", end), ("start", start)):
            if not isinstance(value, str) or value not in _PROFILE_CHOICES[what]:
                raise ValueError(f"{what}: one of {sorted(_PROFILE_CHOICES[what])}, not {value!r}")
        if profile_tau is not None and not (np.ndim(profile_tau) == 0 and np.isfinite(float(profile_tau)) and float(profile_tau) > 0):
            raise ValueError(f"profile_tau: a positive sampling time or None (the system's tau), not {profile_tau!r}")
        self.profiles = profiles
        self.reference_states = None if reference_states is None else tuple(s.lower() for s in ([reference_states] if isinstance(reference_states, str) else reference_states))
        if self.reference_states is not None and len(set(self.reference_states)) != len(self.reference_states):
            raise ValueError(f"reference_states names a state twice: {list(self.reference_states)}")
        if self.reference_states is not None and len(self.reference_states) != shape[-1]:
            raise ValueError(f"profiles carry {shape[-1]} columns for the {len(self.reference_states)} reference_states {list(self.reference_states)}")
        self.profile_tau = None if profile_tau is None else float(profile_tau)
        self.interpolation, self.end, self.start = interpolation, end, start
        self.seed = None if seed is None else int(seed)
        self.shape = shape

    per_env = property(lambda self: len(self.shape) == 3, doc="one profile per env ([T, N, n_ref])")

    def shard(self, lo, hi, n_total):
        """-> the holder of envs [lo, hi) of a job of n_total: a per-env table is sliced to the shard, a shared one is kept."""
        if not self.per_env:
            return self
        if self.shape[1] != int(n_total):
            raise ValueError(f"profiles are for {self.shape[1]} envs, the job has n_envs_total = {int(n_total)}")
        return ProfileReferenceGenerator(self.profiles[:, int(lo):int(hi)], self.reference_states, self.profile_tau, self.interpolation, self.end, self.start, self.seed)

    def __repr__(self):
        return (f"ProfileReferenceGenerator(profiles{list(self.shape)}, reference_states={self.reference_states!r}, profile_tau={self.profile_tau!r}, "
                f"interpolation={self.interpolation!r}, end={self.end!r}, start={self.start!r}, seed={self.seed!r})")


def as_profile_holder(generator):
    """-> the ProfileReferenceGenerator holder `generator` is (alone, or as a list of one), else None.  A list that mixes one with other
    holders is refused: ValueError."""
    if isinstance(generator, ProfileReferenceGenerator):
        return generator
    if isinstance(generator, (list, tuple)) and any(isinstance(g, ProfileReferenceGenerator) for g in generator):
        if len(generator) != 1:
            raise ValueError("reference_generator: " + PROFILE_MIXED_REFUSAL)
        return generator[0]
    return None


class ProfileReferences(_DeviceGenerators):
    """The device generator behind a ProfileReferenceGenerator holder (gemx_refprofile_*): the surface and the calling contract of the
    other device generators -- `reset(mask)`, `step(done)` (restart first, then show and advance), `rollout` (restarts after row k),
    `rollout_shell` (before it: K x step), `bind_step` / `bind_rollout_shell` (graph-capturable), `get_state` / `set_state`.  The table is
    this object's tensor, in the state order of the physical system; the handle borrows it."""

    _ABI = dict(reset="gemx_refprofile_reset", step="gemx_refprofile_step", rollout="gemx_refprofile_rollout", rollout_shell="gemx_refprofile_rollout_shell",
                state_bytes="gemx_refprofile_state_bytes", get_blob="gemx_refprofile_get_blob", set_blob="gemx_refprofile_set_blob", destroy="gemx_refprofile_destroy")

    def __init__(self, holder, seed=0, env_base=None):
        holder = as_profile_holder(holder)
        if holder is None:
            raise TypeError("ProfileReferences is built from a ProfileReferenceGenerator holder")
        self.holder = holder
        self._seed = int(holder.seed if holder.seed is not None else seed) & (2**64 - 1)
        self._env_base = None if env_base is None else int(env_base)
        self._handle = None
        self._refs = None

    def set_modules(self, physical_system, _defer_create=False, default_states=None):
        ps, h = physical_system, self.holder
        states = h.reference_states if h.reference_states is not None else tuple(default_states or ())
        n_ref = h.shape[-1]
        if len(states) != n_ref:
            raise ValueError(f"profiles carry {n_ref} columns for the {len(states)} referenced states {list(states)}")
        missing = [s for s in states if s not in ps.state_positions]
        if missing:
            raise ValueError(f"reference_states {missing} are not states of the physical system {list(ps.state_names)}")
        if h.per_env and h.shape[1] != ps.n_envs:
            raise ValueError(f"profiles are for N = {h.shape[1]} envs, the system has {ps.n_envs}")
        self._order = sorted(range(n_ref), key=lambda j: ps.state_positions[states[j]])  # the caller's columns -> state order
        self._ordered = tuple(states[j] for j in self._order)
        self._n_envs = ps.n_envs
        cfg = _lib.GemxRefprofileConfig()
        cfg.struct_size = C.sizeof(cfg)
        cfg.n_ref, cfg.n_rows, cfg.per_env = n_ref, h.shape[0], int(h.per_env)
        cfg.tau = float(ps.tau)
        cfg.profile_tau = h.profile_tau if h.profile_tau is not None else float(ps.tau)
        # (rows sampled at tau itself are shown as they are: w == 0 at every step, and nothing is interpolated)
        cfg.interpolation = _lib.PROFILE_INTERP_HOLD if cfg.profile_tau == cfg.tau else _PROFILE_CHOICES["interpolation"][h.interpolation]
        cfg.end, cfg.start = _PROFILE_CHOICES["end"][h.end], _PROFILE_CHOICES["start"][h.start]
        cfg.seed = self._seed
        cfg.env_base = self._env_base if self._env_base is not None else int(getattr(ps, "env_base", 0))
        self._cfg = cfg
        idx = [ps.state_positions[n] for n in self._ordered]
        self._space = (np.asarray(ps.state_space.low, dtype=float)[idx], np.asarray(ps.state_space.high, dtype=float)[idx])
        if _defer_create:
            return self
        import torch

        self._L = _lib.load()
        self._tdev, self._tdtype = ps._tdev, ps._tdtype
        self._table = torch.as_tensor(h.profiles).to(device=self._tdev, dtype=self._tdtype)[..., self._order].contiguous()
        handle = C.c_void_p()
        _lib.check(self._L.gemx_refprofile_create(C.byref(cfg), C.c_void_p(self._table.data_ptr()), self._n_envs, ps.device,
                                                  _lib.F64 if self._tdtype == torch.float64 else _lib.F32, C.byref(handle)))
        self._handle = handle
        self._refs = torch.zeros((self._n_envs, n_ref), dtype=self._tdtype, device=self._tdev)
        return self

    ratio = property(lambda self: self._cfg.tau / self._cfg.profile_tau, doc="rows per control step: tau / profile_tau")
    reference_space = property(lambda self: self._space, doc="(low, high) arrays [n_ref]: the state space's bounds of the referenced states")
    table = property(lambda self: self._table, doc="the device table the handle reads, columns in state order")

    def state(self):
        """dict(k, s, e) of int32 [N] tensors, for tests / inspection: steps shown since the episode began, its start row, episodes begun."""
        import torch

        out = torch.empty((3, self._n_envs), dtype=torch.int32, device=self._tdev)
        _lib.check(self._L.gemx_refprofile_get_state(self._handle, C.c_void_p(out.data_ptr()), self._stream()))
        torch.cuda.current_stream(self._tdev).synchronize()
        return dict(k=out[0], s=out[1], e=out[2])
