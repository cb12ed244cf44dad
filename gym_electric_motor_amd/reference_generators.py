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

The numpy PCG64 streams of the reference cannot be reproduced on a device; the generated process is the same in distribution
(tests/test_gpu_parity.py), chunked generation equals one-shot generation bit for bit (counter-based Philox).
"""
import ctypes as C

import numpy as np

from . import _lib


class BatchedWienerProcessReferenceGenerator:
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

    reference_names = property(lambda self: self._ordered)
    n_envs = property(lambda self: self._n_envs)
    is_set = property(lambda self: hasattr(self, "_cfg"), doc="set_modules has run")

    @staticmethod
    def _for_state(value, name, default):
        """A setting given for all generators, or as a dict by state name (states not named: the default)."""
        if isinstance(value, dict):
            return {k.lower(): v for k, v in value.items()}.get(name, default)
        return value

    def _margins(self, ps, name):
        """subepisoded_reference_generator.py:66-84."""
        i = ps.state_positions[name]
        low, high = ps.state_space.low[i], ps.state_space.high[i]
        lm = self._for_state(self._limit_margin, name, None)
        if lm is None:
            f = ps.nominal_state[i] / ps.limits[i]
            return f * low, f * high
        if isinstance(lm, (float, int)):
            return lm * low, lm * high
        if isinstance(lm, tuple):
            return lm[0] * low, lm[1] * high
        raise Exception("Unknown type for the limit margin.")

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
        import torch

        self._L = _lib.load()
        self._tdev = ps._tdev
        self._tdtype = ps._tdtype
        h = C.c_void_p()
        _lib.check(self._L.gemx_refgen_create(C.byref(cfg), self._n_envs, ps.device, _lib.F64 if self._tdtype == torch.float64 else _lib.F32, C.byref(h)))
        self._handle = h
        self._refs = torch.zeros((self._n_envs, int(cfg.n_ref)), dtype=self._tdtype, device=self._tdev)  # step()'s own buffer
        return self

    @property
    def reference_space(self):
        """(low, high) arrays [n_ref]: the generators' limit margins (MultipleReferenceGenerator.reference_space)."""
        n = int(self._cfg.n_ref)
        return np.array(self._cfg.margin_lo[:n], dtype=float), np.array(self._cfg.margin_hi[:n], dtype=float)

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
        _lib.check(self._L.gemx_refgen_reset(self._handle, C.c_void_p(m.data_ptr()) if m is not None else None, self._stream()))

    def rollout(self, K, done=None, out=None):
        """References of the next K control steps, [K, N, n_ref].  done [K, N] (optional): terminations of those steps known in
        advance (e.g. a recorded rollout): generators restart after a terminating step."""
        import torch

        if out is None:
            out = torch.empty((int(K), self._n_envs, int(self._cfg.n_ref)), dtype=self._tdtype, device=self._tdev)
        d = None if done is None else done.to(device=self._tdev, dtype=torch.uint8).contiguous()
        _lib.check(self._L.gemx_refgen_rollout(self._handle, C.c_void_p(d.data_ptr()) if d is not None else None, int(K),
                                               C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def step(self, done=None, out=None):
        """One env-shell step in ONE launch (gemx_refgen_step): the generators of the envs with done[env] != 0 restart, then every
        generator advances by one step.  Returns the references [N, n_ref] -- the buffer this generator owns (rewritten by every call)
        unless `out` is given.  `done` [N] uint8 device tensor, e.g. the physical system's `done`."""
        import torch

        if out is None:
            out = self._refs
        elif not (torch.is_tensor(out) and tuple(out.shape) == tuple(self._refs.shape) and out.dtype == self._tdtype and out.device == self._tdev and out.is_contiguous()):
            raise ValueError(f"step: out must be a contiguous {self._tdtype} tensor of shape {tuple(self._refs.shape)} on {self._tdev}")
        d = None
        if done is not None:
            d = done if (done.dtype == torch.uint8 and done.device == self._tdev and done.is_contiguous()) else done.to(device=self._tdev, dtype=torch.uint8).contiguous()
            if d.numel() != self._n_envs:
                raise ValueError(f"step: done must have {self._n_envs} elements")
        _lib.check(self._L.gemx_refgen_step(self._handle, C.c_void_p(d.data_ptr()) if d is not None else None, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def bind_step(self, done, stream=None):
        """-> zero-argument step(): `gemx_refgen_step(done) -> references` with the handle, both pointers and the stream resolved once."""
        import torch

        if not (torch.is_tensor(done) and done.dtype == torch.uint8 and done.device == self._tdev and done.is_contiguous() and done.numel() == self._n_envs):
            raise ValueError(f"bind_step needs a contiguous uint8 tensor of {self._n_envs} elements on {self._tdev}")
        stream = stream if stream is not None else torch.cuda.current_stream(self._tdev)
        call, check, refs = self._L.gemx_refgen_step, _lib.check, self._refs
        args = (C.c_void_p(done.data_ptr()), C.c_void_p(refs.data_ptr()), C.c_void_p(stream.cuda_stream))
        keep = (done, stream)

        def step(_args=args, _call=call, _keep=keep):
            rc = _call(self._handle, *_args)
            if rc:
                check(rc)
            return refs

        return step

    def apply_done(self, done):
        """After a rollout: envs with any termination in `done` ([K, N] or [N]) restart their generators (closed-loop use)."""
        import torch

        d = done if done.dim() == 1 else done.any(dim=0)
        self.reset(mask=d.to(torch.uint8))

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

    def close(self):
        if self._handle is not None:
            self._L.gemx_refgen_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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

    def close(self):
        pass
