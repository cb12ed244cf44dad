"""Device-side StateNoiseProcessor: the stage behind a physical system that runs WITHOUT constraints, auto-reset and fused reward
(csrc/gemx_statenoise.hip, include/gemx.h: gemx_noise_*).

The reference adds the noise inside the wrapped system's `simulate()` / `reset()` (physical_system_wrappers/state_noise_processor.py:
62-92), so its env shell checks the constraints and computes the reward on the NOISY state (core.py:344-350).  `StateNoiseStage` is that
order on the device: ONE launch adds the draws to the noisy columns, decides `done` on the noisy row with the stepping kernels'
constraint expressions and rewards it with the arithmetic of `gemx_reward_rows`; the env feeds the done mask back as the mask of the
next step's `gemx_reset` (envs.py, observation.py: ObservationPipeline).

`spec`: what `fold_wrappers` reads off the wrapper -- dict(states=, dist=, kwargs=) -- plus, from `make()`, the constraints and the
auto-reset the user asked for: limit_mask, squared_mask, auto_reset.  The three distributions take numpy's keywords and defaults:
normal(loc=0, scale=1), uniform(low=0, high=1), laplace(loc=0, scale=1); a value may be a scalar or a sequence of one value per
noisy state.  The draws are counter-based (Philox) streams keyed by the system's seed and global env index: parity with numpy's
streams is distributional.
"""
import ctypes as C

import numpy as np

from . import _lib

DISTRIBUTIONS = {"normal": (_lib.NOISE_NORMAL, ("loc", "scale"), (0.0, 1.0)), "uniform": (_lib.NOISE_UNIFORM, ("low", "high"), (0.0, 1.0)),
                 "laplace": (_lib.NOISE_LAPLACE, ("loc", "scale"), (0.0, 1.0))}
REFUSAL = ("StateNoiseProcessor: the reference checks the constraints and computes the reward on the NOISY state (core.py:344-350); the device-side "
           "stage (csrc/gemx_statenoise.hip) serves ONE wrapper with random_dist 'normal', 'uniform' or 'laplace' on states of the base physical "
           "system, listed before every observation-side processor and FluxObserver, with obs_layout='aos': ")
ROLLOUT_REFUSAL = ("fused K-step rollouts cannot run with a StateNoiseProcessor: the constraints are checked on the noisy state behind the physics, and a "
                   "fused K-step launch cannot restart an env on a done mask it has not seen; step the env (step / bind_step, HIP-graph capturable)")


class StateNoiseStage:
    """The resolved state-noise stage of one physical system (see the module docstring)."""

    def __init__(self, physical_system, spec, reward_config=None):
        ps = physical_system
        names = [str(n) for n in ps.state_names]
        self.n_in = len(names)
        if self.n_in > _lib.MAX_OUT:
            raise ValueError(f"the physical system has {self.n_in} states, the state-noise stage reads at most {_lib.MAX_OUT}")
        states = spec["states"]
        if isinstance(states, str):  # (the docstring's 'all' included: the reference's set_physical_system looks up its characters)
            raise KeyError(states)
        self.states = tuple(states)
        self.indices = [ps.state_positions[s] for s in self.states]  # (KeyError for an unknown name, as state_noise_processor.py:68)
        if len(set(self.indices)) != len(self.indices):
            raise ValueError(f"StateNoiseProcessor({list(self.states)}): a state is listed twice")
        self.dist = str(spec["dist"])
        kind, keys, defaults = DISTRIBUTIONS[self.dist]
        kwargs = dict(spec.get("kwargs") or {})
        unknown = sorted(set(kwargs) - set(keys))
        if unknown:
            raise TypeError(f"StateNoiseProcessor(random_dist={self.dist!r}): unknown random_kwargs {unknown}; known: {list(keys)}")
        n = len(self.indices)
        # numpy broadcasts the keywords over size=(random_length, n_states): a scalar, or one value per noisy state
        self.params = [np.broadcast_to(np.asarray(kwargs.get(k, d), dtype=float), (n,)).copy() for k, d in zip(keys, defaults)]
        if self.dist == "uniform":
            if (self.params[1] < self.params[0]).any():
                raise ValueError("StateNoiseProcessor(random_dist='uniform'): high < low")
        elif (self.params[1] < 0).any():
            raise ValueError("scale < 0")  # (numpy's message)
        self.limit_mask, self.squared_mask = int(spec.get("limit_mask", 0)), int(spec.get("squared_mask", 0))
        self.auto_reset = bool(spec.get("auto_reset", False))
        self.seed, self.env_base = int(getattr(ps, "_seed", 0)), int(getattr(ps, "_env_base", 0))
        self.reward_config = reward_config
        self._kind = kind
        self._cfg = self._build_config()
        self._handle = None

    def _build_config(self):
        cfg = _lib.GemxNoiseConfig()
        cfg.struct_size = C.sizeof(_lib.GemxNoiseConfig)
        cfg.n_in, cfg.n_noisy = self.n_in, len(self.indices)
        for j, i in enumerate(self.indices):
            cfg.index[j], cfg.dist[j] = i, self._kind
            cfg.param0[j], cfg.param1[j] = float(self.params[0][j]), float(self.params[1][j])
        cfg.seed, cfg.env_base = self.seed, self.env_base
        cfg.limit_mask, cfg.squared_mask = self.limit_mask, self.squared_mask
        cfg.has_reward = int(self.reward_config is not None)
        if self.reward_config is not None:
            C.memmove(C.byref(cfg.reward), C.byref(self.reward_config), C.sizeof(_lib.GemxRewardConfig))
        return cfg

    @property
    def n_ref(self):
        return int(self.reward_config.n_ref) if self.reward_config is not None else 0

    # ------------------------------------------------------------------ device side
    def create(self, n_envs, device, dtype_name="float32"):
        """Create the device handle (no CPU fallback: without a HIP device this raises).  Nothing is allocated afterwards."""
        import torch

        L = _lib.load()
        h = C.c_void_p()
        _lib.check(L.gemx_noise_create(C.byref(self._cfg), int(n_envs), _lib.F64 if dtype_name == "float64" else _lib.F32, int(device), C.byref(h)))
        self._handle, self._L, self.n_envs = h, L, int(n_envs)
        self._tdev = torch.device("cuda", int(device))
        self._tdtype = torch.float64 if dtype_name == "float64" else torch.float32
        return self

    def close(self):
        if getattr(self, "_handle", None) is not None:
            self._L.gemx_noise_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _st(self, stream):
        import torch

        return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(self._tdev)).cuda_stream)

    def _check(self, t, shape, what, dtype=None):
        import torch

        dtype = dtype or self._tdtype
        if not (torch.is_tensor(t) and t.device == self._tdev and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise ValueError(f"{what} must be a contiguous {dtype} tensor {tuple(shape)} on {self._tdev}")

    def bind_step(self, state, refs, out, done, reward=None, stream=None):
        """-> zero-argument launch() of gemx_noise_step on fixed tensors: state [N, n_in] -> out [N, n_in] (may be `state` itself), done [N]
        uint8, reward [N] | None against refs [N, n_ref].  A launch advances the stream position by one."""
        import torch

        if self._handle is None:
            raise _lib.GemxError("the state-noise stage has no device handle (built with _defer_create, or closed)")
        self._check(state, (self.n_envs, self.n_in), "state")
        self._check(out, (self.n_envs, self.n_in), "out")
        self._check(done, (self.n_envs,), "done", torch.uint8)
        need_refs = reward is not None and self.n_ref > 0
        if reward is not None:
            if self.reward_config is None:
                raise ValueError("the state-noise stage has no reward description")
            self._check(reward, (self.n_envs,), "reward")
        if need_refs:
            self._check(refs, (self.n_envs, self.n_ref), "refs")
        args = (C.c_void_p(state.data_ptr()), C.c_void_p(refs.data_ptr()) if need_refs else None, C.c_void_p(out.data_ptr()), C.c_void_p(done.data_ptr()),
                C.c_void_p(reward.data_ptr()) if reward is not None else None, self._st(stream))
        return _lib.bound_call(self._L.gemx_noise_step, self, args, (state, refs, out, done, reward, stream))

    def step(self, state, refs=None, out=None, done=None, reward=None, stream=None):
        """`bind_step`, run once -> (out, done, reward); `out` and `done` are allocated unless given."""
        import torch

        out = torch.empty_like(state) if out is None else out
        done = torch.empty(self.n_envs, dtype=torch.uint8, device=self._tdev) if done is None else done
        self.bind_step(state, refs, out, done, reward, stream)()
        return out, done, reward

    def draws(self, step0, K, stream=None):
        """-> [K, N, n_noisy]: the draws of stream positions step0 .. step0 + K - 1, as `step` adds them; the position does not move."""
        import torch

        out = torch.zeros((int(K), self.n_envs, len(self.indices)), dtype=self._tdtype, device=self._tdev)
        _lib.check(self._L.gemx_noise_draws(self._handle, int(step0), int(K), C.c_void_p(out.data_ptr()), self._st(stream)))
        return out

    def get_position(self, stream=None):
        """The stream position (synchronises)."""
        pos = C.c_uint64(0)
        _lib.check(self._L.gemx_noise_get_position(self._handle, C.byref(pos), self._st(stream)))
        return int(pos.value)

    def set_position(self, position, stream=None):
        _lib.check(self._L.gemx_noise_set_position(self._handle, int(position), self._st(stream)))
