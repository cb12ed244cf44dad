"""Device-side episode time limit and episode statistics: the stage behind the launch that writes a step's `done` byte and reward
(csrc/gemx_episode.hip, include/gemx.h: gemx_episode_*).

A well-controlled motor never violates a constraint, so `terminated` never fires; users of the reference wrap `gem.make(...)` in
gymnasium's `TimeLimit` (and `RecordEpisodeStatistics`) for that reason.  `EpisodeStage` is both on the device, per env and in ONE launch
per step: `length += 1`, `ret += reward` (in float64 whatever the env's dtype), `truncated = length >= max_steps and not done`,
`ended = done | truncated`; where an episode ended its totals move to `last_length` / `last_ret`, `n_finished` counts it and the running
counters restart.  `reset_mask` is the mask of the masked `gemx_reset` in front of the NEXT step's physics (observation.py:
ObservationPipeline.bind_before_step): `truncated` when the stepping kernel restarts terminated envs itself, `ended` when it does not
(`auto_reset=False`, or behind a StateNoiseProcessor, whose physics runs without auto-reset).  `ended` replaces `done` as the byte the
reference generators restart on and the flux observer resets on: a truncated env is `env.reset()` in the reference.

`rows(done [K, N], reward [K, N])` is the same arithmetic over the stored rows of a K-step rollout in one pass -- bit for bit what K
calls of `step` leave -- and writes `ended [K, N]` and, optionally, `finished_return` (float64) / `finished_length` (int32) `[K, N]`: an
episode's totals at the row where it ended, 0 elsewhere.

The time limit INSIDE a fused K-step launch: `rollout`, `bind_rollout`, `rollout_complete` and `bind_rollout_complete` refuse an env with a
time limit (ROLLOUT_REFUSAL) -- their kernels cannot restart an env on a mask they have not seen.  The episodic entry points can
(`rollout_episodic`, `bind_rollout_episodic`, `rollout_complete_episodic`, `bind_rollout_complete_episodic`; csrc/gemx_episodic.hip,
gemx_rollout_episodic): truncation is `length >= max_steps and not done`, and `length` depends on nothing but the env's own done history,
so the kernel that steps the env produces the mask itself.  It reads this stage's `length`, keeps it in a register, applies the rule above
behind every control step, restarts every ended env within the launch and writes terminated, truncated and ended [K, N]; `rows` then runs
behind it on the same terminated and reward rows and moves the counters by the same rule from the same value -- the stage stays the one
owner of its state.  `after_episodic_rollout` leaves the stage as K steps would, except that no reset is pending: they have all happened.
What the kernel does not serve is listed by `episodic_refusal`.
"""
import ctypes as C
import operator

from . import _lib

ROLLOUT_REFUSAL = ("fused K-step rollouts cannot run with an episode time limit (max_episode_steps): a truncated env restarts from its reset state, and a "
                   "fused K-step launch cannot restart an env on a mask it has not seen; step the env (step / bind_step, HIP-graph capturable), or build "
                   "it with episode_statistics=True alone: the rollouts then run the statistics pass over their stored rows.  The episodic entry points "
                   "keep the time limit inside the launch: rollout_episodic / bind_rollout_episodic, rollout_complete_episodic / bind_rollout_complete_episodic")
EPISODIC_REFUSAL = "episodic rollouts (the episode time limit inside a fused K-step launch) are not available with "
NO_TIME_LIMIT = "episodic rollouts need an env built with a time limit, make(..., max_episode_steps=M); without one rollout / rollout_complete serve"
FIELDS = ("length", "ret", "last_length", "last_ret", "n_finished")


def episodic_refusal(system, what=None):
    """None, or the message of what the episodic rollout kernel does not serve for this physical system (needs no device: raised before
    anything is launched).  `what`: the message for a refused way of CALLING it (half-precision actions, last_only, synthetic actions)."""
    if what is not None:
        return EPISODIC_REFUSAL + what
    cfg = system._cfg
    if cfg.dtype == _lib.F64:
        return EPISODIC_REFUSAL + "dtype='float64' (the fp64 build is a diagnostic: step it)"
    if cfg.solver_flags & _lib.SOLVER_ADAPTIVE:
        return EPISODIC_REFUSAL + "the error-controlled Dormand-Prince solver (ScipyOdeSolver): EulerSolver or RK4Solver"
    if cfg.solver_kind not in (_lib.SOLVER_EULER, _lib.SOLVER_RK4):
        return EPISODIC_REFUSAL + "DormandPrince5Solver: EulerSolver or RK4Solver"
    if cfg.interlocking_time > 0:
        return EPISODIC_REFUSAL + "a converter interlocking time (dead time)"
    if cfg.action_delay > 0:
        return EPISODIC_REFUSAL + "a DeadTimeProcessor"
    if cfg.supply_kind != _lib.SUPPLY_IDEAL:
        return EPISODIC_REFUSAL + "an RCVoltageSupply"
    if cfg.init_kind != _lib.INIT_CONST:
        return EPISODIC_REFUSAL + "random initial states (an env restarts inside the launch from the system's one initial state)"
    return None


def check_max_episode_steps(value):
    """None (no time limit) or an integer >= 1 -> int | None; everything else is a ValueError."""
    if value is None:
        return None
    if isinstance(value, bool):
        raise ValueError(f"max_episode_steps must be an integer >= 1 or None, not {value!r}")
    try:
        steps = operator.index(value)
    except TypeError:
        raise ValueError(f"max_episode_steps must be an integer >= 1 or None, not {value!r}") from None
    if steps < 1 or steps > 0x7fffffff:
        raise ValueError(f"max_episode_steps must be an integer in [1, 2^31), not {value!r}")
    return int(steps)


class EpisodeStage:
    """The resolved episode stage of one env (see the module docstring).  max_steps: None | int >= 1; statistics: whether the env hands
    the counters out (`episode_statistics()`; the stage counts either way -- the time limit needs `length`); auto_reset_in_kernel: the
    stepping kernel restarts terminated envs itself; has_reward: the launches read a reward (the complete env's)."""

    def __init__(self, max_steps=None, statistics=False, auto_reset_in_kernel=False, has_reward=False):
        self.max_steps = check_max_episode_steps(max_steps) or 0
        self.statistics = bool(statistics)
        self.auto_reset_in_kernel, self.has_reward = bool(auto_reset_in_kernel), bool(has_reward)
        cfg = self._cfg = _lib.GemxEpisodeConfig()
        cfg.struct_size = C.sizeof(_lib.GemxEpisodeConfig)
        cfg.max_steps, cfg.auto_reset_in_kernel, cfg.has_reward = self.max_steps, int(self.auto_reset_in_kernel), int(self.has_reward)
        self._handle = None

    # ------------------------------------------------------------------ device side
    def create(self, n_envs, device, dtype_name="float32"):
        """Create the device handle (no CPU fallback: without a HIP device this raises) and everything a step writes: the state blob --
        the handle works in it, `fields()` are views of it -- and the truncated / ended / reset_mask bytes.  Nothing is allocated afterwards."""
        import torch

        L = _lib.load()
        n = self.n_envs = int(n_envs)
        self._tdev = torch.device("cuda", int(device))
        self._tdtype = torch.float64 if dtype_name == "float64" else torch.float32
        blob = self._blob = torch.zeros(_lib.EPISODE_STATE_BYTES * n, dtype=torch.uint8, device=self._tdev)
        self.ret, self.last_ret = blob[: 8 * n].view(torch.float64), blob[8 * n: 16 * n].view(torch.float64)
        self.length, self.last_length = blob[16 * n: 20 * n].view(torch.int32), blob[20 * n: 24 * n].view(torch.int32)
        self.n_finished = blob[24 * n:].view(torch.int32)  # (the device's u32; torch shows it as int32)
        self.truncated, self.ended, self.reset_mask = (torch.zeros(n, dtype=torch.uint8, device=self._tdev) for _ in range(3))
        h = C.c_void_p()
        _lib.check(L.gemx_episode_create(C.byref(self._cfg), n, _lib.F64 if dtype_name == "float64" else _lib.F32, int(device), C.c_void_p(blob.data_ptr()), C.byref(h)))
        self._handle, self._L = h, L
        return self

    def close(self):
        if getattr(self, "_handle", None) is not None:
            self._L.gemx_episode_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def fields(self):
        """dict(length, ret, last_length, last_ret, n_finished): [N] device tensors, views of the handle's state (nothing is copied)."""
        return {name: getattr(self, name) for name in FIELDS}

    def _st(self, stream):
        import torch

        return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(self._tdev)).cuda_stream)

    def _check(self, t, shape, what, dtype):
        import torch

        if not (torch.is_tensor(t) and t.device == self._tdev and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise ValueError(f"{what} must be a contiguous {dtype} tensor {tuple(shape)} on {self._tdev}")

    def _need_handle(self):
        if self._handle is None:
            raise _lib.GemxError("the episode stage has no device handle (built with _defer_create, or closed)")

    def _reward_arg(self, reward, shape):
        if (reward is not None) != self.has_reward:
            raise ValueError("the episode stage reads a reward exactly when it was built with has_reward")
        if reward is None:
            return None
        self._check(reward, shape, "reward", self._tdtype)
        return C.c_void_p(reward.data_ptr())

    def bind_step(self, done, reward=None, truncated=None, ended=None, reset_mask=None, stream=None):
        """-> zero-argument launch() of gemx_episode_step on fixed tensors: done [N] uint8, reward [N] (with has_reward) -> truncated, ended,
        reset_mask [N] uint8 (default: the stage's own buffers; `reset_mask` may be `done` itself)."""
        import torch

        self._need_handle()
        n = (self.n_envs,)
        truncated = self.truncated if truncated is None else truncated
        ended = self.ended if ended is None else ended
        reset_mask = self.reset_mask if reset_mask is None else reset_mask
        for t, what in ((done, "done"), (truncated, "truncated"), (ended, "ended"), (reset_mask, "reset_mask")):
            self._check(t, n, what, torch.uint8)
        args = (C.c_void_p(done.data_ptr()), self._reward_arg(reward, n), C.c_void_p(truncated.data_ptr()), C.c_void_p(ended.data_ptr()),
                C.c_void_p(reset_mask.data_ptr()), self._st(stream))
        return _lib.bound_call(self._L.gemx_episode_step, self, args, (done, reward, truncated, ended, reset_mask, stream))

    def step(self, done, reward=None, stream=None):
        """`bind_step` on the stage's own output buffers, run once -> (truncated, ended, reset_mask)."""
        self.bind_step(done, reward, stream=stream)()
        return self.truncated, self.ended, self.reset_mask

    def bind_rows(self, done, reward, ended, finished_return=None, finished_length=None, stream=None):
        """-> zero-argument launch() of gemx_episode_rows on fixed tensors: done [K, N] uint8, reward [K, N] (with has_reward) -> ended
        [K, N] uint8, finished_return [K, N] float64 | None, finished_length [K, N] int32 | None."""
        import torch

        self._need_handle()
        if not (torch.is_tensor(done) and done.dim() == 2):
            raise ValueError("done must be a uint8 tensor [K, N]")
        shape = (int(done.shape[0]), self.n_envs)
        self._check(done, shape, "done", torch.uint8)
        self._check(ended, shape, "ended", torch.uint8)
        if finished_return is not None:
            self._check(finished_return, shape, "finished_return", torch.float64)
        if finished_length is not None:
            self._check(finished_length, shape, "finished_length", torch.int32)
        args = (C.c_void_p(done.data_ptr()), self._reward_arg(reward, shape), shape[0], C.c_void_p(ended.data_ptr()),
                C.c_void_p(finished_return.data_ptr()) if finished_return is not None else None,
                C.c_void_p(finished_length.data_ptr()) if finished_length is not None else None, self._st(stream))
        return _lib.bound_call(self._L.gemx_episode_rows, self, args, (done, reward, ended, finished_return, finished_length, stream),
                               (ended, finished_return, finished_length))

    def rows(self, done, reward=None, ended=None, finished_return=None, finished_length=None, stream=None):
        """`bind_rows`, run once -> (ended, finished_return, finished_length); all three are allocated unless given."""
        import torch

        new = lambda dtype: torch.empty(tuple(done.shape), dtype=dtype, device=self._tdev)  # noqa: E731
        return self.bind_rows(done, reward, new(torch.uint8) if ended is None else ended, new(torch.float64) if finished_return is None else finished_return,
                              new(torch.int32) if finished_length is None else finished_length, stream)()

    def bind_after_episodic_rollout(self, truncated_rows, ended_rows, stream=None):
        """-> zero-argument launch() behind an episodic rollout and its `rows` pass: `truncated` and `ended` [N] take row K-1 of
        truncated_rows / ended_rows [K, N] (what the last of K steps would have left: `env.truncated` shows it), and `reset_mask` is
        cleared -- every ended env has restarted inside the launch, so the reset in front of the next step's physics has nothing to do.
        Three asynchronous device operations on `stream`, capturable."""
        import torch

        self._need_handle()
        shape = (int(truncated_rows.shape[0]), self.n_envs)
        self._check(truncated_rows, shape, "truncated", torch.uint8)
        self._check(ended_rows, shape, "ended", torch.uint8)
        stream = stream if stream is not None else torch.cuda.current_stream(self._tdev)
        truncated, ended, mask, last_t, last_e = self.truncated, self.ended, self.reset_mask, truncated_rows[shape[0] - 1], ended_rows[shape[0] - 1]

        def launch(_current=torch.cuda.current_stream, _on=torch.cuda.stream):
            if _current(self._tdev) == stream:
                truncated.copy_(last_t), ended.copy_(last_e), mask.zero_()
            else:
                with _on(stream):
                    truncated.copy_(last_t), ended.copy_(last_e), mask.zero_()

        return launch

    def restart(self):
        """`env.reset()`: every running episode is dropped (length = 0, ret = 0) and no env waits for a restart; the totals of finished
        episodes stay."""
        for t in (self.length, self.ret, self.truncated, self.ended, self.reset_mask):
            t.zero_()

    def get_state(self, stream=None):
        """All five fields as one uint8 device blob [28 N] (a copy; synchronises), for a checkpoint."""
        import torch

        self._need_handle()
        out = torch.empty_like(self._blob)
        _lib.check(self._L.gemx_episode_get_state(self._handle, C.c_void_p(out.data_ptr()), self._st(stream)))
        return out

    def set_state(self, state, stream=None):
        import torch

        self._need_handle()
        s = torch.as_tensor(state).to(device=self._tdev, dtype=torch.uint8).contiguous()
        if s.numel() != self._blob.numel():
            raise ValueError(f"the episode state of {self.n_envs} envs has {self._blob.numel()} bytes, not {s.numel()}")
        _lib.check(self._L.gemx_episode_set_state(self._handle, C.c_void_p(s.data_ptr()), self._st(stream)))
