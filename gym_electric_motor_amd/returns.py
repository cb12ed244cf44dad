"""Discounted returns and generalised advantage estimates, GAE(lambda), over the stored rows of a rollout, on the device and in ONE launch
(csrc/gemx_returns.hip, include/gemx.h: gemx_returns_rows): the reverse scan over K per env that every learner runs on what
`rollout_complete` hands out -- `reward [K, N]`, `done [K, N]` (and `ended [K, N]` with `episode_statistics=True`) -- and a critic's
`value [K, N]`.  Per env, for k = K-1 ... 0, with one float64 accumulator A and everything converted to float64 first:

    term = terminated[k] != 0;  end = ended[k] != 0 (no `ended`: end = term);  trunc = end and not term
    v      = value[k]
    v_next = last_value if k == K-1 else value[k+1]                       (no `last_value`: 0)
    if end:  v_next = final_value[k] if trunc and final_value given else 0
    t1 = gamma * v_next;  delta = (reward[k] + t1) - v
    t2 = gamma * lam;     t3 = t2 * A;   A = delta if end else delta + t3
    advantage[k] = A;  returns[k] = A + v                                 (rounded to the tensors' dtype)

A starts as `carry_in` (0 without) and `carry_out` receives it after row 0, so a long trajectory can be scanned in pieces, the later rows
first: rows [k0, K) and then rows [0, k0) with `carry_out -> carry_in` and `last_value = value[k0]` equal one scan, bit for bit.
`terminated` is the env's `done`; `ended` is `terminated | truncated`, what an env with `episode_statistics=True` hands out;
`final_value` is the critic's value of a truncated episode's final observation and is read ONLY at rows with `ended and not terminated`.
A truncated row WITHOUT `final_value` is treated as terminated: the next row's value belongs to another episode, so nothing is
bootstrapped from it.  Every product and sum is rounded on its own in float64 (no fused multiply-add): a numpy restatement of the lines
above gives the same bits.

`discounted_returns` is the same pass without a critic: v = 0 and v_next = 0 in every row, lam = 1, and the accumulator starts as
`carry_in` if given, else as `last_value` if given, else as 0 (giving both is a ValueError): returns[k] = reward[k] + gamma *
returns[k+1], cut where an episode ended (a truncated row is treated as terminated).

There is no fallback: without the library or a HIP device the calls raise.  The outputs must not overlap the inputs or each other.
"""
import ctypes as C

from . import _lib

GROUP_ROWS = 16  # csrc/gemx_returns.hip: the rows a lane has in flight; K below, at and above a multiple of it take different paths of the kernel


class _Bound:
    """What a launcher keeps: the config struct; `_handle` is the first argument of gemx_returns_rows (`_lib.bound_call`)."""

    def __init__(self, gamma, lam):
        cfg = self._cfg = _lib.GemxReturnsConfig()
        cfg.struct_size = C.sizeof(_lib.GemxReturnsConfig)
        cfg.gamma, cfg.lam, cfg.flags = float(gamma), float(lam), 0
        self._handle = C.pointer(cfg)


def _unit_interval(x, what):
    try:
        x = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number in [0, 1], not {x!r}") from None
    if not 0.0 <= x <= 1.0:  # (NaN fails too)
        raise ValueError(f"{what} must be in [0, 1], not {x!r}")
    return x


def _check(t, what, shape, dtype):
    """t: a contiguous tensor of `shape` and `dtype`; None passes (an optional argument)."""
    import torch

    if t is None:
        return
    if not torch.is_tensor(t):
        raise ValueError(f"{what} must be a torch tensor, not {type(t).__name__}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, not {tuple(t.shape)}")
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, not {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def _validate(reward, value, terminated, last_value, ended, final_value, carry_in, carry_out, advantage_out, return_out, out_name="return_out"):
    """Every ValueError of the surface, before anything touches a device -> (K, N).  Shapes, dtypes and strides first, the devices last:
    a call with host tensors of the wrong shape names the shape."""
    import torch

    if not torch.is_tensor(reward):
        raise ValueError(f"reward must be a torch tensor, not {type(reward).__name__}")
    if reward.dim() != 2 or reward.shape[0] < 1 or reward.shape[1] < 1:
        raise ValueError(f"reward must have shape [K, N] with K, N >= 1, not {tuple(reward.shape)}")
    if reward.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"reward must be float32 or float64, not {reward.dtype}")
    if not reward.is_contiguous():
        raise ValueError("reward must be contiguous")
    K, N = int(reward.shape[0]), int(reward.shape[1])
    if K > 0x7fffffff:
        raise ValueError(f"reward has K = {K} rows: K must be below 2^31")
    if terminated is None:
        raise ValueError("terminated must be given (the env's done, uint8 [K, N])")
    named = (("terminated", terminated, (K, N), torch.uint8), ("ended", ended, (K, N), torch.uint8), ("value", value, (K, N), reward.dtype),
             ("final_value", final_value, (K, N), reward.dtype), ("last_value", last_value, (N,), reward.dtype), ("carry_in", carry_in, (N,), torch.float64),
             ("carry_out", carry_out, (N,), torch.float64), ("advantage_out", advantage_out, (K, N), reward.dtype), (out_name, return_out, (K, N), reward.dtype))
    for what, t, shape, dtype in named:
        _check(t, what, shape, dtype)
    if reward.device.type != "cuda":
        raise ValueError(f"reward must be a device tensor (cuda), not on {reward.device}: there is no CPU fallback")
    for what, t, _, _ in named:
        if t is not None and t.device != reward.device:
            raise ValueError(f"{what} must be on {reward.device} like reward, not on {t.device}")
    return K, N


def _bind(gamma, lam, reward, value, terminated, last_value, ended, final_value, carry_in, carry_out, advantage_out, return_out, stream, result, out_name="return_out"):
    import torch

    K, N = _validate(reward, value, terminated, last_value, ended, final_value, carry_in, carry_out, advantage_out, return_out, out_name)
    L = _lib.load()
    owner = _Bound(gamma, lam)
    st = stream if stream is not None else torch.cuda.current_stream(reward.device)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    tensors = (reward, value, last_value, terminated, ended, final_value, carry_in, carry_out, advantage_out, return_out)
    args = (N, K, _lib.F64 if reward.dtype == torch.float64 else _lib.F32, reward.device.index if reward.device.index is not None else torch.cuda.current_device(),
            *(ptr(t) for t in tensors), C.c_void_p(st.cuda_stream))
    return _lib.bound_call(L.gemx_returns_rows, owner, args, tensors + (st,), result)


def bind_advantages(reward, value, terminated, *, gamma, lam, last_value=None, ended=None, final_value=None, carry_in=None, advantage_out=None, return_out=None,
                    carry_out=None, stream=None):
    """-> zero-argument launch() of the GAE pass on fixed tensors, returning (advantage_out, return_out).  Nothing is allocated: at least
    one of `advantage_out` / `return_out` must be given, and an output that is None is not written.  One launch on one stream (`stream`, or the
    current stream at bind time): it can be captured with `torch.cuda.graph` behind `bind_rollout_complete`.  See the module docstring."""
    gamma, lam = _unit_interval(gamma, "gamma"), _unit_interval(lam, "lam")
    if value is None:
        raise ValueError("value must be given (a critic's values [K, N]); discounted_returns is the pass without one")
    if advantage_out is None and return_out is None:
        raise ValueError("at least one of advantage_out and return_out must be given")
    return _bind(gamma, lam, reward, value, terminated, last_value, ended, final_value, carry_in, carry_out, advantage_out, return_out, stream,
                 (advantage_out, return_out))


def advantages(reward, value, terminated, *, gamma, lam, last_value=None, ended=None, final_value=None, carry_in=None, advantage_out=None, return_out=None,
               carry_out=None, stream=None):
    """GAE(lambda) advantages and returns (advantage + value) of the stored rows -> (advantage, returns), [K, N] of reward's dtype; both are
    allocated unless given.  See the module docstring for the row function and the optional tensors."""
    import torch

    gamma, lam = _unit_interval(gamma, "gamma"), _unit_interval(lam, "lam")
    if value is None:
        raise ValueError("value must be given (a critic's values [K, N]); discounted_returns is the pass without one")
    _validate(reward, value, terminated, last_value, ended, final_value, carry_in, carry_out, advantage_out, return_out)
    advantage_out = torch.empty_like(reward) if advantage_out is None else advantage_out
    return_out = torch.empty_like(reward) if return_out is None else return_out
    return bind_advantages(reward, value, terminated, gamma=gamma, lam=lam, last_value=last_value, ended=ended, final_value=final_value, carry_in=carry_in,
                           advantage_out=advantage_out, return_out=return_out, carry_out=carry_out, stream=stream)()


def bind_discounted_returns(reward, terminated, *, gamma, out, last_value=None, ended=None, carry_in=None, carry_out=None, stream=None):
    """-> zero-argument launch() of the discounted return-to-go on fixed tensors, returning `out`.  Nothing is allocated; one launch on one
    stream, capturable like `bind_advantages`.  `last_value` and `carry_in` both seed the accumulator: give one of them at most."""
    gamma = _unit_interval(gamma, "gamma")
    if out is None:
        raise ValueError("out must be given: bind_discounted_returns allocates nothing")
    if last_value is not None and carry_in is not None:
        raise ValueError("last_value and carry_in both seed the accumulator of discounted_returns: give one of them, not both")
    return _bind(gamma, 1.0, reward, None, terminated, last_value, ended, None, carry_in, carry_out, None, out, stream, out, "out")


def discounted_returns(reward, terminated, *, gamma, last_value=None, ended=None, carry_in=None, out=None, carry_out=None, stream=None):
    """Discounted return-to-go of the stored rows -> returns [K, N] of reward's dtype (allocated unless `out` is given):
    returns[k] = reward[k] + gamma * returns[k+1], cut where an episode ended, the row above K-1 being `last_value` (or `carry_in`, the
    float64 accumulator of the scan over the rows behind these; at most one of the two)."""
    import torch

    gamma = _unit_interval(gamma, "gamma")
    if last_value is not None and carry_in is not None:
        raise ValueError("last_value and carry_in both seed the accumulator of discounted_returns: give one of them, not both")
    _validate(reward, None, terminated, last_value, ended, None, carry_in, carry_out, None, out, "out")
    out = torch.empty_like(reward) if out is None else out
    return bind_discounted_returns(reward, terminated, gamma=gamma, out=out, last_value=last_value, ended=ended, carry_in=carry_in, carry_out=carry_out, stream=stream)()
