"""A device MLP actor for policy-in-the-loop rollouts (csrc/gemx_policy.hip, include/gemx.h: gemx_policy_*, gemx_rollout_policy).

`MLPPolicy(layers=[(W1, b1), ..., (WL, bL)], activation="relu" | "tanh", columns=None, squash="tanh" | "clip")`: `W_l` is `[out, in]`,
float32.  The weights are uploaded once into one device blob, at the first rollout that uses the policy; `set_weights(layers)` copies
into the same blob, so a bound launch and a captured graph see the new weights at their next replay.  The input of control step k is
`x = [obs_prev[columns], references[k]]` (columns: all of the row by default), the action `squash(out + noise[k])` for a continuous
converter and the lowest index among the maxima of `out + noise[k]` for a finite one; `env.rollout_policy_episodic` documents the rest.
The limits (1 to 3 layers, widths <= 64, input width <= 48) are checked here, before any device call.
"""
import ctypes as C

import numpy as np

from . import _lib

_ACTIVATIONS = {"relu": _lib.POLICY_RELU, "tanh": _lib.POLICY_TANH}
_SQUASHES = {"tanh": _lib.POLICY_SQUASH_TANH, "clip": _lib.POLICY_SQUASH_CLIP}


def _check_layers(layers):
    try:
        layers = [(np.asarray(W), np.asarray(b)) for W, b in layers]
    except (TypeError, ValueError):
        raise ValueError("MLPPolicy: layers must be a list of (W [out, in], b [out]) pairs") from None
    if not 1 <= len(layers) <= _lib.POLICY_MAX_LAYERS:
        raise ValueError(f"MLPPolicy: {len(layers)} layers; 1 to {_lib.POLICY_MAX_LAYERS}")
    out = []
    for l, (W, b) in enumerate(layers):
        if W.ndim != 2 or b.ndim != 1 or b.shape[0] != W.shape[0]:
            raise ValueError(f"MLPPolicy: layer {l} needs W [out, in] and b [out], not {W.shape} and {b.shape}")
        if W.dtype == np.float16 or b.dtype == np.float16:
            raise ValueError(f"MLPPolicy: layer {l} is half precision; the actor is an fp32 function of fp32 weights")
        if not 1 <= W.shape[0] <= _lib.POLICY_MAX_WIDTH:
            raise ValueError(f"MLPPolicy: layer {l} has width {W.shape[0]}; every width is at most {_lib.POLICY_MAX_WIDTH}")
        if l > 0 and W.shape[1] != out[-1][0].shape[0]:
            raise ValueError(f"MLPPolicy: layer {l} takes {W.shape[1]} inputs, layer {l - 1} gives {out[-1][0].shape[0]}")
        if not (np.isfinite(W).all() and np.isfinite(b).all()):
            raise ValueError(f"MLPPolicy: layer {l} holds a value that is not finite")
        out.append((np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)))
    if not 1 <= out[0][0].shape[1] <= _lib.POLICY_MAX_INPUT:
        raise ValueError(f"MLPPolicy: input width {out[0][0].shape[1]}; at most {_lib.POLICY_MAX_INPUT}")
    return out


class MLPPolicy:
    def __init__(self, layers, activation="relu", columns=None, squash="tanh"):
        if activation not in _ACTIVATIONS:
            raise ValueError(f"MLPPolicy: activation must be 'relu' or 'tanh', not {activation!r}")
        if squash not in _SQUASHES:
            raise ValueError(f"MLPPolicy: squash must be 'tanh' or 'clip', not {squash!r}")
        self.layers = _check_layers(layers)
        self.activation, self.squash = activation, squash
        if columns is not None:
            columns = [int(c) for c in columns]
            if len(set(columns)) != len(columns) or any(c < 0 for c in columns):
                raise ValueError(f"MLPPolicy: columns must be distinct non-negative indices, not {columns}")
        self.columns = columns
        self._handle, self._device = None, None

    n_in = property(lambda self: int(self.layers[0][0].shape[1]))
    n_out = property(lambda self: int(self.layers[-1][0].shape[0]))
    widths = property(lambda self: [int(W.shape[0]) for W, _ in self.layers])

    def _pointers(self, layers):
        n = len(layers)
        fp = C.POINTER(C.c_float)
        W = (fp * n)(*[w.ctypes.data_as(fp) for w, _ in layers])
        b = (fp * n)(*[v.ctypes.data_as(fp) for _, v in layers])
        return W, b

    def _on_device(self, device):
        """The C handle, created (and the weights uploaded) at the first call; a policy belongs to the device of its first rollout."""
        if self._handle is not None:
            if device != self._device:
                raise ValueError(f"MLPPolicy: the weights live on device {self._device}, the env on device {device}")
            return self._handle
        L = _lib.load()
        cfg = _lib.GemxPolicyConfig()
        cfg.struct_size, cfg.n_layers, cfg.n_in = C.sizeof(cfg), len(self.layers), self.n_in
        for l, w in enumerate(self.widths):
            cfg.width[l] = w
        cfg.activation, cfg.squash = _ACTIVATIONS[self.activation], _SQUASHES[self.squash]
        W, b = self._pointers(self.layers)
        handle = C.c_void_p()
        _lib.check(L.gemx_policy_create(C.byref(cfg), W, b, int(device), C.byref(handle)))
        self._handle, self._device = handle, device
        return handle

    def set_weights(self, layers):
        """New weights of the SAME shapes, into the same device blob (synchronous; not inside a stream capture)."""
        new = _check_layers(layers)
        if [(W.shape, b.shape) for W, b in new] != [(W.shape, b.shape) for W, b in self.layers]:
            raise ValueError("MLPPolicy.set_weights: the layers must keep their shapes")
        self.layers = new
        if self._handle is not None:
            W, b = self._pointers(new)
            _lib.check(_lib.load().gemx_policy_set_weights(self._handle, W, b))

    def close(self):
        if self._handle is not None:
            _lib.load().gemx_policy_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_tanh(system, x):
    """tanh of a float32 device tensor as the actor computes it (the policy unit's `tanhf`, `gemx_policy_tanh_probe`) -> a new tensor;
    `system`: a physical system with a device handle.  The tests' epsilon_tanh is measured with it (profiles/policy_rollout.md)."""
    import torch

    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.is_contiguous() and x.device == system._tdev):
        raise ValueError(f"device_tanh: x must be a contiguous float32 tensor on {system._tdev}")
    y = torch.empty_like(x)
    st = torch.cuda.current_stream(system._tdev).cuda_stream
    _lib.check(system._L.gemx_policy_tanh_probe(system._handle, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), x.numel(), C.c_void_p(st)))
    return y
