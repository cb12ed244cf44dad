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

    # ------------------------------------------------------------------ evaluation over the stored rows of a rollout (csrc/gemx_policy_eval.hip)
    def _evaluate(self, what, bound, traj, head, mode, last, obs0, ended, reset_obs, n_ref, references, last_references, references_next, refs, shown0, actions,
                  pre_squash, log_std, squash_correction, dtype, outs, system, stream):
        """-> launch() of `gemx_policy_eval_rows` on fixed tensors.  Everything is refused before any device call, in one order: the mode /
        head / last combination; half precision anywhere; what the head needs; the input width; every input tensor (dtype, shape,
        contiguity), then their devices; a bound call's outputs given, then the outputs as tensors and their devices."""
        import torch

        heads = {"none": _lib.EVAL_HEAD_NONE, "value": _lib.EVAL_HEAD_VALUE, "categorical": _lib.EVAL_HEAD_CATEGORICAL, "gaussian": _lib.EVAL_HEAD_GAUSSIAN}
        if head not in heads:
            raise ValueError(f"{what}: head must be 'none', 'value', 'categorical' or 'gaussian', not {head!r}")
        if mode not in ("seen", "next"):
            raise ValueError(f"{what}: mode must be 'seen' or 'next', not {mode!r}")
        last = bool(last)
        if mode == "next" and last:
            raise ValueError(f"{what}: mode='next' cannot be combined with last=True (there is no row behind the last one; last=True belongs to mode='seen')")
        if last and head in ("categorical", "gaussian"):
            raise ValueError(f"{what}: last=True has no meaning with head={head!r} (no action was taken behind the last row)")
        out, out_last, value_out, value_last, log_prob_out, entropy_out = outs
        inputs = (("traj", traj), ("obs0", obs0), ("ended", ended), ("reset_obs", reset_obs), ("references", references), ("last_references", last_references),
                  ("references_next", references_next), ("refs", refs), ("shown0", shown0), ("actions", actions), ("pre_squash", pre_squash), ("log_std", log_std))
        outputs = (("out", out), ("out_last", out_last), ("value_out", value_out), ("value_last", value_last), ("log_prob_out", log_prob_out), ("entropy_out", entropy_out))
        for name, t in inputs + outputs:
            if torch.is_tensor(t) and t.dtype in (torch.float16, torch.bfloat16):
                raise NotImplementedError(f"{what}: {name} is half precision; the evaluation is an fp32 function of fp32 rows (float32 tensors)")
        if dtype not in (None, torch.float32, torch.float64):
            raise NotImplementedError(f"{what}: dtype must be torch.float32 or torch.float64 (the head outputs), not {dtype}")
        real = torch.float32 if dtype is None else dtype
        if head == "value" and self.n_out != 1:
            raise ValueError(f"{what}: head='value' needs a policy with one output (a critic), this one has n_out = {self.n_out}")
        if head == "categorical":
            if actions is None:
                raise ValueError(f"{what}: head='categorical' needs actions [K, N] uint8 (the stored actions)")
            if torch.is_tensor(actions) and actions.is_floating_point():
                raise ValueError(f"{what}: head='categorical' takes the stored uint8 actions [K, N], not a {actions.dtype} tensor (a continuous converter's actions go with head='gaussian')")
        elif actions is not None:
            raise ValueError(f"{what}: actions belong to head='categorical'")
        if head == "gaussian":
            if pre_squash is None or log_std is None:
                raise ValueError(f"{what}: head='gaussian' needs pre_squash [K, N, n_out] (out + noise, what was squashed into the action) and log_std [n_out], both float32 device tensors")
        elif pre_squash is not None or log_std is not None or squash_correction:
            raise ValueError(f"{what}: pre_squash, log_std and squash_correction belong to head='gaussian'")
        if not torch.is_tensor(traj) or traj.dim() != 3 or min(traj.shape) < 1:
            raise ValueError(f"{what}: traj must be a tensor [K, N, S] (the rows a policy rollout wrote)")
        K, N, S = (int(v) for v in traj.shape)
        if S > _lib.MAX_OUT:
            raise ValueError(f"{what}: traj has {S} columns; a stored row has at most {_lib.MAX_OUT} (GEMX_MAX_OUT)")
        columns = list(range(S)) if self.columns is None else list(self.columns)
        if any(c >= S for c in columns):
            raise ValueError(f"{what}: the policy selects column {max(columns)}, a stored row has {S} columns")
        complete = refs is not None or shown0 is not None
        if mode == "seen":
            if references_next is not None:
                raise ValueError(f"{what}: references_next belongs to mode='next'")
            if complete and (references is not None or last_references is not None):
                raise ValueError(f"{what}: give references (the physics-only form) or refs and shown0 (the complete form), not both")
            if complete and (refs is None or shown0 is None):
                raise ValueError(f"{what}: the complete form needs both refs [K, N, n_ref] and shown0 [N, n_ref]")
            shifted, along, first = complete, (refs if complete else references), shown0
        else:
            if obs0 is not None or ended is not None or reset_obs is not None or shown0 is not None or references is not None or last_references is not None:
                raise ValueError(f"{what}: mode='next' reads traj and refs (the complete form) or references_next only")
            if refs is not None and references_next is not None:
                raise ValueError(f"{what}: give refs (the complete form) or references_next, not both")
            shifted, along, first = False, (refs if refs is not None else references_next), None
        if n_ref is None:
            n_ref = int(along.shape[-1]) if torch.is_tensor(along) and along.dim() == 3 else 0
        if len(columns) + n_ref != self.n_in:
            raise ValueError(f"{what}: {len(columns)} observation columns + {n_ref} references = {len(columns) + n_ref} inputs, the policy's first layer takes {self.n_in}")
        if not 0 <= n_ref <= _lib.MAX_REF:
            raise ValueError(f"{what}: {n_ref} reference columns; 0 to {_lib.MAX_REF}")
        if n_ref > 0 and along is None:
            raise ValueError(f"{what}: the policy reads {n_ref} references: give {'refs' if complete else 'references_next or refs' if mode == 'next' else 'references'} [K, N, {n_ref}]")
        if mode == "seen":
            if obs0 is None:
                raise ValueError(f"{what}: obs0 [N, S] must be given (the observation in front of step 0)")
            if (K > 1 or last) and (ended is None or reset_obs is None):
                raise ValueError(f"{what}: ended [K, N] (terminated | truncated) and reset_obs [S] or [N, S] must be given")
            if last and n_ref > 0 and not complete and last_references is None:
                raise ValueError(f"{what}: last=True needs last_references [N, n_ref] in the physics-only form")
            if last_references is not None and not last:
                raise ValueError(f"{what}: last_references belongs to last=True")
        per_env = torch.is_tensor(reset_obs) and reset_obs.dim() == 2
        specs = [("traj", traj, torch.float32, (K, N, S)), ("obs0", obs0, torch.float32, (N, S)), ("ended", ended, torch.uint8, (K, N)),
                 ("reset_obs", reset_obs, torch.float32, (N, S) if per_env else (S,)), ("references", references, torch.float32, (K, N, n_ref)),
                 ("last_references", last_references, torch.float32, (N, n_ref)), ("references_next", references_next, torch.float32, (K, N, n_ref)),
                 ("refs", refs, torch.float32, (K, N, n_ref)), ("shown0", shown0, torch.float32, (N, n_ref)), ("actions", actions, torch.uint8, (K, N)),
                 ("pre_squash", pre_squash, torch.float32, (K, N, self.n_out)), ("log_std", log_std, torch.float32, (self.n_out,))]
        want = {"none": [("out", torch.float32, (K, N, self.n_out))] + ([("out_last", torch.float32, (N, self.n_out))] if last else []),
                "value": [("value_out", real, (K, N))] + ([("value_last", real, (N,))] if last else []),
                "categorical": [("log_prob_out", real, (K, N)), ("entropy_out", real, (K, N))],
                "gaussian": [("log_prob_out", real, (K, N)), ("entropy_out", real, (K, N))]}[head]
        given = dict(outputs)
        for name, t, dt, shape in specs:
            _check_eval_tensor(what, name, t, dt, shape)
        if traj.device.type != "cuda":
            raise ValueError(f"{what}: traj must be a device tensor (cuda), not on {traj.device}: there is no CPU fallback")
        for name, t in inputs:
            if t is not None and t.device != traj.device:
                raise ValueError(f"{what}: {name} must be on {traj.device} like traj, not on {t.device}")
        for name, t in outputs:
            if t is not None and name not in [w[0] for w in want]:
                raise ValueError(f"{what}: {name} is not an output of head={head!r}{' with last=True' if last else ''}")
        if bound:
            for name, _, _ in want:
                if given[name] is None:
                    raise ValueError(f"{what}: {name} must be given (a bound launch allocates nothing)")
        for name, dt, shape in want:
            _check_eval_tensor(what, name, given[name], dt, shape)
        for name, t in outputs:
            if t is not None and t.device != traj.device:
                raise ValueError(f"{what}: {name} must be on {traj.device} like traj, not on {t.device}")
        device = traj.device.index if traj.device.index is not None else torch.cuda.current_device()
        if system is not None and getattr(system, "_handle", None) is None:
            raise _lib.GemxError("the physical system has no device handle (built with _defer_create, or closed)")
        made = {name: (given[name] if given[name] is not None else torch.empty(shape, dtype=dt, device=traj.device)) for name, dt, shape in want}
        handle = self._on_device(device)
        call = _lib.GemxPolicyEvalCall()
        call.struct_size, call.mode, call.head = C.sizeof(call), (_lib.EVAL_NEXT if mode == "next" else _lib.EVAL_SEEN), heads[head]
        call.flags = (_lib.EVAL_LAST if last else 0) | (_lib.EVAL_SQUASH_CORRECTION if squash_correction else 0)
        call.out_dtype, call.n_state, call.n_cols, call.n_ref = (_lib.F64 if real == torch.float64 else _lib.F32), S, len(columns), n_ref
        for i, c in enumerate(columns):
            call.columns[i] = c
        call.reset_per_env = 1 if per_env else 0
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        call.obs0_dev, call.rows_dev, call.reset_obs_dev, call.ended_dev = ptr(obs0), ptr(traj), ptr(reset_obs), ptr(ended)
        if n_ref > 0:
            call.refs_dev, call.refs0_dev, call.last_refs_dev = ptr(along), (ptr(first) if shifted else None), ptr(last_references)
        call.actions_dev, call.pre_squash_dev, call.log_std_dev = ptr(actions), ptr(pre_squash), ptr(log_std)
        call.out_dev, call.out_last_dev, call.value_out_dev, call.value_last_dev = (ptr(made.get(k)) for k in ("out", "out_last", "value_out", "value_last"))
        call.log_prob_out_dev, call.entropy_out_dev = ptr(made.get("log_prob_out")), ptr(made.get("entropy_out"))
        call.error_handle = system._handle if system is not None else None
        st = stream if stream is not None else torch.cuda.current_stream(traj.device)
        result = tuple(made[name] for name, _, _ in want)
        keep = (call, st, system) + tuple(t for _, t in inputs) + result
        return _lib.bound_call(_lib.load().gemx_policy_eval_rows, self, (C.byref(call), N, K, device, C.c_void_p(st.cuda_stream)), keep,
                               result[0] if len(result) == 1 else result)

    def bind_evaluate_rollout(self, traj, *, head="none", mode="seen", last=False, obs0=None, ended=None, reset_obs=None, n_ref=None, references=None,
                              last_references=None, references_next=None, refs=None, shown0=None, actions=None, pre_squash=None, log_std=None,
                              squash_correction=False, dtype=None, out=None, out_last=None, value_out=None, value_last=None, log_prob_out=None,
                              entropy_out=None, system=None, stream=None):
        """-> zero-argument launch() of `evaluate_rollout` on fixed tensors: every output of the head must be given, nothing is allocated,
        one launch on one stream (`stream`, or the current stream at bind time) with no host synchronisation -- it can be captured with
        `torch.cuda.graph` behind `bind_rollout_policy_*`; `set_weights` and new values in `log_std` are read at the next replay."""
        return self._evaluate("bind_evaluate_rollout", True, traj, head, mode, last, obs0, ended, reset_obs, n_ref, references, last_references, references_next, refs,
                              shown0, actions, pre_squash, log_std, squash_correction, dtype, (out, out_last, value_out, value_last, log_prob_out, entropy_out), system, stream)

    def evaluate_rollout(self, traj, *, head="none", mode="seen", last=False, obs0=None, ended=None, reset_obs=None, n_ref=None, references=None,
                         last_references=None, references_next=None, refs=None, shown0=None, actions=None, pre_squash=None, log_std=None,
                         squash_correction=False, dtype=None, out=None, out_last=None, value_out=None, value_last=None, log_prob_out=None, entropy_out=None,
                         system=None, stream=None):
        """This MLP on every row of a stored policy rollout, in ONE launch with the rollout kernel's own arithmetic (csrc/gemx_policy_eval.hip).
        `traj [K, N, S]` are the rows the rollout wrote.  Row k's input is `[o[k][columns], r[k]]`:

        mode="seen" (what the actor saw): `o[0] = obs0 [N, S]`, `o[k] = traj[k-1]`, or `reset_obs` ([S] or [N, S]) where `ended[k-1]`
            (`ended [K, N]` uint8 = terminated | truncated); `r[k] = references[k]` (the physics-only form), or `r[0] = shown0 [N, n_ref]`,
            `r[k] = refs[k-1]` (the complete form: what `rollout_policy_complete_episodic` returned).  For rows and a policy that came from
            a policy rollout, head="none" gives bit for bit the value that rollout had in front of `+ noise[k]`.  last=True evaluates one
            more row, k = K (`r[K] = last_references [N, n_ref]`, or `refs[K-1]`): a critic's row K is the `last_value` of `ga.advantages`.
        mode="next": `o[k] = traj[k]` without reset substitution, `r[k] = refs[k]` or `references_next[k]`: a critic's rows are the
            `final_value` of `ga.advantages` (read at truncated rows only).

        head="none" -> out [K, N, n_out] float32 (last=True: (out, out_last [N, n_out]));  head="value" (n_out == 1) -> value [K, N]
        (last=True: (value, last_value [N]));  head="categorical" (`actions [K, N]` uint8) -> (log_prob, entropy) [K, N], log_prob =
        out[a] - logsumexp(out), an action >= n_out sets the error word of `system` (a physical system; `system.check_errors()` raises as for
        any bad action) and gives NaN;  head="gaussian" (`pre_squash [K, N, n_out]` = out_old + noise, `log_std [n_out]`, float32 on the
        device) -> (log_prob, entropy), with squash_correction=True minus the tanh change of variables sum_j 2 (log 2 - u_j - softplus(-2 u_j)).
        Heads compute in float64 from the float32 `out`, every operation rounded on its own, and round once to `dtype` (torch.float32, the
        default, or torch.float64).  No gradients; there is no CPU fallback."""
        return self._evaluate("evaluate_rollout", False, traj, head, mode, last, obs0, ended, reset_obs, n_ref, references, last_references, references_next, refs, shown0,
                              actions, pre_squash, log_std, squash_correction, dtype, (out, out_last, value_out, value_last, log_prob_out, entropy_out), system, stream)()

    def close(self):
        if self._handle is not None:
            _lib.load().gemx_policy_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_eval_tensor(what, name, t, dtype, shape):
    """One tensor of an evaluation call: dtype, shape, contiguity, in this order; None passes (an optional argument)."""
    import torch

    if t is None:
        return
    if not torch.is_tensor(t):
        raise ValueError(f"{what}: {name} must be a tensor")
    if t.dtype != dtype:
        raise ValueError(f"{what}: {name} must have dtype {dtype}, not {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must have shape {tuple(shape)}, not {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")


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
