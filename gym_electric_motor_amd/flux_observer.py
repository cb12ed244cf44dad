"""Device-side FluxObserver and flux-oriented dq actions of the induction machines (csrc/gemx_fluxobs.hip, include/gemx.h:
gemx_fluxobs_*): the reference's `FluxObserver` (physical_system_wrappers/flux_observer.py:54-102) and the 'SCIM' / 'DFIM' variants of
its `DqToAbcActionProcessor` (dq_to_abc_action_processor.py:57-148) resolved for one batched physical system.

`FluxObserverStage(physical_system, current_names, action_mode=None)` holds

* the metadata of the two columns the observer appends, `psi_abs` and `psi_angle` (flux_observer.py:66-74);
* the configuration of the device handle (`create`, `reset`, `step`, `rows`, `actions`, `get_state`, `set_state`);
* the same recursion on the host in float64, `evaluate(state, done)`: stateful over a trajectory, with the reference's order -- the
  terminating step still shows the updated flux, the reset that follows clears it -- and `host_actions(dq)`, what the dq processor hands
  to the system beneath it.  Both are test infrastructure and serve data that never was on a device.

DEVIATION: the reference asserts that the motor is an induction machine (an AssertionError, flux_observer.py:56-59); here it is a
NotImplementedError that names the FluxObserver, raised before any attribute of the wrapper is read.
"""
import ctypes as C

import numpy as np

from . import _lib

_T23 = 2 / 3 * np.array([[1, -0.5, -0.5], [0, 0.5 * np.sqrt(3), -0.5 * np.sqrt(3)]])
_T32 = np.array([[1, 0], [-0.5, 0.5 * np.sqrt(3)], [-0.5, -0.5 * np.sqrt(3)]])
_MODES = {None: _lib.FLUX_ACT_NONE, "SCIM": _lib.FLUX_ACT_SCIM, "DFIM": _lib.FLUX_ACT_DFIM}

ROLLOUT_REFUSAL = ("fused K-step rollouts cannot run with the flux-oriented dq action processor: each step's Park angle depends on the previous "
                   "step's observation (psi_angle, omega), so a fused K-step launch cannot hold it; step the env (step / bind_step, which a "
                   "HIP graph can replay) or pass abc actions")


def _q(dq, angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.stack((c * dq[..., 0] - s * dq[..., 1], s * dq[..., 0] + c * dq[..., 1]), axis=-1)


class FluxObserverStage:
    """The resolved flux observer of one physical system (see the module docstring)."""

    def __init__(self, physical_system, current_names=("i_sa", "i_sb", "i_sc"), action_mode=None, current_indices=None):
        ps = physical_system
        motor = ps.electrical_motor
        if not {c.__name__ for c in type(motor).__mro__} & {"InductionMotor", "SquirrelCageInductionMotor", "DoublyFedInductionMotor"}:
            raise NotImplementedError(f"a FluxObserver needs an induction machine (SCIM, DFIM), not a {type(motor).__name__} "
                                      "(the reference asserts the same, flux_observer.py:56-59)")
        if action_mode not in _MODES:
            raise ValueError(f"flux-oriented dq actions exist for 'SCIM' and 'DFIM', not {action_mode!r}")
        names = [str(n) for n in ps.state_names]
        if action_mode == "DFIM" and "i_ra" not in names:
            raise ValueError("the 'DFIM' dq action processor needs a doubly fed induction machine")
        if action_mode == "SCIM" and "i_ra" in names:
            raise ValueError("the 'SCIM' dq action processor drives one B6 bridge; a doubly fed machine takes the 'DFIM' one")
        self.action_mode = action_mode
        self.current_names = tuple(current_names)
        if len(self.current_names) != 3:
            raise ValueError(f"a FluxObserver observes three phase currents, got {list(self.current_names)}")
        self.n_in = len(names)
        self.current_indices = [names.index(c) for c in self.current_names] if current_indices is None else [int(i) for i in current_indices]
        self.omega_index = names.index("omega")
        self.epsilon_index = names.index("epsilon")
        mp = motor.motor_parameter
        self.l_m, self.l_r, self.r_r, self.p = float(mp["l_m"]), float(mp["l_m"] + mp["l_sigr"]), float(mp["r_r"]), float(mp["p"])
        self.tau = float(ps.tau)
        self.limits = np.asarray(ps.limits, dtype=float)
        self.psi_limit = self.l_m * float(self.limits[names.index("i_sd")])
        self.angle_advance = 0.5 + int(getattr(ps, "dead_time", 0) or 0)
        self.auto_reset = bool(getattr(ps, "_auto_reset", False))
        self.n_action = {None: 0, "SCIM": 2, "DFIM": 4}[action_mode]
        # the columns the observer appends (flux_observer.py:66-74): (name, limit, nominal, low, high)
        self.columns = (("psi_abs", self.psi_limit, self.psi_limit, -self.psi_limit, self.psi_limit), ("psi_angle", np.pi, np.pi, -np.pi, np.pi))
        self._reset_obs = None
        self._handle = None
        self.host_reset()

    # ------------------------------------------------------------------ host side (float64)
    def _reset_row(self):
        return np.zeros(self.n_in) if self._reset_obs is None else self._reset_obs

    def set_reset_observation(self, row):
        """The system's constant reset observation (normalised): its omega (and epsilon) give the frame of the first action after a reset."""
        self._reset_obs = np.asarray(row, dtype=float)[: self.n_in].copy()
        self.host_reset()

    def _frames(self, row_norm, psi):
        """(frame 0, frame 1) the NEXT action is rotated by, from a normalised row and Psi (dq_to_abc_action_processor.py:86-88, 135-139)."""
        state = row_norm * self.limits
        psi_angle = np.angle(psi) / np.pi * np.pi  # (the processor reads the normalised column times its limit)
        adv = self.angle_advance * self.tau * state[..., self.omega_index] * self.p
        if self.action_mode == "DFIM":
            f0 = state[..., self.epsilon_index] + adv
            return f0, psi_angle - f0
        return psi_angle + adv, np.zeros_like(adv)

    def host_reset(self, n=None):
        """Psi = 0 and the reset frames, for `n` lanes (default: keep the lane count, or one lane)."""
        n = int(n) if n is not None else (len(self._psi) if getattr(self, "_psi", None) is not None else 1)
        self._psi = np.zeros(n, dtype=complex)
        f0, f1 = self._frames(self._reset_row(), 0j)
        self._frame = np.tile(np.array([[float(f0)], [float(f1)]]), (1, n))

    def evaluate(self, state, done=None):
        """state [K, N, n_in] | [K, n_in] (normalised rows, in time order) and done [K, N] | [K] (lanes whose env was reset after that
        row) -> the rows extended by psi_abs, psi_angle, in float64.  Stateful: continues from the last call (see `host_reset`)."""
        s = np.asarray(state, dtype=np.float64)
        single = s.ndim == 2
        if single:
            s = s[:, None, :]
        if s.shape[-1] != self.n_in:
            raise ValueError(f"state has {s.shape[-1]} columns, the observer reads {self.n_in}")
        K, N = s.shape[:2]
        if len(self._psi) != N:
            self.host_reset(N)
        d = np.zeros((K, N), dtype=bool) if done is None else np.asarray(done).reshape(K, N).astype(bool)
        out = np.empty((K, N, self.n_in + 2))
        out[..., : self.n_in] = s
        k_i, k_psi = self.r_r * self.l_m / self.l_r, self.r_r / self.l_r
        r0 = self._frames(self._reset_row(), 0j)
        for k in range(K):
            phys = s[k] * self.limits
            i_ab = phys[:, self.current_indices] @ _T23.T
            w_el = phys[:, self.omega_index] * self.p
            delta = (i_ab[:, 0] + 1j * i_ab[:, 1]) * k_i - self._psi * (k_psi - 1j * w_el)
            self._psi = self._psi + delta * self.tau
            out[k, :, self.n_in] = np.abs(self._psi) / self.psi_limit
            out[k, :, self.n_in + 1] = np.angle(self._psi) / np.pi
            f0, f1 = self._frames(s[k], self._psi)
            self._frame = np.stack((f0, f1))
            if done is not None and self.auto_reset:
                self._psi = np.where(d[k], 0j, self._psi)
                self._frame = np.where(d[k], np.array([[float(r0[0])], [float(r0[1])]]), self._frame)
        return out[:, 0] if single else out

    def host_actions(self, dq):
        """dq [N, 2 | 4] -> abc [N, 3 | 6] = t_32(q(dq, frame)) with the frames the last `evaluate` / `host_reset` left."""
        a = np.asarray(dq, dtype=np.float64).reshape(-1, self.n_action)
        out = [_q(a[:, :2], self._frame[0]) @ _T32.T]
        if self.action_mode == "DFIM":
            out.append(_q(a[:, 2:], self._frame[1]) @ _T32.T)
        return np.concatenate(out, axis=-1)

    # ------------------------------------------------------------------ device side
    def _build_config(self):
        cfg = _lib.GemxFluxobsConfig()
        cfg.struct_size = C.sizeof(_lib.GemxFluxobsConfig)
        cfg.n_in, cfg.omega_index, cfg.epsilon_index = self.n_in, self.omega_index, self.epsilon_index
        for j, i in enumerate(self.current_indices):
            cfg.current_index[j], cfg.current_limit[j] = i, float(self.limits[i])
        cfg.action_mode, cfg.auto_reset = _MODES[self.action_mode], int(self.auto_reset)
        cfg.omega_limit, cfg.epsilon_limit, cfg.psi_limit = float(self.limits[self.omega_index]), float(self.limits[self.epsilon_index]), self.psi_limit
        cfg.p, cfg.tau, cfg.k_current, cfg.k_flux = self.p, self.tau, self.r_r * self.l_m / self.l_r, self.r_r / self.l_r
        cfg.angle_advance = self.angle_advance
        row = self._reset_row()
        cfg.reset_omega, cfg.reset_epsilon = float(row[self.omega_index]), float(row[self.epsilon_index])
        return cfg

    def create(self, n_envs, device, dtype_name="float32"):
        """Create the device handle (no CPU fallback: without a HIP device this raises)."""
        import torch

        L = _lib.load()
        h = C.c_void_p()
        self._cfg = self._build_config()
        _lib.check(L.gemx_fluxobs_create(C.byref(self._cfg), int(n_envs), _lib.F64 if dtype_name == "float64" else _lib.F32, int(device), C.byref(h)))
        self._handle, self._L, self.n_envs = h, L, int(n_envs)
        self._tdev = torch.device("cuda", int(device))
        self._tdtype = torch.float64 if dtype_name == "float64" else torch.float32
        return self

    def close(self):
        if getattr(self, "_handle", None) is not None:
            self._L.gemx_fluxobs_destroy(self._handle)
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

    def reset(self, mask=None, stream=None):
        import torch

        m = None if mask is None else torch.as_tensor(mask).to(device=self._tdev, dtype=torch.uint8).contiguous()
        _lib.check(self._L.gemx_fluxobs_reset(self._handle, C.c_void_p(m.data_ptr()) if m is not None else None, self._st(stream)))

    def bind_step(self, state, done, out, stream=None):
        """-> zero-argument launch() of gemx_fluxobs_step on fixed tensors: state [N, n_in], done [N] uint8 | None, out [N, n_in + 2]."""
        import torch

        self._check(state, (self.n_envs, self.n_in), "state")
        self._check(out, (self.n_envs, self.n_in + 2), "out")
        if done is not None:
            self._check(done, (self.n_envs,), "done", torch.uint8)
        args = (C.c_void_p(state.data_ptr()), C.c_void_p(done.data_ptr()) if done is not None else None, C.c_void_p(out.data_ptr()), self._st(stream))
        return _lib.bound_call(self._L.gemx_fluxobs_step, self, args, (state, done, out, stream))

    def step(self, state, done, out, stream=None):
        self.bind_step(state, done, out, stream)()
        return out

    def bind_rows(self, state, done, out, stream=None):
        """-> zero-argument launch() of gemx_fluxobs_rows: state [K, N, n_in], done [K, N] uint8 | None, out [K, N, n_in + 2]."""
        import torch

        K = int(state.shape[0])
        self._check(state, (K, self.n_envs, self.n_in), "state")
        self._check(out, (K, self.n_envs, self.n_in + 2), "out")
        if done is not None:
            self._check(done, (K, self.n_envs), "done", torch.uint8)
        args = (C.c_void_p(state.data_ptr()), C.c_void_p(done.data_ptr()) if done is not None else None, K, C.c_void_p(out.data_ptr()), self._st(stream))
        return _lib.bound_call(self._L.gemx_fluxobs_rows, self, args, (state, done, out, stream))

    def rows(self, state, done, out=None, stream=None):
        import torch

        if out is None:
            out = torch.empty(tuple(state.shape[:-1]) + (self.n_in + 2,), dtype=self._tdtype, device=self._tdev)
        self.bind_rows(state, done, out, stream)()
        return out

    def bind_actions(self, dq, abc, stream=None):
        """-> zero-argument launch() of gemx_fluxobs_actions: dq [N, 2 | 4] -> abc [N, 3 | 6]."""
        self._check(dq, (self.n_envs, self.n_action), "dq actions")
        self._check(abc, (self.n_envs, self.n_action * 3 // 2), "abc actions")
        args = (C.c_void_p(dq.data_ptr()), C.c_void_p(abc.data_ptr()), self._st(stream))
        return _lib.bound_call(self._L.gemx_fluxobs_actions, self, args, (dq, abc, stream))

    def get_state(self, stream=None):
        """float64 device tensor [4, N]: Psi re, Psi im, frame 0, frame 1."""
        import torch

        out = torch.empty((4, self.n_envs), dtype=torch.float64, device=self._tdev)
        _lib.check(self._L.gemx_fluxobs_get_state(self._handle, C.c_void_p(out.data_ptr()), self._st(stream)))
        return out

    def set_state(self, state, stream=None):
        import torch

        s = torch.as_tensor(state).to(device=self._tdev, dtype=torch.float64).reshape(4, self.n_envs).contiguous()
        _lib.check(self._L.gemx_fluxobs_set_state(self._handle, C.c_void_p(s.data_ptr()), self._st(stream)))
        torch.cuda.current_stream(self._tdev).synchronize()  # (`s` may be a temporary)
