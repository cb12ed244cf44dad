"""Parameter-holder mirrors of the reference's physical-system wrappers that run on the device.  They contain no logic:
`make(..., physical_system_wrappers=(...))` splits the tuple with `fold_wrappers`.

ACTION side, in front of `simulate()`: folded into the kernel's action stage (or passed as the
`action_delay=` / `action_frame=` arguments of `BatchedSCMLSystem`), so the fused rollout stays on the device.

    DeadTimeProcessor(steps[, reset_action]) physical_system_wrappers/dead_time_processor.py:8-85
    DqToAbcActionProcessor.make(motor_type)  physical_system_wrappers/dq_to_abc_action_processor.py:9-175

OBSERVATION side, behind `simulate()`: resolved by `observation.ObservationStage` into the column program of ONE post-processing
kernel (csrc/gemx_obsproc.hip) that reads the state rows the stepping kernels wrote.

    CurrentSumProcessor(currents[, limit])          physical_system_wrappers/current_sum_processor.py:7-65
    CosSinProcessor([angle][, remove_angle])        physical_system_wrappers/cos_sin_processor.py:7-89

FLUX OBSERVER (induction machines), a stage of its own between the two (flux_observer.py, csrc/gemx_fluxobs.hip): one launch behind
`simulate()` appends `psi_abs` and `psi_angle` to the row, keeps the flux estimate per env and the frame of the NEXT action; with
`FluxOrientedDqToAbcActionProcessor` one launch in front of `simulate()` rotates the dq actions by that frame.

    FluxObserver([current_names])                   physical_system_wrappers/flux_observer.py:9-102
    FluxOrientedDqToAbcActionProcessor(motor_type)  physical_system_wrappers/dq_to_abc_action_processor.py:91-148 ('SCIM', 'DFIM')

As in the reference, wrappers are applied innermost first: `(DeadTimeProcessor(2), DqToAbcActionProcessor.make("PMSM"))`
delays the abc action by two steps and lets the dq processor advance its angle by 0.5 + 2 steps (lines 83-86); an observation-side
processor sees the state names of everything listed before it.  The two sides do not interact, so they may be listed in any order.
The flux-oriented processor reads the observer's angle: it must be listed after a `FluxObserver` and after any `DeadTimeProcessor`.

STATE NOISE, a stage of its own directly behind `simulate()` (state_noise.py, csrc/gemx_statenoise.hip): the reference checks the
constraints and computes the reward on the NOISY state (core.py:344-350), so with this wrapper the physics runs without constraints,
auto-reset and fused reward, ONE launch adds the noise and decides `done` and the reward on the noisy row, and the env restarts the
terminated envs with a masked reset in front of the next step.  At most one, on states of the base system, listed before every
observation-side processor and `FluxObserver` (which then read the noisy row); the fused K-step rollouts refuse it.

    StateNoiseProcessor(states[, random_dist][, random_kwargs])   physical_system_wrappers/state_noise_processor.py:4-92
                                                                  ('normal', 'uniform', 'laplace')
"""


class DeadTimeProcessor:
    """The converter receives the action submitted `steps` control steps earlier; every reset refills the queue with the
    reset actions: zeros (the reference's default), or what a custom `reset_action` callable returns (dead_time_processor.py:27-50:
    a list of `steps` actions of the wrapped system's action space) -- on the accelerated path those `steps` actions must be ONE
    and the same action, which travels as a per-handle constant (gemx_config.action_delay_reset); a list of different actions is
    refused with a message."""

    def __init__(self, steps=1, reset_action=None, physical_system=None):
        self._steps = int(steps)
        assert self._steps > 0, f'The number of steps has to be greater than 0. A "{steps}" has been passed.'
        self._reset_actions = reset_action

    @property
    def dead_time(self):
        return self._steps


def _reset_action_row(w):
    """The ONE action a DeadTimeProcessor's custom reset_action refills the queue with, as a flat list of numbers (a MultiDiscrete
    action stays [a0, a1]: the system flattens it), or None for the default zeros.  Works on this module's holder and on the
    reference's own instance (whose set_physical_system() wraps the default into a callable as well: zeros come back as zeros)."""
    import numpy as np

    fn = getattr(w, "_reset_actions", None)
    if fn is None:
        return None
    acts = list(fn()) if callable(fn) else list(fn)
    steps = int(getattr(w, "dead_time", getattr(w, "_steps", len(acts))))
    if len(acts) != steps:
        raise ValueError(f"reset_action returned {len(acts)} actions for a dead time of {steps} steps (dead_time_processor.py:13-16)")
    rows = [np.atleast_1d(np.asarray(a, dtype=float)).ravel() for a in acts]
    if any(r.shape != rows[0].shape or not np.array_equal(r, rows[0]) for r in rows[1:]):
        raise NotImplementedError("DeadTimeProcessor(reset_action=...): the accelerated path refills the queue with `steps` copies of ONE action; "
                                  f"got different actions {[r.tolist() for r in rows]}")
    return [float(x) for x in rows[0]]


class DqToAbcActionProcessor:
    """(u_d, u_q[, u_e]) actions -> abc converter actions with the Park angle advanced by (0.5 + dead time) * tau * omega * p.
    Motor types 'PMSM' (any SynchronousMotorSystem) and 'EESM': folded into the stepping kernel's action stage.  The reference's
    'SCIM' / 'DFIM' variants read a 'psi_angle' state that only a FluxObserver wrapper provides: they are a holder of their own,
    `FluxOrientedDqToAbcActionProcessor`, served by the flux-observer stage."""

    _SUPPORTED = ("PMSM", "EESM")

    def __init__(self, motor_type="PMSM"):
        if motor_type not in self._SUPPORTED:
            raise NotImplementedError(f"DqToAbcActionProcessor for {motor_type!r} needs a flux observer; folded into the kernel's "
                                      f"action stage: {self._SUPPORTED}; for 'SCIM' / 'DFIM' list FluxOrientedDqToAbcActionProcessor(motor_type) "
                                      "after a FluxObserver()")
        self.motor_type = motor_type

    @classmethod
    def make(cls, motor_type, *args, **kwargs):
        return cls(motor_type)


class FluxObserver:
    """Appends the estimated rotor flux of an induction machine, `psi_abs` and `psi_angle`, to the state vector (flux_observer.py:9-48):
    an explicit Euler integration of the current model, once per control step, from the three named stator currents and omega."""

    def __init__(self, current_names=("i_sa", "i_sb", "i_sc"), physical_system=None):
        self._current_names = tuple(current_names)


class FluxOrientedDqToAbcActionProcessor:
    """The reference's `DqToAbcActionProcessor.make('SCIM')` / `.make('DFIM')` (dq_to_abc_action_processor.py:91-148): (u_d, u_q) actions
    rotated by psi_angle + (0.5 + dead time) * tau * omega * p; 'DFIM' takes four actions, the stator pair rotated by epsilon + that
    advance, the rotor pair by psi_angle minus the stator's angle.  Must be listed after a `FluxObserver` and after any
    `DeadTimeProcessor`.  Fused K-step rollouts refuse it: each step's angle depends on the previous step's observation."""

    _SUPPORTED = ("SCIM", "DFIM")

    def __init__(self, motor_type="SCIM"):
        if motor_type not in self._SUPPORTED:
            raise ValueError(f"FluxOrientedDqToAbcActionProcessor serves {self._SUPPORTED}, not {motor_type!r} (DqToAbcActionProcessor: 'PMSM', 'EESM')")
        self.motor_type = motor_type

    @classmethod
    def make(cls, motor_type, *args, **kwargs):
        return cls(motor_type)


class CurrentSumProcessor:
    """Appends `i_sum`, the sum of the named currents, to the state vector (current_sum_processor.py:10-22); its limit and nominal
    value are the maximum (`limit='max'`) or the sum (`'sum'`) of the source currents'."""

    def __init__(self, currents, limit="max", physical_system=None):
        self._currents = currents
        assert limit in ["max", "sum"]
        self._limit_name = limit


class CosSinProcessor:
    """Appends `cos(angle)` and `sin(angle)` of one state (an angle normalised to pi) to the state vector, optionally removing the
    angle itself (cos_sin_processor.py:19-31)."""

    def __init__(self, angle="epsilon", physical_system=None, remove_angle=False):
        self._angle = angle
        self._remove_angle = remove_angle

    @property
    def angle(self):
        return self._angle


class StateNoiseProcessor:
    """Adds random noise to the named states (state_noise_processor.py:31-92; the reference's keywords and defaults): `random_dist` is
    'normal', 'uniform' or 'laplace', `random_kwargs` numpy's keywords of that distribution -- scalars, or sequences of one value per
    state, as numpy broadcasts them over size=(random_length, len(states)).  `random_length` is accepted and unused: it only batches
    numpy's draws.  Constraints, reward and `terminated` are evaluated on the noisy state, as in the reference's env shell."""

    def __init__(self, states, random_dist="normal", random_kwargs=(), random_length=1000, physical_system=None):
        self._random_kwargs = dict(random_kwargs)
        self._random_length = int(random_length)
        self._states = states
        self._random_dist = random_dist

    @property
    def random_kwargs(self):
        return self._random_kwargs

    @random_kwargs.setter
    def random_kwargs(self, value):
        self._random_kwargs = dict(value)


def _state_noise_spec(w):
    """dict(states=, dist=, kwargs=) of a StateNoiseProcessor (this module's holder or the reference's instance, read by its attributes);
    NotImplementedError for an object whose parameters cannot be read and for a distribution the device does not draw."""
    from .state_noise import DISTRIBUTIONS, REFUSAL

    try:
        states, dist, kwargs = w._states, w._random_dist, dict(w._random_kwargs)
    except (AttributeError, TypeError, ValueError):
        raise NotImplementedError(REFUSAL + f"the parameters of this {type(w).__name__} cannot be read (_states, _random_dist, _random_kwargs)") from None
    if dist not in DISTRIBUTIONS:
        raise NotImplementedError(REFUSAL + f"random_dist {dist!r} is not drawn on the device")
    return dict(states=states if isinstance(states, str) else tuple(states), dist=dist, kwargs=kwargs)


def _observation_spec(w, names):
    """('sum', currents, 'max' | 'sum') | ('cossin', angle, remove_angle) | ('flux', wrapper) | None for an observation-side wrapper (holder or
    the reference's instance).  A FluxObserver travels as it is: ObservationStage checks the motor before it reads any attribute."""
    if "FluxObserver" in names:
        return ("flux", w)
    if "CurrentSumProcessor" in names:
        limit = getattr(w, "_limit_name", None)
        if limit is None:  # the reference's instance keeps the function: `max` or `np.sum`
            limit = "max" if getattr(w, "_limit", max) is max else "sum"
        return ("sum", tuple(w._currents), limit)
    if "CosSinProcessor" in names:
        return ("cossin", w._angle, bool(w._remove_angle))
    return None


def _flux_action_kind(w, names):
    """'SCIM' | 'DFIM' for a dq processor that reads the flux observer's angle (this module's holder, the reference's
    _ClassicDqToAbcActionProcessor with _angle_name == 'psi_angle', its _DFIMDqToAbcActionProcessor), else None."""
    if "FluxOrientedDqToAbcActionProcessor" in names:
        return w.motor_type
    if "_DFIMDqToAbcActionProcessor" in names:
        return "DFIM"
    if "DqToAbcActionProcessor" in names and getattr(w, "_angle_name", "epsilon") == "psi_angle":
        return "SCIM"
    return None


def fold_wrappers(wrappers, observation_chain=None):
    """-> dict(action_delay=..., action_frame=...[, action_delay_reset=...]) for BatchedSCMLSystem from a reference-style wrapper tuple (innermost first).
    Accepts this module's holders and the reference's own instances (by class name).  The observation-side processors
    (CurrentSumProcessor, CosSinProcessor, FluxObserver), in any position, are appended to the list `observation_chain` as specs for
    `observation.ObservationStage`, innermost first; without such a list they are refused like any other wrapper the kernels' action stage
    cannot hold.  A StateNoiseProcessor comes back as `state_noise=dict(states=, dist=, kwargs=)` -- not a BatchedSCMLSystem argument
    either: make() hands it to the env."""
    from .state_noise import REFUSAL as NOISE_REFUSAL

    delay, frame, seen_dq, reset_row = 0, None, False, None  # frame None: leave it to the system's control_space
    seen_flux, flux_action, noise, seen_obs = False, None, None, False
    for w in wrappers:
        names = {c.__name__ for c in type(w).__mro__}
        spec = _observation_spec(w, names)
        flux_kind = _flux_action_kind(w, names)
        if spec is not None and observation_chain is not None:
            seen_obs = True
            if spec[0] == "flux":
                if seen_flux:
                    raise ValueError("one FluxObserver per system")
                if flux_action:
                    raise ValueError("the FluxObserver must be listed BEFORE the flux-oriented dq action processor, which reads its psi_angle")
                seen_flux = True
            observation_chain.append(spec)
        elif flux_kind is not None and seen_flux:
            if seen_dq:
                raise ValueError("one dq action processor per system")
            flux_action, seen_dq = flux_kind, True
        elif "StateNoiseProcessor" in names:
            if noise is not None:
                raise NotImplementedError(NOISE_REFUSAL + "a second StateNoiseProcessor was listed")
            if seen_obs:  # (an inner observation-side processor would read the clean row, and its columns could be noised)
                raise NotImplementedError(NOISE_REFUSAL + "this one is listed behind an observation-side processor (noise on appended columns)")
            noise = _state_noise_spec(w)
        elif "DeadTimeProcessor" in names:
            if seen_dq:
                raise ValueError("DeadTimeProcessor must be wrapped INSIDE the DqToAbcActionProcessor (listed before it), as the "
                                 "reference's processor expects (dq_to_abc_action_processor.py:83-86)")
            row = _reset_action_row(w)
            if delay and (row or reset_row) and row != reset_row:
                raise NotImplementedError("several DeadTimeProcessors with different reset actions are not on the accelerated path")
            reset_row = row if row is not None else reset_row
            delay += int(getattr(w, "dead_time", getattr(w, "_steps", 0)))
        elif "FluxOrientedDqToAbcActionProcessor" in names:
            raise NotImplementedError("FluxOrientedDqToAbcActionProcessor needs a flux observer: list a FluxObserver() before it")
        elif "DqToAbcActionProcessor" in names:
            if "_DFIMDqToAbcActionProcessor" in names or getattr(w, "_angle_name", "epsilon") != "epsilon":
                raise NotImplementedError("dq processors that need a flux observer (SCIM, DFIM) are not on the accelerated path")
            frame, seen_dq = "dq_processor", True
        else:
            raise NotImplementedError(f"physical-system wrapper {type(w).__name__} is not on the accelerated path (observation "
                                      "post-processing stays on the host: wrap the n_envs=1 system with the reference's wrapper)")
    out = dict(action_delay=delay, action_frame=frame)
    if flux_action:
        out["flux_action"] = flux_action  # (not a BatchedSCMLSystem argument: make() takes it out and hands it to the env)
    if reset_row is not None and any(reset_row):
        out["action_delay_reset"] = reset_row
    if noise is not None:
        out["state_noise"] = noise
    return out
