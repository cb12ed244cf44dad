"""The waveform kinds of the reference's sub-episoded generators, restated in closed form (numpy, float64) -- the yardstick of
tests/test_refgen_kinds_cpu.py (against what the reference tabulated, tests/golden/refgen/refgen_kinds.npz) and of
tests/test_gpu_refgen_kinds.py (against what the device evaluates from the parameters it drew).  Paths relative to the reference's
reference_generators/:

    sinusoidal   sinusoidal_reference_generator.py:50-68   A sin(2 pi f t_k + phi) + o
    sawtooth     sawtooth_reference_generator.py:45-63     A saw(2 pi f t_k + phi, 1) + o
    triangular   triangle_reference_generator.py:49-75     A saw(2 pi f t_k + phi, w) + o
    step         step_reference_generator.py:37-61         A sign(f (t_j mod 1/f) - r) + o,  j = (k - roll) mod L  (numpy's roll over the
                                                           sub-episode of L steps), roll = int(U / (f tau))

with t_k = k tau, k = 0 .. L-1, each clipped to the limit margin afterwards.  `saw(x, w)` is scipy.signal.sawtooth: with
m = x mod 2 pi it rises as m / (pi w) - 1 while m < 2 pi w and falls as (pi (w + 1) - m) / (pi (1 - w)) after.

TOLERANCE: float64 rounding of a phase below 40 rad (2^-47 absolute ~ 7e-15, also what `k tau` differs from the reference's linspace by)
times an amplitude of at most 1, with the libm's sine: 1e-12 absolute; sawtooth and triangular waves magnify a phase error by their
slope, so there the bound is multiplied by max(1, 1/w, 1/(1-w)).

JUMPS: the sawtooth's wrap, the two edges of the step and the seam of its roll are discontinuities: a phase error of one rounding flips
the branch.  `waveform` therefore also evaluates at phase -/+ 1e-9 and reports the samples whose two evaluations take different branches;
only those may be left out of a comparison, and `MAX_EXCLUDED` (1e-3 of the compared samples) caps their share -- asserted by the tests.
"""
import numpy as np

TWO_PI = 2.0 * np.pi
ATOL = 1e-12
PHASE_EPS = 1e-9
MAX_EXCLUDED = 1e-3
KINDS = ("sinusoidal", "step", "triangular", "sawtooth")


def _saw_branch(x, w):
    """-> (value, branch index) of saw(x, w)."""
    m = np.mod(x, TWO_PI)
    rising = m < TWO_PI * w
    with np.errstate(divide="ignore", invalid="ignore"):
        up = m / (np.pi * w) - 1.0
        down = (np.pi * (w + 1.0) - m) / (np.pi * (1.0 - w))
    # the branch index also counts the periods, so that a wrap (rising -> rising of the next period when w = 1) is seen
    return np.where(rising, up, down), 2 * np.floor(x / TWO_PI) + np.where(rising, 0, 1)


def _step_branch(j, tau, f, ratio, shift=0.0):
    """-> (sign(f (t mod 1/f) - r), branch index) at t = j tau + shift."""
    t = j * tau + shift
    x = f * np.mod(t, 1.0 / f) - ratio
    return np.sign(x), 2 * np.floor(t * f) + (x > 0)


def evaluate(kind, k, length, tau, amplitude, frequency, offset, margin, phase=0.0, width=1.0, roll=0):
    """The waveform at the step indices k of sub-episodes of `length` steps -> (values, on_jump, tolerance); every argument may be an
    array (numpy broadcasting).  phase: radians (sinusoidal, sawtooth, triangular); width: the triangular wave's width, the step's
    high / low ratio; roll: the step's shift in samples."""
    k = np.asarray(k, dtype=np.float64)
    lo, hi = margin
    tol = np.full(np.broadcast(k, amplitude, frequency, phase, width).shape, ATOL)
    if kind == "step":
        j = np.mod(k - np.trunc(np.asarray(roll, dtype=np.float64)), np.asarray(length, dtype=np.float64))
        w = _step_branch(j, tau, frequency, width)[0]
        dt = PHASE_EPS / (TWO_PI * frequency)
        on_jump = (_step_branch(j, tau, frequency, width, -dt)[1] != _step_branch(j, tau, frequency, width, dt)[1]) | (w == 0)
    elif kind == "sinusoidal":
        w = np.sin(TWO_PI * frequency * (k * tau) + phase)
        on_jump = np.zeros(w.shape, dtype=bool)
    elif kind in ("sawtooth", "triangular"):
        x = TWO_PI * frequency * (k * tau) + phase
        wd = np.ones_like(x) if kind == "sawtooth" else np.broadcast_to(np.asarray(width, dtype=np.float64), x.shape)
        w = _saw_branch(x, wd)[0]
        on_jump = _saw_branch(x - PHASE_EPS, wd)[1] != _saw_branch(x + PHASE_EPS, wd)[1]
        with np.errstate(divide="ignore"):  # (w = 1: no falling branch, w = 0: no rising one)
            slope = np.maximum(np.where(wd > 0, 1.0 / wd, 1.0), np.where(wd < 1, 1.0 / (1.0 - wd), 1.0))
        tol = tol * np.maximum(1.0, slope)
    else:
        raise KeyError(kind)
    return np.minimum(np.maximum(amplitude * w + offset, lo), hi), np.broadcast_to(on_jump, tol.shape), tol


def waveform(kind, length, tau, amplitude, frequency, offset, margin, phase=0.0, width=1.0, roll=0):
    """One whole sub-episode: `evaluate` at k = 0 .. length-1."""
    return evaluate(kind, np.arange(int(length)), int(length), tau, amplitude, frequency, offset, margin, phase=phase, width=width, roll=roll)


def step_roll(frequency, tau, u):
    """int(steps_per_period * phase), step_reference_generator.py:56-58."""
    return int(1.0 / frequency / tau * u)


def offset_bounds(kind, amplitude, offset_range, margin):
    """The sub-episode's offset range: np.clip(offset_range, a, b) = min(max(x, a), b) with [a, b] = [-m_hi + A, m_hi - A], for the step
    generator [m_lo + A, m_hi - A] (e.g. sinusoidal_reference_generator.py:53-57, step_reference_generator.py:41-45)."""
    lo, hi = margin
    a = (lo if kind == "step" else -hi) + amplitude
    b = hi - amplitude
    return tuple(np.minimum(np.maximum(float(x), a), b) for x in offset_range)  # (amplitude may be an array)


def compare(got, want, on_jump, tol):
    """-> (largest error over the samples off the jumps, number of samples left out).  A sample on a jump that agrees is compared too."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bad = err > tol
    left_out = bad & on_jump
    keep = ~left_out
    return (err[keep].max() if keep.any() else 0.0), int(left_out.sum())
