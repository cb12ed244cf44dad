"""The complete env with every device stage on at once -- state noise, episode time limit and statistics, flux observer, reference
generators, reward, the observation program -- against the float64 HOST shell (tests/env_shell_restatement.py, pinned to recorded runs of
the reference by tests/test_env_shell_cpu.py), not against a twin built from the same library.

Each case (tests/env_shell_cases.py) is built with `ga.make(...)` as a user would, stepped K times with `env.step`, and every returned
tensor, the state rows behind the observation and `env.episode_statistics()` are compared with the shell, every lane, every step.  Two
device streams are handed to the shell, not restated: the noise through `StateNoiseStage.draws(step0, K + 1)` and every sub-episode's
waveform parameters through `reference_generator.state()` (collected per lane in the order they appear; the shell takes the next set
whenever ITS rules start a sub-episode, so a restart the device makes too often, too rarely or for the wrong lane puts the two out of step).

float64: values within TOL_FP64_SAME_INTEGRATOR (absolute, angles on the circle); terminated, truncated, length, last_length, n_finished exact;
no lane left out.  float32: values within TOL_FP32 relative to max(max|column|, REL_FLOOR), the induction machines' field-oriented
columns weighted by min(1, |psi_r| / (FLUX_FLOOR max|psi_r|)); masks and counters
exact; a lane is compared up to its first close call only -- a step whose constraint margin IN THE SHELL is below DONE_MARGIN -- and at
most 2 % of the lane-steps may be left out that way (asserted, printed; tests/test_env_shell_cpu.py establishes it for the inputs).

Case A runs once per noise distribution: `make()` takes one StateNoiseProcessor, and it has one distribution; each run noises three
columns, so the second Philox block is half used.  Case C: `make()` accepts the flux-oriented dq processor beside the noise wrapper, so
the case runs.  Every case's run is repeated through `bind_step` in a HIP graph and must equal the eager run bit for bit.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)  # (sibling modules: the shell, its cases, the contract)

import env_shell_cases as cases  # noqa: E402
import env_shell_restatement as esr  # noqa: E402
from parity_contract import DONE_MARGIN, FLUX_FLOOR, REL_FLOOR, TOL_FP32, TOL_FP64_SAME_INTEGRATOR  # noqa: E402

MAX_LEFT_OUT = 0.02
WARM_UP = 3
EXACT = ("terminated", "truncated", "length", "last_length", "n_finished")
STATS = ("length", "ret", "last_length", "last_ret", "n_finished")


def _collect_params(gen, seen, sets):
    """Append, per column and lane, the parameter set the generator holds now if it is not the one seen last."""
    s = {k: v.cpu().numpy() for k, v in gen.state().items()}
    rows = np.stack([s[k].astype(np.float64) for k in esr.PARAM_KEYS], axis=-1)  # [n_ref, N, 7]
    for c in range(rows.shape[0]):
        for j in range(rows.shape[1]):
            if seen[c][j] is None or not np.array_equal(seen[c][j], rows[c, j]):
                seen[c][j] = rows[c, j]
                sets[c][j].append(dict(zip(esr.PARAM_KEYS, rows[c, j])))


def _device_run(torch, ga, spec, dtype, acts, graph=False):
    """The case's env: reset, WARM_UP steps on zero actions, reset, K steps -> dict of stacked host arrays (+ what the shell is handed).
    graph: the K steps are replays of ONE captured `bind_step`, with the warm-up on the capture stream."""
    env = ga.make(spec["env_id"], **cases.make_kwargs(ga, spec, dtype))
    ps, K = env.physical_system, spec["K"]
    a = torch.as_tensor(acts).to(device="cuda", dtype=ps._want_dtype).contiguous()
    buf = torch.zeros_like(a[0])
    keys = ("obs", "rows", "refs", "reward", "terminated", "truncated") + STATS
    out = {k: [] for k in keys}

    def snapshot(obs, reward, term, trunc):
        stats = env.episode_statistics()
        for k, t in zip(keys, (obs if torch.is_tensor(obs) else obs[0], env.pipeline.rows, env.reference_generator.references, reward, term, trunc) + tuple(stats[f] for f in STATS)):
            out[k].append(t.clone())

    seen = [[None] * spec["N"] for _ in spec["generators"]]
    sets = [[[] for _ in range(spec["N"])] for _ in spec["generators"]]
    info = {}
    if graph:
        side = torch.cuda.Stream()
        step, obs, reward, term = env.bind_step(buf, stream=side)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on the capture stream, then a fresh start
            env.reset()
            for _ in range(WARM_UP):
                step()
            env.reset()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step()
        torch.cuda.synchronize()
        for k in range(K):
            buf.copy_(a[k])
            g.replay()
            torch.cuda.synchronize()
            snapshot(obs, reward, term, env.truncated)
    else:
        env.reset()
        for _ in range(WARM_UP):
            env.step(buf)
        info["position"] = env.state_noise.get_position() if env.state_noise is not None else 0
        first, _ = env.reset()
        info["first"] = {k: t.double().cpu().numpy() for k, t in (("obs", first if torch.is_tensor(first) else first[0]), ("rows", env.pipeline.rows), ("refs", env.reference_generator.references))}
        _collect_params(env.reference_generator, seen, sets)
        for k in range(K):
            obs, reward, term, trunc, _ = env.step(a[k])
            snapshot(obs, reward, term, trunc)
            _collect_params(env.reference_generator, seen, sets)
        if env.state_noise is not None:
            info["draws"] = env.state_noise.draws(info["position"], K + 1).double().cpu().numpy()
            assert env.state_noise.get_position() == info["position"] + K + 1
    torch.cuda.synchronize()
    res = {k: torch.stack(v) for k, v in out.items()}
    env.close()
    return res, sets, info


def _errors(got, want, dtype, weight=None, circle=()):
    """per-column errors of [K, N, C] (or [K, N]) arrays over the lane-steps where `weight` > 0 -> worst, by the contract's measure:
    float64 absolute, float32 relative to max(max|column|, REL_FLOOR); weight [K, N] | [K, N, C] multiplies the deviation."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.ndim == 2:
        got, want = got[..., None], want[..., None]
    d = np.abs(got - want)
    for c in circle:
        d[..., c] = np.minimum(d[..., c], 2.0 - d[..., c])
    if weight is not None:
        d = d * (weight if np.ndim(weight) == 3 else np.asarray(weight)[..., None])
    d = d.reshape(-1, d.shape[-1]).max(axis=0)
    if dtype == "float32":
        d = d / np.maximum(np.abs(want).reshape(-1, want.shape[-1]).max(axis=0), REL_FLOOR)
    return float(d.max())


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_complete_env_matches_the_host_shell(case, dtype):
    import torch

    import gym_electric_motor_amd as ga

    spec = cases.CASES[case]
    K, N = spec["K"], spec["N"]
    acts = cases.actions(spec)
    dev, sets, info = _device_run(torch, ga, spec, dtype, acts)
    shell = cases.build_shell(ga, spec, sets)
    first, out = shell.run(acts, info.get("draws"), 0)

    # what the inputs must show, read off the SHELL
    term, trunc = out["terminated"], out["truncated"]
    assert term.any() and trunc.any() and (term.any(axis=0) & trunc.any(axis=0)).any()
    decided = int((term != out["clean_terminated"]).any(axis=0).sum())
    assert decided >= 1 or spec["noise"] is None

    keep = np.ones((K, N), dtype=bool)
    if dtype == "float32":
        keep = np.arange(K)[:, None] < esr.first_close_call(out["margin"], DONE_MARGIN)[None, :]
    share = 1.0 - float(keep.mean())
    tol = TOL_FP32 if dtype == "float32" else TOL_FP64_SAME_INTEGRATOR

    # the conditioning of the field-oriented columns (float32, induction machines): per lane, |psi_r| at the start of the step
    names, wrapped = shell.names, shell.wrapped
    w_rows, w_obs = keep.astype(np.float64), keep.astype(np.float64)
    obs_names = (spec.get("observed") or wrapped) + ([g["state"] + "_ref" for g in shell.generators] if spec.get("observed") else [])
    if spec.get("observer") and dtype == "float32":
        w = np.minimum(1.0, out["psi_r"] / (FLUX_FLOOR * np.maximum(out["psi_r"].max(axis=0), 1e-300)[None, :]))
        w_flux = np.minimum(1.0, out["state"][..., wrapped.index("psi_abs")] / (FLUX_FLOOR * max(float(out["state"][..., wrapped.index("psi_abs")].max()), 1e-300)))
        w_rows = np.repeat(w_rows[..., None], len(wrapped), axis=-1)
        w_obs = np.repeat(w_obs[..., None], len(obs_names), axis=-1)
        for tab, cols in ((w_rows, wrapped), (w_obs, obs_names)):
            for c, n in enumerate(cols):
                if n in ("i_sd", "i_sq", "u_sd", "u_sq"):
                    tab[..., c] *= w
                elif n == "psi_angle":
                    tab[..., c] *= w_flux
    circle_rows = [c for c, n in enumerate(wrapped) if n in ("epsilon", "psi_angle")]
    circle_obs = [c for c, n in enumerate(obs_names) if n in ("epsilon", "psi_angle")]

    got = {k: v.double().cpu().numpy() if v.dtype.is_floating_point else v.cpu().numpy() for k, v in dev.items()}
    e_first = max(_errors(info["first"][k][None], first[s][None], dtype, circle=c) for k, s, c in (("obs", "obs", circle_obs), ("rows", "state", circle_rows), ("refs", "refs", ())))
    errs = dict(reset=e_first,
                state=_errors(got["rows"], out["state"], dtype, w_rows, circle_rows),
                references=_errors(got["refs"], out["refs"], dtype, keep),
                reward=_errors(got["reward"], out["reward"], dtype, keep),
                observation=_errors(got["obs"], out["obs"], dtype, w_obs, circle_obs))
    errs["ret"] = _errors(got["ret"], out["statistics"]["ret"], dtype, keep)
    errs["last_ret"] = _errors(got["last_ret"], out["statistics"]["last_ret"], dtype, keep)
    exact = {k: int(((got[k].astype(np.int64) != (out[k] if k in out else out["statistics"][k]).astype(np.int64)) & keep).sum()) for k in EXACT}
    worst = max(errs.values())
    print(f"| {case} | {dtype} | {worst:.2e} | {share:.4f} | {int(term.sum())} | {int(trunc.sum())} | {decided} |  errors {({k: f'{v:.1e}' for k, v in errs.items()})}, "
          f"mask / counter mismatches {exact}, ref samples on a jump {int(out['ref_on_jump'].sum())}")
    assert share <= MAX_LEFT_OUT and (dtype == "float32" or share == 0.0)
    assert not any(exact.values()), exact
    assert worst <= tol, errs


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_graph_replay_equals_the_eager_run(case, dtype):
    """Device against device, on the run the shell comparison already paid for: K replays of one captured `bind_step` == K x `env.step`."""
    import torch

    import gym_electric_motor_amd as ga

    spec = cases.CASES[case]
    acts = cases.actions(spec)
    eager, _, _ = _device_run(torch, ga, spec, dtype, acts)
    graphed, _, _ = _device_run(torch, ga, spec, dtype, acts, graph=True)
    assert int(eager["terminated"].sum()) > 0 and int(eager["truncated"].sum()) > 0
    for k in eager:
        assert torch.equal(eager[k], graphed[k]), (k, int((eager[k] != graphed[k]).sum()))
