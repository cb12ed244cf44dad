#!/usr/bin/env python3
"""Timing of the device-side profile references on one GPU -> profiles/refprofile.md (written with --write).

  1. microseconds per closed-loop step of the complete Cont-CC-PMSM-v0 env at --envs envs, 64 steps per HIP graph, in the same build and
     process: the profile generator with a shared table, with a table per env, the default Wiener generators, and -- stepped eagerly, it
     cannot be captured -- a ReplayReferenceGenerator;
  2. GB/s of one gemx_refprofile_rollout_shell pass over --rows-envs envs x --rows rows, in algorithmic bytes per row and env: 1 read (the
     done byte) and n_ref * sizeof(R) written, plus n_ref * sizeof(R) read from a per-env table.

Device time between two events on the launching stream, median over --windows windows (an untimed window first).

    python tools/time_refprofile.py [--envs 16384] [--steps 640] [--windows 9] [--rows-envs 1048576] [--rows 64] [--write]
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T_ROWS = 1024  # rows of the timed profiles


def timed(fn, windows, stream=None):
    import torch

    ms = []
    for w in range(windows + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if w:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def generator(variant, n, steps):
    import numpy as np

    import gym_electric_motor_amd as ga

    rng = np.random.default_rng(0)
    if variant == "shared":
        return ga.ProfileReferenceGenerator(rng.uniform(-0.5, 0.5, (T_ROWS, 2)).astype(np.float32), end="wrap")
    if variant == "per_env":
        return ga.ProfileReferenceGenerator(rng.uniform(-0.5, 0.5, (T_ROWS, n, 2)).astype(np.float32), end="wrap", start="random", seed=1)
    if variant == "replay":  # (no wrap there: one row per step of the whole timed run)
        return ga.ReplayReferenceGenerator(rng.uniform(-0.5, 0.5, (steps + 8, 2)).astype(np.float32))
    return "default"


def step_time(variant, n, steps, windows):
    """-> us per step: from a HIP graph of 64 steps, or (replay) from eager steps"""
    import torch

    import gym_electric_motor_amd as ga

    eager = variant == "replay"
    total = (windows + 1) * steps + 8
    env = ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator=generator(variant, n, total), seed=1)
    action = torch.full((n, env.action_space.shape[0]), 0.01, device="cuda")
    stream = torch.cuda.current_stream() if eager else torch.cuda.Stream()
    step, _, reward, done = env.bind_step(action, stream=stream)
    env.reset()
    torch.cuda.synchronize()
    if eager:
        ms = timed(lambda: [step() for _ in range(steps)], windows, stream)
        env.close()
        return ms * 1e3 / steps
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for _ in range(64):
            step()
    reps = max(1, steps // 64)
    with torch.cuda.stream(stream):
        ms = timed(lambda: [graph.replay() for _ in range(reps)], windows, stream)
    env.close()
    return ms * 1e3 / (reps * 64)


class _System:
    """what ProfileReferences.set_modules reads of a physical system"""

    def __init__(self, ps, n):
        import torch

        self.state_positions, self.state_space, self.state_names, self.tau = ps.state_positions, ps.state_space, ps.state_names, ps.tau
        self.n_envs, self.env_base, self.device, self._tdev, self._tdtype = n, 0, ps.device, ps._tdev, torch.float32


def rows_rate(n, K, windows, per_env, reps=5):
    import torch

    import gym_electric_motor_amd as ga

    host = ga.make("Cont-CC-PMSM-v0", n_envs=2)
    rows = 16 if per_env else T_ROWS  # (16 rows x 2^20 envs x 2 columns: 134 MB of table)
    table = torch.rand((rows, n, 2) if per_env else (rows, 2), device="cuda") - 0.5
    gen = ga.ProfileReferences(ga.ProfileReferenceGenerator(table, reference_states=("i_sd", "i_sq"), end="wrap")).set_modules(_System(host.physical_system, n))
    done = (torch.rand((K, n), device="cuda") < 0.01).to(torch.uint8)
    out = torch.empty((K, n, 2), device="cuda")
    launch = gen.bind_rollout_shell(done, out)
    gen.reset()
    ms = timed(lambda: [launch() for _ in range(reps)], windows) / reps
    gb = (1 + 8 + (8 if per_env else 0)) * n * K / 1e9
    gen.close()
    host.close()
    return ms, gb / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=640)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--rows-envs", type=int, default=1 << 20)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--write", action="store_true", help="write profiles/refprofile.md")
    args = ap.parse_args()
    lines = ["# Device-side profile references: step time and rollout bandwidth", "",
             f"Measured with `python tools/time_refprofile.py --write` on one MI355X (fp32, device time between two events on the launching stream, median of "
             f"{args.windows} windows after an untimed window).  Every variant is built and timed in the same process from the same build.", "",
             f"Complete `Cont-CC-PMSM-v0` env, {args.envs} envs, two referenced states, default reward, 64 steps per HIP graph (profiles of {T_ROWS} rows, `end='wrap'`):", "",
             "| reference generator | µs per step |", "|---|---|"]
    labels = (("shared", "ProfileReferenceGenerator, shared table [T, 2], start zero"), ("per_env", "ProfileReferenceGenerator, table per env [T, N, 2], random start rows"),
              ("wiener", "default Wiener generators"), ("replay", "ReplayReferenceGenerator, stepped eagerly through bind_step (it cannot be captured)"))
    us = {}
    for variant, label in labels:
        us[variant] = step_time(variant, args.envs, args.steps, args.windows)
        lines.append(f"| {label} | {us[variant]:.2f} |")
        print(lines[-1], flush=True)
    slower = [v for v in ("shared", "per_env") if us[v] > us["wiener"]]
    lines += ["", "Expectation: the profile generator's graph step is no slower than the Wiener generators' (it does strictly less arithmetic).  "
              + ("Confirmed by the numbers above." if not slower else f"NOT confirmed for: {', '.join(slower)} (numbers above); nothing was tuned past it.")]
    lines += ["", f"`gemx_refprofile_rollout_shell` alone, {args.rows_envs} envs x {args.rows} rows, two fp32 columns, 1 % done bytes (algorithmic bytes per row and env: "
              "1 read + 8 written; + 8 read from a per-env table), against the 6.29 TB/s a float4 copy reaches on this part:", "",
              "| table | ms per pass | GB/s algorithmic | of the copy rate |", "|---|---|---|---|"]
    for per_env, label in ((False, f"shared [{T_ROWS}, 2]"), (True, "per env [16, N, 2]")):
        ms, rate = rows_rate(args.rows_envs, args.rows, args.windows, per_env)
        lines.append(f"| {label} | {ms:.3f} | {rate:.0f} | {rate / 6290 * 100:.0f} % |")
        print(lines[-1], flush=True)
    lines += ["", "Not measured: fp64, interpolating profiles (`profile_tau != tau`), other column counts, other K."]
    if args.write:
        with open(os.path.join(REPO, "profiles", "refprofile.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
