#!/usr/bin/env python3
"""Timing of the device-side StateNoiseProcessor on one GPU -> the tables of profiles/state_noise.md.

  1. microseconds per closed-loop step of the complete Cont-CC-PMSM-v0 env at --envs envs (bind_step, eager and 64 steps per HIP graph)
     with StateNoiseProcessor(i_sd, i_sq) (four launches: masked reset, physics, noise + done + reward, generators) against the same env
     without the wrapper (two launches: physics with fused constraints and reward, generators) in the same build;
  2. GB/s of one gemx_noise_step pass over [N, 14] rows, in algorithmic bytes 4 (2 n_in + n_ref + 1) + 1 per row.

Device time between two events on the launching stream, median over --windows windows (an untimed window first).

    python tools/time_state_noise.py [--envs 16384] [--steps 640] [--windows 9] [--stage-envs 1048576]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def _wrappers(ga, variant):
    return (ga.StateNoiseProcessor(["i_sd", "i_sq"], "normal", dict(scale=0.01)),) if variant == "noise" else ()


def loop_times(variant, n, steps, windows):
    """-> {mode: us per step}"""
    import torch

    import gym_electric_motor_amd as ga

    out = {}
    for mode in ("bind_step", "graph64"):
        env = ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator="default", seed=1, physical_system_wrappers=_wrappers(ga, variant))
        action = torch.full((n, env.action_space.shape[0]), 0.01, device="cuda")
        stream = torch.cuda.Stream() if mode == "graph64" else torch.cuda.current_stream()
        step, _, _, _ = env.bind_step(action, stream=stream)
        env.reset()
        torch.cuda.synchronize()
        if mode == "graph64":
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
            out[mode] = ms * 1e3 / (reps * 64)
        else:
            ms = timed(lambda: [step() for _ in range(steps)], windows)
            out[mode] = ms * 1e3 / steps
        env.close()
    return out


def stage_rate(n, windows, reps=20):
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator="default", physical_system_wrappers=_wrappers(ga, "noise"))
    stage = env.state_noise
    rows = torch.rand((n, stage.n_in), device="cuda") * 0.2 - 0.1
    refs = torch.rand((n, stage.n_ref), device="cuda") * 0.2 - 0.1
    out, done, reward = torch.empty_like(rows), torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, device="cuda")
    launch = stage.bind_step(rows, refs, out, done, reward)
    ms = timed(lambda: [launch() for _ in range(reps)], windows) / reps
    gb = (4 * (2 * stage.n_in + stage.n_ref + 1) + 1) * n / 1e9
    env.close()
    return ms, gb / (ms * 1e-3), stage.n_in


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=640)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--stage-envs", type=int, default=1 << 20)
    args = ap.parse_args()
    print(f"| variant | bind_step us/step | 64 steps per graph us/step |  ({args.envs} envs, median of {args.windows} windows of {args.steps} steps)")
    print("|---|---|---|")
    for variant, label in (("none", "no wrapper"), ("noise", "StateNoiseProcessor(i_sd, i_sq)")):
        t = loop_times(variant, args.envs, args.steps, args.windows)
        print(f"| {label} | {t['bind_step']:.2f} | {t['graph64']:.2f} |", flush=True)
    for n in (args.envs, args.stage_envs):
        ms, rate, n_in = stage_rate(n, args.windows)
        print(f"gemx_noise_step over [{n}, {n_in}] rows (2 noisy columns, done, reward): {ms * 1e3:.2f} us, {rate:.0f} GB/s algorithmic", flush=True)


if __name__ == "__main__":
    main()
