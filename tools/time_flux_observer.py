#!/usr/bin/env python3
"""Timing of the device-side flux observer on one GPU -> the tables of profiles/flux_observer.md.

  1. microseconds per closed-loop step of the complete Cont-CC-SCIM-v0 env at --envs envs (bind_step, eager and 64 steps per HIP graph),
     with FluxObserver + FluxOrientedDqToAbcActionProcessor (four launches: dq -> abc actions, physics, observer, generators) against the
     same env without the wrappers in the same build;
  2. GB/s of one gemx_fluxobs_rows pass over a [K, N, 14] trajectory, in algorithmic bytes 4 (2 n_in + 2) + 1 per row.

Device time between two events on the launching stream, median over --windows windows (an untimed window first).

    python tools/time_flux_observer.py [--envs 16384] [--steps 640] [--windows 9] [--traj-steps 1000]
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
    return (ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor("SCIM")) if variant == "flux" else ()


def loop_times(variant, n, steps, windows):
    """-> {mode: us per step}"""
    import torch

    import gym_electric_motor_amd as ga

    out = {}
    for mode in ("bind_step", "graph64"):
        env = ga.make("Cont-CC-SCIM-v0", n_envs=n, reference_generator="default", seed=1, physical_system_wrappers=_wrappers(ga, variant))
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


def rows_rate(n, K, windows):
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make("Cont-CC-SCIM-v0", n_envs=n, physical_system_wrappers=(ga.FluxObserver(),))
    flux = env.flux
    traj = torch.rand((K, n, flux.n_in), device="cuda") * 2 - 1
    done = torch.zeros((K, n), dtype=torch.uint8, device="cuda")
    out = torch.empty((K, n, flux.n_in + 2), device="cuda")
    launch = flux.bind_rows(traj, done, out)
    ms = timed(launch, windows)
    gb = (4 * (2 * flux.n_in + 2) + 1) * K * n / 1e9
    env.close()
    return ms, gb / (ms * 1e-3), flux.n_in


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=640)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--traj-steps", type=int, default=1000)
    args = ap.parse_args()
    print(f"| variant | bind_step us/step | 64 steps per graph us/step |  ({args.envs} envs, median of {args.windows} windows of {args.steps} steps)")
    print("|---|---|---|")
    for variant, label in (("none", "no wrappers"), ("flux", "FluxObserver + flux-oriented dq actions")):
        t = loop_times(variant, args.envs, args.steps, args.windows)
        print(f"| {label} | {t['bind_step']:.2f} | {t['graph64']:.2f} |", flush=True)
    ms, rate, n_in = rows_rate(args.envs, args.traj_steps, args.windows)
    print(f"gemx_fluxobs_rows over [{args.traj_steps}, {args.envs}, {n_in}] -> [.., {n_in + 2}]: {ms:.3f} ms, {rate:.0f} GB/s algorithmic")


if __name__ == "__main__":
    main()
