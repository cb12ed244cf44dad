#!/usr/bin/env python3
"""Timing of the device-side observation stage on one GPU -> the tables of profiles/obs_stage.md.

  1. microseconds per closed-loop step of the complete Cont-CC-PMSM-v0 env at --envs envs (eager step / bind_step / 64 steps per HIP
     graph), in three variants: without a stage; with the stage (cos / sin of the angle, flat observation); and with the same processing
     written in torch ops on the env without a stage (index_select, cos, sin, cat) -- the baseline the stage exists to beat;
  2. GB/s of one ObservationStage.apply over a [K, N, 14] trajectory, in algorithmic bytes 4 (n_in + n_out) per row.

Device time between two events on the launching stream, median over --windows windows (an untimed window first).

    python tools/time_obs_stage.py [--envs 16384] [--steps 640] [--windows 9] [--traj-steps 1000]
"""
import argparse
import math
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


def loop_times(variant, n, steps, windows):
    """-> {mode: us per step}"""
    import torch

    import gym_electric_motor_amd as ga

    kw = dict(n_envs=n, reference_generator="default", seed=1)
    if variant == "stage":
        kw.update(physical_system_wrappers=(ga.CosSinProcessor(remove_angle=True),), flatten_observation=True)
    out = {}
    for mode in ("eager", "bind_step", "graph64"):
        env = ga.make("Cont-CC-PMSM-v0", **kw)
        ps = env.physical_system
        action = torch.full((n, 3), 0.01, device="cuda")
        eps = ps.state_positions["epsilon"]
        keep = torch.tensor([j for j in range(len(ps.state_names)) if j != eps], device="cuda")
        flat = torch.empty((n, 15 + 2), device="cuda")

        def post(state, ref):  # the stage's work in torch ops
            a = state[:, eps] * math.pi
            torch.cat((state.index_select(1, keep), torch.cos(a)[:, None], torch.sin(a)[:, None], ref), dim=1, out=flat)

        stream = torch.cuda.Stream() if mode == "graph64" else torch.cuda.current_stream()
        if mode == "eager":
            def one():
                obs = env.step(action)[0]
                if variant == "torch":
                    post(*obs)
        else:
            step, obs, _, _ = env.bind_step(action, stream=stream)

            def one():
                step()
                if variant == "torch":
                    post(*obs)
        env.reset()
        torch.cuda.synchronize()
        if mode == "graph64":
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                for _ in range(3):
                    one()
            torch.cuda.current_stream().wait_stream(stream)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                for _ in range(64):
                    one()
            reps = max(1, steps // 64)
            with torch.cuda.stream(stream):
                ms = timed(lambda: [graph.replay() for _ in range(reps)], windows, stream)
            out[mode] = ms * 1e3 / (reps * 64)
        else:
            ms = timed(lambda: [one() for _ in range(steps)], windows)
            out[mode] = ms * 1e3 / steps
        env.close()
    return out


def apply_rate(n, K, windows):
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make("Cont-CC-PMSM-v0", n_envs=n, physical_system_wrappers=(ga.CosSinProcessor(remove_angle=True),))
    st = env.observation_stage
    traj = torch.rand((K, n, st.n_in), device="cuda") * 2 - 1
    out = torch.empty((K, n, st.n_out), device="cuda")
    ms = timed(lambda: st.apply(traj, out=out), windows)
    gb = 4 * (st.n_in + st.n_out) * K * n / 1e9
    env.close()
    return ms, gb / (ms * 1e-3), st.n_in, st.n_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=640)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--traj-steps", type=int, default=1000)
    args = ap.parse_args()
    print(f"| variant | eager us/step | bind_step us/step | 64 steps per graph us/step |  ({args.envs} envs, median of {args.windows} windows of {args.steps} steps)")
    print("|---|---|---|---|")
    for variant, label in (("none", "no stage"), ("stage", "stage: cos/sin + flat"), ("torch", "the same in torch ops")):
        t = loop_times(variant, args.envs, args.steps, args.windows)
        print(f"| {label} | {t['eager']:.2f} | {t['bind_step']:.2f} | {t['graph64']:.2f} |", flush=True)
    ms, rate, n_in, n_out = apply_rate(args.envs, args.traj_steps, args.windows)
    print(f"apply over [{args.traj_steps}, {args.envs}, {n_in}] -> [.., {n_out}]: {ms:.3f} ms, {rate:.0f} GB/s algorithmic")


if __name__ == "__main__":
    main()
