#!/usr/bin/env python3
"""Timing of the device-side episode stage on one GPU -> profiles/episode_stage.md (written with --write).

  1. microseconds per closed-loop step of the complete Cont-CC-PMSM-v0 env at --envs envs, 64 steps per HIP graph, in the same build and
     process: without the stage (what the parent commit's env launches), with `max_episode_steps` + `episode_statistics`, and without the
     stage but with the counters kept by torch ops on [N] tensors behind every step -- what the stage replaces (no masked reset there: the
     torch loop only counts);
  2. GB/s of one gemx_episode_rows pass over --rows-envs envs x --rows rows, in algorithmic bytes per row and env: sizeof(R) + 1 read,
     1 written (`ended`), plus 8 + 4 for the optional finished_return / finished_length outputs.

Device time between two events on the launching stream, median over --windows windows (an untimed window first).

    python tools/time_episode_stage.py [--envs 16384] [--steps 640] [--windows 9] [--rows-envs 1048576] [--rows 64] [--write]
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


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


def graph_time(variant, n, steps, windows, limit):
    """-> us per step from a HIP graph of 64 steps"""
    import torch

    import gym_electric_motor_amd as ga

    kw = dict(max_episode_steps=limit, episode_statistics=True) if variant == "stage" else {}
    env = ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator="default", seed=1, **kw)
    action = torch.full((n, env.action_space.shape[0]), 0.01, device="cuda")
    stream = torch.cuda.Stream()
    step, _, reward, done = env.bind_step(action, stream=stream)
    if variant == "torch":  # the counters a user keeps by hand today, behind every step
        length, ret = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
        last_length, last_ret, n_finished = torch.zeros_like(length), torch.zeros_like(ret), torch.zeros_like(length)
        physics = step

        def step():
            physics()
            length.add_(1)
            ret.add_(reward)
            ended = (done != 0) | (length >= limit)
            torch.where(ended, length, last_length, out=last_length)
            torch.where(ended, ret, last_ret, out=last_ret)
            n_finished.add_(ended)
            length.masked_fill_(ended, 0)
            ret.masked_fill_(ended, 0.0)

    env.reset()
    torch.cuda.synchronize()
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


def rows_rate(n, K, windows, optional, reps=5):
    import torch

    import gym_electric_motor_amd as ga

    stage = ga.EpisodeStage(1000, statistics=True, has_reward=True).create(n, 0, "float32")
    done = (torch.rand((K, n), device="cuda") < 0.01).to(torch.uint8)
    reward = torch.rand((K, n), device="cuda")
    ended = torch.empty_like(done)
    fin_ret = torch.empty((K, n), dtype=torch.float64, device="cuda") if optional else None
    fin_len = torch.empty((K, n), dtype=torch.int32, device="cuda") if optional else None
    launch = stage.bind_rows(done, reward, ended, fin_ret, fin_len)
    ms = timed(lambda: [launch() for _ in range(reps)], windows) / reps
    gb = (4 + 1 + 1 + (12 if optional else 0)) * n * K / 1e9
    stage.close()
    return ms, gb / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=640)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--limit", type=int, default=1000)
    ap.add_argument("--rows-envs", type=int, default=1 << 20)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--write", action="store_true", help="write profiles/episode_stage.md")
    args = ap.parse_args()
    lines = ["# Device-side episode stage: step time and rows-pass bandwidth", "",
             f"Measured with `python tools/time_episode_stage.py --write` on one MI355X (fp32, device time between two events on the launching stream, median of "
             f"{args.windows} windows after an untimed window).  Every variant is built and timed in the same process from the same build.", "",
             f"Complete `Cont-CC-PMSM-v0` env, {args.envs} envs, default Wiener references and reward, 64 steps per HIP graph, `max_episode_steps={args.limit}`:", "",
             "| variant | µs per step |", "|---|---|"]
    labels = (("none", "no stage (the env as the parent commit builds it)"), ("stage", "max_episode_steps + episode_statistics (masked reset + stage: two launches more)"),
              ("torch", "no stage, the counters kept by torch ops on [N] tensors behind every step"))
    for variant, label in labels:
        lines.append(f"| {label} | {graph_time(variant, args.envs, args.steps, args.windows, args.limit):.2f} |")
        print(lines[-1], flush=True)
    lines += ["", f"`gemx_episode_rows` alone, {args.rows_envs} envs x {args.rows} rows, fp32 rewards (algorithmic bytes per row and env: 4 + 1 read, 1 written; "
              "+ 8 + 4 with finished_return and finished_length), against the 6.29 TB/s a float4 copy reaches on this part:", "",
              "| outputs | ms per pass | GB/s algorithmic | of the copy rate |", "|---|---|---|---|"]
    for optional, label in ((False, "ended"), (True, "ended, finished_return, finished_length")):
        ms, rate = rows_rate(args.rows_envs, args.rows, args.windows, optional)
        lines.append(f"| {label} | {ms:.3f} | {rate:.0f} | {rate / 6290 * 100:.0f} % |")
        print(lines[-1], flush=True)
    lines += ["", "The pass moves single bytes per lane for `done` and `ended` (a wave reads 64 bytes of a row), which is why it stays below the copy rate; "
              "several envs per lane would widen those accesses and has not been tried.", "", "Not measured: fp64 rewards, other K, the eager (not graphed) loop."]
    if args.write:
        with open(os.path.join(REPO, "profiles", "episode_stage.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
