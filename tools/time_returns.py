#!/usr/bin/env python3
"""Timing of the device-side returns / GAE pass (gemx_returns_rows) on one GPU -> profiles/returns_pass.md (written with --write).

Per shape ([K, N], fp32 and fp64 rows): microseconds per call of the bound launcher (`ga.bind_advantages`) and algorithmic GB/s, where the
bytes per row and env are sizeof(R) * (2 or 3 read + 1 or 2 written) + 2 -- reward, value (and final_value, counted in full although the
kernel reads it at truncated rows only), advantage and / or returns, the two mask bytes.  Beside it, at the same shape and on the same
tensors, what users do today: a reversed Python loop of torch ops over the rows computing the same advantages and returns in the rows'
dtype (a baseline to compare against, never a fallback), and the 6.29 TB/s a float4 copy reaches on this part.

Device time between two events on the launching stream, median over --windows windows (an untimed window first).

    python tools/time_returns.py [--windows 9] [--torch-windows 3] [--write]
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GAMMA, LAM = 0.99, 0.95
COPY_GBS = 6290.0
SHAPES = ((1000, 16384), (64, 1 << 20))  # the headline rollout's learner batch; many envs, few rows


def timed(fn, windows):
    import torch

    ms = []
    for w in range(windows + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if w:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def torch_loop(reward, value, ended, last_value, advantage, returns):
    """The reversed loop of torch ops: `ended` cuts the recursion and the bootstrap (a truncated row is treated as terminated)."""
    import torch

    K = reward.shape[0]
    cont = 1.0 - ended.to(reward.dtype)
    A = torch.zeros_like(last_value)
    for k in range(K - 1, -1, -1):
        v_next = last_value if k == K - 1 else value[k + 1]
        delta = reward[k] + GAMMA * v_next * cont[k] - value[k]
        A = delta + (GAMMA * LAM) * cont[k] * A
        advantage[k] = A
    torch.add(advantage, value, out=returns)


def measure(K, N, dtype, windows, torch_windows):
    import torch

    import gym_electric_motor_amd as ga

    gen = torch.Generator(device="cuda").manual_seed(1)
    reward, value, final_value = (torch.randn((K, N), generator=gen, device="cuda", dtype=dtype) for _ in range(3))
    last_value = torch.randn(N, generator=gen, device="cuda", dtype=dtype)
    u = torch.rand((K, N), generator=gen, device="cuda")
    ended = (u < 0.01).to(torch.uint8)  # 1 % of the rows end an episode, a quarter of them by truncation
    terminated = (u < 0.0075).to(torch.uint8)
    advantage, returns = torch.empty_like(reward), torch.empty_like(reward)
    size = reward.element_size()
    rows = []
    variants = (("advantage and returns", dict(advantage_out=advantage, return_out=returns), 2, 2), ("advantage alone", dict(advantage_out=advantage), 2, 1),
                ("advantage and returns, with final_value", dict(advantage_out=advantage, return_out=returns, final_value=final_value), 3, 2))
    reps = 5
    for label, kw, n_read, n_written in variants:
        launch = ga.bind_advantages(reward, value, terminated, gamma=GAMMA, lam=LAM, last_value=last_value, ended=ended, **kw)
        ms = timed(lambda: [launch() for _ in range(reps)], windows) / reps
        gb = (size * (n_read + n_written) + 2) * K * N / 1e9
        rows.append((label, ms * 1e3, gb / (ms * 1e-3)))
    # the torch loop on the same tensors (terminated = ended there: no final_value), and how far its results are from the kernel's
    ga.bind_advantages(reward, value, ended, gamma=GAMMA, lam=LAM, last_value=last_value, advantage_out=advantage, return_out=returns)()
    a_t, r_t = torch.empty_like(reward), torch.empty_like(reward)
    ms = timed(lambda: torch_loop(reward, value, ended, last_value, a_t, r_t), torch_windows)
    torch.cuda.synchronize()
    diff = float((a_t - advantage).abs().max())
    gb = (size * 4 + 2) * K * N / 1e9
    rows.append((f"reversed loop of torch ops (advantage and returns; largest difference of an advantage to the kernel's {diff:.1e})", ms * 1e3, gb / (ms * 1e-3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--torch-windows", type=int, default=3)
    ap.add_argument("--write", action="store_true", help="write profiles/returns_pass.md")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "time_returns.py needs a GPU: a timing taken anywhere else says nothing"
    lines = ["# Device-side returns / GAE pass: time per call and algorithmic bandwidth", "",
             f"Measured with `python tools/time_returns.py --write` on one MI355X ({torch.cuda.get_device_name(0)}): device time between two events on the launching "
             f"stream, median of {args.windows} windows of 5 calls after an untimed window ({args.torch_windows} windows of one pass for the torch loop).  "
             "Everything is timed in one process from one build.  Algorithmic bytes per row and env: sizeof(R) x (2 or 3 read + 1 or 2 written) + 2 mask bytes; "
             "`final_value` is counted in full although the kernel reads it at truncated rows only.  1 % of the rows end an episode, a quarter of those by "
             f"truncation; gamma {GAMMA}, lambda {LAM}.  Copy rate for comparison: 6.29 TB/s (a float4 copy on this part)."]
    for K, N in SHAPES:
        for dtype in (torch.float32, torch.float64):
            lines += ["", f"{N} envs x {K} rows, {str(dtype).split('.')[1]}:", "", "| pass | µs per call | GB/s algorithmic | of the copy rate |", "|---|---|---|---|"]
            for label, us, rate in measure(K, N, dtype, args.windows, args.torch_windows):
                lines.append(f"| {label} | {us:.1f} | {rate:.0f} | {rate / COPY_GBS * 100:.1f} % |")
                print(lines[-1], flush=True)
    lines += ["", "The torch loop is several launches per row in the rows' dtype (its accumulator included); the kernel is one launch with a float64 accumulator.  "
              "At 16384 envs the grid is 64 workgroups of 256 lanes, so at most 64 of the 256 CUs take part, each lane with GROUP_ROWS = 16 rows in flight; "
              "at 2^20 envs it is 4096 workgroups.  Why the smaller grid stays this far below the larger one's rate, and float32 below float64 there, has not "
              "been profiled.", "", "Not measured: the pass inside a HIP graph behind `bind_rollout_complete`, other K, other GROUP_ROWS, `discounted_returns`."]
    if args.write:
        with open(os.path.join(REPO, "profiles", "returns_pass.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
