#!/usr/bin/env python3
"""Timing of the policy evaluation pass (gemx_policy_eval_rows) on one GPU -> the "Rates" section of profiles/policy_eval.md (--write).

Per env and shape, from ONE HIP graph each and on the tensors of one policy rollout: (a) the launch `policy.bind_evaluate_rollout` with
the env's learner head (categorical for the finite PMSM, gaussian for the continuous SCIM), (b) the same evaluation as torch ops --
`torch.where` on `ended` between the previous row and the reset row, the concat with the references, three `linear` calls with tanh
between them, and the head -- a baseline to compare against, never a fallback.  A 64 x 64 tanh MLP on the state row and two references.
Medians of --windows alternated windows of graph replays of at least 50 ms each (an untimed window first), device time between two
events.  Beside the rows/s: the ratio, the FMAs and the algorithmic bytes per row, and the fractions of the fp32 vector FMA rate
(157.3 TFLOP/s = 78.65e12 FMA/s) and of the 6.29 TB/s a float4 copy reaches on this part.

    python tools/time_policy_eval.py [--windows 9] [--write]
"""
import argparse
import os
import re
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FMA_RATE, COPY_GBS = 78.65e12, 6290.0
SHAPES = ((256, 16384), (16, 1 << 20))  # rows x envs
ENVS = (("Finite-CC-PMSM-v0", "categorical"), ("Cont-SC-SCIM-v0", "gaussian"))
N_REF = 2


def window(graph, reps):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def capture(make):
    """make(stream) -> the zero-argument function to capture, bound to that stream"""
    import torch

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn = make(side)
        fn()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
    torch.cuda.synchronize()
    return g


def measure(env_id, head, K, N, windows):
    import numpy as np
    import torch
    import torch.nn.functional as F

    import gym_electric_motor_amd as ga

    env = ga.make(env_id, n_envs=N, device=0, max_episode_steps=100)
    env.reset()
    ps = env.physical_system
    S = len(ps.state_names)
    A = int(ps.action_space.n) if head == "categorical" else int(ps.action_space.shape[0])
    rng = np.random.default_rng(0)
    layers = [((rng.uniform(-1, 1, (o, i)) / np.sqrt(i)).astype(np.float32), rng.uniform(-0.1, 0.1, o).astype(np.float32)) for o, i in ((64, S + N_REF), (64, 64), (A, 64))]
    policy = ga.MLPPolicy(layers, activation="tanh")
    dev = ps._tdev
    refs = torch.rand((K, N, N_REF), device=dev) - 0.5
    noise = -torch.log(-torch.log(torch.rand((K, N, A), device=dev))) if head == "categorical" else 0.1 * torch.randn((K, N, A), device=dev)
    obs0 = ps._obs.clone()
    traj, actions, term, trunc = env.rollout_policy_episodic(policy, K, references=refs, noise=noise)
    ended = torch.bitwise_or(term, trunc)
    reset = torch.as_tensor(ps.reset_observation, dtype=torch.float32).to(dev)
    lp, ent = torch.empty((K, N), device=dev), torch.empty((K, N), device=dev)
    kw = dict(obs0=obs0, ended=ended, reset_obs=reset, references=refs, log_prob_out=lp, entropy_out=ent)
    log_std = torch.full((A,), -0.5, device=dev)
    if head == "categorical":
        kw.update(actions=actions)
    else:
        out = policy.evaluate_rollout(traj, obs0=obs0, ended=ended, reset_obs=reset, references=refs)
        pre = (out + noise).contiguous()
        kw.update(pre_squash=pre, log_std=log_std, squash_correction=True)
    W = [(torch.as_tensor(w, device=dev), torch.as_tensor(b, device=dev)) for w, b in layers]
    t_lp, t_ent = torch.empty_like(lp), torch.empty_like(ent)

    def torch_ops():
        prev = torch.cat([obs0[None], traj[:-1]], dim=0)
        gone = torch.cat([torch.zeros_like(ended[:1]), ended[:-1]], dim=0).bool()
        x = torch.cat([torch.where(gone[..., None], reset, prev), refs], dim=2)
        z = F.linear(torch.tanh(F.linear(torch.tanh(F.linear(x, *W[0])), *W[1])), *W[2])
        if head == "categorical":
            logp = torch.log_softmax(z, dim=2)
            t_lp.copy_(logp.gather(2, actions.long()[..., None])[..., 0])
            t_ent.copy_(-(logp.exp() * logp).sum(dim=2))
        else:
            var = torch.exp(2 * log_std)
            g = (-(pre - z) ** 2 / (2 * var) - log_std - 0.9189385332046727).sum(dim=2)
            t_lp.copy_(g - (2 * (0.6931471805599453 - pre - F.softplus(-2 * pre))).sum(dim=2))
            t_ent.copy_((log_std + 1.4189385332046727).sum().expand_as(t_ent))

    graphs = [capture(lambda st: policy.bind_evaluate_rollout(traj, head=head, stream=st, **kw)), capture(lambda st: torch_ops)]
    torch.cuda.synchronize()
    diff = float((t_lp - lp).abs().max())
    reps = [max(1, int(50.0 / max(window(g, 1), 1e-3)) + 1) for g in graphs]
    ms = [[], []]
    for w in range(windows + 1):  # alternated; the first window of each is untimed
        for i, g in enumerate(graphs):
            t = window(g, reps[i])
            if w:
                ms[i].append(t)
    env.close()
    med = [statistics.median(m) for m in ms]
    fma = (S + N_REF) * 64 + 64 * 64 + 64 * ((A + 7) // 8 * 8)
    nbytes = 4 * S + 1 + 4 * N_REF + 8 + (1 if head == "categorical" else 4 * A)
    rows = K * N
    rate = [rows / (m * 1e-3) for m in med]
    return (f"| {env_id} ({head}) | {N} x {K} | {rate[0]:.3e} | {rate[1]:.3e} | {rate[0] / rate[1]:.1f} | {fma} | {nbytes} | {rate[0] * fma / FMA_RATE * 100:.1f} % | "
            f"{rate[0] * nbytes / 1e9 / COPY_GBS * 100:.1f} % | {diff:.1e} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--write", action="store_true", help="replace the Rates section of profiles/policy_eval.md")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "time_policy_eval.py needs a GPU: a timing taken anywhere else says nothing"
    lines = ["## Rates", "",
             f"Measured with `python tools/time_policy_eval.py --write` on one MI355X ({torch.cuda.get_device_name(0)}), everything in one process from one build: the launch and "
             f"the same evaluation as torch ops, one HIP graph each, medians of {args.windows} alternated windows of replays of at least 50 ms after an untimed window.  A 64 x 64 "
             "tanh MLP on the state row and two references, the rows of one policy rollout with a time limit of 100 steps; float32 head outputs.  FMA fraction: of 78.65e12 "
             "FMA/s (157.3 TFLOP/s fp32 vector); bandwidth fraction: algorithmic bytes against the 6.29 TB/s of a float4 copy.  The last column is the largest difference "
             "between the two log-probs (the torch ops compute in float32 with another summation order).", "",
             "| env (head) | envs x rows | rows/s, launch | rows/s, torch ops | ratio | FMAs per row | bytes per row | of the FMA rate | of the copy rate | max log-prob difference |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for env_id, head in ENVS:
        for K, N in SHAPES:
            lines.append(measure(env_id, head, K, N, args.windows))
            print(lines[-1], flush=True)
    lines += ["", "Not measured: the value and none heads, other plans, the float64 output dtype, the pass behind the rollout in one graph."]
    if args.write:
        path = os.path.join(REPO, "profiles", "policy_eval.md")
        text = open(path).read()
        text = re.sub(r"## Rates\n.*\Z", lambda _: "\n".join(lines) + "\n", text, flags=re.S)
        with open(path, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
