"""One-step finite-control-set model predictive control inside the fused rollout launch, beside uniform random actions on the same env and
seed: mean reward and mean episode length of both.

    python examples/lookahead_rollout.py [--env Finite-CC-PMSM-v0] [--n-envs 4096] [--steps 256] [--max-episode-steps 100] [--temperature 0]

--temperature T > 0 samples the action from softmax(score / T) (Gumbel noise of scale T on the scores) instead of taking the best one."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gym_electric_motor_amd as ga  # noqa: E402


def episode_length(terminated, truncated, max_steps):
    """mean length of the episodes that ended inside the rollout (nan if none did)"""
    ended = (terminated | truncated).bool()
    n_ended = int(ended.sum())
    if n_ended == 0:
        return float("nan")
    # every env starts an episode at row 0: rows per env / episodes ended per env, over the envs that ended at least one
    per_env = ended.sum(dim=0)
    last = torch.where(ended, torch.arange(ended.shape[0], device=ended.device)[:, None] + 1, 0).max(dim=0).values
    return float((last[per_env > 0].float() / per_env[per_env > 0].float()).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Finite-CC-PMSM-v0")
    ap.add_argument("--n-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--max-episode-steps", type=int, default=100)
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    N, K, M = args.n_envs, args.steps, args.max_episode_steps

    def make():
        env = ga.make(args.env, n_envs=N, device=0, reference_generator="default", max_episode_steps=M, seed=args.seed)
        env.reset()
        return env

    env, baseline = make(), make()
    n_actions = env.n_lookahead_actions()
    rng = np.random.default_rng(args.seed)
    noise = None
    if args.temperature > 0:
        gumbel = -np.log(-np.log(rng.uniform(1e-9, 1.0, (K, N, n_actions))))
        noise = torch.as_tensor((args.temperature * gumbel).astype(np.float32), device="cuda:0")
    state, refs, reward, actions, terminated, truncated, scores = env.rollout_lookahead_complete_episodic(K, noise=noise, return_scores=True)
    random_actions = torch.as_tensor(rng.integers(0, n_actions, (K, N)).astype(np.uint8), device="cuda:0")
    _, _, r_reward, r_terminated, r_truncated = baseline.rollout_complete_episodic(random_actions)
    torch.cuda.synchronize()
    print(f"{args.env}: {N} envs x {K} steps, time limit {M}, {n_actions} actions ({env.physical_system.last_launch()})")
    print(f"  lookahead controller   mean reward {float(reward.mean()):+.4f}   terminated {float(terminated.float().mean()):.4f} of rows   "
          f"mean episode length {episode_length(terminated, truncated, M):.1f}")
    print(f"  uniform random actions mean reward {float(r_reward.mean()):+.4f}   terminated {float(r_terminated.float().mean()):.4f} of rows   "
          f"mean episode length {episode_length(r_terminated, r_truncated, M):.1f}")
    print(f"  mean one-step regret of a random action: {float((scores.max(dim=2).values - scores.mean(dim=2)).mean()):.4f}")
    env.close(), baseline.close()


if __name__ == "__main__":
    main()
