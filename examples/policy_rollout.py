"""A tanh MLP current controller acting inside the fused launch: 256 control steps of 4096 PMSM envs, one physics launch.
--complete: the same on the complete env -- its own reference generators are stepped inside that launch and the reward pass follows, so
the results are what a learner collects: state, references, reward, actions, terminated, truncated -> ga.advantages."""
import sys

import numpy as np
import torch

import gym_electric_motor_amd as ga

N, K, M = 4096, 256, 100
complete = "--complete" in sys.argv[1:]
env = ga.make("Finite-CC-PMSM-v0", n_envs=N, device=0, max_episode_steps=M, **(dict(reference_generator="default") if complete else {}))
env.reset()
n_state, n_actions = len(env.physical_system.state_names), int(env.physical_system.action_space.n)
rng = np.random.default_rng(0)


def layer(n_out, n_in):
    return (rng.uniform(-1, 1, (n_out, n_in)) / np.sqrt(n_in)).astype(np.float32), np.zeros(n_out, np.float32)


policy = ga.MLPPolicy([layer(64, n_state + 2), layer(64, 64), layer(n_actions, 64)], activation="tanh")  # (the state row and i_sd*, i_sq*)
gumbel = -torch.log(-torch.log(torch.rand((K, N, n_actions), device="cuda:0")))  # categorical sampling
if complete:
    state, refs, reward, actions, terminated, truncated = env.rollout_policy_complete_episodic(policy, K, noise=gumbel)
    torch.cuda.synchronize()
    print(state.shape, refs.shape, actions.shape, "mean reward", float(reward.mean()), int(truncated.sum()), "truncations", env.physical_system.last_launch())
else:
    references = torch.zeros((K, N, 2), device="cuda:0")  # i_sd*, i_sq*
    traj, actions, terminated, truncated = env.rollout_policy_episodic(policy, K, references=references, noise=gumbel)
    torch.cuda.synchronize()
    print(traj.shape, actions.shape, int(truncated.sum()), "truncations", env.physical_system.last_launch() if hasattr(env.physical_system, "last_launch") else "")
env.close()
