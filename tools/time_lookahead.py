"""Time the lookahead rollout (`bind_rollout_lookahead_complete_episodic`, csrc/gemx_lookahead.hip) against the two launches of the complete
env that write the same tensors: `bind_rollout_complete_episodic` with given (uniform random) actions, and
`bind_rollout_policy_complete_episodic` with a 64 x 64 tanh MLP.  Every launch is replayed from one HIP graph of its own.
Finite-CC-PMSM-v0 and Finite-SC-SCIM-v0 at 16384 and 2^20 envs, K = 256, M = 100, reference_generator='default'; medians of 9 alternated
windows of at least 50 ms, the spread (min .. max of the windows) beside each.  Prints the markdown table of profiles/lookahead_rollout.md.
The three envs of a row share their output tensors (nothing reads them)."""
import statistics
import time

import numpy as np
import torch

import gym_electric_motor_amd as ga

K, M, WINDOWS, MIN_WINDOW = 256, 100, 9, 0.05
DEV = "cuda:0"


def layers_for(n_in, n_out, rng):
    plan, out, fan = (64, 64, n_out), [], n_in
    for w in plan:
        out.append(((rng.uniform(-1, 1, (w, fan)) / np.sqrt(fan)).astype(np.float32), np.zeros(w, np.float32)))
        fan = w
    return out


def window(replay):
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        replay()
        n += 1
        if n % 4 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= MIN_WINDOW:
                break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def capture(fn):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn(side)()  # (outside the capture: loads the unit, builds the one-step map)
        side.synchronize()
        launch = fn(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    return g.replay


def rate(samples, n_steps):
    """-> (median, slowest, fastest) in G env-steps/s"""
    return tuple(n_steps / t / 1e9 for t in (statistics.median(samples), max(samples), min(samples)))


def main():
    print("| env | envs | actions | lookahead G env-steps/s (min .. max) | given actions G env-steps/s (min .. max) | 64 x 64 MLP policy G env-steps/s (min .. max) | "
          "lookahead / given | lookahead x actions / given | lookahead / policy |\n|---|---|---|---|---|---|---|---|---|")
    for env_id in ("Finite-CC-PMSM-v0", "Finite-SC-SCIM-v0"):
        for N in (16384, 2 ** 20):
            rng = np.random.default_rng(0)
            envs = [ga.make(env_id, n_envs=N, device=0, max_episode_steps=M, reference_generator="default") for _ in range(3)]
            for env in envs:
                env.reset()
            look, given, pol = envs
            ns, n_ref, na = len(look.physical_system.state_names), len(look.reference_names), look.n_lookahead_actions()
            policy = ga.MLPPolicy(layers_for(ns + n_ref, na, rng), activation="tanh")
            state, refs, reward = torch.empty((K, N, ns), device=DEV), torch.empty((K, N, n_ref), device=DEV), torch.empty((K, N), device=DEV)
            acts, term, trunc = (torch.empty((K, N), dtype=torch.uint8, device=DEV) for _ in range(3))
            random_actions = torch.as_tensor(rng.integers(0, na, (K, N)).astype(np.uint8), device=DEV)
            replays = [capture(lambda st: look.bind_rollout_lookahead_complete_episodic(K, state, refs, reward, acts, term, trunc, stream=st)),
                       capture(lambda st: given.bind_rollout_complete_episodic(random_actions, state, refs, reward, term, trunc, stream=st)),
                       capture(lambda st: pol.bind_rollout_policy_complete_episodic(policy, K, state, refs, reward, acts, term, trunc, stream=st))]
            samples = [[], [], []]
            for _ in range(WINDOWS):  # alternated: every window of one launch stands between windows of the others
                for s, replay in zip(samples, replays):
                    s.append(window(replay))
            (la, la_lo, la_hi), (gv, gv_lo, gv_hi), (pl, pl_lo, pl_hi) = (rate(s, K * N) for s in samples)
            print(f"| {env_id} | {N} | {na} | {la:.3f} ({la_lo:.3f} .. {la_hi:.3f}) | {gv:.3f} ({gv_lo:.3f} .. {gv_hi:.3f}) | {pl:.3f} ({pl_lo:.3f} .. {pl_hi:.3f}) | "
                  f"{la / gv:.3f} | {la * na / gv:.2f} | {la / pl:.2f} |", flush=True)
            for env in envs:
                env.close()
            del state, refs, reward, acts, term, trunc, random_actions, replays
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
