"""Time the policy rollout against K bound step()s with the same MLP as torch ops, both replayed from one HIP graph.
Finite-CC-PMSM-v0 and Cont-SC-SCIM-v0 at 16384 and 2^20 envs, K = 256, M = 100, medians of 9 alternated windows of at least 50 ms.
Prints a markdown table for profiles/policy_rollout.md.
--complete: the complete env (reference_generator='default'): the bound `rollout_policy_complete_episodic` launch -- generators in the lane,
reward pass behind it -- against K bound complete step()s with the same MLP on [state, references] as torch ops; the table of
profiles/policy_complete_rollout.md."""
import statistics
import sys
import time

import numpy as np
import torch

import gym_electric_motor_amd as ga

K, M, WINDOWS, MIN_WINDOW = 256, 100, 9, 0.05
COMPLETE = "--complete" in sys.argv[1:]
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
        fn(side)()
        side.synchronize()
        launch = fn(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    return g.replay


def main():
    print("| env | envs | complete policy rollout G env-steps/s | K bound complete step()s + torch MLP G env-steps/s | ratio |\n|---|---|---|---|---|" if COMPLETE else
          "| env | envs | policy rollout G env-steps/s | K bound step()s + torch MLP G env-steps/s | ratio |\n|---|---|---|---|---|")
    for env_id in ("Finite-CC-PMSM-v0", "Cont-SC-SCIM-v0"):
        for N in (16384, 2 ** 20):
            rng = np.random.default_rng(0)
            kw = dict(reference_generator="default") if COMPLETE else {}
            env, ref = ga.make(env_id, n_envs=N, device=0, max_episode_steps=M, **kw), ga.make(env_id, n_envs=N, device=0, max_episode_steps=M, **kw)
            env.reset(), ref.reset()
            ps = env.physical_system
            ns = len(ps.state_names)
            discrete = hasattr(ps.action_space, "n")
            n_out = int(ps.action_space.n) if discrete else int(ps.action_space.shape[0])
            n_ref = len(env.reference_names) if COMPLETE else 0
            layers = layers_for(ns + n_ref, n_out, rng)
            policy = ga.MLPPolicy(layers, activation="tanh")
            traj = torch.empty((K, N, ns), device=DEV)
            acts = torch.empty((K, N), dtype=torch.uint8, device=DEV) if discrete else torch.empty((K, N, n_out), device=DEV)
            term, trunc = torch.empty((K, N), dtype=torch.uint8, device=DEV), torch.empty((K, N), dtype=torch.uint8, device=DEV)
            if COMPLETE:
                refs, reward = torch.empty((K, N, n_ref), device=DEV), torch.empty((K, N), device=DEV)
                fused = capture(lambda st: env.bind_rollout_policy_complete_episodic(policy, K, traj, refs, reward, acts, term, trunc, stream=st))
            else:
                fused = capture(lambda st: env.bind_rollout_policy_episodic(policy, K, traj, acts, term, trunc, stream=st))
            tl = [(torch.as_tensor(W, device=DEV).t().contiguous(), torch.as_tensor(b, device=DEV)) for W, b in layers]
            act1 = torch.empty((N,), dtype=torch.uint8, device=DEV) if discrete else torch.empty((N, n_out), device=DEV)

            def stepped(st):
                if COMPLETE:  # (state [N, S], references [N, n_ref]): the observation the complete step() hands out
                    step, shown = ref.bind_step(act1, stream=st)[:2]
                else:
                    step = ref.bind_step(act1, stream=st)
                    obs = ref.physical_system._obs

                def run():
                    for _ in range(K):
                        h = torch.cat(shown, dim=1) if COMPLETE else obs
                        for i, (W, b) in enumerate(tl):
                            h = torch.addmm(b, h, W)
                            if i + 1 < len(tl):
                                h = torch.tanh(h)
                        act1.copy_(h.argmax(1).to(torch.uint8) if discrete else torch.tanh(h))
                        step()
                return run

            loop = capture(stepped)
            a, b = [], []
            for _ in range(WINDOWS):
                a.append(window(fused))
                b.append(window(loop))
            ra, rb = K * N / statistics.median(a) / 1e9, K * N / statistics.median(b) / 1e9
            print(f"| {env_id} | {N} | {ra:.2f} | {rb:.2f} | {ra / rb:.2f} |", flush=True)
            env.close(), ref.close()


if __name__ == "__main__":
    main()
