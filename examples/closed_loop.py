#!/usr/bin/env python3
"""Closed-loop use of the batched stepper: N current-controlled PMSM drives, device-side Wiener references, fused reward, a
trivial proportional dq controller as the "policy" -- everything stays on the GPU.

    python examples/closed_loop.py [--envs 16384] [--steps 2000]                        # generator and reward wired by hand
    python examples/closed_loop.py --complete [--bind | --graph 64]                     # the same loop through the complete env
    python examples/closed_loop.py --complete --graph 64 --reference step               # ... on step (sinusoidal, ...) profiles
    python examples/closed_loop.py --complete --graph 64 --reference profile            # ... on a given two-column cycle, periodic, per env
    python examples/closed_loop.py --complete --rollout 500                             # open loop: (state, reference, reward, done) datasets
    python examples/closed_loop.py --complete --rollout 500 --gae                       # ... and GAE advantages of each dataset, one launch
    python examples/closed_loop.py --complete --graph 64 --time-limit 500               # episodes of 500 steps, counted on the device
    python examples/closed_loop.py --complete --rollout 256 --max-episode-steps 100     # the time limit INSIDE the fused rollout, then GAE

Hand-wired (the baseline to time against): the physics launch with the fused reward, then a generator reset and a generator rollout of one
step per control step.  `--complete`: `ga.make(..., reference_generator="default")` does the wiring -- two launches per control step (physics +
reward, then the fused generator step), `--bind` with everything resolved once (`env.bind_step`), `--graph S` with S control steps per HIP graph.
`--complete --rollout K`: no policy in the loop -- random actions generated on the device, K control steps per `rollout_complete_synthetic`
call (physics rollout, generator rollout in the shell's order, reward pass: three launches per K steps), i.e. the dataset a closed loop
of K `step()`s on the same actions would have produced, bit for bit.
`--complete --rollout K --gae`: a value head beside the policy (the negative tracking error, scaled to the horizon of the discount) and
`ga.bind_advantages` on each dataset's reward and done rows: advantages and returns [K, N] in one more launch per K steps.
`--complete --time-limit M`: `make(..., max_episode_steps=M, episode_statistics=True)` -- an env is truncated after M steps and restarts in
front of its next step; the mean return and length of the finished episodes come from the device counters (`env.episode_statistics()`).
`--complete --rollout K --max-episode-steps M`: what a learner on time-limited episodes runs per K steps, all on the device -- the episodic
rollout (`bind_rollout_complete_episodic`: the time limit inside the fused launch; terminated and truncated rows), the episode statistics,
and `ga.advantages(..., ended=terminated | truncated, final_value=...)`, which cuts the recursion where an episode ended and bootstraps a
truncated one from the value of its final observation.  Works with `--env-parameters` (domain randomisation) too.

The same loop with the reference package is `env.step(policy(obs))` on ONE env per Python call (reference: core.py:329-372).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# --reference KIND -> the holder class of the reference's generator of that kind ('wiener': the env id's default generators)
REFERENCES = dict(wiener=None, sinusoidal="SinusoidalReferenceGenerator", step="StepReferenceGenerator", triangular="TriangularReferenceGenerator",
                  sawtooth="SawtoothReferenceGenerator", laplace="LaplaceProcessReferenceGenerator", constant="ConstReferenceGenerator",
                  profile="ProfileReferenceGenerator")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--complete", action="store_true", help="run the loop through the complete env of make(..., reference_generator='default')")
    ap.add_argument("--bind", action="store_true", help="--complete: the pre-bound stepper (env.bind_step)")
    ap.add_argument("--graph", type=int, default=0, metavar="S", help="--complete: S control steps per HIP graph")
    ap.add_argument("--reference", default="wiener", metavar="KIND", choices=sorted(REFERENCES),
                    help="--complete: the kind of the i_sd / i_sq reference generators: " + ", ".join(sorted(REFERENCES)))
    ap.add_argument("--flat", action="store_true", help="--complete: the device-side observation stage hands the policy ONE flat tensor "
                                                        "(i_sd, i_sq, cos(epsilon), sin(epsilon), reference i_sd, reference i_sq)")
    ap.add_argument("--rollout", type=int, default=0, metavar="K", help="--complete: open-loop datasets, K control steps per rollout_complete_synthetic call")
    ap.add_argument("--gae", action="store_true", help="--complete --rollout K: GAE(0.99, 0.95) advantages of every dataset (ga.bind_advantages, one launch)")
    ap.add_argument("--time-limit", type=int, default=0, metavar="M", help="--complete: episodes of at most M steps (max_episode_steps) and the device-side "
                                                                            "episode statistics")
    ap.add_argument("--max-episode-steps", type=int, default=0, metavar="M", dest="max_episode_steps",
                    help="--complete --rollout K: episodes of at most M steps with the time limit inside the fused rollout (rollout_complete_episodic), "
                         "ending in ga.advantages(..., ended=terminated | truncated)")
    ap.add_argument("--env-parameters", type=float, default=0.0, metavar="SPREAD", dest="env_parameters",
                    help="domain randomisation: every env gets its own r_s, l_d, l_q and J_load, uniform within +-SPREAD (relative) of the motor's, from a seeded numpy Generator")
    args = ap.parse_args()
    if args.max_episode_steps and (not args.rollout or args.time_limit or args.gae):
        ap.error("--max-episode-steps needs --complete --rollout K (and neither --time-limit nor --gae: it runs its own advantages)")
    if args.env_parameters and args.rollout and not args.max_episode_steps:
        ap.error("--env-parameters: the synthetic-action rollouts are not available with per-env parameters")
    if args.time_limit and (not args.complete or args.rollout):  # (--max-episode-steps: the episodic rollout)
        ap.error("--time-limit needs --complete (and no --rollout: with --rollout K the time limit goes inside the fused launch, --max-episode-steps M)")
    if args.rollout and (not args.complete or args.bind or args.graph):
        ap.error("--rollout needs --complete (and neither --bind nor --graph)")
    if args.gae and not args.rollout:
        ap.error("--gae needs --complete --rollout K")
    if args.reference != "wiener" and not args.complete:
        ap.error("--reference needs --complete")
    if args.flat and not args.complete:
        ap.error("--flat needs --complete")
    if args.complete:
        return complete(args)
    import torch

    import gym_electric_motor_amd as ga

    n = args.envs
    # Cont-CC-PMSM-v0 with (u_d, u_q) actions: the reference's DqToAbcActionProcessor folded into the kernel
    env = ga.make("Cont-CC-PMSM-v0", n_envs=n, ode_solver=ga.RK4Solver(), physical_system_wrappers=(ga.DqToAbcActionProcessor.make("PMSM"),),
                  **env_parameter_kw(args, ga))
    ps = env.physical_system
    gen = ga.BatchedWienerProcessReferenceGenerator(reference_states=("i_sd", "i_sq"), seed=1).set_modules(ps)
    ps.set_reward(reward_weights=dict(i_sd=0.5, i_sq=0.5), referenced_states=gen.reference_names)
    isd, isq = ps.state_positions["i_sd"], ps.state_positions["i_sq"]
    obs, _ = env.reset()
    gen.reset()
    ref = gen.rollout(1)[0]  # the reference the agent sees before acting
    ret = torch.zeros(n, device="cuda")
    n_done = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        err = ref - obs[:, [isd, isq]]
        action = (8.0 * err).clamp(-1, 1)                    # "policy": proportional current controller in dq
        obs, reward, terminated, _, _ = env.step(action, references=ref)
        ret += reward
        n_done += int(terminated.sum()) if k % 200 == 199 else 0
        gen.apply_done(terminated)                           # terminated envs get a fresh reference process (auto-reset envs)
        ref = gen.rollout(1)[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"hand-wired: {n} envs x {args.steps} closed-loop steps in {dt:.3f} s = {n * args.steps / dt / 1e6:.1f} M env-steps/s ({dt / args.steps * 1e6:.1f} us/step); "
          f"mean return {float(ret.mean()):.2f}; kernel: {ps.last_launch().split(' grid')[0]}")
    assert torch.isfinite(ret).all()
    env.close()
    gen.close()


def env_parameter_kw(args, ga):
    """make() keywords of --env-parameters SPREAD: +-SPREAD relative uniform spread on the resistances, inductances and J_load."""
    if not args.env_parameters:
        return dict()
    import numpy as np

    rng = np.random.default_rng(7)
    own = ga.make("Cont-CC-PMSM-v0", n_envs=1, _defer_create=True).physical_system  # (host side only: the env's own motor and load)
    mp, j_load = own.electrical_motor.motor_parameter, float(own.mechanical_load._j_load)  # (the ConstantSpeedLoad's J_load is 0: the speed is held)
    spread = lambda v: v * rng.uniform(1.0 - args.env_parameters, 1.0 + args.env_parameters, args.envs)  # noqa: E731
    return dict(env_parameters=ga.EnvParameters(motor={k: spread(mp[k]) for k in ("r_s", "l_d", "l_q")}, load={"j_load": spread(j_load)}))


def complete(args):
    import torch

    import gym_electric_motor_amd as ga

    n = args.envs
    generator = "default"  # default generators (i_sd, i_sq) and reward weights (0.5, 0.5) of the env id
    if args.reference == "profile":  # a given trajectory: a synthetic two-column cycle of 500 rows sampled at 2 tau, repeated (end="wrap")
        import numpy as np

        t = np.arange(500) / 500.0
        cycle = np.stack([-0.2 + 0.1 * np.sin(2 * np.pi * t), 0.3 * np.sign(np.sin(6 * np.pi * t))], axis=1)  # columns: i_sd, i_sq
        generator = ga.ProfileReferenceGenerator(cycle, reference_states=("i_sd", "i_sq"), profile_tau=2e-4, end="wrap", start="random", seed=1)
    elif args.reference != "wiener":  # one holder per referenced state; the columns of one device handle
        holder = getattr(ga, REFERENCES[args.reference])
        kw = dict() if args.reference in ("laplace", "constant") else dict(frequency_range=(5, 50), amplitude_range=(0.1, 0.4))
        generator = [holder(reference_state=s, **kw) for s in ("i_sd", "i_sq")]
    wrappers, obs_kw = (ga.DqToAbcActionProcessor.make("PMSM"),), dict()
    if args.flat:  # cos / sin instead of the angle, the four columns the policy reads, state and references in one tensor
        wrappers += (ga.CosSinProcessor(remove_angle=True),)
        obs_kw = dict(observed_states=["i_sd", "i_sq", "cos(epsilon)", "sin(epsilon)"], flatten_observation=True)
    if args.time_limit or args.max_episode_steps:
        obs_kw.update(max_episode_steps=args.time_limit or args.max_episode_steps, episode_statistics=True)
    env = ga.make("Cont-CC-PMSM-v0", n_envs=n, ode_solver=ga.RK4Solver(), physical_system_wrappers=wrappers, reference_generator=generator, seed=1, **obs_kw,
                  **env_parameter_kw(args, ga))
    ps = env.physical_system
    if args.max_episode_steps:
        return episodic_rollout_loop(args, env)
    if args.rollout:
        return rollout_loop(args, env)
    if args.flat:
        return flat_loop(args, env)
    cols = torch.tensor([ps.state_positions[s] for s in env.reference_names], device="cuda")
    gain = torch.tensor(8.0, device="cuda")
    ret = torch.zeros(n, device="cuda")
    action = torch.zeros((n, 2), device="cuda")
    mode = "eager"
    if args.bind or args.graph:
        mode = "bind_step"
        stream = torch.cuda.Stream() if args.graph else None
        step, (state, ref), reward, done = env.bind_step(action, stream=stream)

        def control_step():
            torch.clamp(gain * (ref - state.index_select(1, cols)), -1, 1, out=action)
            step()
            ret.add_(reward)
    (state, ref), _ = env.reset()
    reps = args.steps
    if args.graph:
        mode = f"HIP graph of {args.graph} steps"
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(3):
                control_step()
            env.reset()
            ret.zero_()
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for _ in range(args.graph):
                control_step()
        reps = args.steps // args.graph
        run_one = graph.replay
    elif args.bind:
        run_one = control_step
    else:
        def run_one():
            nonlocal state, ref
            torch.clamp(gain * (ref - state.index_select(1, cols)), -1, 1, out=action)
            (state, ref), reward, terminated, _, _ = env.step(action)
            ret.add_(reward)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run_one()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = reps * (args.graph or 1)
    print(f"complete env ({mode}, {args.reference} references): {n} envs x {steps} closed-loop steps in {dt:.3f} s = {n * steps / dt / 1e6:.1f} M env-steps/s "
          f"({dt / steps * 1e6:.1f} us/step); mean return {float(ret.mean()):.2f}; kernel: {ps.last_launch().split(' grid')[0]}")
    assert torch.isfinite(ret).all()
    episode_report(env)
    env.close()


def episode_report(env):
    """--time-limit: the finished episodes, from the device counters."""
    if env.episodes is None:
        return
    stats = env.episode_statistics()
    finished = stats["n_finished"] > 0
    if not bool(finished.any()):
        print("episodes: none finished yet")
        return
    print(f"episodes (limit {env.episodes.max_steps}): {int(stats['n_finished'].sum())} finished; last finished per env: mean return "
          f"{float(stats['last_ret'][finished].mean()):.2f}, mean length {float(stats['last_length'][finished].double().mean()):.1f}")


def episodic_rollout_loop(args, env):
    """Open loop on time-limited episodes: K control steps per launch of `bind_rollout_complete_episodic`, then GAE with the episode ends."""
    import torch

    import gym_electric_motor_amd as ga

    n, K, M = args.envs, args.rollout, args.max_episode_steps
    ps = env.physical_system
    shapes = env._complete_shapes(K)
    state, refs, reward = (torch.empty(s, device="cuda") for s in shapes[:3])
    terminated, truncated, ended = (torch.empty(shapes[3], dtype=torch.uint8, device="cuda") for _ in range(3))
    stats = dict(ended=ended, finished_return=torch.empty(shapes[3], dtype=torch.float64, device="cuda"),
                 finished_length=torch.empty(shapes[3], dtype=torch.int32, device="cuda"))
    env.reset()
    actions = ps.synthetic_actions(K, seed=1, step0=0)  # (fixed random actions: the policy of a learner would overwrite this tensor)
    rollout = env.bind_rollout_complete_episodic(actions, state, refs, reward, terminated, truncated, episode_statistics=stats)
    gamma, lam = 0.99, 0.95
    cols = torch.tensor([ps.state_positions[s] for s in env.reference_names], device="cuda")
    value, advantage, returns = (torch.empty_like(reward) for _ in range(3))
    ret = torch.zeros(n, device="cuda")

    def dataset():
        rollout()  # pending reset, episodic physics, generators, reward pass, episode rows, row K-1 shown: all on one stream
        # the value head: minus the tracking error over the discount's horizon.  (A row that ended shows the episode's FINAL state, so the
        # value of that row is the final_value of a truncated episode.)
        torch.sum((state[..., cols] - refs).abs(), dim=-1, out=value).mul_(-0.5 / (1.0 - gamma))
        ga.advantages(reward, value, terminated, gamma=gamma, lam=lam, ended=ended, final_value=value, advantage_out=advantage, return_out=returns)
        ret.add_(reward.sum(dim=0))

    dataset()  # (untimed: first launches)
    assert torch.equal(ended, terminated | truncated)
    reps = max(1, args.steps // K)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        dataset()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = reps * K
    print(f"complete env (bind_rollout_complete_episodic, K = {K}, max_episode_steps = {M}, {args.reference} references): {n} envs x {steps} steps in {dt:.3f} s = "
          f"{n * steps / dt / 1e6:.1f} M env-steps/s ({dt / steps * 1e6:.2f} us/step), GAE included; last chunk: {int(terminated.sum())} terminations, "
          f"{int(truncated.sum())} truncations; kernel: {ps.last_launch().split(' grid')[0]}")
    print(f"GAE(gamma {gamma}, lambda {lam}) with ended = terminated | truncated: advantage mean {float(advantage.mean()):+.4f} std {float(advantage.std()):.4f}; "
          f"returns mean {float(returns.mean()):+.3f}")
    assert torch.isfinite(ret).all() and torch.isfinite(advantage).all() and torch.isfinite(returns).all()
    assert int(truncated.sum()) > 0 or M > steps
    episode_report(env)
    env.close()


def rollout_loop(args, env):
    """Open loop: K control steps per call on the device's synthetic action stream, into fixed output tensors."""
    import torch

    n, K = args.envs, args.rollout
    ps = env.physical_system
    shapes = env._complete_shapes(K)
    state, refs, reward = (torch.empty(s, device="cuda") for s in shapes[:3])
    done = torch.empty(shapes[3], dtype=torch.uint8, device="cuda")
    ret = torch.zeros(n, device="cuda")
    gae = None
    if args.gae:  # the value head: minus the tracking error of the referenced currents over the discount's horizon; everything bound once
        import gym_electric_motor_amd as ga

        gamma, lam = 0.99, 0.95
        cols = torch.tensor([ps.state_positions[s] for s in env.reference_names], device="cuda")
        value, advantage, returns = (torch.empty_like(reward) for _ in range(3))
        gae = ga.bind_advantages(reward, value, done, gamma=gamma, lam=lam, advantage_out=advantage, return_out=returns)

        def value_head():
            torch.sum((state[..., cols] - refs).abs(), dim=-1, out=value).mul_(-0.5 / (1.0 - gamma))

    env.reset()
    env.rollout_complete_synthetic(K, seed=1, state_out=state, refs_out=refs, reward_out=reward, done_out=done)  # (untimed: first launches)
    if gae:
        value_head(), gae()
    reps = max(1, args.steps // K)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        env.rollout_complete_synthetic(K, seed=1, state_out=state, refs_out=refs, reward_out=reward, done_out=done)
        ret.add_(reward.sum(dim=0))
        if gae:
            value_head(), gae()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = reps * K
    print(f"complete env (rollout_complete_synthetic, K = {K}, {args.reference} references): {n} envs x {steps} steps in {dt:.3f} s = "
          f"{n * steps / dt / 1e6:.1f} M env-steps/s ({dt / steps * 1e6:.2f} us/step); state {tuple(state.shape)}, refs {tuple(refs.shape)}; "
          f"{int(done.sum())} terminations in the last chunk; mean return {float(ret.mean()):.2f}; kernel: {ps.last_launch().split(' grid')[0]}")
    assert torch.isfinite(ret).all()
    if gae:
        assert torch.isfinite(advantage).all() and torch.isfinite(returns).all()
        print(f"GAE(gamma {gamma}, lambda {lam}) of every dataset, one launch per {K} steps (in the time above): advantage {tuple(advantage.shape)} mean "
              f"{float(advantage.mean()):+.4f} std {float(advantage.std()):.4f}; returns mean {float(returns.mean()):+.3f}; value head mean {float(value.mean()):+.3f}")
    env.close()


def flat_loop(args, env):
    """The same closed loop on the flat observation [N, 4 + 2]: the policy reads its input as it is, nothing is selected or concatenated."""
    import torch

    n = args.envs
    gain = torch.tensor(8.0, device="cuda")
    ret = torch.zeros(n, device="cuda")
    action = torch.zeros((n, 2), device="cuda")
    stream = torch.cuda.Stream() if args.graph else None
    step, obs, reward, done = env.bind_step(action, stream=stream)
    assert obs.shape == (n, 6)

    def control_step():
        torch.clamp(gain * (obs[:, 4:6] - obs[:, 0:2]), -1, 1, out=action)
        step()
        ret.add_(reward)

    env.reset()
    mode, reps, run_one = "bind_step, flat observation", args.steps, control_step
    if args.graph:
        mode = f"HIP graph of {args.graph} steps, flat observation"
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(3):
                control_step()
            env.reset()
            ret.zero_()
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for _ in range(args.graph):
                control_step()
        reps, run_one = args.steps // args.graph, graph.replay
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run_one()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = reps * (args.graph or 1)
    print(f"complete env ({mode}, {args.reference} references): {n} envs x {steps} closed-loop steps in {dt:.3f} s = {n * steps / dt / 1e6:.1f} M env-steps/s "
          f"({dt / steps * 1e6:.1f} us/step); mean return {float(ret.mean()):.2f}")
    assert torch.isfinite(ret).all()
    episode_report(env)
    env.close()


if __name__ == "__main__":
    main()
