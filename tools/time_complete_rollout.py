#!/usr/bin/env python3
"""Timing of the complete env's fused K-step rollout on one GPU -> the table of profiles/complete_rollout.md.

Cont-CC-PMSM-v0 complete env (default Wiener generators, default reward) at --envs envs, K = --steps control steps per launch:

  1. `bind_rollout_complete`: physics rollout + generator rollout in the shell's order + reward pass, three launches per K steps;
  2. the physics-only `bind_rollout` of the same env: what the references and the reward cost on top;
  3. K bound `step()`s (two launches each), 64 steps per HIP graph, replayed: the closed-loop path the rollout replaces;
  4. the reward pass (gemx_reward_rows) alone over the stored trajectory, in algorithmic bytes per row
     4 (S_out + n_ref + 1) + 1, beside the chip's measured float4-copy rate.

Device time between two events on the launching stream, median over --windows windows (an untimed window first).

    python tools/time_complete_rollout.py [--envs 16384] [--steps 1000] [--windows 9]

`--host`: instead, the HOST's share of a call -> the tables of profiles/env_shell_refactor.md.  Python time per call (perf_counter
around --calls enqueues, the synchronise outside the clock; median, min and max over --repeats such batches, after a warm-up batch)
of the complete env's `bind_step` closure, its `bind_rollout_complete` closure at K = 1 and eager `step()` on a reused action tensor,
and of the eager `apply` / `rollout_shell` / `step(done)` of the stage and the generators, for the env without an observation stage
(PMSM) and with observer + column program (SCIM, FluxObserver, observed_states); one JSON line.

`--against DIR` (a second checkout of the package, e.g. the parent commit's) times both in ONE process, batch by batch alternately:
host clocks and core placement move a whole process by 20 % from run to run, which is more than any difference between two shells.

    python tools/time_complete_rollout.py --host [--envs 4096] [--calls 200] [--repeats 60] [--against DIR]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBPS = 6.29  # the chip's measured float4-copy rate (profiles/obs_stage.md quotes the same figure)


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


def _load_package(root, name):
    """The package of another checkout under another module name (its imports are relative; both use the library loaded first)."""
    import importlib.util

    pkg = os.path.join(root, "gym_electric_motor_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def host_overhead(packages, torch, n, calls, repeats):
    """packages: {label: package}; every row is timed on all of them alternately, batch by batch."""
    import json
    import time

    def per_call(fns):
        us = {label: [] for label in fns}
        for r in range(repeats + 1):
            for label, fn in (list(fns.items())[::-1] if r % 2 else fns.items()):  # (the order within a pair alternates too)
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                if r:
                    us[label].append((t1 - t0) / calls * 1e6)
        return {label: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for label, v in us.items()}

    def rows_of(ga, env_id, kw):
        env = ga.make(env_id, n_envs=n, reference_generator="default", seed=1, **kw(ga))
        env.reset()
        action = torch.full((n, 3), 0.01, device="cuda")
        sh = env._complete_shapes(1)
        outs = [torch.empty(s, device="cuda") for s in sh[:3]] + [torch.empty(sh[3], dtype=torch.uint8, device="cuda")]
        gen, stage = env.reference_generator, env.observation_stage
        done = torch.zeros(n, dtype=torch.uint8, device="cuda")
        done1, refs1 = done.view(1, n), outs[1]
        rows = {"bind_step closure": env.bind_step(action)[0],
                "bind_rollout_complete closure, K = 1": env.bind_rollout_complete(action.view(1, n, 3), *outs),
                "eager step(), reused action tensor": lambda: env.step(action),
                "eager generator step(done)": lambda: gen.step(done),
                "eager generator rollout_shell(1, done, out)": lambda: gen.rollout_shell(1, done1, out=refs1)}
        if stage is not None:
            state, post = torch.zeros((n, stage.n_in), device="cuda"), torch.zeros((n, stage.n_out), device="cuda")
            rows["eager stage apply(state, refs, out)"] = lambda: stage.apply(state, gen.references, out=post)
        return env, rows

    shapes = {"no stage": ("Cont-CC-PMSM-v0", lambda ga: dict()),
              "observer + program": ("Cont-CC-SCIM-v0", lambda ga: dict(physical_system_wrappers=(ga.FluxObserver(),),
                                                                        observed_states=["omega", "i_sd", "i_sq", "psi_abs", "psi_angle"]))}
    out = dict(envs=n, calls=calls, repeats=repeats, unit="us of Python per call", rows={})
    for name, (env_id, kw) in shapes.items():
        built = {label: rows_of(ga, env_id, kw) for label, ga in packages.items()}
        first = next(iter(built.values()))[1]
        out["rows"][name] = {row: per_call({label: rows[row] for label, (_, rows) in built.items()}) for row in first}
        for env, _ in built.values():
            env.close()
    print(json.dumps(out))


def main():
    import torch

    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=None, help="default: 16384, with --host 4096")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--host", action="store_true", help="Python time per call of the env shell's bound and eager forms (one JSON line)")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--against", metavar="DIR", default=None, help="with --host: another checkout whose package is timed alternately in the same process")
    args = ap.parse_args()
    if args.host:
        packages = {"this": ga}
        if args.against:
            packages["against"] = _load_package(args.against, "gym_electric_motor_amd_against")
        return host_overhead(packages, torch, args.envs or 4096, args.calls, args.repeats)
    n, K = args.envs or 16384, args.steps

    def make():
        env = ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator="default", seed=1)
        env.reset()
        return env

    acts = torch.rand((K, n, 3), device="cuda") * 0.02 - 0.01
    # 1. the complete rollout
    env = make()
    ps = env.physical_system
    shapes = env._complete_shapes(K)
    state, refs, reward = (torch.empty(s, device="cuda") for s in shapes[:3])
    done = torch.empty(shapes[3], dtype=torch.uint8, device="cuda")
    launch = env.bind_rollout_complete(acts, state, refs, reward, done)
    us_complete = timed(launch, args.windows) * 1e3 / K
    # 4. the reward pass alone, on the trajectory just stored
    n_ref, s_out = shapes[1][2], shapes[0][2]
    first = env.reference_generator.references.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: _lib.check(ps._L.gemx_reward_rows(ps._handle, C.c_void_p(state.data_ptr()), C.c_void_p(first.data_ptr()), C.c_void_p(refs.data_ptr()),  # noqa: E731
                                                        C.c_void_p(done.data_ptr()), K, C.c_void_p(reward.data_ptr()), st))
    ms_pass = timed(call, args.windows)
    gb = (4 * (s_out + n_ref + 1) + 1) * K * n / 1e9
    env.close()
    # 2. physics only
    env = make()
    launch = env.physical_system.bind_rollout(acts, state, done)
    us_physics = timed(launch, args.windows) * 1e3 / K
    env.close()
    # 3. bound steps from a HIP graph
    env = make()
    action = torch.full((n, 3), 0.01, device="cuda")
    stream = torch.cuda.Stream()
    step = env.bind_step(action, stream=stream)[0]
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for _ in range(64):
            step()
    reps = max(1, K // 64)
    with torch.cuda.stream(stream):
        us_steps = timed(lambda: [graph.replay() for _ in range(reps)], args.windows, stream) * 1e3 / (reps * 64)
    env.close()
    print(f"Cont-CC-PMSM-v0, {n} envs, K = {K}, median of {args.windows} windows")
    print("| path | us per control step |")
    print("|---|---|")
    print(f"| (1) bind_rollout_complete: physics + generators + reward pass | {us_complete:.3f} |")
    print(f"| (2) bind_rollout: physics only | {us_physics:.3f} |")
    print(f"| (3) bound step() x K, 64 steps per HIP graph | {us_steps:.3f} |")
    print(f"(1) against (3): {us_steps / us_complete:.2f} x faster; (1) against (2): {us_complete / us_physics:.2f} x the physics alone")
    rate = gb / (ms_pass * 1e-3)
    print(f"reward pass alone over [{K}, {n}, {s_out}]: {ms_pass:.3f} ms, {rate:.0f} GB/s algorithmic = {rate / (COPY_TBPS * 1e3):.2f} of the {COPY_TBPS} TB/s copy rate")


if __name__ == "__main__":
    main()
