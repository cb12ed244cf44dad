"""Digests and launch timings of the four support units of libgemx.so (csrc/gemx_obsproc.hip, gemx_rewardpass.hip, gemx_fluxobs.hip,
gemx_refgen.hip), for changes that must leave their bits and their speed alone (profiles/support_units_refactor.md).

    python tools/support_unit_digest.py digest OUT.json     SHA-256 of every output tensor and state array
    python tools/support_unit_digest.py time OUT.json       median launch time per unit, device events, 20 launches after 5 warm-ups
    python tools/support_unit_digest.py compare A.json B.json

`digest` drives each unit through the public Python API at the smallest shapes that reach every branch of the tile staging: N = 67 and
259 envs (a partial last tile of the 256-row fp32 and of the 128-row fp64 tile, more than one tile), K = 5, fp32 and fp64, rows of 14 and
24 states (PMSM / SCIM, DFIM: row lengths in dwords that are and are not multiples of four), a flat observation with references, inputs
and outputs as views at an odd element offset.  The generators: an all-Wiener handle, mixed handles over every kind, a switched handle
with a plain column beside it; each through reset, step, rollout, rollout_shell with a done mask, state().  The reward pass runs behind
`rollout_complete`, whose physics rollout needs a 16-byte aligned state tensor: there the references and the reward are the odd views
(the pass on an odd view of the rows is tests/test_gpu_complete_rollout.py's).  The digests depend on the ROCm math library: they are a
record to compare two builds on one machine, not a test."""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gym_electric_motor_amd as ga  # noqa: E402

K = 5
ENVS = {"PMSM": "Cont-CC-PMSM-v0", "SCIM": "Cont-CC-SCIM-v0", "DFIM": "Cont-CC-DFIM-v0"}
SUB = dict(episode_lengths=(2, 4))


def sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def view(shape, dtype, off, fill=None):
    """A contiguous tensor at element offset `off` of its allocation."""
    numel = int(np.prod(shape))
    buf = torch.zeros(numel + 4, dtype=dtype, device="cuda")
    v = buf[off:off + numel].view(shape)
    if fill is not None:
        v.copy_(fill)
    return v


def rand(shape, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) * 2 - 1).to(dtype)


def done_mask(shape, seed, share=0.2):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(shape, generator=g, device="cuda") < share).to(torch.uint8)


def currents(motor):
    return ("i_a", "i_b", "i_c") if motor == "PMSM" else ("i_sa", "i_sb", "i_sc")


def obs_stage(out, motor, dtype, n):
    base = ga.make(ENVS[motor], n_envs=2)  # (for its names, limits and state box)
    ps = base.physical_system
    tdt = getattr(torch, dtype)
    rows = K * n
    for name, chain, flat, n_ref in (("flat_cossin", (("sum", currents(motor), "max"), ("cossin", "epsilon", True)), True, 2),
                                     ("sum_keep", (("sum", currents(motor)[:2], "sum"), ("cossin", "epsilon", False)), False, 0),
                                     ("flat_copy3", (), True, 3)):
        stage = ga.ObservationStage(ps, chain, flatten=flat, n_ref=n_ref).create(0, dtype)
        for off in (0, 1):
            x = view((rows, stage.n_in), tdt, off, rand((rows, stage.n_in), tdt, 1))
            r = view((rows, n_ref), tdt, off, rand((rows, n_ref), tdt, 2)) if n_ref else None
            y = stage.apply(x, r, out=view((rows, stage.n_out), tdt, 1 - off))
            out[f"obsproc/{motor}/{dtype}/N{n}/{name}/off{off}"] = sha(y)
        stage.close()
    base.close()


def flux_observer(out, motor, dtype, n):
    tdt = getattr(torch, dtype)
    mk = lambda: ga.make(ENVS[motor], n_envs=n, dtype=dtype, auto_reset=True,  # noqa: E731
                         physical_system_wrappers=(ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor(motor)))
    for off in (0, 1):
        ea, eb = mk(), mk()
        fa, fb = ea.flux, eb.flux  # (the envs' own observer handles, fresh)
        nb = fa.n_in
        state = view((K, n, nb), tdt, off, rand((K, n, nb), tdt, 3))
        done = done_mask((K, n), 4)
        key = f"fluxobs/{motor}/{dtype}/N{n}/off{off}"
        out[f"{key}/rows"] = sha(fa.rows(state, done, out=view((K, n, nb + 2), tdt, 1 - off)))
        steps = view((K, n, nb + 2), tdt, off)
        for k in range(K):
            fb.step(state[k], done[k], steps[k])
        out[f"{key}/steps"] = sha(steps)
        dq = view((n, fa.n_action), tdt, off, rand((n, fa.n_action), tdt, 5))
        abc = view((n, fa.n_action * 3 // 2), tdt, 1 - off)
        fa.bind_actions(dq, abc)()
        out[f"{key}/actions"] = sha(abc)
        out[f"{key}/state_rows"] = sha(fa.get_state())
        out[f"{key}/state_steps"] = sha(fb.get_state())
        fa.reset(done[0])
        out[f"{key}/state_reset"] = sha(fa.get_state())
        ea.close(), eb.close()


def reward_pass(out, motor, dtype, n):
    tdt = getattr(torch, dtype)
    for power in (1, 2, 3):
        env = ga.make(ENVS[motor], n_envs=n, dtype=dtype, auto_reset=True, reference_generator="default", reward_function=dict(reward_power=power), seed=7)
        ps = env.physical_system
        env.reset()
        acts = rand((K, n, int(ps.action_space.shape[0])), tdt, 6).contiguous()
        n_ref = len(env.reference_names)
        state, refs, reward, done = env.rollout_complete(acts, refs_out=view((K, n, n_ref), tdt, 1), reward_out=view((K, n), tdt, 1))
        key = f"rewardpass/{motor}/{dtype}/N{n}/power{power}"
        for name, t in (("state", state), ("refs", refs), ("reward", reward), ("done", done)):
            out[f"{key}/{name}"] = sha(t)
        env.close()


def generator_handles(ps):
    wave = dict(frequency_range=(500, 3000), **SUB)
    walk = dict(sigma_range=(1e-3, 1e-2), **SUB)
    yield "wiener", ga.BatchedWienerProcessReferenceGenerator(reference_states=("i_sd", "i_sq", "omega"), episode_lengths=(2, 4), seed=11)
    yield "kinds_a", ga.BatchedMultipleReferenceGenerator([ga.WienerProcessReferenceGenerator(reference_state="omega", **walk),
                                                           ga.LaplaceProcessReferenceGenerator(reference_state="torque", **walk),
                                                           ga.SinusoidalReferenceGenerator(reference_state="i_sd", **wave),
                                                           ga.StepReferenceGenerator(reference_state="i_sq", **wave)], seed=12)
    yield "kinds_b", ga.BatchedMultipleReferenceGenerator([ga.TriangularReferenceGenerator(reference_state="omega", **wave),
                                                           ga.SawtoothReferenceGenerator(reference_state="i_sd", **wave),
                                                           ga.ConstReferenceGenerator(reference_state="i_sq", reference_value=0.25)], seed=13)
    yield "switched", ga.BatchedMultipleReferenceGenerator([
        ga.SwitchedReferenceGenerator([ga.StepReferenceGenerator(reference_state="omega", **wave), ga.SinusoidalReferenceGenerator(reference_state="omega", **wave),
                                       ga.WienerProcessReferenceGenerator(reference_state="omega", **walk), ga.ConstReferenceGenerator(reference_state="omega", reference_value=0.25),
                                       ga.LaplaceProcessReferenceGenerator(reference_state="omega", **walk)], p=[0.25, 0.25, 0.2, 0.1, 0.2], super_episode_length=(2, 5)),
        ga.TriangularReferenceGenerator(reference_state="i_sd", **wave),
        ga.SwitchedReferenceGenerator([ga.SawtoothReferenceGenerator(reference_state="i_sq", **wave), ga.ConstReferenceGenerator(reference_state="i_sq", reference_value=-0.125)],
                                      super_episode_length=(2, 5))], seed=14)


def generators(out, dtype, n):
    tdt = getattr(torch, dtype)
    env = ga.make(ENVS["PMSM"], n_envs=n, dtype=dtype)
    ps = env.physical_system
    for name, gen in generator_handles(ps):
        gen.set_modules(ps)
        key = f"refgen/{name}/{dtype}/N{n}"

        def state(tag):
            s = gen.state()
            for k_, t in (s.items() if isinstance(s, dict) else zip(("value", "sigma", "left"), s)):
                out[f"{key}/{tag}/state/{k_}"] = sha(t)

        n_ref = len(gen.reference_names)
        gen.reset()
        state("reset")
        for k in range(K):
            out[f"{key}/step{k}"] = sha(gen.step(done_mask((n,), 20 + k) if k else None))
        state("steps")
        out[f"{key}/rollout"] = sha(gen.rollout(K, done=done_mask((K, n), 30), out=view((K, n, n_ref), tdt, 1)))
        state("rollout")
        out[f"{key}/rollout_shell"] = sha(gen.rollout_shell(K, done_mask((K, n), 31), out=view((K, n, n_ref), tdt, 1)))
        state("rollout_shell")
        gen.reset(done_mask((n,), 32, share=0.5))
        out[f"{key}/step_after_masked_reset"] = sha(gen.step())
        state("masked_reset")
        gen.close()
    env.close()


def digest(path):
    out = {}
    for dtype in ("float32", "float64"):
        for n in (67, 259):
            for motor in ("PMSM", "SCIM", "DFIM"):
                obs_stage(out, motor, dtype, n)
            for motor in ("SCIM", "DFIM"):
                flux_observer(out, motor, dtype, n)
            for motor in ("PMSM", "SCIM"):
                reward_pass(out, motor, dtype, n)
            generators(out, dtype, n)
            torch.cuda.synchronize()
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    print(f"{len(out)} digests -> {path}")


def median_ms(launch, warmup=5, timed=20):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(timed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def timings(path, n=16384, k=100):
    """One launch per unit at N = 16384, K = 100, fp32 (the generators: one K-step rollout_shell per handle kind and one step)."""
    tdt, out = torch.float32, {}
    env = ga.make(ENVS["PMSM"], n_envs=n, auto_reset=True, reference_generator="default", reward_function="default", seed=7)
    ps = env.physical_system
    env.reset()
    stage = ga.ObservationStage(ps, (("sum", currents("PMSM"), "max"), ("cossin", "epsilon", True)), flatten=True, n_ref=2).create(0, "float32")
    x, r = rand((k, n, stage.n_in), tdt, 1), rand((k, n, 2), tdt, 2)
    out["obsproc_apply"] = median_ms(stage.bind_apply(x, r, torch.empty((k, n, stage.n_out), dtype=tdt, device="cuda")))
    stage.close()

    fenv = ga.make(ENVS["SCIM"], n_envs=n, auto_reset=True, physical_system_wrappers=(ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor("SCIM")))
    flux = fenv.flux
    state, done = rand((k, n, flux.n_in), tdt, 3), done_mask((k, n), 4, share=0.01)
    ext = torch.empty((k, n, flux.n_in + 2), dtype=tdt, device="cuda")
    out["fluxobs_rows"] = median_ms(flux.bind_rows(state, done, ext))
    out["fluxobs_step"] = median_ms(flux.bind_step(state[0], done[0], ext[0]))
    out["fluxobs_actions"] = median_ms(flux.bind_actions(rand((n, 2), tdt, 5), torch.empty((n, 3), dtype=tdt, device="cuda")))
    fenv.close()

    rows, dn = ps.rollout(rand((k, n, 3), tdt, 6))  # the physics' rows and done mask: what the reward pass reads
    refs_rows = rand((k, n, len(env.reference_names)), tdt, 8)
    out["rewardpass_rows"] = median_ms(env.bind_reward_rows(rows, refs_rows, dn, torch.empty((k, n), dtype=tdt, device="cuda")))
    for name, gen in generator_handles(ps):
        gen.set_modules(ps)
        gen.reset()
        refs = torch.empty((k, n, len(gen.reference_names)), dtype=tdt, device="cuda")
        out[f"refgen_{name}_rollout_shell"] = median_ms(gen.bind_rollout_shell(dn, refs))
        out[f"refgen_{name}_step"] = median_ms(gen.bind_step(dn[0].contiguous()))
        gen.close()
    env.close()
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
    for k in diff:
        print("DIFFERS", k)
    print(f"{len(A)} entries, {len(diff)} differ")
    return 1 if diff else 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 2 else ""
    if mode == "digest":
        digest(sys.argv[2])
    elif mode == "time":
        timings(sys.argv[2])
    elif mode == "compare" and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
