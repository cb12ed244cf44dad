#!/usr/bin/env python3
"""Time `gemx_refgen_step` per generator kind: microseconds per pre-bound step (`bind_step`) of a one-column handle of each kind, of a
four-column mix and of the all-Wiener handle, at 16384 and 131072 envs, float32.  Launches are enqueued back to back and timed with
device events (median of REPEATS runs of STEPS steps after a warm-up), so the figure is the kernel's turnaround behind a full queue,
not a launch latency seen from the host.  Prints a markdown table (profiles/refgen_kinds.md).

`--switched`: instead, the same two columns (sinusoidal, step) at 16384 envs once as plain columns (refgen_kinds_kernel) and once each as
a two-alternative switched column (refgen_switched_kernel), super-episodes of 100..10000 steps (profiles/refgen_switched.md).

    python tools/time_refgen_kinds.py [--steps 2000] [--repeats 7] [--switched]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_steps(torch, g, ps, done, steps, repeats):
    """-> µs per pre-bound step: (median, min, max) over the repeats"""
    g.set_modules(ps)
    g.reset()
    step = g.bind_step(done)
    for _ in range(200):
        step()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            step()
        t1.record()
        torch.cuda.synchronize()
        us.append(t0.elapsed_time(t1) * 1e3 / steps)
    g.close()
    return statistics.median(us), min(us), max(us)


def switched_table(torch, ga, a, n=16384):
    env = ga.make("Cont-CC-PMSM-v0", n_envs=n)
    ps = env.physical_system
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    pair = lambda s: [ga.SinusoidalReferenceGenerator(reference_state=s), ga.StepReferenceGenerator(reference_state=s)]  # noqa: E731
    gens = {"plain: sinusoidal (i_sd), step (i_sq)": (ga.BatchedMultipleReferenceGenerator([ga.SinusoidalReferenceGenerator(reference_state="i_sd"), ga.StepReferenceGenerator(reference_state="i_sq")], seed=1),
                                                      "refgen_kinds_kernel"),
            "switched: {sinusoidal, step} on i_sd and on i_sq": (ga.BatchedMultipleReferenceGenerator([ga.SwitchedReferenceGenerator(pair("i_sd")), ga.SwitchedReferenceGenerator(pair("i_sq"))], seed=1),
                                                                 "refgen_switched_kernel")}
    print(f"| generator | columns | kernel | {n} envs, µs/step |")
    print("|---|---|---|---|")
    for name, (g, kernel) in gens.items():
        med, lo, hi = time_steps(torch, g, ps, done, a.steps, a.repeats)
        print(f"| {name} | 2 | `{kernel}` | {med:.2f} (min {lo:.2f}, max {hi:.2f}) |")
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--switched", action="store_true")
    a = ap.parse_args()
    import torch

    import gym_electric_motor_amd as ga

    if a.switched:
        return switched_table(torch, ga, a)

    one = dict(wiener=ga.WienerProcessReferenceGenerator, laplace=ga.LaplaceProcessReferenceGenerator, sinusoidal=ga.SinusoidalReferenceGenerator,
               step=ga.StepReferenceGenerator, triangular=ga.TriangularReferenceGenerator, sawtooth=ga.SawtoothReferenceGenerator,
               constant=ga.ConstReferenceGenerator)
    print("| generator | columns | kernel | 16384 envs, µs/step | 131072 envs, µs/step |")
    print("|---|---|---|---|---|")
    rows = {}
    for n in (16384, 131072):
        env = ga.make("Cont-CC-PMSM-v0", n_envs=n)
        ps = env.physical_system
        done = torch.zeros(n, dtype=torch.uint8, device="cuda")
        gens = {"Wiener handle (BatchedWienerProcessReferenceGenerator)": (ga.BatchedWienerProcessReferenceGenerator(reference_states=("i_sd",), seed=1), 1, "refgen_step_kernel"),
                "Wiener handle, 4 columns": (ga.BatchedWienerProcessReferenceGenerator(reference_states=("omega", "torque", "i_sd", "i_sq"), seed=1), 4, "refgen_step_kernel")}
        for name, cls in one.items():
            kernel = "refgen_step_kernel (all Wiener)" if name == "wiener" else "refgen_kinds_kernel"
            gens[name] = (ga.BatchedMultipleReferenceGenerator(cls(reference_state="i_sd"), seed=1), 1, kernel)
        gens["mix: sinusoidal, step, laplace, wiener"] = (ga.BatchedMultipleReferenceGenerator(
            [ga.SinusoidalReferenceGenerator(reference_state="omega"), ga.StepReferenceGenerator(reference_state="torque"),
             ga.LaplaceProcessReferenceGenerator(reference_state="i_sd"), ga.WienerProcessReferenceGenerator(reference_state="i_sq")], seed=1), 4, "refgen_kinds_kernel")
        for name, (g, cols, kernel) in gens.items():
            med, lo, hi = time_steps(torch, g, ps, done, a.steps, a.repeats)
            rows.setdefault(name, [cols, kernel]).append(f"{med:.2f} (min {lo:.2f}, max {hi:.2f})")
        env.close()
    for name, r in rows.items():
        print(f"| {name} | {r[0]} | `{r[1]}` | {r[2]} | {r[3]} |")


if __name__ == "__main__":
    main()
