"""Per-env parameters: what the table costs.  For Finite-CC-PMSM-v0 and Cont-SC-SCIM-v0 at 16384 and 2^20 envs, the same env with a
parameter table (all rows equal) and without one, on the same box: us per control step from a HIP graph of bound steps, and env-steps/s of
256-step rollouts -- each the median of alternated windows of at least 50 ms with the lowest and highest window beside it --, plus the achieved fraction of the algorithmic bytes (actions read, rows and done bytes written; with a table: its column
read once per launch) of 8 TB/s.  Writes profiles/env_parameters.md (the build figures at its end are kept).

    python tools/time_env_parameters.py [--out profiles/env_parameters.md]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gym_electric_motor_amd as ga  # noqa: E402
from gym_electric_motor_amd.env_parameters import table_fields  # noqa: E402

ENVS = (("Finite-CC-PMSM-v0", dict(tau=1e-4)), ("Cont-SC-SCIM-v0", dict()))
SIZES = (16384, 1 << 20)
K, GRAPH_STEPS, REPS = 256, 64, 9
WINDOW = 0.05  # seconds of device work per timed window at the least: the graph / the rollout is launched back to back that often
PEAK = 8.0e12


def actions_of(ps, shape):
    if ps._discrete:
        return torch.randint(0, int(ps.action_space.n), shape, dtype=torch.uint8, device="cuda")
    return torch.rand(shape + (ps._n_act,), device="cuda") * 2 - 1


class Timed:
    """One env (with or without a table) with its two timed workloads bound: `step_window()` and `roll_window()` each run one timed
    window of at least WINDOW seconds and return the seconds per graph replay / per rollout launch."""

    def __init__(self, env_id, kw, n, table):
        self.table, self.n = table, n
        self.env = ga.make(env_id, n_envs=n, env_parameters=ga.EnvParameters() if table else None, **kw)
        ps = self.ps = self.env.physical_system
        self.a1 = actions_of(ps, (n,))
        side = torch.cuda.Stream()
        step, _, _ = ps.bind_step(self.a1, stream=side)
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            for _ in range(GRAPH_STEPS):
                step()
        self.step_kernel = ps.last_launch().split("<")[0]
        self.aK = actions_of(ps, (K, n))
        self.obs = torch.empty((K,) + tuple(ps._obs.shape), device="cuda")
        self.done = torch.empty((K, n), dtype=torch.uint8, device="cuda")
        self.launch = ps.bind_rollout(self.aK, self.obs, self.done)
        for _ in range(2):
            self.launch()
        torch.cuda.synchronize()
        self.roll_kernel = ps.last_launch().split("<")[0]
        self.counts = {}

    def _window(self, name, fn):
        if name not in self.counts:  # how many back-to-back launches fill WINDOW: from one untimed-for-the-record trial of 8
            self.counts[name] = max(8, int(8 * WINDOW / self._run(fn, 8)) + 1)
        return self._run(fn, self.counts[name]) / self.counts[name]

    @staticmethod
    def _run(fn, count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def step_window(self):
        return self._window("step", self.graph.replay) / GRAPH_STEPS

    def roll_window(self):
        return self._window("roll", self.launch)

    def result(self, steps, rolls):
        ps, n = self.ps, self.n
        step, roll = statistics.median(steps), statistics.median(rolls)
        abytes = 1 if ps._discrete else 4 * ps._n_act
        per_step = abytes + 4 * ps._n_out + 1
        table_bytes = 4 * table_fields(ps._SYSTEM_KIND) if self.table else 0
        state_bytes = 2 * 4 * (ps._n_ode)
        return dict(step_us=step * 1e6, step_lo=min(steps) * 1e6, step_hi=max(steps) * 1e6, step_kernel=self.step_kernel,
                    frac_step=n * (per_step + table_bytes + state_bytes) / step / PEAK, rate=n * K / roll, rate_lo=n * K / max(rolls),
                    rate_hi=n * K / min(rolls), roll_kernel=self.roll_kernel, frac_roll=n * (K * per_step + table_bytes + state_bytes) / roll / PEAK)


def measure(env_id, kw, n):
    """-> (result without a table, result with one): both envs alive at once, their windows ALTERNATED, REPS windows each, so that drift of
    the box (clocks, neighbours) falls on both alike; median, with the lowest and highest window as the spread."""
    pair = [Timed(env_id, kw, n, False), Timed(env_id, kw, n, True)]
    steps, rolls = ([], []), ([], [])
    for _ in range(REPS):
        for i, t in enumerate(pair):
            steps[i].append(t.step_window())
    for _ in range(REPS):
        for i, t in enumerate(pair):
            rolls[i].append(t.roll_window())
    out = [t.result(steps[i], rolls[i]) for i, t in enumerate(pair)]
    for t in pair:
        t.env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "env_parameters.md"))
    args = ap.parse_args()
    rows = []
    for env_id, kw in ENVS:
        for n in SIZES:
            for table, r in zip((False, True), measure(env_id, kw, n)):
                rows.append((env_id, n, table, r))
                print(env_id, n, "table" if table else "plain", r, flush=True)
    lines = ["## Timing (tools/time_env_parameters.py, one box; median of %d alternated windows of >= %d ms, lowest .. highest window)" % (REPS, int(WINDOW * 1e3)), "",
             "| env | envs | table | us / step (graph of %d) | of 8 TB/s | kernel | G env-steps/s (%d-step rollout) | of 8 TB/s | kernel |" % (GRAPH_STEPS, K),
             "|---|---|---|---|---|---|---|---|---|"]
    for env_id, n, table, r in rows:
        lines.append(f"| {env_id} | {n} | {'all rows equal' if table else 'none'} | {r['step_us']:.2f} ({r['step_lo']:.2f} .. {r['step_hi']:.2f}) | {r['frac_step']:.3f} | "
                     f"{r['step_kernel'].replace('gemx::', '')} | {r['rate'] / 1e9:.1f} ({r['rate_lo'] / 1e9:.1f} .. {r['rate_hi'] / 1e9:.1f}) | {r['frac_roll']:.3f} | "
                     f"{r['roll_kernel'].replace('gemx::', '')} |")
    text = "\n".join(lines) + "\n"
    old = open(args.out).read() if os.path.exists(args.out) else "# Per-env parameters\n\n"
    marker = "## Timing"
    head = old.split(marker)[0]
    tail = ""
    if marker in old and "\n## " in old.split(marker, 1)[1]:
        tail = "\n## " + old.split(marker, 1)[1].split("\n## ", 1)[1]
    with open(args.out, "w") as fh:
        fh.write(head + text + tail)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
