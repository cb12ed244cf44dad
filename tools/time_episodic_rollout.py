"""Episodic rollouts: what the time limit inside the fused launch costs and what it saves.  For Finite-CC-PMSM-v0 and Cont-SC-SCIM-v0 at
16384 and 2^20 envs, K = 256, max_episode_steps = 100, the complete env (default references and reward), on the same box and alternated:

    episodic        bind_rollout_complete_episodic, uniform handle and handle with a parameter table (all rows equal)
    (a) steps       K bound complete step()s with the same time limit, replayed from ONE HIP graph: what such an env had before
    (b) no limit    bind_rollout_complete of the same env WITHOUT a time limit, uniform handle and handle with a table

Each figure is the median of alternated windows of at least 50 ms with the lowest and highest window beside it: env-steps/s, and the
fraction of 8 TB/s in algorithmic bytes of the physics launch (actions read, rows and the three mask bytes written -- one done byte for (b)
--, plus the table column and `length` once per launch).  Writes the "## Rates" section of profiles/episodic_rollout.md.

    python tools/time_episodic_rollout.py [--out profiles/episodic_rollout.md]
    python tools/time_episodic_rollout.py --resources      # no GPU: the compiler's resource remarks per unit, the section above it
"""
import argparse
import collections
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ENVS = (("Finite-CC-PMSM-v0", dict(tau=1e-4)), ("Cont-SC-SCIM-v0", dict()))
SIZES = (16384, 1 << 20)
K, M, REPS = 256, 100, 9
WINDOW = 0.05  # seconds of device work per timed window at the least
PEAK = 8.0e12
VARIANTS = ("episodic", "episodic, table", "(a) graph of K steps", "(b) rollout_complete, no limit", "(b) with a table")


def _run(torch, fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


class Workload:
    """One variant with its launcher bound on the shared output tensors; `window()` -> seconds per K control steps of every env."""

    def __init__(self, torch, ga, name, env_id, kw, n, outs):
        from gym_electric_motor_amd.env_parameters import table_fields

        self.torch, self.name, self.n = torch, name, n
        table = "table" in name
        limit = not name.startswith("(b)")
        env = self.env = ga.make(env_id, n_envs=n, reference_generator="default", seed=1, max_episode_steps=M if limit else None,
                                 env_parameters=ga.EnvParameters() if table else None, **kw)
        env.reset()
        ps = env.physical_system
        if ps._discrete:
            self.a = torch.randint(0, int(ps.action_space.n), (K, n), dtype=torch.uint8, device="cuda")
        else:
            self.a = torch.rand((K, n, ps._n_act), device="cuda") * 2 - 1
        state, refs, reward, term, trunc = outs
        if name.startswith("(a)"):
            buf = self.a[0].clone()
            side = torch.cuda.Stream()
            step = env.bind_step(buf, stream=side)[0]
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step()
            torch.cuda.synchronize()
            graph = self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(K):
                    step()
            self.fn = graph.replay
        elif limit:
            self.fn = env.bind_rollout_complete_episodic(self.a, state, refs, reward, term, trunc)
        else:
            self.fn = env.bind_rollout_complete(self.a, state, refs, reward, term)
        for _ in range(2):
            self.fn()
        torch.cuda.synchronize()
        abytes = 1 if ps._discrete else 4 * ps._n_act
        masks = 3 if limit else 1
        once = (4 * table_fields(ps._SYSTEM_KIND) if table else 0) + (4 if limit and not name.startswith("(a)") else 0)
        self.bytes = n * (K * (abytes + 4 * ps._n_out + masks) + once)
        self.count = max(4, int(4 * WINDOW / _run(torch, self.fn, 4)) + 1)

    def window(self):
        return _run(self.torch, self.fn, self.count) / self.count


def measure(torch, ga, env_id, kw, n):
    """All variants of one (env, size) alive at once on shared output tensors, their windows alternated REPS times."""
    probe = ga.make(env_id, n_envs=4, reference_generator="default", _defer_create=True, **kw)
    S, R = len(probe.state_names), len(probe.reference_names)
    outs = (torch.empty((K, n, S), device="cuda"), torch.empty((K, n, R), device="cuda"), torch.empty((K, n), device="cuda"),
            torch.empty((K, n), dtype=torch.uint8, device="cuda"), torch.empty((K, n), dtype=torch.uint8, device="cuda"))
    work = [Workload(torch, ga, name, env_id, kw, n, outs) for name in VARIANTS]
    times = [[] for _ in work]
    for _ in range(REPS):
        for i, w in enumerate(work):
            times[i].append(w.window())
    rows = []
    for w, t in zip(work, times):
        med = statistics.median(t)
        rows.append(dict(name=w.name, rate=n * K / med, lo=n * K / max(t), hi=n * K / min(t), frac=w.bytes / med / PEAK))
        w.env.close()
    return rows


def resources():
    """The compiler's resource remarks of every episodic unit -> markdown table (VGPRs and scratch bytes per instantiation)."""
    from gym_electric_motor_amd import build

    csrc = os.path.join(REPO, "gym_electric_motor_amd", "csrc")
    table = collections.OrderedDict()
    with tempfile.TemporaryDirectory() as tmp:
        for s, c in build.UNITS:
            cmd = [build.hipcc_path()] + build.FLAGS + ["-I" + csrc, "-I" + os.path.join(REPO, "include"), f"-DGEMX_INST_SYS={s}", f"-DGEMX_INST_CONV={c}",
                                                      "-fvisibility=hidden", "-shared", os.path.join(csrc, "gemx_episodic.hip"), "-o", os.path.join(tmp, "unit.so"),
                                                      "-Rpass-analysis=kernel-resource-usage"]
            err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
            cur = None
            for line in err.splitlines():
                m = re.search(r"Function Name: (\S+)", line)
                if m:
                    cur = m.group(1)
                    continue
                m = re.search(r"\s(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
                if m and cur and "episodic_rollout_kernel" in cur:
                    t = re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])", cur)
                    table.setdefault((s, c, int(t.group(3)), int(t.group(4)), int(t.group(5))), {})[m.group(1)] = int(m.group(2))
    vg = max(v["VGPRs"] for v in table.values())
    sc = max(v["ScratchSize [bytes/lane]"] for v in table.values())
    lines = ["## Compiler resource report per unit", "",
             "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `gemx_episodic.hip`, once per (system, converter unit)",
             f"(`tools/time_episodic_rollout.py --resources`): `episodic_rollout_kernel<SYS, CONV, LOAD, SOLVER, TAB, float>`, {len(table)} instantiations,",
             f"at most {vg} VGPRs, at most {sc} bytes of scratch.  (The units also carry `linmap_kernel`, the existing one-thread kernel that builds a",
             "handle's one-step map once; it is not an instantiation of this kernel.)", "",
             "| unit (system, converter) | load | solver | table | VGPRs | scratch bytes/lane |", "|---|---|---|---|---|---|"]
    for (s, c, ld, sv, tab), v in table.items():
        lines.append(f"| libgemx_tl{s}_{c}.so | {'ConstantSpeed' if ld == 0 else 'PolynomialStatic'} | {'Euler' if sv == 0 else 'RK4'} | {'yes' if tab else 'no'} | "
                     f"{v['VGPRs']} | {v['ScratchSize [bytes/lane]']} |")
    return "\n".join(lines) + "\n"


def replace_section(path, marker, text):
    """Write `text` (which starts with `marker`) in place of the section of that heading, or append it; other sections are kept."""
    old = open(path).read() if os.path.exists(path) else "# Episodic rollout kernel (`csrc/gemx_episodic.hip`)\n\n"
    if marker not in old:
        new = old.rstrip("\n") + "\n\n" + text
    else:
        head, rest = old.split(marker, 1)
        tail = "\n## " + rest.split("\n## ", 1)[1] if "\n## " in rest else ""
        new = head + text + tail
    with open(path, "w") as fh:
        fh.write(new)
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "episodic_rollout.md"))
    ap.add_argument("--resources", action="store_true", help="write the compiler's resource remarks per unit instead of timing (needs hipcc, no GPU)")
    args = ap.parse_args()
    if args.resources:
        replace_section(args.out, "## Compiler resource report per unit", resources())
        return
    import torch

    import gym_electric_motor_amd as ga

    lines = ["## Rates", "", f"`tools/time_episodic_rollout.py`, one box, complete env, K = {K}, max_episode_steps = {M}; median of {REPS} alternated windows of >= "
             f"{int(WINDOW * 1e3)} ms (lowest .. highest window).", "", "| env | envs | variant | G env-steps/s | of 8 TB/s (algorithmic bytes) | against (b) |", "|---|---|---|---|---|---|"]
    for env_id, kw in ENVS:
        for n in SIZES:
            rows = measure(torch, ga, env_id, kw, n)
            base = {False: rows[3]["rate"], True: rows[4]["rate"]}
            for r in rows:
                rel = r["rate"] / base["table" in r["name"]]
                lines.append(f"| {env_id} | {n} | {r['name']} | {r['rate'] / 1e9:.2f} ({r['lo'] / 1e9:.2f} .. {r['hi'] / 1e9:.2f}) | {r['frac']:.3f} | {rel:.2f} |")
                print(lines[-1], flush=True)
    replace_section(args.out, "## Rates", "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
