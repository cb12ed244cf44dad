"""Registers, LDS and scratch of every policy_rollout_kernel (csrc/gemx_policy_kernel.hpp) instantiation, from the compiler's own remarks:
compiles the 19 policy units (csrc/gemx_policy.hip: the kernel without a generator) with build.py's flags plus
-Rpass-analysis=kernel-resource-usage into a temporary directory and prints the markdown table of profiles/policy_rollout.md.  Exit status
1 if any instantiation has scratch.
--complete: the same for the kernel's instantiations in the 19 complete policy units (csrc/gemx_policy_complete.hip; one more column, the
generator kind: 0 all-Wiener, 1 profile) -- the table of profiles/policy_complete_rollout.md.
--eval: the four policy_eval_kernel instantiations of csrc/gemx_policy_eval.hip (one per head), compiled once as libgemx.so's object is --
the table of profiles/policy_eval.md.
--lookahead: the lookahead_rollout_kernel instantiations of the 8 lookahead units (csrc/gemx_lookahead.hip, finite converters only; the
generator column as with --complete) -- the table of profiles/lookahead_rollout.md."""
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_electric_motor_amd import build  # noqa: E402

COMPLETE = "--complete" in sys.argv[1:]
EVAL = "--eval" in sys.argv[1:]
LOOKAHEAD = "--lookahead" in sys.argv[1:]
EVAL_NAME = re.compile(r"policy_eval_kernelILi(\d+)E")
HEADS = ("none", "value", "categorical", "gaussian")
SOURCE = "gemx_lookahead.hip" if LOOKAHEAD else "gemx_policy_complete.hip" if COMPLETE else "gemx_policy.hip"
COMPLETE = COMPLETE or LOOKAHEAD  # (the generator column)
NAME = re.compile(r"(?:policy|lookahead)_rollout_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi(\d+)E")  # SYS, CONV, LOAD, SOLVER, TAB, GEN (2 in the policy units: none)
FIELD = re.compile(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)")


def parse(text, name):
    rows, cur = [], None
    for line in text.splitlines():
        m = name.search(line)
        if "Function Name" in line:
            cur = dict(key=tuple(int(x) for x in m.groups())) if m else None
            if cur is not None:
                rows.append(cur)
        elif cur is not None:
            f = FIELD.search(line)
            if f:
                cur[f.group(1).split(" [")[0]] = int(f.group(2))
    return rows


def eval_main():
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.hipcc_path()] + build.FLAGS + ["-I" + build.CSRC, "-I" + os.path.dirname(build.HEADER), "-c", os.path.join(build.CSRC, "gemx_policy_eval.hip"),
               "-o", os.path.join(tmp, "policy_eval.o"), "-Rpass-analysis=kernel-resource-usage"]
        rows = parse(subprocess.run(cmd, capture_output=True, text=True, check=True).stderr, EVAL_NAME)
    print("| kernel | head | VGPRs | AGPRs | SGPR spills | scratch B/lane | static LDS B | waves/SIMD |\n|---|---|---|---|---|---|---|---|")
    for r in sorted(rows, key=lambda r: r["key"]):
        h = r["key"][0]
        print(f"| `policy_eval_kernel<{h}>` | {HEADS[h]} | {r['VGPRs']} | {r['AGPRs']} | {r.get('SGPRs Spill', 0)} | {r['ScratchSize']} | {r['LDS Size']} | {r['Occupancy']} |")
    print(f"\n{len(rows)} instantiations; max scratch {max(r['ScratchSize'] for r in rows)} bytes/lane")
    return 1 if len(rows) != 4 or any(r["ScratchSize"] for r in rows) else 0


def unit(sc, tmp):
    s, c = sc
    cmd = [build.hipcc_path()] + build.FLAGS + ["-I" + build.CSRC, "-I" + os.path.dirname(build.HEADER), f"-DGEMX_INST_SYS={s}", f"-DGEMX_INST_CONV={c}",
           "-fvisibility=hidden", "-shared", os.path.join(build.CSRC, SOURCE), "-o", os.path.join(tmp, f"pl{s}_{c}.so"), "-Rpass-analysis=kernel-resource-usage"]
    return parse(subprocess.run(cmd, capture_output=True, text=True, check=True).stderr, NAME)


def main():
    if EVAL:
        return eval_main()
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:
        rows = [r for unit_rows in ex.map(lambda sc: unit(sc, tmp), build.LA_UNITS if LOOKAHEAD else build.UNITS) for r in unit_rows]
    gen = " generator |" if COMPLETE else ""
    print(f"| sys/conv | load | solver | table |{gen} VGPRs | AGPRs | SGPR spills | scratch B/lane | static LDS B | waves/SIMD |\n|---|---|---|---|---|---|---|---|---|---|{'---|' if COMPLETE else ''}")
    for r in sorted(rows, key=lambda r: r["key"]):
        s, c, ld, sv, tab = r["key"][:5]
        gen = f" {r['key'][5]} |" if COMPLETE else ""
        print(f"| {s}/{c} | {ld} | {sv} | {tab} |{gen} {r['VGPRs']} | {r['AGPRs']} | {r.get('SGPRs Spill', 0)} | {r['ScratchSize']} | {r['LDS Size']} | {r['Occupancy']} |")
    print(f"\n{len(rows)} instantiations; max VGPRs {max(r['VGPRs'] for r in rows)}, max AGPRs {max(r['AGPRs'] for r in rows)}, "
          f"max scratch {max(r['ScratchSize'] for r in rows)} bytes/lane")
    return 1 if any(r["ScratchSize"] for r in rows) else 0


if __name__ == "__main__":
    sys.exit(main())
