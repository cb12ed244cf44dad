"""The pure layer of csrc/gemx_launch_plan.hpp without a GPU: a stand-alone program (tests/launch_plan_replay.cpp, its own main) is built
against the header by a plain host compiler with -fsanitize=address,undefined -- no HIP header, nothing loaded into Python -- and
  * replays every launch recorded on an MI355X (tests/golden/launch_plans.txt, written by tools/record_launch_plans.py --plans): from the
    recorded inputs (the instantiation's facts, registers and occupancy per shape, workgroups, K, CUs, LDS limit, limiter settings) the
    planner must return the recorded shape, D, OW, LDS bytes, block ticks, tail ticks, first tail workgroup and resident count;
  * scripts the closed-loop calibration's decision step with made-up timings and checks what its comments promise.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gym_electric_motor_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "launch_plans.txt")


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_replay")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(REPO, "tests", "launch_plan_replay.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_pure_layer_includes_no_hip_header():
    src = open(os.path.join(CSRC, "gemx_launch_plan.hpp")).read()
    pure = src[:src.index("#ifdef __HIPCC__")]
    assert [ln.strip() for ln in pure.splitlines() if ln.lstrip().startswith("#include")] == ["#include <cstddef>", "#include <cstdint>"]
    assert all(name in pure for name in ("lds_bytes", "resident", "choose_shape", "builtin_target", "ticks_for", "pace_for", "cal_signature", "cal_turn"))


def test_recorded_launches_replay_to_the_recorded_plans(replay):
    rows = [ln for ln in open(GOLDEN) if ln.strip() and not ln.startswith("#")]
    shapes = {int(ln.split("->")[1].split()[0]) for ln in rows}
    assert len(rows) >= 100 and shapes >= {0, 1, 2, 3, 4, 6, 7}, (len(rows), shapes)  # every built shape of the pipelined kernel was planned
    assert any(ln.split("->")[1].split()[5] != "0" for ln in rows)  # ... and a shorter last round
    r = subprocess.run([replay, GOLDEN], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"replayed {len(rows)} rows, 0 unreadable, 0 differ" in r.stdout, r.stdout


def test_calibration_decisions(replay):
    r = subprocess.run([replay], capture_output=True, text=True)
    assert r.returncode == 0 and "calibration script: 0 failed" in r.stdout, r.stdout + r.stderr
