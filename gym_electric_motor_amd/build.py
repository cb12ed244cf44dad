"""Build the in-tree HIP libraries for gfx950 (explicit hipcc, no JIT cache).

Sources (gym_electric_motor_amd/csrc):
    gemx_common.hpp, gemx_kernels.hpp   device templates
    gemx_reward.hpp                     the WeightedSumOfErrors reward, once: description, checks, builder, the reward of one row (gemx_common.hpp includes it)
    gemx_unit_host.hpp                  the host code every dlopen'ed unit repeats: error sink, unit_init, (load, solver) dispatch, one-step map, KArgs
    gemx_launch_plan.hpp                how a fused rollout is launched (shape, LDS, rate limiter): a pure layer a host compiler builds, and the
                                        runtime queries behind it; host code only (gemx_kernels.hpp includes it)
    gemx_inst.hip                       ONE kernel unit, compiled once per (system, converter unit, dtype) into its OWN shared object
                                        libgemx_u<S>_<C>_<F>.so, which gemx_create loads with dlopen (round 6: a handle maps the C ABI and
                                        the one unit it runs, not all 38)
    gemx_capi.hip                       C ABI (include/gemx.h), validation, small kernels, unit loader  } libgemx.so
    gemx_support.hpp                    row tile in LDS and entry-point checks of the nine support units below (SUPPORT) }
    gemx_refgen.hip                     device-side reference generators: Wiener, the other kinds, switched (gemx_refgen_*) }
    gemx_obsproc.hip                    device-side observation stage (gemx_obsproc_*)                  }
    gemx_fluxobs.hip                    device-side FluxObserver and flux-oriented dq actions (gemx_fluxobs_*) }
    gemx_rewardpass.hip                 reward pass over a stored trajectory (gemx_reward_rows)         }
    gemx_statenoise.hip                 device-side StateNoiseProcessor: noise, done and reward on the noisy row (gemx_noise_*) }
    gemx_episode.hip                    device-side episode time limit and episode statistics (gemx_episode_*) }
    gemx_refprofile.hip                 device-side profile references: drive cycles per env (gemx_refprofile_*) }
    gemx_returns.hip                    discounted returns and GAE(lambda) over stored rollout rows (gemx_returns_rows) }
    gemx_policy_eval.hip                an MLPPolicy evaluated on every row of a stored policy rollout, with value / log-prob heads (gemx_policy_eval_rows) }
    gemx_envparams.hpp, gemx_envparams.hip   per-env motor / load / supply parameters: the two per-env kernels, compiled once per (system,
                                        converter unit), fp32, into libgemx_ep<S>_<C>.so, which gemx_set_env_params loads with dlopen
    gemx_envparams_dev.hpp              the device helpers the per-env units and the episodic units share (table column, row store, control step)
    gemx_episodic.hip                   K-step rollout with the episode time limit inside the launch: one kernel, with and without a parameter
                                        table, compiled once per (system, converter unit), fp32, into libgemx_tl<S>_<C>.so, which the first
                                        gemx_rollout_episodic of such a handle loads with dlopen
    gemx_policy_kernel.hpp              THE policy rollout kernel and its launcher: the episodic kernel with a device MLP actor in front of every
                                        step, with or without a reference generator in the lane; included by the two kinds of policy unit
    gemx_policy.hpp, gemx_policy.hip    the policy rollout: that kernel without a generator, compiled once per (system, converter unit), fp32,
                                        into libgemx_pl<S>_<C>.so, which the first gemx_rollout_policy of such a handle loads with dlopen
    gemx_policy_dev.hpp                 the actor's device helpers, shared by the policy kernel and gemx_policy_eval.hip
    gemx_refgen_lane.hpp, gemx_refprofile_lane.hpp   the per-lane functions of the all-Wiener and the profile generators, shared by their
                                        units of libgemx.so and the complete policy units
    gemx_policy_complete.hpp, gemx_policy_complete.hip   the policy rollout of the complete env: that kernel with the reference generators
                                        stepped in the lane, once per generator kind, compiled once per (system, converter unit), fp32, into
                                        libgemx_pc<S>_<C>.so, which the first gemx_rollout_policy_complete of such a handle loads with dlopen
    gemx_lookahead.hpp, gemx_lookahead.hip   one-step finite-control-set predictive control: the episodic kernel with every switching action
                                        tried one step ahead and scored with the env's reward, generators in the lane, compiled once per
                                        (system, FINITE converter unit), fp32, into libgemx_la<S>_<C>.so, which the first
                                        gemx_rollout_lookahead_complete of such a handle loads with dlopen
The 38 units (19 system/converter pairs x fp32, fp64), the 19 per-env units, the 19 episodic units, the 19 policy units, the 19 complete policy
units, the 8 lookahead units and the ten objects of libgemx.so are compiled in parallel.
"""
import concurrent.futures as cf
import glob
import hashlib
import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
# the support objects of libgemx.so beside the C ABI: (name, source, headers beside gemx_common.hpp, compile cost)
_PC_HEADERS = ["gemx_policy.hpp", "gemx_refgen_lane.hpp", "gemx_refprofile_lane.hpp", "gemx_policy_complete.hpp"]  # gemx_policy_complete.hpp and what it includes
_LANE_HEADERS = ["gemx_refgen_lane.hpp", "gemx_refprofile_lane.hpp"]  # gemx_support.hpp includes them: the two generator units' lane functions
SUPPORT = [("refgen", "gemx_refgen.hip", ["gemx_support.hpp"], 0.2), ("obsproc", "gemx_obsproc.hip", ["gemx_support.hpp"], 0.1),
           ("fluxobs", "gemx_fluxobs.hip", ["gemx_support.hpp"], 0.1), ("rewardpass", "gemx_rewardpass.hip", ["gemx_support.hpp"], 0.1),
           ("statenoise", "gemx_statenoise.hip", ["gemx_support.hpp"], 0.1), ("episode", "gemx_episode.hip", ["gemx_support.hpp"], 0.05),
           ("refprofile", "gemx_refprofile.hip", ["gemx_support.hpp"], 0.05), ("returns", "gemx_returns.hip", ["gemx_support.hpp"], 0.05),
           ("policy_eval", "gemx_policy_eval.hip", ["gemx_support.hpp", "gemx_policy.hpp", "gemx_policy_dev.hpp"], 0.1)]
SOURCES = [os.path.join(CSRC, f) for f in ["gemx_common.hpp", "gemx_reward.hpp", "gemx_kernels.hpp", "gemx_launch_plan.hpp", "gemx_unit_host.hpp", "gemx_inst.hip", "gemx_capi.hip", "gemx_support.hpp",
                                           "gemx_envparams.hpp", "gemx_envparams.hip", "gemx_envparams_dev.hpp", "gemx_episodic.hip", "gemx_policy.hpp", "gemx_policy.hip",
                                           "gemx_policy_dev.hpp", "gemx_policy_kernel.hpp", "gemx_refgen_lane.hpp", "gemx_refprofile_lane.hpp", "gemx_policy_complete.hpp", "gemx_policy_complete.hip",
                                           "gemx_lookahead.hpp", "gemx_lookahead.hip"] + [u[1] for u in SUPPORT]]
HEADER = os.path.join(REPO, "include", "gemx.h")
LIB = os.path.join(PKG_DIR, "libgemx.so")


def unit_lib(s, c, f64):
    """the shared object of one kernel unit (beside libgemx.so: gemx_capi.hip's load_unit looks there)"""
    return os.path.join(PKG_DIR, f"libgemx_u{s}_{c}_{int(f64)}.so")


def ep_unit_lib(s, c):
    """the shared object of one per-env-parameter unit (fp32 only; gemx_capi.hip's load_ep_unit looks beside libgemx.so)"""
    return os.path.join(PKG_DIR, f"libgemx_ep{s}_{c}.so")


def tl_unit_lib(s, c):
    """the shared object of one episodic rollout unit (fp32 only; gemx_capi.hip's load_tl_unit looks beside libgemx.so)"""
    return os.path.join(PKG_DIR, f"libgemx_tl{s}_{c}.so")


def pc_unit_lib(s, c):
    """the shared object of one complete policy rollout unit (fp32 only; gemx_capi.hip's load_pc_unit looks beside libgemx.so)"""
    return os.path.join(PKG_DIR, f"libgemx_pc{s}_{c}.so")


def la_unit_lib(s, c):
    """the shared object of one lookahead rollout unit (fp32, finite converters only; gemx_capi.hip's load_la_unit looks beside libgemx.so)"""
    return os.path.join(PKG_DIR, f"libgemx_la{s}_{c}.so")


def pl_unit_lib(s, c):
    """the shared object of one policy rollout unit (fp32 only; gemx_capi.hip's load_pl_unit looks beside libgemx.so)"""
    return os.path.join(PKG_DIR, f"libgemx_pl{s}_{c}.so")


OBJ_DIR = os.path.join(PKG_DIR, "build")
STAMP = LIB + ".sha256"  # next to the library (the object directory does not travel to the GPU box: .gpurunignore)

# (system_kind, converter_kind) pairs on the accelerated path; each for fp32 (0) and fp64 (1)
UNITS = [(0, 0), (1, 1), (1, 2), (2, 1), (2, 2), (0, 3), (3, 0), (3, 3), (4, 0), (4, 3), (5, 4), (5, 5), (6, 6), (6, 7), (7, 8), (7, 9), (1, 10), (2, 10), (6, 11)]
FINITE_CONVERTERS = (1, 3, 5, 7, 9)  # GEMX_CONV_FINITE_*: the converter units with a finite action set (ConvTraits<...>::DISCRETE)
LA_UNITS = [(s, c) for s, c in UNITS if c in FINITE_CONVERTERS]  # the lookahead units: a continuous converter has no action set to enumerate
# --offload-compress: the gfx950 code objects are stored zstd-compressed in the shared objects (the HIP runtime inflates them when a library
# is loaded): 144 MB of libraries -> ~20 MB pushed to every GPU lease, nothing else changes
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-fPIC", "-Wno-unused-variable", "--offload-compress"]


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build gym_electric_motor_amd/libgemx.so")


def _digest(sources=None, header=None):
    h = hashlib.sha256()
    for p in (SOURCES if sources is None else sources) + [header or HEADER]:
        h.update(open(p, "rb").read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


# what each kind of object is compiled from (an edit to the C ABI alone does not recompile the 38 kernel units)
_COMMON = ["gemx_common.hpp", "gemx_reward.hpp"]  # every object (gemx_common.hpp includes gemx_reward.hpp)
_UNIT = _COMMON + ["gemx_kernels.hpp", "gemx_launch_plan.hpp", "gemx_unit_host.hpp"]  # every dlopen'ed unit
_DEPS = {"inst": _UNIT + ["gemx_inst.hip"], "capi": _COMMON + ["gemx_envparams.hpp"] + _PC_HEADERS + ["gemx_lookahead.hpp", "gemx_capi.hip"],
         "envparams": _UNIT + ["gemx_envparams.hpp", "gemx_envparams_dev.hpp", "gemx_envparams.hip"],
         "episodic": _UNIT + ["gemx_envparams.hpp", "gemx_envparams_dev.hpp", "gemx_episodic.hip"],
         "policy": _UNIT + ["gemx_envparams.hpp", "gemx_envparams_dev.hpp", "gemx_policy.hpp", "gemx_policy_dev.hpp", "gemx_policy_kernel.hpp", "gemx_policy.hip"],
         "policy_complete": _UNIT + ["gemx_envparams.hpp", "gemx_envparams_dev.hpp", "gemx_policy_dev.hpp", "gemx_policy_kernel.hpp"] + _PC_HEADERS +
                            ["gemx_support.hpp", "gemx_refprofile.hip", "gemx_policy_complete.hip"],  # (gemx_refprofile.hip: its head section, the one definition of profile_row)
         "lookahead": _UNIT + ["gemx_envparams.hpp", "gemx_envparams_dev.hpp"] + _PC_HEADERS + ["gemx_lookahead.hpp", "gemx_support.hpp", "gemx_refprofile.hip", "gemx_lookahead.hip"],
         **{name: _COMMON + headers + _LANE_HEADERS + [src] for name, src, headers, _ in SUPPORT}}
# compile cost of an fp32 unit by system kind (object size, MB: induction > synchronous > DC); fp64 units take the single-wave kernel only
_COST = {7: 6.0, 2: 5.3, 6: 4.9, 1: 4.5, 5: 4.0, 4: 3.9, 3: 3.5, 0: 3.5}


def all_libs():
    return [LIB] + [unit_lib(s, c, f) for s, c in UNITS for f in (0, 1)]


def ep_libs():
    """the per-env-parameter units (one per system/converter pair, fp32)"""
    return [ep_unit_lib(s, c) for s, c in UNITS]


def tl_libs():
    """the episodic rollout units (one per per-env unit: the same system/converter pairs, fp32)"""
    return [tl_unit_lib(s, c) for s, c in UNITS]


def pl_libs():
    """the policy rollout units (one per episodic unit: the same system/converter pairs, fp32)"""
    return [pl_unit_lib(s, c) for s, c in UNITS]


def pc_libs():
    """the complete policy rollout units (one per policy unit: the same system/converter pairs, fp32)"""
    return [pc_unit_lib(s, c) for s, c in UNITS]


def la_libs():
    """the lookahead rollout units (one per system/converter pair with a finite converter, fp32)"""
    return [la_unit_lib(s, c) for s, c in LA_UNITS]


def is_stale():
    if not os.path.exists(STAMP) or not all(os.path.exists(p) for p in all_libs() + ep_libs() + tl_libs() + pl_libs() + pc_libs() + la_libs()):
        return True
    return open(STAMP).read().strip() != _digest()


def build_library(force=False, verbose=False, jobs=None):
    """hipcc --offload-arch=gfx950 -> gym_electric_motor_amd/libgemx.so (cross-compiles without a GPU)."""
    if not force and not is_stale():
        return LIB
    hipcc = hipcc_path()
    os.makedirs(OBJ_DIR, exist_ok=True)
    # ONE build at a time (a CPU test calls build() too: two builds racing for the snapshot directory and the objects produce garbage);
    # a second caller waits here and then finds the objects the first one made
    import fcntl

    lock = open(os.path.join(OBJ_DIR, ".build.lock"), "w")
    fcntl.flock(lock, fcntl.LOCK_EX)
    try:
        if not force and not is_stale():
            return LIB
        return _build_locked(hipcc, force, verbose, jobs)
    finally:
        fcntl.flock(lock, fcntl.LOCK_UN)
        lock.close()


def _build_locked(hipcc, force, verbose, jobs):
    # compile from a SNAPSHOT of the sources taken now: a full build runs for minutes with the units starting at different times, and an
    # edit of a header in between would otherwise give objects of two different versions of it (and a stamp that matches neither)
    snap = os.path.join(OBJ_DIR, "src_snapshot")
    shutil.rmtree(snap, ignore_errors=True)
    os.makedirs(snap)
    for f in SOURCES + [HEADER]:
        shutil.copy2(f, snap)
    snap_sources = [os.path.join(snap, os.path.basename(f)) for f in SOURCES]
    snap_header = os.path.join(snap, os.path.basename(HEADER))
    csrc = snap
    inc = ["-I" + snap]
    cmds = []  # (output, command, kind, cost)
    for s, c in UNITS:
        for f64 in (0, 1):
            out = unit_lib(s, c, f64)
            cmds.append((out, [hipcc] + FLAGS + inc + [f"-DGEMX_INST_SYS={s}", f"-DGEMX_INST_CONV={c}", f"-DGEMX_INST_F64={f64}", "-fvisibility=hidden",
                                                      "-shared", os.path.join(csrc, "gemx_inst.hip"), "-o", out], "inst", _COST[s] * (0.15 if f64 else 1.0)))
    for s, c in UNITS:  # the per-env units: two single-wave kernels per (load, solver), seconds each
        out = ep_unit_lib(s, c)
        cmds.append((out, [hipcc] + FLAGS + inc + [f"-DGEMX_INST_SYS={s}", f"-DGEMX_INST_CONV={c}", "-fvisibility=hidden", "-shared",
                                                  os.path.join(csrc, "gemx_envparams.hip"), "-o", out], "envparams", 0.05))
    for s, c in UNITS:  # the episodic units: one single-wave kernel per (load, solver), with and without a table
        out = tl_unit_lib(s, c)
        cmds.append((out, [hipcc] + FLAGS + inc + [f"-DGEMX_INST_SYS={s}", f"-DGEMX_INST_CONV={c}", "-fvisibility=hidden", "-shared",
                                                  os.path.join(csrc, "gemx_episodic.hip"), "-o", out], "episodic", 0.05))
    for s, c in UNITS:  # the policy units: the episodic kernel with the actor in front of every step
        out = pl_unit_lib(s, c)
        cmds.append((out, [hipcc] + FLAGS + inc + [f"-DGEMX_INST_SYS={s}", f"-DGEMX_INST_CONV={c}", "-fvisibility=hidden", "-shared",
                                                  os.path.join(csrc, "gemx_policy.hip"), "-o", out], "policy", 0.1))
    for s, c in UNITS:  # the complete policy units: the policy kernel with the generators in the lane, once per generator kind
        out = pc_unit_lib(s, c)
        cmds.append((out, [hipcc] + FLAGS + inc + [f"-DGEMX_INST_SYS={s}", f"-DGEMX_INST_CONV={c}", "-fvisibility=hidden", "-shared",
                                                  os.path.join(csrc, "gemx_policy_complete.hip"), "-o", out], "policy_complete", 0.2))
    for s, c in LA_UNITS:  # the lookahead units: the episodic kernel around a rolled loop over the actions, once per generator kind
        out = la_unit_lib(s, c)
        cmds.append((out, [hipcc] + FLAGS + inc + [f"-DGEMX_INST_SYS={s}", f"-DGEMX_INST_CONV={c}", "-fvisibility=hidden", "-shared",
                                                  os.path.join(csrc, "gemx_lookahead.hip"), "-o", out], "lookahead", 0.1))
    objects = []  # of libgemx.so
    for name, src, cost in [("capi", "gemx_capi.hip", 0.3)] + [(u[0], u[1], u[3]) for u in SUPPORT]:
        obj = os.path.join(OBJ_DIR, os.path.splitext(src)[0] + ".o")
        objects.append(obj)
        cmds.append((obj, [hipcc] + FLAGS + inc + ["-c", os.path.join(csrc, src), "-o", obj], name, cost))
    digests = {k: _digest([os.path.join(csrc, f) for f in v], snap_header) for k, v in _DEPS.items()}

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    def compile_one(job):  # skipped when the object was built from the same sources with the same flags
        obj, cmd, kind, _ = job
        stamp = os.path.join(OBJ_DIR, os.path.basename(obj) + ".sha256")
        if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read().strip() == digests[kind]:
            return
        run(cmd)
        with open(stamp, "w") as fh:
            fh.write(digests[kind])

    jobs = jobs or min(len(cmds), os.cpu_count() or 4)
    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:  # longest first: the big induction-machine units do not end up as the tail
        list(ex.map(compile_one, sorted(cmds, key=lambda j: -j[3])))
    run([hipcc, "--offload-arch=gfx950", "--offload-compress", "-shared", "-fPIC", "-o", LIB] + objects + ["-ldl"])
    for stale in glob.glob(os.path.join(PKG_DIR, "libgemx_u*.so")) + glob.glob(os.path.join(PKG_DIR, "libgemx_ep*.so")) + glob.glob(os.path.join(PKG_DIR, "libgemx_tl*.so")) + glob.glob(os.path.join(PKG_DIR, "libgemx_pl*.so")) + glob.glob(os.path.join(PKG_DIR, "libgemx_pc*.so")) + glob.glob(os.path.join(PKG_DIR, "libgemx_la*.so")):  # a unit that is no longer in UNITS must not be found by dlopen
        if stale not in [j[0] for j in cmds]:
            os.remove(stale)
    with open(STAMP, "w") as fh:
        fh.write(_digest(snap_sources, snap_header))  # (of what was compiled: an edit made meanwhile leaves the library stale, as it should)
    return LIB
