"""The recorded runs of the reference's FluxObserver and flux-oriented dq processors (tools/record_flux_goldens.py -> tests/golden/flux/flux_*.npz)
and how to build the same env from this package's holders."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flux")
CASES = ("flux_scim_abc", "flux_scim_dq", "flux_scim_dq_deadtime", "flux_dfim_dq")
DQ_CASES = CASES[1:]
# the runs away from the reference's default machine (the recorder's PARAM_CASES): three runs per file, on a leading axis
PARAM_CASES = ("flux_param_scim_abc", "flux_param_scim_dq_dead2", "flux_param_dfim_dq", "flux_scim_abc_perm")
PARAM_DQ_CASES = PARAM_CASES[1:3]
N_RUNS = 3
RUNS = tuple(f"{c}-run{r}" for c in PARAM_CASES for r in range(N_RUNS))  # one run: load_any("flux_param_scim_abc-run1")
DQ_RUNS = tuple(r for r in RUNS if r.rsplit("-run", 1)[0] in PARAM_DQ_CASES)
_PER_RUN = ("actions", "abc_actions", "state", "terminated")


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    d["meta"] = json.loads(str(d["meta"]))
    d["state_names"] = [str(n) for n in d["state_names"]]
    assert int(d["terminated"].sum()) >= 2, f"{name}: the recorded run must contain at least two terminations"
    return d


def episode_lengths(terminated):
    ends = np.nonzero(np.asarray(terminated))[0]
    return np.diff(np.concatenate([[-1], ends, [len(terminated) - 1]]))


@functools.lru_cache(maxsize=None)
def load_runs(name):
    """The runs of one PARAM_CASES fixture, each shaped like what `load` returns (the system's arrays and the meta are shared; nobody
    writes to them).  Asserts what the recorder asserted when it wrote the file."""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    meta = d["meta"] = json.loads(str(d["meta"]))
    d["state_names"] = [str(n) for n in d["state_names"]]
    ov = meta["overrides"]
    mp = ov.get("motor", {}).get("motor_parameter")
    assert meta["seeds"] == [7, 8, 9] and meta["solver"] == "euler" and d["state"].shape[:2] == (N_RUNS, 200)
    if "_param_" in name:
        assert mp["l_sigs"] != mp["l_sigr"], f"{name}: a `param` case needs l_sigs != l_sigr"
    if any(c.startswith("DqToAbc") for c in meta["chain"]):
        advance = (0.5 + meta["dead_time"]) * meta["tau"] * abs(ov["load"]["omega_fixed"]) * mp["p"]
        assert advance >= 0.02, f"{name}: an angle advance of {advance} rad"
    runs = []
    for r in range(N_RUNS):
        term = d["terminated"][r]
        assert int(term.sum()) >= 2, f"{name}, run {r}: the recorded run must contain at least two terminations"
        assert int(episode_lengths(term).max()) >= 30, f"{name}, run {r}: the longest episode must have at least 30 steps"
        runs.append({k: (v[r] if k in _PER_RUN else v) for k, v in d.items()})
    return tuple(runs)


def load_any(case):
    """A CASES name, or one run of a PARAM_CASES fixture as RUNS spells it."""
    name, sep, r = case.rpartition("-run")
    return load_runs(name)[int(r)] if sep else load(case)


def make_kwargs(d):
    """The make-kwargs the run was recorded with, exactly as the reference was handed them (a fresh copy; none for CASES)."""
    return json.loads(json.dumps(d["meta"].get("overrides", {})))


def holders(ga, chain):
    out = []
    for spec in chain:
        kind, _, arg = spec.partition(":")
        if kind == "FluxObserver":  # "FluxObserver" | "FluxObserver:i_sb,i_sc,i_sa"
            out.append(ga.FluxObserver(tuple(arg.split(","))) if arg else ga.FluxObserver())
        elif kind == "DeadTimeProcessor":
            out.append(ga.DeadTimeProcessor(int(arg)))
        else:
            out.append(ga.FluxOrientedDqToAbcActionProcessor(arg))
    return tuple(out)
