"""The recorded runs of the reference's FluxObserver and flux-oriented dq processors (tools/record_flux_goldens.py -> tests/golden/flux/flux_*.npz)
and how to build the same env from this package's holders."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flux")
CASES = ("flux_scim_abc", "flux_scim_dq", "flux_scim_dq_deadtime", "flux_dfim_dq")
DQ_CASES = CASES[1:]


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    d["meta"] = json.loads(str(d["meta"]))
    d["state_names"] = [str(n) for n in d["state_names"]]
    assert int(d["terminated"].sum()) >= 2, f"{name}: the recorded run must contain at least two terminations"
    return d


def holders(ga, chain):
    out = []
    for spec in chain:
        kind, _, arg = spec.partition(":")
        if kind == "FluxObserver":
            out.append(ga.FluxObserver())
        elif kind == "DeadTimeProcessor":
            out.append(ga.DeadTimeProcessor(int(arg)))
        else:
            out.append(ga.FluxOrientedDqToAbcActionProcessor(arg))
    return tuple(out)
