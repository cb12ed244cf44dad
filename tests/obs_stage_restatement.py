"""Plain numpy restatement of what the reference's observation-side wrappers do to a state in `simulate()`, one processor at a time,
each seeing the names of what is beneath it (current_sum_processor.py:51-65, cos_sin_processor.py:57-89), followed by the env shell's
state filter (core.py:366).  It neither imports the reference nor the product's ObservationStage: the tests compare the two with it.

A chain is a list of specs as recorded in tests/golden/obs_stage/metadata.json:
    {"kind": "CurrentSumProcessor", "currents": [...], "limit": "max" | "sum"}
    {"kind": "CosSinProcessor", "angle": "epsilon", "remove_angle": bool}
"""
import numpy as np


def wrapped_names(names, chain):
    names = list(names)
    for spec in chain:
        if spec["kind"] == "CurrentSumProcessor":
            names = names + ["i_sum"]
        else:
            if spec["remove_angle"]:
                names = [n for i, n in enumerate(names) if i != names.index(spec["angle"])]
            names = names + [f"cos({spec['angle']})", f"sin({spec['angle']})"]
    return names


def simulate_chain(state, names, chain, state_filter=None, dtype=np.float64):
    """state [..., len(names)] of the inner system -> the wrapped system's state (then filtered), computed in `dtype` with the current
    sum added sequentially in ascending column order (numpy's own order for so few summands)."""
    s = np.asarray(state, dtype=dtype)
    names = list(names)
    for spec in chain:
        if spec["kind"] == "CurrentSumProcessor":
            idx = sorted(names.index(c) for c in spec["currents"])
            acc = s[..., idx[0]].copy()
            for j in idx[1:]:
                acc = (acc + s[..., j]).astype(dtype)
            s = np.concatenate((s, acc[..., None]), axis=-1)
            names = names + ["i_sum"]
        elif spec["kind"] == "CosSinProcessor":
            i = names.index(spec["angle"])
            x = s[..., i].astype(np.float64) * np.pi
            ext = np.stack((np.cos(x), np.sin(x)), axis=-1).astype(dtype)
            if spec["remove_angle"]:
                s = np.delete(s, i, axis=-1)
                names = names[:i] + names[i + 1:]
            s = np.concatenate((s, ext), axis=-1)
            names = names + [f"cos({spec['angle']})", f"sin({spec['angle']})"]
        else:
            raise ValueError(spec)
    if state_filter is not None:
        s = s[..., list(state_filter)]
    return s
