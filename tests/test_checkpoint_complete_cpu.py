"""The complete env's checkpoint, the parts that need no device: the header's three new prototypes against `_lib.py`'s symbol list and
argtypes, the ABI number, the blob size formula against the table of lane arrays in csrc/gemx_refgen.hip and the header's comment, and
the refusals `set_checkpoint` makes before it touches a device.  (The restore itself: tests/test_gpu_checkpoint_complete.py.)"""
import ctypes as C
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HEADER = open(os.path.join(REPO, "include", "gemx.h")).read()
SOURCE = open(os.path.join(REPO, "gym_electric_motor_amd", "csrc", "gemx_refgen.hip")).read()
NEW = ("gemx_refgen_state_bytes", "gemx_refgen_get_blob", "gemx_refgen_set_blob")


def _prototypes():
    """name -> (return type, [parameter declarations]) of the three entry points, from the header."""
    out = {}
    for ret, name, params in re.findall(r"^(int|int64_t) (gemx_refgen_(?:state_bytes|get_blob|set_blob))\(([^)]*)\);", HEADER, flags=re.M):
        out[name] = (ret, [p.strip() for p in params.split(",")])
    return out


def test_prototypes_exports_and_argtypes_agree():
    import __graft_entry__ as g
    from gym_electric_motor_amd import _lib

    protos = _prototypes()
    assert set(protos) == set(NEW)
    assert protos["gemx_refgen_state_bytes"] == ("int64_t", ["gemx_refgen *r"])
    assert protos["gemx_refgen_get_blob"] == ("int", ["gemx_refgen *r", "void *out_dev", "void *stream"])
    assert protos["gemx_refgen_set_blob"] == ("int", ["gemx_refgen *r", "const void *in_dev", "void *stream"])
    assert set(NEW) <= set(_lib.EXPORTS) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    for name in NEW:  # defined in the source with the header's signature
        ret, params = protos[name]
        assert re.search(rf"^{ret} {name}\({re.escape(', '.join(params))}\) \{{", SOURCE, flags=re.M), name
    g.build()
    L = _lib.load()
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params) and all(t is C.c_void_p for t in fn.argtypes), name
        assert fn.restype is (C.c_int64 if ret == "int64_t" else C.c_int), name
    # a null handle is refused with a message, no device is looked for
    assert L.gemx_refgen_state_bytes(None) == 0
    assert L.gemx_refgen_get_blob(None, None, None) == -1 and b"null" in L.gemx_last_error()
    assert L.gemx_refgen_set_blob(None, None, None) == -1 and b"null" in L.gemx_last_error()


def test_abi_number_stays():
    """Entry points only: no struct changed, so the number that guards the structs' layout stays 9."""
    from gym_electric_motor_amd import _lib

    assert _lib.ABI_VERSION == 9 and re.search(r"^#define GEMX_ABI_VERSION 9\b", HEADER, flags=re.M)


def _table():
    """The rows of refgen_lane_arrays: [(member, bytes per lane, owner)], in the table's order."""
    body = SOURCE[SOURCE.index("const LaneArrayRow rows[] = {"):]
    body = body[:body.index("};")]
    n_par = int(re.search(r"N_PAR = (\d+)", SOURCE).group(1))
    rows = re.findall(r"\{\(void \*\*\)&r->(\w+), ([^,]+), (OWN_\w+)\}", body)
    return [(m, eval(b, {"N_PAR": n_par}), o) for m, b, o in rows]  # noqa: S307  (the table's own arithmetic: "8 * N_PAR")


def test_blob_size_formula_is_the_table():
    from gym_electric_motor_amd import _lib

    rows = _table()
    assert [m for m, _, _ in rows] == ["value", "sigma", "left", "n_sub", "n_reset", "t", "len", "par", "alt", "sk", "slen", "n_super"]
    by_owner = {o: tuple(b for _, b, own in rows if own == o) for o in ("OWN_ALL", "OWN_KINDS", "OWN_SWITCHED")}
    assert by_owner == dict(OWN_ALL=_lib.REFGEN_LANE_BYTES["all"], OWN_KINDS=_lib.REFGEN_LANE_BYTES["kinds"], OWN_SWITCHED=_lib.REFGEN_LANE_BYTES["switched"])
    # the owners come in the table in the order the blob's groups are documented in: every handle, + kinds, + switched
    assert [o for _, _, o in rows] == ["OWN_ALL"] * 6 + ["OWN_KINDS"] * 2 + ["OWN_SWITCHED"] * 4
    # the header's comment states the same widths
    comment = HEADER[HEADER.index("Checkpoint of a handle's whole device state"):HEADER.index("#define GEMX_REFGEN_BLOB_HEADER_BYTES")]
    stated = [(m, int(b)) for m, b in re.findall(r"\b(value|sigma|left|n_sub|n_reset|t|len|par|alt|sk|slen|n_super) (\d+)", comment)]
    assert stated == [(m, b) for m, b, _ in rows]
    head = int(re.search(r"#define GEMX_REFGEN_BLOB_HEADER_BYTES (\d+)", HEADER).group(1))
    assert head == _lib.REFGEN_BLOB_HEADER_BYTES == 64
    pad = lambda b: (b + 7) // 8 * 8  # noqa: E731
    for n, n_ref in ((1, 1), (35, 1), (35, 3), (70, 2), (70, 4), (4096, 4)):  # (35 lanes: the 4-byte sections need their padding)
        lanes = n * n_ref
        want = {(False, False): by_owner["OWN_ALL"], (True, False): by_owner["OWN_ALL"] + by_owner["OWN_KINDS"],
                (True, True): by_owner["OWN_ALL"] + by_owner["OWN_KINDS"] + by_owner["OWN_SWITCHED"]}
        for (kinds, switched), widths in want.items():
            assert _lib.refgen_state_bytes(n, n_ref, kinds=kinds, switched=switched) == head + sum(pad(lanes * b) for b in widths), (n, n_ref, kinds, switched)
    assert _lib.refgen_state_bytes(35, 1) == 64 + 280 + 280 + 3 * 144 + 280
    assert _lib.refgen_state_bytes(2, 1, switched=True) == _lib.refgen_state_bytes(2, 1, kinds=True, switched=True)  # (a switched handle is a kinds handle)


def test_refusals_before_any_device():
    """`set_checkpoint` of an env that never created a handle: a checkpoint that lacks an entry this env reads raises, and names it."""
    import gym_electric_motor_amd as ga

    env = ga.make("Cont-CC-PMSM-v0", n_envs=8, reference_generator="default", max_episode_steps=4, _defer_create=True)
    physics = dict(state=None, switch_state=None, aux=None, k=0)
    with pytest.raises(ValueError, match="episodes"):
        env.set_checkpoint(physics)
    with pytest.raises(ValueError, match="reference_generator"):
        env.set_checkpoint(dict(physics, episodes=dict()))
    with pytest.raises(ValueError, match="aux"):
        env.set_checkpoint(dict(reference_generator=dict()))
    plain = ga.make("Cont-CC-PMSM-v0", n_envs=8, _defer_create=True)
    assert plain._checkpoint_keys() == [] and env._checkpoint_keys() == ["episodes"]
    for doc, words in (("README.md", "reference_generator"), ("INTEGRATION.md", "gemx_refgen_get_blob")):
        assert words in open(os.path.join(REPO, doc)).read(), doc
