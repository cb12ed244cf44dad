"""`_lib.bound_call` / `_lib.sequence`: the one pre-bound launcher every bind_* of the package returns.  No device: a Python stand-in
for the FFI function and a stub owner."""
import gc
import weakref


class _Owner:
    _handle = "handle"


class _Kept:
    pass


def test_bound_call(monkeypatch):
    from gym_electric_motor_amd import _lib

    seen, checked, rc = [], [], [0]

    def fn(*a):
        seen.append(a)
        return rc[0]

    monkeypatch.setattr(_lib, "check", checked.append)
    owner, kept, result = _Owner(), _Kept(), object()
    alive = weakref.ref(kept)
    launch = _lib.bound_call(fn, owner, (1, None, "x"), (kept,), result)
    del kept
    gc.collect()
    assert launch() is result and seen == [("handle", 1, None, "x")] and checked == []  # status 0 does not reach check
    assert alive() is not None  # `keep` lives as long as the launcher does
    owner._handle = None  # a closed owner: the handle is read per call, the C ABI sees the null handle
    assert launch() is result and seen[-1] == (None, 1, None, "x")
    rc[0] = -2
    assert launch() is result and checked == [-2]
    assert _lib.bound_call(fn, owner, ())() is None and seen[-1] == (None,)
    del launch
    gc.collect()
    assert alive() is None


def test_sequence():
    from gym_electric_motor_amd import _lib

    order = []
    a, b = (lambda: order.append("a")), (lambda: order.append("b"))
    assert _lib.sequence() is None and _lib.sequence(None, None) is None
    assert _lib.sequence(None, a) is a  # one launcher, no result: no frame around it
    result = object()
    assert _lib.sequence(a, None, b, result=result)() is result and order == ["a", "b"]
    assert _lib.sequence(b, result=result)() is result and order == ["a", "b", "b"]
    assert _lib.sequence(b, a)() is None and order[-2:] == ["b", "a"]
