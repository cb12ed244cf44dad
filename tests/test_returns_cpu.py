"""Device-side returns and GAE without a GPU: the numpy restatement of the row function against the textbook sums, its chunk property,
the agreement of header, binding and build list, and every ValueError of the Python surface on host tensors."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)  # (sibling module: the restatement)

GAMMA_LAM = [(0.99, 0.95), (0.0, 0.5), (0.9, 0.0), (1.0, 1.0), (0.5, 1.0), (1.0, 0.0), (0.0, 0.0)]


def _masks(K, N, rng):
    """ended / terminated [K, N] with, over the envs: no end, every row ended, an end at row 0, at row K-1, at both, two consecutive ended
    rows, and random ends; every second end is a truncation."""
    ended = np.zeros((K, N), np.uint8)
    ended[:, 1] = 1
    ended[0, 2] = 1
    ended[K - 1, 3] = 1
    ended[0, 4] = ended[K - 1, 4] = 1
    ended[K // 2, 5] = ended[min(K // 2 + 1, K - 1), 5] = 1
    ended[:, 6:] = rng.random((K, N - 6)) < 0.3
    truncated = ended & (rng.random((K, N)) < 0.5)
    truncated[0, 2], truncated[K - 1, 3] = 1, 0  # (both kinds at the edge rows)
    truncated[0, 4], truncated[K - 1, 4] = 0, 1
    return ended, (ended & ~truncated).astype(np.uint8)


def _textbook_gae(reward, value, terminated, ended, gamma, lam, last_value, final_value, carry_in):
    """A_k = sum_l (gamma lam)^l delta_{k+l} up to the row where the episode ends; beyond row K-1 the sum continues in carry_in."""
    K, N = reward.shape
    adv = np.zeros((K, N))
    for i in range(N):
        delta = np.zeros(K)
        for j in range(K):
            if ended[j, i]:
                nxt = final_value[j, i] if (final_value is not None and not terminated[j, i]) else 0.0
            else:
                nxt = value[j + 1, i] if j + 1 < K else last_value[i]
            delta[j] = reward[j, i] + gamma * nxt - value[j, i]
        for k in range(K):
            total, l = 0.0, 0
            while True:
                total += (gamma * lam) ** l * delta[k + l]
                if ended[k + l, i]:
                    break
                l += 1
                if k + l == K:
                    total += (gamma * lam) ** l * carry_in[i]
                    break
            adv[k, i] = total
    return adv


def _textbook_returns(reward, ended, gamma, seed):
    K, N = reward.shape
    ret = np.zeros((K, N))
    for i in range(N):
        for k in range(K):
            total, l = 0.0, 0
            while True:
                total += gamma ** l * reward[k + l, i]
                if ended[k + l, i]:
                    break
                l += 1
                if k + l == K:
                    total += gamma ** l * seed[i]
                    break
            ret[k, i] = total
    return ret


@pytest.mark.parametrize("K", [1, 2, 7])
@pytest.mark.parametrize("gamma,lam", GAMMA_LAM)
def test_restatement_against_textbook_sums(K, gamma, lam):
    import returns_restatement as rr

    N = 12
    rng = np.random.default_rng(K * 100 + int(gamma * 10) + int(lam * 7))
    ended, terminated = _masks(K, N, rng)
    reward, value, final_value = (rng.normal(size=(K, N)) for _ in range(3))
    last_value, carry_in = rng.normal(size=N), rng.normal(size=N)
    for fv in (final_value, None):  # truncated rows with and without final_value (without: treated as terminated)
        adv, ret, carry = rr.gae(reward, value, terminated, gamma, lam, last_value=last_value, ended=ended, final_value=fv, carry_in=carry_in)
        want = _textbook_gae(reward, value, terminated, ended, gamma, lam, last_value, fv, carry_in)
        scale = np.abs(want).max()
        assert np.abs(adv - want).max() <= 1e-12 * scale
        assert np.abs(ret - (want + value)).max() <= 1e-12 * max(scale, np.abs(want + value).max())
        assert np.array_equal(carry, adv[0])
    # absent optional tensors are zeros / terminated
    zero = np.zeros(N)
    adv, _, _ = rr.gae(reward, value, terminated, gamma, lam)
    want = _textbook_gae(reward, value, terminated, terminated, gamma, lam, zero, None, zero)
    assert np.abs(adv - want).max() <= 1e-12 * np.abs(want).max()
    # the return-to-go, seeded by last_value or by carry_in
    for kw in (dict(last_value=last_value), dict(carry_in=carry_in), dict()):
        ret, carry = rr.discounted(reward, terminated, gamma, ended=ended, **kw)
        want = _textbook_returns(reward, ended, gamma, next(iter(kw.values()), zero))
        assert np.abs(ret - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(carry, ret[0])


def test_truncation_without_final_value_is_termination():
    import returns_restatement as rr

    rng = np.random.default_rng(5)
    K, N = 6, 12
    ended, terminated = _masks(K, N, rng)
    reward, value = rng.normal(size=(K, N)), rng.normal(size=(K, N))
    a = rr.gae(reward, value, terminated, 0.9, 0.8, ended=ended)
    b = rr.gae(reward, value, ended, 0.9, 0.8)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # final_value is looked at only where a row is truncated: NaN everywhere else changes nothing
    fv = rng.normal(size=(K, N))
    masked = np.where((ended != 0) & (terminated == 0), fv, np.nan)
    a = rr.gae(reward, value, terminated, 0.9, 0.8, ended=ended, final_value=fv)
    b = rr.gae(reward, value, terminated, 0.9, 0.8, ended=ended, final_value=masked)
    assert all(np.array_equal(x, y) and np.isfinite(x).all() for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chunked_restatement_is_one_scan(dtype):
    """Rows [K/2, K) and then rows [0, K/2) with carry_out -> carry_in and last_value = value[K/2]: one scan, bit for bit."""
    import returns_restatement as rr

    rng = np.random.default_rng(11)
    K, N = 9, 12
    h = K // 2
    ended, terminated = _masks(K, N, rng)
    reward, value, fv = (rng.normal(size=(K, N)).astype(dtype) for _ in range(3))
    last_value, carry_in = rng.normal(size=N).astype(dtype), rng.normal(size=N)
    adv, ret, carry = rr.gae(reward, value, terminated, 0.97, 0.9, last_value=last_value, ended=ended, final_value=fv, carry_in=carry_in)
    a1, r1, c1 = rr.gae(reward[h:], value[h:], terminated[h:], 0.97, 0.9, last_value=last_value, ended=ended[h:], final_value=fv[h:], carry_in=carry_in)
    a0, r0, c0 = rr.gae(reward[:h], value[:h], terminated[:h], 0.97, 0.9, last_value=value[h], ended=ended[:h], final_value=fv[:h], carry_in=c1)
    assert np.array_equal(np.concatenate([a0, a1]), adv) and np.array_equal(np.concatenate([r0, r1]), ret) and np.array_equal(c0, carry)
    ret, carry = rr.discounted(reward, terminated, 0.97, last_value=last_value, ended=ended)
    r1, c1 = rr.discounted(reward[h:], terminated[h:], 0.97, last_value=last_value, ended=ended[h:])
    r0, c0 = rr.discounted(reward[:h], terminated[:h], 0.97, ended=ended[:h], carry_in=c1)
    assert np.array_equal(np.concatenate([r0, r1]), ret) and np.array_equal(c0, carry)


def test_build_and_header_agree_with_the_binding():
    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd import _lib, build, returns

    assert os.path.join(build.CSRC, "gemx_returns.hip") in build.SOURCES
    assert ("returns", "gemx_returns.hip", ["gemx_support.hpp"]) in [u[:3] for u in build.SUPPORT]
    src = open(os.path.join(build.CSRC, "gemx_returns.hip")).read()
    assert re.findall(r'#include [<"]([^>"]+)[>"]', src) == ["gemx_support.hpp"]
    header = open(build.HEADER).read()
    assert re.search(r"#define GEMX_ABI_VERSION 9\b", header) and _lib.ABI_VERSION == 9  # new struct and entry point only
    assert "gemx_returns_rows" in _lib.EXPORTS and re.search(r"\bint gemx_returns_rows\(", header) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    # the struct, laid out by C's rules from the header's own field list
    m = re.search(r"typedef struct gemx_returns_config \{(.*?)\} gemx_returns_config;", header, re.S)
    fields = re.findall(r"^\s*(int32_t|double) (\w+);", m.group(1), re.M)
    assert [f[1] for f in fields] == [f[0] for f in _lib.GemxReturnsConfig._fields_] == ["struct_size", "gamma", "lam", "flags"]
    offset, offsets = 0, {}
    for ctype, name in fields:
        size = {"int32_t": 4, "double": 8}[ctype]
        offset = -(-offset // size) * size
        offsets[name] = offset
        offset += size
    size = -(-offset // 8) * 8
    assert size == C.sizeof(_lib.GemxReturnsConfig) == 32
    assert offsets == {name: getattr(_lib.GemxReturnsConfig, name).offset for name in offsets}
    # the entry point's arguments: the config, n_envs, K, dtype, device, ten tensors, the stream
    proto = re.search(r"int gemx_returns_rows\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == 16
    # ONE row function, called from one place, without contraction; the group depth the tests are built around
    assert len(re.findall(r"ReturnsOut returns_row\(", src)) == 1 and len(re.findall(r"= returns_row\(", src)) == 1
    assert "__dmul_rn" in src and "__dadd_rn" in src and "fp contract(off)" in src
    assert int(re.search(r"constexpr int GROUP_ROWS = (\d+);", src).group(1)) == returns.GROUP_ROWS == 16
    for name in ("advantages", "discounted_returns", "bind_advantages", "bind_discounted_returns"):
        assert getattr(ga, name) is getattr(returns, name)


def test_value_errors_on_host_tensors(monkeypatch):
    """Every ValueError of the surface raises before a library is loaded or a device is touched, and names the argument."""
    import torch

    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd import _lib

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_load)
    K, N = 3, 4
    r, v, fv = (torch.zeros(K, N) for _ in range(3))
    t, e = (torch.zeros(K, N, dtype=torch.uint8) for _ in range(2))
    lv, c = torch.zeros(N), torch.zeros(N, dtype=torch.float64)
    good = dict(last_value=lv, ended=e, final_value=fv, carry_in=c, carry_out=c.clone(), advantage_out=torch.zeros(K, N), return_out=torch.zeros(K, N))
    gl = dict(gamma=0.9, lam=0.9)
    for fn in (ga.advantages, ga.bind_advantages):
        # host tensors of the right shapes: the device is what is wrong
        with pytest.raises(ValueError, match="reward must be a device tensor"):
            fn(r, v, t, **gl, **good)
        for name, bad in (("gamma", -0.1), ("gamma", 1.5), ("gamma", float("nan")), ("gamma", "x"), ("lam", 1.01), ("lam", -1)):
            with pytest.raises(ValueError, match=name):
                fn(r, v, t, **{**gl, name: bad}, **good)
        with pytest.raises(ValueError, match="value must be given"):
            fn(r, None, t, **gl, **good)
        for name in good:
            shape = (K, N + 1) if good[name].dim() == 2 else (N + 1,)
            wrong_dtype = torch.float32 if good[name].dtype == torch.float64 else torch.float64
            for bad, what in ((torch.zeros(shape, dtype=good[name].dtype), "shape"), (good[name].to(wrong_dtype), "torch"), (np.zeros(shape), "torch tensor")):
                with pytest.raises(ValueError, match=rf"^{name} must .*{what}"):
                    fn(r, v, t, **gl, **{**good, name: bad})
        with pytest.raises(ValueError, match="^final_value must be contiguous"):
            fn(r, v, t, **gl, **{**good, "final_value": torch.zeros(N, K).t()})
        with pytest.raises(ValueError, match="^terminated must be torch.uint8"):
            fn(r, v, t.bool(), **gl, **good)
        with pytest.raises(ValueError, match="^ended must be torch.uint8"):
            fn(r, v, t, **gl, **{**good, "ended": e.to(torch.int32)})
        with pytest.raises(ValueError, match="^value must have shape"):
            fn(r, v[:2], t, **gl, **good)
        with pytest.raises(ValueError, match="^terminated must be given"):
            fn(r, v, None, **gl, **good)
        for bad, what in ((torch.zeros(N), r"shape \[K, N\]"), (torch.zeros(0, N), "K, N >= 1"), (torch.zeros(K, N, dtype=torch.float16), "float32 or float64"),
                          (torch.zeros(N, K).t(), "contiguous"), (np.zeros((K, N)), "torch tensor")):
            with pytest.raises(ValueError, match=f"^reward must .*{what}"):
                fn(bad, v, t, **gl, **good)
    with pytest.raises(ValueError, match="at least one of advantage_out and return_out"):
        ga.bind_advantages(r, v, t, **gl)
    # float64 rows want float64 companions
    with pytest.raises(ValueError, match="^value must be torch.float64"):
        ga.advantages(r.double(), v, t, **gl)
    # the pass without a critic
    for fn, kw in ((ga.discounted_returns, dict()), (ga.bind_discounted_returns, dict(out=torch.zeros(K, N)))):
        with pytest.raises(ValueError, match="reward must be a device tensor"):
            fn(r, t, gamma=0.9, last_value=lv, ended=e, **kw)
        with pytest.raises(ValueError, match="gamma"):
            fn(r, t, gamma=1.1, **kw)
        with pytest.raises(ValueError, match="last_value and carry_in both seed"):
            fn(r, t, gamma=0.9, last_value=lv, carry_in=c, **kw)
        with pytest.raises(ValueError, match="^last_value must have shape"):
            fn(r, t, gamma=0.9, last_value=torch.zeros(N + 1), **kw)
        with pytest.raises(ValueError, match="^carry_in must be torch.float64"):
            fn(r, t, gamma=0.9, carry_in=lv, **kw)
        with pytest.raises(ValueError, match="^out must have shape"):
            fn(r, t, gamma=0.9, **{**kw, "out": torch.zeros(K, N + 1)})
    with pytest.raises(ValueError, match="^out must be given"):
        ga.bind_discounted_returns(r, t, gamma=0.9, out=None)
