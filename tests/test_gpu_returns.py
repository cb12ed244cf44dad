"""Device-side returns and GAE (csrc/gemx_returns.hip) against the float64 numpy restatement of its row function, BIT FOR BIT: the
doubles are the same sequence on both sides (every product and sum rounded on its own, no fused multiply-add), so fp64 outputs equal the
restatement and fp32 outputs equal its float64 result cast to float32 -- `torch.equal` on every element, no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)  # (sibling module: the restatement)

pytestmark = pytest.mark.gpu

G = 16  # the kernel's group depth (gym_electric_motor_amd.returns.GROUP_ROWS, csrc/gemx_returns.hip: GROUP_ROWS); test_group_depth pins it
NS = [1, 63, 64, 257, 300]  # partial wave, full wave, second workgroup with one lane, partial second workgroup
KS = [1, G - 1, G, G + 1, 2 * G + 1]
PATTERNS = ["none", "all", "edges", "consecutive", "random"]
GAMMA, LAM = 0.99, 0.95


def _np_dtype(dtype):
    return np.float64 if dtype == "float64" else np.float32


def _masks(pattern, K, N, rng):
    """-> (terminated, ended) uint8 [K, N]"""
    ended = np.zeros((K, N), bool)
    if pattern == "all":
        ended[:] = True
    elif pattern == "edges":
        ended[0] = ended[K - 1] = True
    elif pattern == "consecutive":
        ended[K // 2] = ended[min(K // 2 + 1, K - 1)] = True
    elif pattern == "random":
        ended = rng.random((K, N)) < 0.1
    truncated = ended & (rng.random((K, N)) < 0.25)  # a quarter of the ends are truncations
    return (ended & ~truncated).astype(np.uint8), ended.astype(np.uint8)


def _case(K, N, dtype, pattern="random", seed=0):
    rng = np.random.default_rng([seed, K, N])
    R = _np_dtype(dtype)
    terminated, ended = _masks(pattern, K, N, rng)
    c = dict(reward=rng.normal(size=(K, N)).astype(R), value=rng.normal(size=(K, N)).astype(R), final_value=rng.normal(size=(K, N)).astype(R),
             last_value=rng.normal(size=N).astype(R), carry_in=rng.normal(size=N), terminated=terminated, ended=ended)
    return c


def _dev(c):
    import torch

    return {k: None if v is None else torch.as_tensor(v).cuda().contiguous() for k, v in c.items()}


def _same(got, want, name, R=None):
    """every element, bit for bit (want: the restatement's float64, cast to the output's dtype)"""
    import torch

    want = torch.as_tensor(np.asarray(want).astype(R) if R is not None else np.asarray(want))
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert torch.equal(got, want), (name, int((got != want).sum()))
    assert torch.equal(got.view(torch.int64 if got.dtype == torch.float64 else torch.int32), want.view(torch.int64 if got.dtype == torch.float64 else torch.int32)), name


def _check_gae(c, dtype, gamma=GAMMA, lam=LAM, outputs=("advantage_out", "return_out")):
    """one launch through bind_advantages on the case's tensors (None: absent) against the restatement"""
    import returns_restatement as rr
    import torch

    import gym_electric_motor_amd as ga

    R = _np_dtype(dtype)
    d = _dev(c)
    K, N = c["reward"].shape
    out = {name: torch.full((K, N), float("nan"), dtype=d["reward"].dtype, device="cuda") for name in outputs}
    carry_out = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    got = ga.bind_advantages(d["reward"], d["value"], d["terminated"], gamma=gamma, lam=lam, last_value=d["last_value"], ended=d["ended"], final_value=d["final_value"],
                             carry_in=d["carry_in"], carry_out=carry_out, **out)()
    torch.cuda.synchronize()
    adv, ret, carry = rr.gae(c["reward"], c["value"], c["terminated"], gamma, lam, last_value=c["last_value"], ended=c["ended"], final_value=c["final_value"],
                             carry_in=c["carry_in"])
    assert got[0] is out.get("advantage_out") and got[1] is out.get("return_out")
    if "advantage_out" in out:
        _same(out["advantage_out"], adv, "advantage", R)
    if "return_out" in out:
        _same(out["return_out"], ret, "returns", R)
    _same(carry_out, carry, "carry_out")
    return adv, ret


def test_group_depth():
    import re

    from gym_electric_motor_amd import build, returns

    src = open(os.path.join(build.CSRC, "gemx_returns.hip")).read()
    assert int(re.search(r"constexpr int GROUP_ROWS = (\d+);", src).group(1)) == returns.GROUP_ROWS == G


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_shapes(N, K, dtype):
    """Every optional tensor given, random ends (10 %, a quarter of them truncations)."""
    _check_gae(_case(K, N, dtype), dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_mask_patterns(pattern, dtype):
    for K, N in ((2 * G + 1, 300), (1, 63), (G, 257)):
        _check_gae(_case(K, N, dtype, pattern, seed=1), dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("gamma,lam", [(0.0, 0.5), (0.9, 0.0), (1.0, 1.0), (0.0, 0.0)])
def test_gamma_and_lambda_at_their_bounds(gamma, lam, dtype):
    _check_gae(_case(G + 1, 257, dtype, seed=2), dtype, gamma=gamma, lam=lam)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("absent", ["ended", "final_value", "last_value", "carry_in", "advantage_out", "return_out"])
def test_each_optional_tensor_absent(absent, dtype):
    c = _case(G + 1, 257, dtype, seed=3)
    outputs = tuple(o for o in ("advantage_out", "return_out") if o != absent)
    if absent in c:
        c[absent] = None
    _check_gae(c, dtype, outputs=outputs)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_final_value_is_read_at_truncated_rows_only(dtype):
    """final_value holds NaN wherever it must not be read: the outputs stay finite and equal the restatement of the unmasked tensor."""
    c = _case(2 * G + 1, 300, dtype, seed=4)
    trunc = (c["ended"] != 0) & (c["terminated"] == 0)
    assert trunc.any() and not trunc.all()
    plain = dict(c)
    c["final_value"] = np.where(trunc, c["final_value"], np.nan).astype(c["final_value"].dtype)
    adv, ret = _check_gae(c, dtype)
    assert np.isfinite(adv).all() and np.isfinite(ret).all()
    adv0, ret0 = _check_gae(plain, dtype)
    assert np.array_equal(adv, adv0) and np.array_equal(ret, ret0)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_advantages_allocates_what_is_not_given(dtype):
    import returns_restatement as rr
    import torch

    import gym_electric_motor_amd as ga

    c = _case(G + 1, 300, dtype, seed=5)
    d = _dev(c)
    adv, ret = ga.advantages(d["reward"], d["value"], d["terminated"], gamma=GAMMA, lam=LAM)
    want = rr.gae(c["reward"], c["value"], c["terminated"], GAMMA, LAM)
    _same(adv, want[0], "advantage", _np_dtype(dtype)), _same(ret, want[1], "returns", _np_dtype(dtype))
    mine = torch.empty_like(d["reward"])
    adv2, ret2 = ga.advantages(d["reward"], d["value"], d["terminated"], gamma=GAMMA, lam=LAM, ended=d["ended"], return_out=mine)
    want = rr.gae(c["reward"], c["value"], c["terminated"], GAMMA, LAM, ended=c["ended"])
    assert ret2 is mine
    _same(adv2, want[0], "advantage", _np_dtype(dtype)), _same(ret2, want[1], "returns", _np_dtype(dtype))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("K,N", [(1, 1), (G - 1, 63), (2 * G + 1, 300)])
def test_discounted_returns(K, N, dtype):
    """with last_value, with carry_in, with neither; with and without `ended`"""
    import returns_restatement as rr
    import torch

    import gym_electric_motor_amd as ga

    R = _np_dtype(dtype)
    c = _case(K, N, dtype, seed=6)
    d = _dev(c)
    for seed in ("last_value", "carry_in", None):
        for ended in ("ended", None):
            kw = {} if seed is None else {seed: d[seed]}
            kw_np = {} if seed is None else {seed: c[seed]}
            carry_out = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
            got = ga.discounted_returns(d["reward"], d["terminated"], gamma=GAMMA, ended=None if ended is None else d["ended"], carry_out=carry_out, **kw)
            want, carry = rr.discounted(c["reward"], c["terminated"], GAMMA, ended=None if ended is None else c["ended"], **kw_np)
            _same(got, want, ("returns", seed, ended), R), _same(carry_out, carry, "carry_out")
    out = torch.empty_like(d["reward"])
    assert ga.bind_discounted_returns(d["reward"], d["terminated"], gamma=1.0, out=out)() is out
    _same(out, rr.discounted(c["reward"], c["terminated"], 1.0)[0], "gamma 1", R)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_chunked_scan_equals_whole_scan(dtype):
    """K = 2G+1 split at an odd row: the upper chunk's carry feeds the lower chunk, last_value = value[k0]."""
    import torch

    import gym_electric_motor_amd as ga

    K, N, k0 = 2 * G + 1, 300, G + 1
    assert k0 % 2 == 1
    c = _case(K, N, dtype, seed=7)
    d = _dev(c)
    common = dict(gamma=GAMMA, lam=LAM)
    carry = torch.empty(N, dtype=torch.float64, device="cuda")
    adv, ret = ga.advantages(d["reward"], d["value"], d["terminated"], last_value=d["last_value"], ended=d["ended"], final_value=d["final_value"],
                             carry_in=d["carry_in"], carry_out=carry, **common)
    mid, low = torch.empty_like(carry), torch.empty_like(carry)
    up = ga.advantages(d["reward"][k0:], d["value"][k0:], d["terminated"][k0:], last_value=d["last_value"], ended=d["ended"][k0:], final_value=d["final_value"][k0:],
                       carry_in=d["carry_in"], carry_out=mid, **common)
    lo = ga.advantages(d["reward"][:k0], d["value"][:k0], d["terminated"][:k0], last_value=d["value"][k0], ended=d["ended"][:k0], final_value=d["final_value"][:k0],
                       carry_in=mid, carry_out=low, **common)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([lo[0], up[0]]), adv) and torch.equal(torch.cat([lo[1], up[1]]), ret) and torch.equal(low, carry)
    _check_gae(c, dtype)  # (and the whole scan is the restatement's)
    # the return-to-go in pieces: last_value seeds the upper chunk, its carry the lower one
    whole = ga.discounted_returns(d["reward"], d["terminated"], gamma=GAMMA, last_value=d["last_value"], ended=d["ended"], carry_out=carry)
    up = ga.discounted_returns(d["reward"][k0:], d["terminated"][k0:], gamma=GAMMA, last_value=d["last_value"], ended=d["ended"][k0:], carry_out=mid)
    lo = ga.discounted_returns(d["reward"][:k0], d["terminated"][:k0], gamma=GAMMA, ended=d["ended"][:k0], carry_in=mid, carry_out=low)
    assert torch.equal(torch.cat([lo, up]), whole) and torch.equal(low, carry)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_on_a_stepped_env_with_a_time_limit(dtype):
    """17 steps of a complete env with a time limit of 5: its terminated / truncated bytes are the masks."""
    import returns_restatement as rr
    import torch

    import gym_electric_motor_amd as ga

    N, K = 300, 17
    env = ga.make("Cont-CC-PMSM-v0", n_envs=N, dtype=dtype, reference_generator="default", max_episode_steps=5, episode_statistics=True, seed=3)
    env.reset()
    gen = torch.Generator(device="cuda").manual_seed(5)
    tdtype = torch.float64 if dtype == "float64" else torch.float32
    a = (torch.rand((N, int(env.physical_system.action_space.shape[0])), generator=gen, device="cuda", dtype=torch.float64) * 2 - 1).to(tdtype).contiguous()
    reward, terminated, truncated = [], [], []
    for _ in range(K):
        _, w, t, tr, _ = env.step(a)  # (held random actions drive the currents towards their limits: some envs terminate)
        reward.append(w.clone()), terminated.append(t.clone()), truncated.append(tr.clone())
    reward, terminated, truncated = torch.stack(reward), torch.stack(terminated), torch.stack(truncated)
    ended = (terminated | truncated).contiguous()
    assert int(truncated.sum()) > 0 and reward.dtype == tdtype
    value, final_value = (torch.randn((K, N), generator=gen, device="cuda", dtype=torch.float64).to(tdtype) for _ in range(2))
    last_value = torch.randn(N, generator=gen, device="cuda", dtype=torch.float64).to(tdtype)
    adv, ret = ga.advantages(reward, value, terminated, gamma=GAMMA, lam=LAM, last_value=last_value, ended=ended, final_value=final_value)
    torch.cuda.synchronize()
    want = rr.gae(reward.cpu().numpy(), value.cpu().numpy(), terminated.cpu().numpy(), GAMMA, LAM, last_value=last_value.cpu().numpy(), ended=ended.cpu().numpy(),
                  final_value=final_value.cpu().numpy())
    _same(adv, want[0], "advantage", _np_dtype(dtype)), _same(ret, want[1], "returns", _np_dtype(dtype))
    env.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_on_a_fused_rollout_with_statistics(dtype):
    """rollout_complete(..., episode_statistics=True) of an env without a time limit: its `ended` rows are passed on."""
    import returns_restatement as rr
    import torch

    import gym_electric_motor_amd as ga

    N, K = 300, 17
    env = ga.make("Cont-CC-PMSM-v0", n_envs=N, dtype=dtype, reference_generator="default", episode_statistics=True, seed=3)
    env.reset()
    gen = torch.Generator(device="cuda").manual_seed(6)
    tdtype = torch.float64 if dtype == "float64" else torch.float32
    a = (torch.rand((N, int(env.physical_system.action_space.shape[0])), generator=gen, device="cuda", dtype=torch.float64) * 2 - 1).to(tdtype)
    actions = a[None].expand(K, *a.shape).contiguous()
    _, _, reward, done, ep = env.rollout_complete(actions, episode_statistics=True)
    value = torch.randn((K, N), generator=gen, device="cuda", dtype=torch.float64).to(tdtype)
    adv, ret = ga.advantages(reward, value, done, gamma=GAMMA, lam=LAM, ended=ep["ended"])
    rtg = ga.discounted_returns(reward, done, gamma=GAMMA, ended=ep["ended"])
    torch.cuda.synchronize()
    args = (reward.cpu().numpy(), value.cpu().numpy(), done.cpu().numpy())
    want = rr.gae(*args, GAMMA, LAM, ended=ep["ended"].cpu().numpy())
    _same(adv, want[0], "advantage", _np_dtype(dtype)), _same(ret, want[1], "returns", _np_dtype(dtype))
    _same(rtg, rr.discounted(args[0], args[2], GAMMA, ended=ep["ended"].cpu().numpy())[0], "return-to-go", _np_dtype(dtype))
    env.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_graph_replay(dtype):
    """bind_advantages captured on one stream; two replays with the inputs overwritten in between, each the restatement of the
    then-current inputs."""
    import returns_restatement as rr
    import torch

    import gym_electric_motor_amd as ga

    K, N = 2 * G + 1, 300
    R = _np_dtype(dtype)
    first, second = _case(K, N, dtype, seed=8), _case(K, N, dtype, seed=9)
    d = _dev(first)
    adv, ret = torch.empty_like(d["reward"]), torch.empty_like(d["reward"])
    carry_out = torch.empty(N, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    launch = ga.bind_advantages(d["reward"], d["value"], d["terminated"], gamma=GAMMA, lam=LAM, last_value=d["last_value"], ended=d["ended"],
                                final_value=d["final_value"], carry_in=d["carry_in"], advantage_out=adv, return_out=ret, carry_out=carry_out, stream=side)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    torch.cuda.synchronize()
    for c in (first, second):
        for name, t in d.items():
            t.copy_(torch.as_tensor(c[name]))
        adv.fill_(float("nan")), ret.fill_(float("nan")), carry_out.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = rr.gae(c["reward"], c["value"], c["terminated"], GAMMA, LAM, last_value=c["last_value"], ended=c["ended"], final_value=c["final_value"],
                      carry_in=c["carry_in"])
        _same(adv, want[0], "advantage", R), _same(ret, want[1], "returns", R), _same(carry_out, want[2], "carry_out")


def test_error_paths_return_a_status():
    """The entry point's own checks: GEMX_ERR_ARG and a text in gemx_last_error(), never a launch (the outputs keep their contents)."""
    import torch

    from gym_electric_motor_amd import _lib

    L = _lib.load()
    K, N = 3, 70
    d = _dev(_case(K, N, "float32"))
    out, out2 = (torch.full((K, N), 7.0, device="cuda") for _ in range(2))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr() if torch.is_tensor(t) else t)  # noqa: E731

    def call(gamma=0.9, lam=0.9, flags=0, size=None, n=N, k=K, dtype=_lib.F32, device=0, reward=d["reward"], value=d["value"], last_value=None,
             terminated=d["terminated"], ended=None, final_value=None, carry_in=None, carry_out=None, advantage_out=out, return_out=out2, cfg=True):
        c = _lib.GemxReturnsConfig()
        c.struct_size, c.gamma, c.lam, c.flags = C.sizeof(c) if size is None else size, gamma, lam, flags
        rc = L.gemx_returns_rows(C.byref(c) if cfg else None, n, k, dtype, device, p(reward), p(value), p(last_value), p(terminated), p(ended), p(final_value),
                                 p(carry_in), p(carry_out), p(advantage_out), p(return_out), st)
        return rc, L.gemx_last_error().decode()

    assert call()[0] == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
    out.fill_(7.0), out2.fill_(7.0)
    bad = [
        (dict(cfg=False), "null"), (dict(size=8), "size mismatch"), (dict(flags=1), "flags"), (dict(gamma=-0.5), "gamma"), (dict(gamma=1.5), "gamma"),
        (dict(gamma=float("nan")), "gamma"), (dict(lam=2.0), "lam"), (dict(lam=float("nan")), "lam"), (dict(reward=None), "reward_dev"),
        (dict(terminated=None), "terminated_dev"), (dict(advantage_out=None, return_out=None), "at least one"), (dict(k=0), "K must be"), (dict(n=0), "n_envs"),
        (dict(dtype=5), "dtype"), (dict(device=999), "device"), (dict(reward=d["reward"].data_ptr() + 2), "aligned"),
        (dict(carry_in=d["carry_in"].data_ptr() + 4), "aligned"), (dict(n=(2 ** 31) * 256 + 1), "exceeds"),
        # the pass without a critic
        (dict(value=None), "only output"), (dict(value=None, advantage_out=None, final_value=d["final_value"]), "final_value_dev"),
        (dict(value=None, advantage_out=None, last_value=d["last_value"], carry_in=d["carry_in"]), "not both"),
    ]
    for kw, text in bad:
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((out2 == 7.0).all())
