"""GPU tests of the device-side SwitchedReferenceGenerator (gemx_refgen_create_switched; the holder `ga.SwitchedReferenceGenerator`):

  1. the device against the host restatement (tests/refgen_switched.py) fed the device's OWN draws, read back after every step through
     `state()` (gemx_refgen_get_params, gemx_refgen_get_switch_state): alternative, sk, slen, the sub-episode's index and length must evolve
     exactly as the restatement says (slen + 1 values after a reset); waveform values to the tolerance and jump rule of
     test_waveforms_match_the_restatement, constants exactly.  The increments of a Wiener / Laplace walk cannot be read back: a walk's
     value must lie within the largest increment the draw can produce of the value shown before -- Box-Muller on a 32-bit uniform gives
     |z| <= sqrt(2 ln 2^33) < 6.77, the Laplace inverse |x| <= ln 2^32 < 22.2 scales -- which is what catches a walk that restarts from
     0 instead of from the carried value;
  2. the invariants of the kinds handle, bit for bit: K x step(done[k]) == rollout_shell(K, done), chunked == one-shot, rollout consistent
     with step, two half shards == one whole, reset(mask) touches the masked envs only, a captured bind_step replayed == eager steps;
  3. unchanged paths: a plain column beside a switched one has the bits of that column of a plain handle; kernel coverage;
  4. distributions of the super-episode draws against samples of the live reference (tests/golden/refgen/refgen_switched.npz);
  5. the complete env: rollout_complete == K x step on top of a switched generator.

Shapes: N = 67 x 3 columns (201 lanes, one partial block) and N = 130 x 2 columns (260 lanes, a partial second block); super-episodes of
2..5 steps, sub-episodes of 3..7, K = 64.
"""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)  # (sibling modules: the restatements)

import refgen_switched as rs  # noqa: E402
import refgen_waveforms as rw  # noqa: E402

FIX = np.load(os.path.join(HERE, "golden", "refgen", "refgen_switched.npz"))
META = json.loads(str(FIX["meta"]))
P_MIN = 1e-3  # the acceptance level of test_parameter_draws_match_the_reference_distribution
SUB, SUPER, K = dict(episode_lengths=(3, 8)), (2, 6), 64
Z_MAX = {0: 6.77, 1: 22.2}  # largest |increment| / scale of a Wiener / Laplace step (module docstring)


class _System:
    """What a generator's set_modules reads of a physical system, for generators tested on their own (other n_envs / dtype / env_base)."""

    def __init__(self, ps, n_envs, dtype, env_base=0):
        self.state_positions, self.state_space, self.nominal_state, self.limits = ps.state_positions, ps.state_space, ps.nominal_state, ps.limits
        self.state_names, self.tau = ps.state_names, ps.tau
        self.n_envs, self.env_base, self.device = n_envs, env_base, ps.device
        self._tdev, self._tdtype = ps._tdev, dtype


def _tdtype(dtype):
    import torch

    return dict(float32=torch.float32, float64=torch.float64)[dtype]


def _wave(freq=(500, 3000), **kw):
    return dict(frequency_range=freq, **SUB, **kw)


def _columns(ga, shape):
    """Cont-CC-PMSM-v0 (states i_sd, i_sq before omega): three columns for N = 67, two for N = 130."""
    if shape == 67:
        return [ga.SwitchedReferenceGenerator([ga.StepReferenceGenerator(reference_state="omega", **_wave()), ga.SinusoidalReferenceGenerator(reference_state="omega", **_wave(limit_margin=0.5)),
                                               ga.WienerProcessReferenceGenerator(reference_state="omega", sigma_range=(1e-3, 1e-2), **SUB),
                                               ga.ConstReferenceGenerator(reference_state="omega", reference_value=0.25)], p=[0.3, 0.3, 0.3, 0.1], super_episode_length=SUPER),
                ga.TriangularReferenceGenerator(reference_state="i_sd", **_wave()),
                ga.SwitchedReferenceGenerator([ga.SawtoothReferenceGenerator(reference_state="i_sq", **_wave()), ga.TriangularReferenceGenerator(reference_state="i_sq", **_wave(limit_margin=(0.2, 0.7))),
                                               ga.LaplaceProcessReferenceGenerator(reference_state="i_sq", sigma_range=(1e-3, 1e-2), **SUB),
                                               ga.StepReferenceGenerator(reference_state="i_sq", **_wave(amplitude_range=(0.1, 0.3))),
                                               ga.SinusoidalReferenceGenerator(reference_state="i_sq", **_wave(offset_range=(-0.2, 0.3)))], p=[0.1, 0.2, 0.3, 0.2, 0.2], super_episode_length=SUPER)]
    return [ga.SwitchedReferenceGenerator([ga.WienerProcessReferenceGenerator(reference_state="i_sd", sigma_range=(1e-3, 1e-2), **SUB), ga.StepReferenceGenerator(reference_state="i_sd", **_wave())],
                                          p=[0.6, 0.4], super_episode_length=SUPER),
            ga.SwitchedReferenceGenerator([ga.ConstReferenceGenerator(reference_state="i_sq", reference_value=-0.125), ga.SinusoidalReferenceGenerator(reference_state="i_sq", **_wave()),
                                           ga.SawtoothReferenceGenerator(reference_state="i_sq", **_wave())], super_episode_length=SUPER)]


@pytest.fixture(scope="module")
def system():
    import gym_electric_motor_amd as ga

    env = ga.make("Cont-CC-PMSM-v0", n_envs=4)
    yield env.physical_system
    env.close()


def _gen(ga, system, shape, dtype, n=None, env_base=5, seed=31):
    g = ga.BatchedMultipleReferenceGenerator(_columns(ga, shape), seed=seed).set_modules(_System(system, shape if n is None else n, _tdtype(dtype), env_base))
    g.reset()
    return g


def _done(torch, K_, n, seed=3, share=0.08):
    rng = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((K_, n), device="cuda", generator=rng) < share).to(torch.uint8)


class DeviceDraws:
    """The draws of column j, read from the state the device is in after the launch that made them."""

    def __init__(self, gen, j):
        self.j, self.S, self.c = j, None, gen._cfg
        self.failures = []

    def read(self, S):
        self.S = {k: v[self.j] for k, v in S.items()}

    def super_episode(self, mask):
        return self.S["super_length"], self.S["alternative"]

    def sub_episode(self, mask, kind):
        d = {k: self.S[k] for k in rs.PARAMS + ("length", "sigma")}
        return d

    def initial(self, mask):
        return np.full(mask.shape, np.nan)  # drawn inside the launch that also made the first step: not readable

    def walk(self, mask, before, sigma, lo, hi):
        """The device's value, which must be reachable from the value before by one increment (a fresh Wiener walk: from its initial range)."""
        from gym_electric_motor_amd import _lib

        v = self.S["value"]
        a0 = self.j * _lib.MAX_ALT
        i_lo = np.array(self.c.initial_lo[a0:a0 + _lib.MAX_ALT])[self.S["alternative"]]
        i_hi = np.array(self.c.initial_hi[a0:a0 + _lib.MAX_ALT])[self.S["alternative"]]
        unknown = np.isnan(before)
        b_lo, b_hi = np.where(unknown, i_lo, before), np.where(unknown, i_hi, before)
        reach = np.where(self.S["kind"] == 0, Z_MAX[0], Z_MAX[1]) * sigma
        ok = (v >= rs.clipped_walk(b_lo, -reach, lo, hi) - 1e-15) & (v <= rs.clipped_walk(b_hi, reach, lo, hi) + 1e-15)
        if not ok[mask].all():
            self.failures.append((int((~ok & mask).sum()), np.abs(v - before)[mask & ~ok].tolist()[:4], reach[mask & ~ok].tolist()[:4]))
        return v


def _alternatives(gen, j):
    from gym_electric_motor_amd import _lib

    c, a0 = gen._cfg, j * _lib.MAX_ALT
    return [dict(kind=int(c.kind[a0 + a]), margin=(c.margin_lo[a0 + a], c.margin_hi[a0 + a]), value=c.reference_value[a0 + a]) for a in range(c.n_alt[j])]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [67, 130])
def test_device_follows_the_restatement(system, shape, dtype):
    import torch

    import gym_electric_motor_amd as ga

    n = shape
    gen = _gen(ga, system, shape, dtype)
    done = _done(torch, K, n)
    done[5] = 1  # a row of all ones
    names = list(gen.reference_names)
    cols = [j for j in range(len(names)) if gen._cfg.n_alt[j] > 0]
    machines, draws, n_super = {}, {}, {}
    S = {k: v.cpu().numpy() for k, v in gen.state().items()}
    for j in cols:
        draws[j] = DeviceDraws(gen, j)
        machines[j] = rs.Switched(_alternatives(gen, j), system.tau, n, draws[j])
        draws[j].read(S)
        machines[j].reset()
        n_super[j] = np.ones(n, dtype=int)
        assert (S["n_super"][j] == 1).all() and (S["super_index"][j] == -1).all()  # reset: one draw, the first value not shown yet
        wiener = machines[j].kind == 0  # K = 0: the initial value of a Wiener alternative is readable
        machines[j].value = np.where(wiener, S["value"][j], machines[j].value)
        assert (S["value"][j][~wiener] == 0).all()  # every other kind restarts from 0
    total = left_out = switches = coincide = reset_when_due = 0
    for k in range(K):
        row = gen.step(None if k == 0 else done[k]).double().cpu().numpy()
        S = {key: v.cpu().numpy() for key, v in gen.state().items()}
        mask = np.zeros(n, dtype=bool) if k == 0 else done[k].bool().cpu().numpy()
        for j in cols:
            m, d = machines[j], draws[j]
            d.read(S)
            due = ~m.fresh & (m.sk >= m.slen)  # a switch is due with this row ...
            sub_over = (m.kind != rs.CONST) & (m.k >= m.L)  # ... and the sub-episode would have ended with it anyway
            m.reset(mask)
            n_super[j] += mask
            want, on_jump, tol, switched = m.show()
            n_super[j] += switched
            switches += int(switched.sum())
            coincide += int((switched & sub_over).sum())
            reset_when_due += int((due & mask).sum())  # the done byte of the row a switch was due on: the reset comes first, one draw
            assert (switched == (due & ~mask)).all()
            # the state machine, exactly
            assert (S["alternative"][j] == m.alt).all() and (S["super_index"][j] == m.sk).all() and (S["super_length"][j] == m.slen).all(), (k, j)
            assert (S["n_super"][j] == n_super[j]).all(), (k, j)
            assert (S["kind"][j] == m.kind).all()
            live = m.kind != rs.CONST
            assert (S["index"][j][live] == m.k[live]).all() and (S["length"][j][live] == m.L[live]).all(), (k, j)
            assert (S["index"][j][~live] == -1).all()
            assert S["super_length"][j].min() >= SUPER[0] and S["super_length"][j].max() < SUPER[1]
            # the values
            got = row[:, j]
            if dtype == "float32":  # one rounding of the value to fp32 on top
                tol = tol + np.abs(want) * 2.0 ** -24
                want = np.where(np.isin(m.kind, rs.WALKS + (rs.CONST,)), want.astype(np.float32).astype(np.float64), want)
            err = np.abs(got - want)
            skip = (err > tol) & on_jump
            total += n
            left_out += int(skip.sum())
            assert (err <= tol)[~skip].all(), (k, j, float(err[~skip].max()))
            assert not d.failures, (k, j, d.failures)
    # (slen + 1 values after a reset, slen after a switch: sk, compared above after every row, says so.)  Enough of every sort happened:
    print(f"N={n} {dtype}: {switches} switches in {K} steps ({coincide} together with a sub-episode's end, {reset_when_due} dones on a row a switch was due on), "
          f"{left_out} of {total} samples left out on jumps")
    assert switches > 10 * n * len(cols) and coincide > 0 and reset_when_due > 0
    assert left_out <= rw.MAX_EXCLUDED * total, (left_out, total)
    gen.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [67, 130])
def test_invariants_bit_for_bit(system, shape, dtype):
    import torch

    import gym_electric_motor_amd as ga

    n, base = shape, 5
    done = _done(torch, K, n)
    done[7] = 1

    def same_state(a, b, what):
        sa, sb = a.state(), b.state()
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (what, key)

    # K x step(done[k]) == rollout_shell(K, done)
    one, stepper = _gen(ga, system, shape, dtype), _gen(ga, system, shape, dtype)
    whole = one.rollout_shell(K, done)
    rows = torch.stack([stepper.step(done[k]).clone() for k in range(K)])
    assert torch.equal(rows, whole)
    same_state(one, stepper, "step x K")
    assert len(torch.unique(whole[:, :, 0])) > 50
    # K = 1 and a done tensor of all ones; K = 0 (reset) of everything again
    a, b = _gen(ga, system, shape, dtype), _gen(ga, system, shape, dtype)
    ones = torch.ones((1, n), dtype=torch.uint8, device="cuda")
    assert torch.equal(a.rollout_shell(1, ones)[0], b.step(ones[0]))
    a.reset(), b.reset(mask=ones[0])
    same_state(a, b, "reset all")
    # chunked == one-shot, shell rollouts and steps mixed
    parts = _gen(ga, system, shape, dtype)
    chunks = [parts.rollout_shell(1, done[:1]), parts.rollout_shell(30, done[1:31]), parts.step(done[31]).clone()[None], parts.rollout_shell(K - 32, done[32:])]
    assert torch.equal(torch.cat(chunks), whole)
    same_state(one, parts, "chunked")
    # rollout (reset AFTER row k) is consistent with step: K x step(done[k-1]) == rollout(K, done)
    r1, r2 = _gen(ga, system, shape, dtype), _gen(ga, system, shape, dtype)
    after = r1.rollout(K, done=done)
    rows = torch.stack([r2.step(None).clone()] + [r2.step(done[k - 1]).clone() for k in range(1, K)])
    assert torch.equal(rows, after)
    r2.reset(mask=done[K - 1])  # (the rollout reset the envs of its last row too)
    same_state(r1, r2, "rollout")
    chunked = _gen(ga, system, shape, dtype)
    assert torch.equal(torch.cat([chunked.rollout(20, done=done[:20]), chunked.rollout(K - 20, done=done[20:])]), after)
    # two half shards == one whole (odd N: the halves differ)
    h = n // 2 if n % 2 else n // 2 - 1
    lo_, hi_ = _gen(ga, system, shape, dtype, n=h, env_base=base), _gen(ga, system, shape, dtype, n=n - h, env_base=base + h)
    assert torch.equal(torch.cat([lo_.rollout_shell(K, done[:, :h].contiguous()), hi_.rollout_shell(K, done[:, h:].contiguous())], dim=1), whole)
    # reset(mask) touches only the masked envs, and does what a done byte does
    g1, g2, g3 = (_gen(ga, system, shape, dtype) for _ in range(3))
    for g in (g1, g2, g3):
        g.rollout_shell(9)
    mask = done[3].clone()
    mask[:11] = 1
    before = {key: v.clone() for key, v in g1.state().items()}
    g1.reset(mask=mask)
    now = g1.state()
    keep = ~mask.bool()
    for key in before:
        assert torch.equal(before[key][:, keep], now[key][:, keep]), key
    switched_cols = [j for j in range(int(g1._cfg.n_ref)) if g1._cfg.n_alt[j] > 0]
    assert (now["n_super"][switched_cols][:, mask.bool()] == before["n_super"][switched_cols][:, mask.bool()] + 1).all()
    assert torch.equal(g1.step(None), g2.step(mask))
    same_state(g1, g2, "reset(mask) == done")
    assert not torch.equal(g3.step(None)[mask.bool()], g2.references[mask.bool()])
    # a captured bind_step replayed 16 times == 16 eager steps
    cap, eager = _gen(ga, system, shape, dtype), _gen(ga, system, shape, dtype)
    dbuf = done[2].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step = cap.bind_step(dbuf, stream=side)
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager.step(dbuf)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # (records the launch; nothing runs)
        step()
    for k in range(16):
        dbuf.copy_(done[10 + k])
        graph.replay()
        want = eager.step(done[10 + k])
        torch.cuda.synchronize()
        assert torch.equal(cap.references, want), k
    same_state(cap, eager, "graph")
    for g in (one, stepper, a, b, parts, r1, r2, chunked, lo_, hi_, g1, g2, g3, cap, eager):
        g.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_plain_column_beside_a_switched_one_keeps_its_bits(system, dtype):
    import torch

    import gym_electric_motor_amd as ga

    n = 67
    done = _done(torch, K, n)
    td = _tdtype(dtype)
    plain = lambda: [ga.TriangularReferenceGenerator(reference_state="i_sd", **_wave()), ga.WienerProcessReferenceGenerator(reference_state="i_sq", **SUB),  # noqa: E731
                     ga.LaplaceProcessReferenceGenerator(reference_state="torque", **SUB)]
    switched = ga.SwitchedReferenceGenerator([ga.StepReferenceGenerator(reference_state="omega", **_wave()), ga.WienerProcessReferenceGenerator(reference_state="omega", **SUB)],
                                             super_episode_length=SUPER)
    step_col = ga.StepReferenceGenerator(reference_state="omega", **_wave())
    mixed = ga.BatchedMultipleReferenceGenerator(plain() + [switched], seed=8).set_modules(_System(system, n, td, 3))
    kinds = ga.BatchedMultipleReferenceGenerator(plain() + [step_col], seed=8).set_modules(_System(system, n, td, 3))
    assert list(mixed.reference_names) == list(kinds.reference_names)
    cols = [list(mixed.reference_names).index(s) for s in ("i_sd", "i_sq", "torque")]
    mixed.reset(), kinds.reset()
    assert torch.equal(mixed.rollout_shell(K, done)[:, :, cols], kinds.rollout_shell(K, done)[:, :, cols])
    assert torch.equal(mixed.step(done[0])[:, cols], kinds.step(done[0])[:, cols])
    assert torch.equal(mixed.rollout(9, done=done[:9])[:, :, cols], kinds.rollout(9, done=done[:9])[:, :, cols])
    sm, sk_ = mixed.state(), kinds.state()
    for key in sk_:
        assert torch.equal(sm[key][cols], sk_[key][cols]), key
    mixed.close(), kinds.close()


def test_kernel_coverage(tmp_path):
    """In fresh processes with GEMX_COVERAGE_FILE: an all-Wiener handle and a plain kinds handle launch only the kernels they launched
    before; the switched handle launches refgen_switched_kernel (and none of the others)."""
    import subprocess

    script = (
        "import torch, gym_electric_motor_amd as ga\n"
        "env = ga.make('Cont-CC-PMSM-v0', n_envs=64)\n"
        "ps = env.physical_system\n"
        "KIND\n"
        "g = ga.BatchedMultipleReferenceGenerator(subs, seed=1).set_modules(ps)\n"
        "g.reset(); g.step(); g.rollout(5); g.rollout_shell(5); torch.cuda.synchronize(); g.close(); env.close()\n")
    subs = dict(wiener="subs = [ga.WienerProcessReferenceGenerator(reference_state='i_sd'), ga.WienerProcessReferenceGenerator(reference_state='i_sq')]",
                kinds="subs = [ga.StepReferenceGenerator(reference_state='i_sd'), ga.WienerProcessReferenceGenerator(reference_state='i_sq')]",
                switched="subs = [ga.SwitchedReferenceGenerator([ga.StepReferenceGenerator(reference_state='i_sd'), ga.ConstReferenceGenerator(reference_state='i_sd')]), "
                         "ga.WienerProcessReferenceGenerator(reference_state='i_sq')]")
    names = {}
    for what, line in subs.items():
        cov = tmp_path / f"cov_{what}.txt"
        subprocess.run([sys.executable, "-c", script.replace("KIND", line)], check=True, cwd=os.path.dirname(HERE), env=dict(os.environ, GEMX_COVERAGE_FILE=str(cov)), timeout=300)
        names[what] = {ln.strip() for ln in open(cov) if "refgen" in ln}
    kernels = {what: {x for x in v if "kernel" in x} for what, v in names.items()}
    print(kernels)
    assert all("refgen_walk_kernel" in x or "refgen_step_kernel" in x or "refgen_normals_kernel" in x for x in kernels["wiener"]) and kernels["wiener"], kernels
    assert all("refgen_kinds_kernel" in x for x in kernels["kinds"]) and kernels["kinds"], kernels
    assert all("refgen_switched_kernel" in x for x in kernels["switched"]) and kernels["switched"], kernels


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_super_episode_draws_match_the_reference_distribution(system, dtype):
    """Lengths: two-sample KS against the reference's recorded samples; choices: chi-square against p; switches independent of the
    previous choice: chi-square on the transition counts -- each accepted at p > 1e-3."""
    from scipy import stats

    import gym_electric_motor_amd as ga

    m = META["samples"]
    p = m["p"]
    n = 4096
    alts = [ga.ConstReferenceGenerator(reference_state="omega", reference_value=0.1 * i) for i in range(len(p))]  # (constants: the draws alone)
    gen = ga.BatchedMultipleReferenceGenerator(ga.SwitchedReferenceGenerator(alts, p=p, super_episode_length=tuple(m["super_episode_length"])), seed=57).set_modules(
        _System(system, n, _tdtype(dtype)))
    gen.reset()
    S = {k: v[0].cpu().numpy() for k, v in gen.state().items()}
    lengths, choices, pairs = [S["super_length"].copy()], [S["alternative"].copy()], []
    for _ in range(24):
        gen.step()
        T = {k: v[0].cpu().numpy() for k, v in gen.state().items()}
        new = T["n_super"] != S["n_super"]
        assert ((T["n_super"] - S["n_super"])[new] == 1).all()
        lengths.append(T["super_length"][new])
        choices.append(T["alternative"][new])
        pairs.append(np.stack([S["alternative"][new], T["alternative"][new]]))
        S = T
    lengths, choices, pairs = np.concatenate(lengths), np.concatenate(choices), np.concatenate(pairs, axis=1)
    assert len(lengths) >= 20000
    p_len = stats.ks_2samp(lengths.astype(float), FIX["samples/length"].astype(float)).pvalue
    counts = np.bincount(choices, minlength=len(p))
    p_choice = stats.chisquare(counts, np.array(p) * counts.sum()).pvalue
    table = np.zeros((len(p), len(p)))
    np.add.at(table, (pairs[0], pairs[1]), 1)
    p_indep = stats.chi2_contingency(table).pvalue
    ref_counts = np.bincount(FIX["samples/choice"], minlength=len(p))
    print(f"{dtype}: {len(lengths)} super-episodes; lengths KS p = {p_len:.3g}; choices {counts.tolist()} (reference {ref_counts.tolist()} of 20000) chi-square p = {p_choice:.3g}; "
          f"transitions p = {p_indep:.3g}")
    assert lengths.min() == 2 and lengths.max() == 5
    assert p_len > P_MIN and p_choice > P_MIN and p_indep > P_MIN
    gen.close()


def test_complete_env_rollout_equals_steps():
    import torch

    import gym_electric_motor_amd as ga

    n, K_ = 67, 48

    def make():
        holder = ga.SwitchedReferenceGenerator([ga.StepReferenceGenerator(**_wave()), ga.SinusoidalReferenceGenerator(**_wave()), ga.WienerProcessReferenceGenerator(**SUB)],
                                               super_episode_length=SUPER)
        return ga.make("Cont-SC-PMSM-v0", n_envs=n, reference_generator=holder, seed=3)

    a, b = make(), make()
    assert isinstance(a, ga.CompleteBatchedElectricMotorEnv) and type(a.reference_generator._cfg).__name__ == "GemxRefgenSwitchedConfig"
    a.reset(), b.reset()
    g = torch.Generator(device="cpu").manual_seed(5)
    A = a.physical_system._n_act
    hot = (torch.arange(n) % 3 == 0)
    sign = torch.tensor([1.0] + [-1.0] * (A - 1))
    noise = torch.rand((K_, n, A), generator=g) * 2 - 1
    acts = torch.where(hot[None, :, None], 0.95 * sign + 0.05 * noise, 0.005 * noise).to(a.physical_system._tdtype).cuda().contiguous()
    got = a.rollout_complete(acts)
    rows = ([], [], [], [])
    for k in range(K_):
        obs, reward, terminated, truncated, _ = b.step(acts[k])
        for lst, t in zip(rows, (obs[0], b.reference_generator.references, reward, terminated)):
            lst.append(t.clone())
    torch.cuda.synchronize()
    for name, x, w in zip(("state", "refs", "reward", "done"), got, (torch.stack(r) for r in rows)):
        assert x.shape == w.shape and torch.equal(x, w), name
    done = got[3].bool()
    assert bool(done[1:K_ - 1].any()) and bool((~done.any(dim=0)).any())
    assert len(torch.unique(got[1])) > 10 * n
    a.close(), b.close()
