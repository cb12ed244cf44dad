"""FluxObserver and flux-oriented dq actions on the device (csrc/gemx_fluxobs.hip) against the float64 host restatement and the
reference's recorded runs.  Shapes: N in {1, 65, 257} (one lane, a partial wave, a partial second workgroup... of 64-lane workgroups: 1, 2
and 5 of them), K in {1, 2, 37}, SCIM rows of 14 and DFIM rows of 24 columns, fp32 and fp64."""
import numpy as np
import pytest

from flux_fixtures import DQ_CASES, holders, load
from parity_contract import DONE_MARGIN, FLUX_FLOOR, REL_FLOOR, TOL_FP32, TOL_FP64_SAME_INTEGRATOR

pytestmark = pytest.mark.gpu
TOL = {"float32": TOL_FP32, "float64": TOL_FP64_SAME_INTEGRATOR}
ENV = {"SCIM": "Cont-CC-SCIM-v0", "DFIM": "Cont-CC-DFIM-v0"}


def _col_err(got, ref, dtype):
    """the contract's column measure: fp32 relative to max(max|ref|, REL_FLOOR), fp64 absolute"""
    d = float(np.abs(got - ref).max())
    return d / max(float(np.abs(ref).max()), REL_FLOOR) if dtype == "float32" else d


def _flux_errors(got, ref, dtype):
    """(psi_abs, complex Psi, weighted circular psi_angle) errors of [..., 2] columns (psi_abs, psi_angle) against the reference's."""
    ga_, gr = got[..., 0] * np.exp(1j * np.pi * got[..., 1]), ref[..., 0] * np.exp(1j * np.pi * ref[..., 1])
    e_abs = _col_err(got[..., 0], ref[..., 0], dtype)
    e_psi = max(_col_err(ga_.real, gr.real, dtype), _col_err(ga_.imag, gr.imag, dtype))
    circ = np.abs(got[..., 1] - ref[..., 1])
    circ = np.minimum(circ, 2.0 - circ)
    w = np.minimum(1.0, ref[..., 0] / (FLUX_FLOOR * max(float(ref[..., 0].max()), 1e-300)))
    return e_abs, e_psi, float((circ * w).max())  # (the angle column's scale is 1: max|angle / pi| ~ 1)


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("motor", ["SCIM", "DFIM"])
def test_observer_arithmetic_alone(motor, dtype, n):
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make(ENV[motor], n_envs=n, dtype=dtype, auto_reset=True, physical_system_wrappers=(ga.FluxObserver(),))
    flux, nb = env.flux, env.flux.n_in
    assert nb == {"SCIM": 14, "DFIM": 24}[motor] and env._flux_only
    rng = np.random.default_rng(5)
    env.reset()
    flux.host_reset(n)
    worst, n_done = np.zeros(3), 0
    for K in (1, 2, 37, 37):
        a = rng.uniform(-1, 1, (K, n, env.action_space.shape[0]))
        if motor == "DFIM":  # held actions: a doubly fed machine under white noise stays inside its limits
            a[:] = a[:1]
        ext, done = env.rollout(torch.as_tensor(a, dtype=getattr(torch, dtype), device="cuda"))
        torch.cuda.synchronize()
        raw = env._raw_scratch
        assert tuple(ext.shape) == (K, n, nb + 2) and torch.equal(ext[..., :nb], raw)  # the copied columns: the same bits
        want = flux.evaluate(raw.double().cpu().numpy(), done.cpu().numpy())
        worst = np.maximum(worst, _flux_errors(ext[..., nb:].double().cpu().numpy(), want[..., nb:], dtype))
        n_done += int(done.sum())
    print(f"{motor} {dtype} N={n}: psi_abs {worst[0]:.2e} Psi {worst[1]:.2e} psi_angle {worst[2]:.2e}; {n_done} terminations")
    if motor == "SCIM" and n >= 65:
        assert n_done > 0  # lanes terminate and restart
    assert worst.max() <= TOL[dtype], worst
    env.close()


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("motor", ["SCIM", "DFIM"])
def test_rows_equal_steps_bit_for_bit(motor, dtype, n):
    import torch

    import gym_electric_motor_amd as ga

    tdtype = getattr(torch, dtype)
    mode = motor
    mk = lambda: ga.make(ENV[motor], n_envs=n, dtype=dtype, auto_reset=True, _defer_create=True,  # noqa: E731
                         physical_system_wrappers=(ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor(mode))).flux.create(n, 0, dtype)
    fa, fb = mk(), mk()
    nb = fa.n_in
    g = torch.Generator(device="cuda").manual_seed(11)

    def view(shape, off):  # a contiguous tensor view at element offset `off` of its allocation
        numel = int(np.prod(shape))
        return torch.empty(numel + 4, dtype=tdtype, device="cuda")[off:off + numel].view(shape)

    for K, off in ((1, 0), (2, 1), (37, 0), (37, 1)):
        state = view((K, n, nb), off)
        state.copy_(torch.rand((K, n, nb), generator=g, device="cuda", dtype=tdtype) * 2 - 1)
        done = (torch.rand((K, n), generator=g, device="cuda") < 0.1).to(torch.uint8)
        out_a = fa.rows(state, done, out=view((K, n, nb + 2), off))
        out_b = view((K, n, nb + 2), 1 - off)
        for k in range(K):
            fb.step(state[k], done[k], out_b[k])
        torch.cuda.synchronize()
        assert torch.equal(out_a, out_b), (K, off)
        assert torch.equal(out_a[..., :nb], state)
        assert torch.equal(fa.get_state(), fb.get_state())
        mask = (torch.rand(n, generator=g, device="cuda") < 0.5).to(torch.uint8)  # a masked reset in between
        fa.reset(mask)
        fb.reset(mask)
        st = fa.get_state()
        assert torch.equal(st, fb.get_state()) and bool((st[:2, mask.bool()] == 0).all())
    fa.close()
    fb.close()


@pytest.mark.parametrize("case", DQ_CASES)
def test_closed_loop_against_the_reference(case):
    import torch

    import gym_electric_motor_amd as ga

    d = load(case)
    n = 4
    env = ga.make(d["meta"]["env_id"], n_envs=n, physical_system_wrappers=holders(ga, d["meta"]["chain"]))
    nb = env.flux.n_in
    state, _ = env.reset()
    torch.cuda.synchronize()
    assert np.abs(state.double().cpu().numpy() - d["reset_state"]).max() <= TOL_FP32
    rows, dones = [], []
    for k in range(len(d["actions"])):
        a = torch.as_tensor(np.tile(d["actions"][k], (n, 1)), dtype=torch.float32, device="cuda")
        state, _, done, _, _ = env.step(a)
        rows.append(state.double().cpu().numpy())
        dones.append(done.cpu().numpy().copy())
    rows, dones, ref = np.array(rows), np.array(dones), d["state"]
    assert all(np.array_equal(rows[:, 0], rows[:, j]) for j in range(1, n))  # every lane the same run
    got = rows[:, 0]
    names = d["state_names"]
    # done flags: exact outside the contract's margin (the squared current constraint of the reference, on normalised currents)
    radius = np.hypot(ref[:, names.index("i_sd")], ref[:, names.index("i_sq")])
    clear = np.abs(radius - 1.0) > DONE_MARGIN
    assert np.array_equal(dones[clear, 0] != 0, d["terminated"][clear] != 0)
    worst = {}
    for j, name in enumerate(names[:nb]):
        delta = np.abs(got[:, j] - ref[:, j])
        if name == "epsilon":
            delta = np.minimum(delta, 2.0 - delta)
        worst[name] = float(delta.max()) / max(float(np.abs(ref[:, j]).max()), REL_FLOOR)
    worst["psi_abs"], worst["Psi"], worst["psi_angle"] = _flux_errors(got[:, nb:], ref[:, nb:], "float32")
    print(case, {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= TOL_FP32, worst
    env.close()


def _complete(ga, n, **kw):
    return ga.make("Cont-CC-SCIM-v0", n_envs=n, reference_generator="default", seed=3,
                   physical_system_wrappers=(ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor("SCIM")), **kw)


def test_graph_replay_equals_eager():
    import torch

    import gym_electric_motor_amd as ga

    n, S, R = 257, 4, 3
    actions = torch.as_tensor(np.random.default_rng(2).uniform(-1, 1, (n, 2)), dtype=torch.float32, device="cuda")
    outs = []
    for graphed in (False, True):
        env = _complete(ga, n)
        buf = actions.clone()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            step, (state, ref), reward, done = env.bind_step(buf, stream=stream)
            step()  # warm-up
            env.reset()
            if graphed:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=stream):
                    for _ in range(S):
                        step()
                for _ in range(R):
                    graph.replay()
            else:
                for _ in range(S * R):
                    step()
        stream.synchronize()
        outs.append((state.clone(), ref.clone(), reward.clone(), done.clone(), env.flux.get_state()))
        env.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float(outs[0][0][:, -2].abs().max()) > 0  # (the flux columns are live)


def test_checkpoint_continues_bit_for_bit():
    import torch

    import gym_electric_motor_amd as ga

    n = 65
    mk = lambda: ga.make("Cont-CC-SCIM-v0", n_envs=n, physical_system_wrappers=(ga.FluxObserver(), ga.FluxOrientedDqToAbcActionProcessor("SCIM")))  # noqa: E731
    a = torch.as_tensor(np.random.default_rng(4).uniform(-1, 1, (30, n, 2)), dtype=torch.float32, device="cuda")
    env = mk()
    env.reset()
    for k in range(15):
        env.step(a[k])
    ck = env.get_checkpoint()
    assert tuple(ck["flux_observer"].shape) == (4, n)
    want = [(env.step(a[k])[0].clone(), env.physical_system.done.clone()) for k in range(15, 30)]
    other = mk()
    other.reset()
    other.set_checkpoint(ck)
    for k, (s, dn) in zip(range(15, 30), want):
        got = other.step(a[k])
        assert torch.equal(got[0], s) and torch.equal(got[2], dn), k
    env.close()
    other.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_stage_composition_over_the_extended_row(dtype):
    """CosSinProcessor('psi_angle') + observed_states + flatten over the SCIM's 16-column extended row against the host program.  (The
    DFIM's 26-column row exceeds what gemx_obsproc_create reads and is refused: tests/test_flux_observer_cpu.py::test_refusals.)"""
    import torch

    import gym_electric_motor_amd as ga

    n = 65
    env = ga.make("Cont-CC-SCIM-v0", n_envs=n, dtype=dtype, reference_generator="default", seed=1, flatten_observation=True,
                  physical_system_wrappers=(ga.FluxObserver(), ga.CosSinProcessor("psi_angle", remove_angle=True)),
                  observed_states=["omega", "i_sd", "i_sq", "psi_abs", "cos(psi_angle)", "sin(psi_angle)"])
    st = env.observation_stage
    rng = np.random.default_rng(9)
    env.reset()
    for k in range(5):
        obs, *_ = env.step(torch.as_tensor(rng.uniform(-1, 1, (n, 3)), dtype=getattr(torch, dtype), device="cuda"))
    torch.cuda.synchronize()
    want = st.evaluate(env._ext.double().cpu().numpy(), env._refs.double().cpu().numpy())
    assert tuple(obs.shape) == (n, 6 + len(env.reference_names))
    err = np.abs(obs.double().cpu().numpy() - want).max()
    print(dtype, "stage over the extended row: max error", err)
    assert err <= TOL[dtype]
    # the K-step rollout: physics, ONE pass of the observer, the stage
    a = torch.as_tensor(rng.uniform(-1, 1, (37, n, 3)), dtype=getattr(torch, dtype), device="cuda")
    state, refs, _, _ = env.rollout_complete(a)
    torch.cuda.synchronize()
    want = st.evaluate(env._ext_scratch_buf.double().cpu().numpy(), refs.double().cpu().numpy())
    assert np.abs(state.double().cpu().numpy() - want).max() <= TOL[dtype]
    env.close()
