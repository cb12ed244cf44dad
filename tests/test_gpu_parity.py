"""GPU parity tests (run with `-m gpu` on an MI355X): HIP path through the C ABI vs the fp64 CPU oracle and the
golden vectors recorded from the live reference.

Tolerances (normalised states are O(1); angle compared on the circle):
  * same integrator, GPU fp64 vs oracle/reference fp64 ............ 1e-9 abs
  * same integrator, GPU fp32 vs reference fp64 .................... 1e-4 rel (north star; observed ~1e-6)
  * GPU RK4 / DP5 fp32 vs reference default dopri5 ................. 1e-4 rel, every system (the device solvers split a step at the
    kinks of the PolynomialStaticLoad, where scipy's adaptive controller splits its own)
  * done masks: exact, except steps whose constraint margin is < 1e-5 in the reference
  * "rel" = max |got - ref| of a column / max(|ref| range of that column, 1e-3)
"""
import glob
import sys
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (sibling test modules: shared transcript helpers)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "*.npz")) if "converter_kats" not in f and "init_samples" not in f and "wiener_samples" not in f)


def _load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return d, json.loads(str(d["meta"]))


def _make_from_meta(meta, n_envs, solver=None, dtype="float32", episodic=None, obs_layout="aos", auto_reset=None, **extra):
    """extra: further make-kwargs (seed, _defer_create).  A meta that carries a recorded custom constraint set (a list, not the string
    "default" / "none": oracle/make_golden.py:main_constraints) gets that set, built from the package's own holders."""
    import gym_electric_motor_amd as ga

    solver = solver or meta["solver"]
    if isinstance(solver, str):
        sol = {"euler": ga.EulerSolver(), "euler4": ga.EulerSolver(nsteps=4), "rk4": ga.RK4Solver(), "rk4x4": ga.RK4Solver(nsteps=4),
               "rk4x8": ga.RK4Solver(nsteps=8), "dp5x8": ga.DormandPrince5Solver(nsteps=8),
               "dopri5": ga.DormandPrince5Solver(), "dp5": ga.DormandPrince5Solver(),
               "rk4k": ga.RK4Solver(split_kinks=True), "dp5k": ga.DormandPrince5Solver(split_kinks=True),
               "default": None}[solver]  # default: whatever make(env_id) picks (envs.default_ode_solver)
    else:
        sol = solver  # a solver object
    kw = dict(n_envs=n_envs, ode_solver=sol, tau=meta["tau"], dtype=dtype, obs_layout=obs_layout, auto_reset=auto_reset)
    if "MultiConverter" in meta["converter"]:
        # Cont/FiniteMultiConverter: the dead time lives in the sub-converters (a dict override would only reach the holder)
        if meta["interlocking_time"] > 0:
            til = meta["interlocking_time"]
            subs = {"FiniteFourQuadrantConverter": ga.FiniteFourQuadrantConverter, "ContFourQuadrantConverter": ga.ContFourQuadrantConverter,
                    "FiniteB6BridgeConverter": ga.FiniteB6BridgeConverter, "ContB6BridgeConverter": ga.ContB6BridgeConverter}
            names = meta["converter"].split("[")[1].rstrip("]").split(",")
            holder = ga.FiniteMultiConverter if meta["converter"].startswith("Finite") else ga.ContMultiConverter
            kw["converter"] = holder(subconverters=[subs[n](interlocking_time=til) for n in names])
    else:
        kw["converter"] = dict(interlocking_time=meta["interlocking_time"])
    if meta["load"] == "ConstantSpeedLoad":
        kw["load"] = ga.ConstantSpeedLoad(omega_fixed=meta["omega_fixed"])
    else:
        kw["load"] = ga.PolynomialStaticLoad(load_parameter=meta["load_parameter"])
    epi = meta["episodic"] if episodic is None else episodic
    if not epi:
        kw["constraints"] = ()
    elif isinstance(meta.get("constraints"), list):
        from constraint_cases import package_constraints

        kw["constraints"] = package_constraints(ga, meta["constraints"])
    # action-side wrappers / control space recorded by oracle/make_golden.py:run_case
    frame = meta.get("action_frame", "abc")
    wrappers = []
    if meta.get("dead_time_steps", 0):
        ra = meta.get("dead_time_reset_action")
        if ra is None:
            wrappers.append(ga.DeadTimeProcessor(steps=meta["dead_time_steps"]))
        else:  # a custom reset action recorded with the fixture (oracle/make_golden.py:main_reset_action): `steps` copies of one action
            one = [int(x) for x in ra] if "Finite" in meta["env_id"] else [float(x) for x in ra]
            one = one[0] if len(one) == 1 and "Finite" in meta["env_id"] else one
            wrappers.append(ga.DeadTimeProcessor(steps=meta["dead_time_steps"], reset_action=lambda one=one, n=meta["dead_time_steps"]: [one] * n))
    if frame == "dq_processor":
        wrappers.append(ga.DqToAbcActionProcessor.make("EESM" if "EESM" in meta["env_id"] else "PMSM"))
    if wrappers:
        kw["physical_system_wrappers"] = tuple(wrappers)
    if frame == "dq":
        kw["control_space"] = "dq"
    if meta["supply"] == "RCVoltageSupply":
        kw["supply"] = ga.RCVoltageSupply(u_nominal=meta["u_nominal"], supply_parameter=meta["supply_parameter"])
    # make-kwargs the fixture was recorded with (oracle/make_golden.py:main_params), exactly as passed to the reference: motor
    # parameters, limits and nominal values, an ideal supply's voltage, the load (the meta's own load rebuild above then gives way)
    ov = meta.get("overrides", {})
    for k in ("motor", "supply", "load"):
        if k in ov:
            kw[k] = json.loads(json.dumps(ov[k]))  # (a fresh copy: the components keep the dicts they are given)
    if "tau" in ov:
        assert kw["tau"] == ov["tau"]
    return ga.make(meta["env_id"], **kw, **extra)


def _param_overrides(name, omega_fixed=False):
    """The motor (and supply) make-kwargs a `param_*` fixture was recorded with, for tests that build their env from an env id;
    omega_fixed: also its ConstantSpeedLoad."""
    ov = _load(name)[1]["overrides"]
    out = {k: json.loads(json.dumps(ov[k])) for k in ("motor", "supply") if k in ov}
    if omega_fixed:
        import gym_electric_motor_amd as ga

        out["load"] = ga.ConstantSpeedLoad(omega_fixed=_load(name)[1]["omega_fixed"])
    return out


def _rel_err(got, ref, names, scale_ref=None):
    """max over columns of (max |got - ref|) / (max |ref| of that column); `scale_ref`: take the column ranges from this
    (longer) reference trajectory instead of `ref` itself."""
    diff = np.abs(got - ref)
    if "epsilon" in names:
        i = names.index("epsilon")
        diff[..., i] = np.minimum(diff[..., i], 2.0 - diff[..., i])
    sr = ref if scale_ref is None else scale_ref
    # floor: a column that never leaves 0.1 % of its limit is held to 1e-7 ABSOLUTE (normalised units) instead -- e.g. the
    # angle of a speed-control env that has barely started to turn (fp32 angle resolution: 2 pi / 2^32 rad per step)
    scale = np.maximum(np.abs(sr).reshape(-1, sr.shape[-1]).max(axis=0), 1e-3)
    return float((diff.reshape(-1, ref.shape[-1]).max(axis=0) / scale).max()), float(diff.max())


def _undefined_dq_steps_checked(meta, d, obs0, masks=None):
    """Steps that START with zero rotor flux (right after a reset; a squirrel-cage machine under zero voltage vectors): the reference's
    field angle there is arctan2 of ~1e-17 Wb of matmul rounding noise, so its dq COLUMNS on those steps are not reproducible by any
    restatement (oracle/oracle.py:undefined_field_angle_steps; at most two steps per episode, asserted in the oracle's own test).
    Rounds 1-3 copied the golden's dq columns over the device's there -- a wrong dq frame on exactly those steps could not fail.  Now
    the frame-independent content of those columns IS compared before they are taken out of the column-wise comparison:
      * |i_sdq|, |u_sdq|, |i_rdq|, |u_rdq| (physical units) against the reference's, 1e-4 of the column limit -- a rotation by the
        reference's noise angle leaves them alone; the abc / def columns and everything else stay in the normal comparison;
      * where the flux is EXACTLY zero this build's field angle is arctan2(0, 0) = 0 (known non-parity corners): its stator
        dq columns must then equal the alpha-beta quantities T23(abc) of its own row -- the device's frame convention, checked."""
    from oracle import oracle as orc

    names, lim = meta["state_names"], np.asarray(meta["limits"], dtype=np.float64)
    bad, zero = orc.undefined_field_angle_steps(orc.params_from_meta(meta, masks=masks), d["actions"], exact=True)  # (masks: a recorded custom constraint set)
    where = {int(k): i for i, k in enumerate(d["state_index"])}
    ks = np.array([k for k in np.nonzero(bad)[0] if int(k) in where], dtype=np.int64)
    if len(ks) == 0:
        return obs0
    js = np.array([where[int(k)] for k in ks], dtype=np.int64)
    ref = d["states"]
    for a, b in (("i_sd", "i_sq"), ("u_sd", "u_sq"), ("i_rd", "i_rq"), ("u_rd", "u_rq")):
        if a not in names:
            continue
        ia, ib = names.index(a), names.index(b)
        got = np.hypot(obs0[ks, ia] * lim[ia], obs0[ks, ib] * lim[ib])
        want = np.hypot(ref[js, ia] * lim[ia], ref[js, ib] * lim[ib])
        assert np.abs(got - want).max() <= 1e-4 * max(lim[ia], lim[ib]), (a, b, float(np.abs(got - want).max()))
    z = zero[ks]
    if z.any():
        for pre in ("i_s", "u_s"):
            ca, cb, cc, cd, cq = (names.index(pre + x) for x in "abcdq")
            xa, xb, xc = (obs0[ks[z], c] * lim[c] for c in (ca, cb, cc))
            alpha, beta = (2 * xa - xb - xc) / 3.0, (xb - xc) / np.sqrt(3.0)
            assert np.abs(obs0[ks[z], cd] * lim[cd] - alpha).max() <= 2e-5 * lim[cd], pre
            assert np.abs(obs0[ks[z], cq] * lim[cq] - beta).max() <= 2e-5 * lim[cq], pre
    out = obs0.copy()
    cols = [names.index(c) for c in orc.DQ_COLUMNS if c in names]
    out[np.ix_(ks, cols)] = ref[np.ix_(js, cols)]  # (verified above as far as the reference defines them)
    return out


def _oracle_solver_for(meta, sol):
    """The oracle's restatement of the integrator a device solver object selects: (solver name, nsteps) or None where it has none."""
    import gym_electric_motor_amd as ga

    if sol is None:
        sol = ga.default_ode_solver(meta["env_id"], tau=meta["tau"], load=meta["load"])
    kind = type(sol).__name__
    ns = int(getattr(sol, "_nsteps", 1))
    kink = bool(getattr(sol, "_split_kinks", False)) and meta["load"] != "ConstantSpeedLoad"
    if kind == "EulerSolver":
        return "euler", ns
    if kind == "RK4Solver":
        return ("rk4_kink" if kink else "rk4"), ns
    if kind == "DormandPrince5Solver":
        return ("dp5_kink", ns) if kink else (("dp5_fixed", 1) if ns == 1 else None)
    if kind == "ScipyOdeSolver":
        return "dopri5", 1  # (error-controlled on both sides: the reference default's tolerance, not its steps)
    return None


LANE_SAMPLE = (1, 31, 33, 63, 65, 68)  # lanes checked against the oracle: both halves of a wave, the wave boundary, the tail workgroup


def _run_golden(name, dtype, solver=None, n_envs=70, plain_make=False):
    """One recorded reference run through the device with n_envs envs.  Lanes 0, 64 and n_envs - 1 carry the RECORDED action sequence
    (compared with the golden by the caller; they must agree bit for bit among themselves); every other lane carries its OWN seeded
    random action stream (round 4: rounds 1-3 fed all lanes the same sequence, so a lane-dependent fault in a feature path -- RC
    supply, DeadTimeProcessor queue, dq action stage -- could not fail), and the lanes of LANE_SAMPLE are compared with the fp64
    oracle run on exactly their streams (episode by episode, done masks included).
    plain_make: the env is `make(env_id, n_envs=N)` and NOTHING else (the `default_*` fixtures: what a user of the 54 ids gets)."""
    import torch

    import gym_electric_motor_amd as ga

    d, meta = _load(name)
    if plain_make:
        assert solver is None and dtype == "float32"
        env = ga.make(meta["env_id"], n_envs=n_envs)
    else:
        env = _make_from_meta(meta, n_envs, solver=solver, dtype=dtype, auto_reset=True)
    ps = env.physical_system
    if plain_make:
        assert ps.tau == meta["tau"] and list(ps.state_names) == meta["state_names"]
        assert np.allclose(ps.limits, meta["limits"], rtol=1e-13, atol=0)
    assert np.abs(ps.reset_observation - d["reset_state"]).max() < 1e-12
    acts = d["actions"]
    K = acts.shape[0]
    a_np = np.repeat(acts.reshape(K, 1, -1), n_envs, axis=1).copy()
    import zlib

    rng = np.random.default_rng(zlib.crc32(name.encode()))
    recorded = sorted({0, 64 % n_envs, n_envs - 1})
    others = [j for j in range(n_envs) if j not in recorded]
    if ps._discrete:
        nvec = [int(v) for v in ps.action_space.nvec] if hasattr(ps.action_space, "nvec") else [int(ps.action_space.n)]
        assert a_np.shape[2] == len(nvec)
        for c, nv in enumerate(nvec):
            a_np[:, others, c] = rng.integers(0, nv, (K, len(others))).astype(a_np.dtype)
    else:
        a_np[:, others, :] = rng.uniform(-1.0, 1.0, (K, len(others), a_np.shape[2]))
    a = torch.as_tensor(a_np)
    if ps._discrete and acts.ndim == 1:
        a = a.reshape(K, n_envs)  # (MultiDiscrete actions stay [K, N, 2]: rollout() packs them into the flat index)
    sol_obj = ps._ode_solver
    obs, done = env.rollout(a.cuda())
    torch.cuda.synchronize()
    obs = obs.double().cpu().numpy()
    done = done.cpu().numpy().astype(bool)
    env.close()
    # lockstep determinism: the lanes that saw the same actions
    for j in recorded[1:]:
        assert np.array_equal(obs[:, 0], obs[:, j]) and np.array_equal(done[:, 0], done[:, j]), j
    _lanes_against_oracle(name, meta, a_np, obs, done, [j for j in LANE_SAMPLE if j < n_envs and j not in recorded], sol_obj, dtype, acts.ndim)
    obs0 = obs[:, 0].copy()
    if meta["system"] in ("DoublyFedInductionMotorSystem", "SquirrelCageInductionMotorSystem") and (
            meta["system"].startswith("Doubly") or name.startswith("default_")):
        obs0 = _undefined_dq_steps_checked(meta, d, obs0)
    return d, meta, obs0, done[:, 0]


def _constraint_margin(meta, d, masks=None):
    """|constraint value - 1| of the env's default constraint on the reference's (every-step) states.
    masks: (limit mask, squared mask) of a custom set instead: |max(max_i |x_i| over the limit mask, sum x_i^2 over the squared mask) - 1|."""
    assert meta["every"] == 1
    s = d["states"]
    names = meta["state_names"]
    if masks is not None:
        from constraint_cases import term_values

        # a limit column that IS the constant +-1.0 on every row (`u_sup` under an ideal supply, in "all_states") sits on the boundary by
        # construction and moves on neither side: it excuses no flip, the margin is that of the moving columns (the device's column is
        # held to exactly 1.0 where such a set runs: tests/test_gpu_constraints.py)
        const = sum(1 << i for i in range(s.shape[-1]) if (masks[0] >> i & 1) and (np.abs(s[..., i]) == 1.0).all())
        return np.abs(np.maximum(*term_values(meta, (masks[0] & ~const, masks[1]), s)) - 1.0)
    if meta["system"] == "ExternallyExcitedSynchronousMotorSystem":
        return np.minimum(np.abs(s[:, names.index("i_sd")] ** 2 + s[:, names.index("i_sq")] ** 2 - 1.0),
                          np.abs(np.abs(s[:, names.index("i_e")]) - 1.0))
    if meta["system"] == "DcMotorSystem" and meta["motor"] in ("DcShuntMotor", "DcExternallyExcitedMotor"):
        return np.minimum(np.abs(np.abs(s[:, names.index("i_a")]) - 1.0), np.abs(np.abs(s[:, names.index("i_e")]) - 1.0))
    if meta["system"] == "DcMotorSystem":
        return np.abs(np.abs(s[:, names.index("i")]) - 1.0)
    return np.abs(s[:, names.index("i_sd")] ** 2 + s[:, names.index("i_sq")] ** 2 - 1.0)


def _check_done(meta, d, got_done, ref_states_full=None):
    ref_done = d["terminated"]
    if np.array_equal(got_done, ref_done):
        return
    # tolerate flips only where the reference's constraint margin is tiny; needs every-step states
    margin = _constraint_margin(meta, d)
    first = int(np.argmax(got_done != ref_done))
    assert margin[first] < 1e-5, f"done mask differs at step {first} with margin {margin[first]:.3e}"


from parity_contract import FLUX_FLOOR, SIGN_MARGIN  # noqa: E402  (0.05: the 1e-4 contract holds as it stands while |psi_r| >= 5 % of its range over the run;
#                                                               2e-5: see below.  One place for both: tests/parity_contract.py, pinned against DESIGN.md section 2)


def compare_trajectory(meta, d, obs, done, min_fraction=0.0, psi=None, stop=None, per_step=False, masks=None, info=None):
    """Whole-trajectory comparison of one env's device rollout with a recorded reference run, EPISODE BY EPISODE: both sides restart
    from the reset state on the step after a termination, so as long as the done masks agree every episode is compared, not just the
    first.  A done flip is accepted only where the reference's constraint margin is < 1e-5 (fp32 vs fp64 at the boundary); from there
    on the two runs are out of phase for good (same action sequence, different episode starts), so the comparison ends at the flip.
    stop: compare steps < stop only (dead-time lanes: up to the first current-sign decision within rounding of zero).
    psi [K] (induction machines; the oracle's |psi_r| at the START of each step): the CONDITIONING of the field-oriented columns.  Their
    frame is eps_field = arctan2(psi_rbeta, psi_ralpha) (physical_systems.py:765-769), so a flux error d_psi turns every dq pair by
    d_psi / |psi_r|: an fp32 flux that is right to 1e-6 of its range -- what this function measures on the flux-driven abc columns --
    gives 1e-4 on u_sd once |psi_r| falls to 1 % of the range (random switching walks the flux through zero; round 4 recorded 1.6e-4
    on u_sd of Finite-TC-DFIM at |psi_r| = 1.2e-4 Wb of 0.35).  No arithmetic in the observation can undo that; the contract for those
    columns is therefore stated on what is well-posed:
      * the dq columns' error WEIGHTED by min(1, |psi_r| / (FLUX_FLOOR max|psi_r|)) within the tolerance -- i.e. 1e-4 as it stands
        wherever the flux is above 5 % of its range, and the flux itself within 5e-6 of its range below;
      * the rotation-invariant content, |i_sdq|, |u_sdq|, |i_rdq|, |u_rdq|, within the tolerance at EVERY step, unweighted.
    masks: the margin of a custom constraint set (_constraint_margin) instead of the env's default one.
    info: a dict that receives flip_step (None: no accepted flip), flip_margin and compared (the number of steps compared).
    Returns (worst rel err, max abs err, worst column, description of the done-mask comparison); per_step: the worst relative error
    of every compared step instead (an array)."""
    names = meta["state_names"]
    idx, ref, ref_done = d["state_index"], d["states"], d["terminated"]
    K = len(ref_done)
    n_cmp, dmsg = K, "free run"
    flip_step = flip_margin = None
    if meta["episodic"]:
        if np.array_equal(done, ref_done):
            dmsg = f"identical, {int(ref_done.sum())} terminations"
        else:
            first = int(np.argmax(done != ref_done))
            if stop is None or first < stop:
                margin = _constraint_margin(meta, d, masks=masks)[first]
                assert margin < 1e-5, f"done mask differs at step {first} with margin {margin:.3e}"
                n_cmp = first + 1  # the state returned by step `first` is still the same episode on both sides
                flip_step, flip_margin = first, float(margin)
                dmsg = f"flip at step {first} (reference margin {margin:.1e}): {n_cmp}/{K} steps, {int(ref_done[:first].sum())} terminations compared"
    if stop is not None and stop < n_cmp:
        n_cmp = stop
        dmsg += f"; compared up to step {stop} (first current-sign decision within rounding of zero)"
    assert n_cmp >= min_fraction * K, dmsg
    if info is not None:
        info.update(flip_step=flip_step, flip_margin=flip_margin, compared=n_cmp)
    sel = idx < n_cmp
    diff = np.abs(obs[idx[sel]] - ref[sel])
    if "epsilon" in names:
        i = names.index("epsilon")
        diff[:, i] = np.minimum(diff[:, i], 2.0 - diff[:, i])
    scale = np.maximum(np.abs(ref).max(axis=0), 1e-3)
    if psi is not None and "InductionMotorSystem" in meta["system"]:
        from oracle import oracle as orc

        w = np.minimum(1.0, psi[idx[sel]] / (FLUX_FLOOR * max(float(psi.max()), 1e-30)))
        lim = np.asarray(meta["limits"], dtype=np.float64)
        for a, b in (("i_sd", "i_sq"), ("u_sd", "u_sq"), ("i_rd", "i_rq"), ("u_rd", "u_rq")):
            if a not in names:
                continue
            ia, ib = names.index(a), names.index(b)
            got = np.hypot(obs[idx[sel], ia] * lim[ia], obs[idx[sel], ib] * lim[ib])
            want = np.hypot(ref[sel, ia] * lim[ia], ref[sel, ib] * lim[ib])
            mag = np.abs(got - want) / max(lim[ia] * scale[ia], lim[ib] * scale[ib])  # |pair|: rotation invariant, unweighted
            diff[:, ia] = np.maximum(diff[:, ia] * w, mag * scale[ia])
            diff[:, ib] = np.maximum(diff[:, ib] * w, mag * scale[ib])
        assert set(n for n in names if n.endswith(("d", "q")) and n[0] in "iu") <= set(orc.DQ_COLUMNS)
    if per_step:
        return (diff / scale).max(axis=1)
    per_col = diff.max(axis=0) / scale
    j = int(np.argmax(per_col))
    return float(per_col[j]), float(diff.max()), names[j], dmsg


# SIGN_MARGIN (tests/parity_contract.py: 2e-5): dead-time lanes -- a current-sign decision is "within rounding of zero" below this fraction of the current limit


def _lanes_against_oracle(name, meta, a_np, obs, done, lanes, sol_obj, dtype, acts_ndim, masks=None, stats=None):
    """Sampled lanes of a device rollout, each on its OWN action stream, against the fp64 oracle with the same integrator (episode by
    episode, done masks included).  Induction machines: field-oriented columns by their conditioning (compare_trajectory, psi).
    Converter dead time: a dead leg's voltage follows the SIGN of its phase current (converters.py:277-285, 144-158), so an fp32 run
    and the fp64 oracle part ways for good when a stream catches a current within rounding of zero at such a decision and the two
    decide it differently.  Rounds 1-4 skipped these lanes altogether; now a lane is compared over the whole run, and a divergence
    is accepted only if it BEGINS at a step where the oracle's decision margin is below SIGN_MARGIN of the current limit (then the
    lane is compared up to that step) -- a lane that leaves the oracle anywhere else fails.
    masks: (limit mask, squared mask) of a custom constraint set: the oracle terminates by it, and a done flip is judged by its margin.
    stats: a list that receives one dict per lane (lane, rel, col, compared steps, flip or not, what the done comparison said)."""
    from oracle import oracle as orc

    osol = _oracle_solver_for(meta, sol_obj)
    if osol is None:
        return None
    p = orc.params_from_meta(meta, solver=osol[0], masks=masks)
    p.nsteps = osol[1]
    K = a_np.shape[0]
    meta1 = dict(meta, every=1)
    names = meta["state_names"]
    i_lim = max(meta["limits"][names.index(c)] for c in names if c.startswith("i"))
    worst, covered = 0.0, []
    for j in lanes:
        e = orc.OracleEnv(p)
        e.reset()
        aj = a_np[:, j, :] if acts_ndim > 1 else a_np[:, j, 0]
        ro, rd, psi, margin = e.rollout_diag(aj.astype(np.float64), auto_reset=True)
        dj = {"states": ro, "terminated": rd, "state_index": np.arange(K)}
        same = osol[0] != "dopri5"
        # fp32: the north star's 1e-4, whatever the solver pair (round 4 allowed the error-controlled pair 3e-4 to cover the DFIM's
        # ill-conditioned steps; those are now weighted by their conditioning instead).  fp64, same integrator: 1e-7.
        tol = 1e-4 if dtype == "float32" or not same else 1e-7
        psi_j = psi if "InductionMotorSystem" in meta["system"] else None
        stop = None
        if meta["interlocking_time"] > 0:
            free = dict(meta1, episodic=False)  # (step by step, done masks aside: they are compared below, up to `stop`)
            over = np.nonzero(compare_trajectory(free, dj, obs[:, j], done[:, j], psi=psi_j, per_step=True, masks=masks) >= tol)[0]
            flips = np.nonzero(done[:, j] != rd)[0]  # (a done flip at the constraint boundary comes first: compare_trajectory's business)
            if len(over) and (len(flips) == 0 or over[0] <= flips[0]):
                stop = int(over[0])
                assert margin[stop] < SIGN_MARGIN * i_lim, (name, "lane", j, "leaves the oracle at step", stop, "where no current-sign decision is near zero",
                                                            float(margin[stop]), i_lim)
        info = {}
        rel, ab, col, dmsg = compare_trajectory(meta1, dj, obs[:, j], done[:, j], min_fraction=0.0 if stop is not None else 0.3, psi=psi_j, stop=stop,
                                                masks=masks, info=info)
        covered.append(K if stop is None else stop)
        if stats is not None:
            stats.append(dict(lane=j, rel=rel, col=col, compared=info["compared"], flip=info["flip_step"] is not None, flip_margin=info["flip_margin"],
                              done=dmsg, terminations=int(rd.sum())))
        assert rel < tol, (name, "lane", j, rel, col, dmsg)
        worst = max(worst, rel)
    if meta["interlocking_time"] > 0:  # the dead-time lanes together must still cover a fair share of the run
        assert sum(covered) >= 0.5 * K * len(lanes), (name, covered)
    return worst


SAME_SOLVER = [c for c in CASES if c.endswith("euler") or c.endswith("euler4")]
DEFAULTS = [c for c in CASES if c.startswith("default_")]  # gem.make(env_id) with nothing else, all 54 ids (oracle/make_golden.py:main_defaults)
DOPRI = [c for c in CASES if c.endswith("dopri5") and c not in DEFAULTS]


@pytest.mark.parametrize("name", SAME_SOLVER)
def test_fp32_euler_matches_reference_euler(name):
    d, meta, obs, done = _run_golden(name, "float32")
    rel, _ = _rel_err(obs[d["state_index"]], d["states"], meta["state_names"])
    assert rel < 1e-4, rel
    if meta["episodic"]:
        _check_done(meta, d, done)


@pytest.mark.parametrize("name", SAME_SOLVER)
def test_fp64_euler_matches_reference_euler(name):
    d, meta, obs, done = _run_golden(name, "float64")
    _, ab = _rel_err(obs[d["state_index"]], d["states"], meta["state_names"])
    assert ab < 1e-9, ab
    if meta["episodic"]:
        assert np.array_equal(done, d["terminated"])


@pytest.mark.parametrize("name", DEFAULTS)
def test_make_env_id_as_the_user_gets_it_matches_the_reference_default_solver(name):
    """`gym_electric_motor_amd.make(env_id, n_envs=N)` and NOTHING else -- the env's own supply, converter, motor, load, tau, constraints
    and the solver make() picks (envs.default_ode_solver) -- against `gem.make(env_id)` with the reference's default solver (scipy
    dopri5), for every one of the reference's 54 env ids: fp32 within 1e-4, episode by episode, done masks exact (margin-guarded).
    Lanes 0 / 64 / 69 replay the recorded sequence (against the recording); the sampled other lanes run their own random streams and
    are held to the same 1e-4 against the fp64 oracle with the integrator make() picked (round 5: the per-lane check used to leave
    this test out -- and Finite-TC-DFIM's u_sd on a random lane sat at 1.6e-4 unasserted; see compare_trajectory on the conditioning
    of the field-oriented columns)."""
    d, meta, obs0, done0 = _run_golden(name, "float32", plain_make=True)
    rel, _, col, dmsg = compare_trajectory(meta, d, obs0, done0, min_fraction=0.5)
    assert rel < 1e-4, (rel, col, dmsg)


@pytest.mark.parametrize("name", DOPRI)
@pytest.mark.parametrize("scheme", ["rk4", "dp5"])
def test_fp32_fixed_step_matches_reference_default_dopri5(name, scheme):
    """Both fixed-step schemes of the device, with the sub-stepping / kink splitting make() would choose for the fixture's env id, control
    step and load (envs.default_ode_solver -- the product's rule, not a test-side rewrite), against the reference's default solver."""
    import gym_electric_motor_amd as ga

    _, meta0 = _load(name)
    s = ga.default_ode_solver(meta0["env_id"], tau=meta0["tau"], load=meta0["load"])
    solver = (ga.RK4Solver if scheme == "rk4" else ga.DormandPrince5Solver)(nsteps=s._nsteps, split_kinks=s._split_kinks)
    d, meta, obs, done = _run_golden(name, "float32", solver=solver)
    # north-star tolerance for EVERY system (round 1 held SCIM + PolynomialStaticLoad to 2e-4); episodic runs episode by episode
    rel, _, col, dmsg = compare_trajectory(meta, d, obs, done)
    assert rel < 1e-4, (rel, col, dmsg)


@pytest.mark.parametrize("name", [c for c in DOPRI if "_sc_" not in c and not c.startswith("scim_") and "refdata" not in c])
def test_fp32_plain_rk4_on_constant_speed_loads_matches_reference_default_dopri5(name):
    """One classical RK4 step per control step, no options: the headline's solver, on every recorded dopri5 run of an env whose speed is
    held by a ConstantSpeedLoad (linear electrical subsystem)."""
    d, meta, obs, done = _run_golden(name, "float32", solver="rk4")
    if meta["load"] != "ConstantSpeedLoad":
        pytest.skip("speed-dependent load")
    rel, _, col, dmsg = compare_trajectory(meta, d, obs, done)
    assert rel < 1e-4, (rel, col, dmsg)


@pytest.mark.parametrize("name", ["pmsm_free_held_til_dopri5", "pmsm_free_uniform_til_dopri5", "dfim_fin_free_held_til_dopri5"])
@pytest.mark.parametrize("nsteps", [1, 8])
def test_dead_time_maps_keep_the_stage_by_stage_accuracy(name, nsteps):
    """Converter dead time through the per-segment one-step maps must be as accurate as the stage-by-stage solver: a map formed in fp32
    as I + D loses D to an absolute 6e-8, i.e. 1e-3 of the decay over a 1 us segment -- the first version of these maps took the PMSM
    fixtures from 7.7e-7 to 7.5e-6 and, sub-stepped, flipped a freewheeling leg (u_a off by 2.0).  Maps evaluated in double, D-form for the
    dead-time segments, none for sub-stepped solvers: within 1.5x + 1e-6 of the run with GEMX_LINMAP=0, and far inside the contract."""
    import gym_electric_motor_amd as ga

    errs = {}
    for lm in ("1", "0"):
        os.environ["GEMX_LINMAP"] = lm
        try:
            d, meta, obs, done = _run_golden(name, "float32", solver=ga.RK4Solver(nsteps=nsteps))
        finally:
            os.environ.pop("GEMX_LINMAP", None)
        errs[lm] = compare_trajectory(meta, d, obs, done)[0]
    assert errs["1"] < 1.5 * errs["0"] + 1e-6 and errs["1"] < 2e-5, errs


ADAPTIVE_CASES = DOPRI + [c for c in DEFAULTS if "_sc_" in c or "_tc_" in c][::3]


@pytest.mark.parametrize("name", ADAPTIVE_CASES)
def test_error_controlled_solver_tracks_the_reference_default_solver(name):
    """GEMX_SOLVER_ADAPTIVE (ga.ScipyOdeSolver(): Dormand-Prince 5(4) with the embedded error estimate, rtol 1e-6 in scipy's norm, each
    lane cutting its own steps) against the runs the reference's default solver -- scipy's adaptive dopri5 at the same tolerance --
    recorded: every dopri5 fixture of every machine and a third of the speed- and torque-control default fixtures, fp32, within the
    north star's 1e-4 (observed: the fp32 noise floor of the machine, a few 1e-6), done masks exact, and the tolerance flag down."""
    import gym_electric_motor_amd as ga

    d, meta, obs, done = _run_golden(name, "float32", solver=ga.ScipyOdeSolver())
    rel, _, col, dmsg = compare_trajectory(meta, d, obs, done)
    assert rel < 1e-4, (rel, col, dmsg)


@pytest.mark.parametrize("name", ["scim_free_held_dopri5", "pmsm_sc_free_held_dopri5", "permexdc_epi_held_dopri5", "synrm_cont_sc_epi_held_dopri5",
                                  "pmsm_epi_uniform_tau1e-4_dopri5"])
def test_error_controlled_solver_fp64_against_the_reference_default_solver(name):
    """The fp64 build of the same code against the reference's dopri5 runs: two error-controlled integrations at rtol 1e-6 with different
    step sequences stay within a few 1e-6 of each other (bound 2e-5), where the device's fixed steps are at 1e-5 ... 7e-5."""
    import gym_electric_motor_amd as ga

    d, meta, obs, done = _run_golden(name, "float64", solver=ga.ScipyOdeSolver())
    rel, _, col, dmsg = compare_trajectory(meta, d, obs, done)
    assert rel < 2e-5, (rel, col, dmsg)


@pytest.mark.parametrize("name", ["scim_epi_uniform_euler", "pmsm_sc_free_held_dopri5", "scim_free_held_dopri5", "permexdc_sc_free_held_dopri5",
                                  # non-default machines, PolynomialStaticLoad with c != 0 (oracle/make_golden.py:main_params)
                                  "param_scim_cont_sc_free_held_dopri5", "param_pmsm_cont_sc_free_held_dopri5", "param_permexdc_cont_sc_u80_free_held_dopri5",
                                  "param_dfim_cont_sc_free_held_dopri5", "param_series_cont_sc_free_held_dopri5"])
@pytest.mark.parametrize("split_kinks", [True, False])
def test_error_controlled_solver_fp64_equals_its_cpu_restatement(name, split_kinks):
    """Round 6: the device's error controller -- carried proposal, first try = segment / ceil(0.9 segment / proposal), rejections cut by
    clamp(0.9 err^-1/5, 0.2, 1), omega's absolute tolerance in normalised units and, with split_kinks, every attempt on the smooth model
    system with the kink's defect in closed form -- is restated step for step in the test infrastructure (ORC_SOLVER_DEV_ADAPTIVE[_KINK]),
    which is where its wave statistics come from (tools/wave_step_statistics.py).  The fp64 build must reproduce that restatement:
    same accept / reject decisions, same sub-steps -- 1e-9 absolute over per-lane random action streams with auto-resets, done masks equal."""
    import torch

    import gym_electric_motor_amd as ga
    from oracle import oracle as orc

    d, meta = _load(name)
    n, K = 6, min(1200, d["actions"].shape[0])
    env = _make_from_meta(meta, n, solver=ga.ScipyOdeSolver(split_kinks=split_kinks), dtype="float64", auto_reset=True)
    ps = env.physical_system
    rng = np.random.default_rng(11)
    a = rng.uniform(-1.0, 1.0, (K, n, ps._n_act))
    a[K // 2:] = a[K // 2]  # (second half held: long smooth stretches, the carried proposal at work)
    obs, done = env.rollout(torch.as_tensor(a, device="cuda"))
    ps.check_errors()
    obs, done = obs.cpu().numpy(), done.cpu().numpy().astype(bool)
    env.close()
    L = orc.lib()
    L.orc_dev_set_atol_omega_scaled(1)
    try:
        p = orc.params_from_meta(meta, solver="dev_adaptive_kink" if split_kinks else "dev_adaptive")
        for j in range(n):
            e = orc.OracleEnv(p)
            e.reset()
            ro, rd = e.rollout(a[:, j], auto_reset=True)
            diff = np.abs(obs[:, j] - ro)
            k_eps = list(meta["state_names"]).index("epsilon") if "epsilon" in meta["state_names"] else None
            if k_eps is not None:
                diff[:, k_eps] = np.minimum(diff[:, k_eps], 2.0 - diff[:, k_eps])
            assert (rd == done[:, j]).all(), (name, j)
            assert diff.max() < 1e-9, (name, split_kinks, j, float(diff.max()), int(np.argmax(diff.max(axis=1))))
    finally:
        L.orc_dev_set_atol_omega_scaled(0)


def test_error_controlled_solver_is_the_same_in_every_kernel_and_chunking():
    """One fused rollout == the same steps in uneven chunks == step by step (gemx_step), and the pipelined kernel == the single-wave
    kernel: the step-size decisions are per control step and per lane, so nothing may depend on how the steps are batched."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 256, 60
    outs = {}
    for tag, pipe in (("pipe", "1"), ("wave", "0")):
        os.environ["GEMX_PIPE"] = pipe
        try:
            env = ga.make("Cont-SC-SCIM-v0", n_envs=n, ode_solver=ga.ScipyOdeSolver(), tau=1e-4)
            g = torch.Generator(device="cuda").manual_seed(11)
            acts = torch.rand((K, n, 3), device="cuda", generator=g) * 2 - 1
            env.reset()
            obs, done = env.rollout(acts)
            outs[tag] = (obs.clone(), done.clone(), env.physical_system.last_launch())
            if tag == "pipe":
                env.reset()
                parts = [env.rollout(acts[a:b]) for a, b in ((0, 7), (7, 8), (8, 41), (41, K))]
                assert torch.equal(torch.cat([p[0] for p in parts]), obs) and torch.equal(torch.cat([p[1] for p in parts]), done)
                env.reset()
                ps = env.physical_system
                for k in range(K):
                    o = ps.simulate(acts[k])
                    assert torch.equal(o, obs[k]), k
            env.physical_system.check_errors()
            env.close()
        finally:
            os.environ.pop("GEMX_PIPE", None)
    assert "advance_pipe_kernel" in outs["pipe"][2] and "advance_kernel" in outs["wave"][2]
    assert torch.equal(outs["pipe"][0], outs["wave"][0]) and torch.equal(outs["pipe"][1], outs["wave"][1])


def test_error_controlled_solver_raises_its_flag_at_the_floor():
    """A tolerance below the arithmetic's resolution (rtol 1e-12 in fp32) cannot be met: the steps end at the floor of 1/1024 of the
    control step and bit GEMX_ERRFLAG_TOLERANCE goes up -- check_errors() warns.  At the default tolerance the flag stays down."""
    import warnings

    import torch

    import gym_electric_motor_amd as ga

    for rtol, expect in ((1e-6, False), (1e-12, True)):
        env = ga.make("Cont-SC-PMSM-v0", n_envs=128, ode_solver=ga.ScipyOdeSolver(rtol=rtol, atol=1e-30 if expect else 1e-9), tau=1e-4)
        env.reset()
        g = torch.Generator(device="cuda").manual_seed(3)
        env.rollout(torch.rand((50, 128, 3), device="cuda", generator=g) * 2 - 1)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            env.physical_system.check_errors()
        assert any("error-controlled" in str(x.message) for x in w) == expect, (rtol, [str(x.message) for x in w])
        env.close()


SCIM_POLY_DOPRI = [c for c in DOPRI if c.startswith("scim_") and "constspeed" not in c]


# the free-running non-default machines behind a PolynomialStaticLoad with its quadratic term on (c != 0)
PARAM_POLY_DOPRI = [c for c in DOPRI if c.startswith("param_") and "_sc_" in c and "_epi_" not in c]


@pytest.mark.parametrize("name", SCIM_POLY_DOPRI + ["pmsm_sc_free_held_dopri5", "permexdc_sc_free_held_dopri5", "refdata_cont_sc_permexdc_dopri5"] + PARAM_POLY_DOPRI)
@pytest.mark.parametrize("solver", ["rk4k", "dp5k"])
def test_split_kinks_tracks_the_reference_adaptive_solver(name, solver):
    """GEMX_SOLVER_SPLIT_KINKS (RK4Solver / DormandPrince5Solver(split_kinks=True)): steps cut at the PolynomialStaticLoad's kinks, the
    device's stand-in for scipy dopri5's step-size control.  fp32 against the reference's default-solver trajectories: 3e-5 (plain
    fixed steps: up to 7.2e-5 on the same fixtures, profiles/r02_parity.md); fp64 against the oracle's restatement of the same
    algorithm (oracle/gemx_oracle.c:integrate_kink): 1e-9."""
    from oracle import oracle as orc

    d, meta, obs, done = _run_golden(name, "float32", solver=solver)
    rel, _, col, dmsg = compare_trajectory(meta, d, obs, done)
    assert rel < 3e-5, (rel, col, dmsg)
    if name.startswith("scim_free") or name.startswith("pmsm_sc") or name.startswith("param_"):
        d, meta, obs64, _ = _run_golden(name, "float64", solver=solver)
        e = orc.OracleEnv(orc.params_from_meta(meta, solver={"rk4k": "rk4_kink", "dp5k": "dp5_kink"}[solver], episodic=False))
        e.reset()
        ref, _ = e.rollout(d["actions"])
        _, ab = _rel_err(obs64, ref, meta["state_names"])
        assert ab < 1e-9, ab


@pytest.mark.parametrize("name", ["scim_epi_uniform_euler", "synrm_cont_sc_epi_held_euler"])
def test_split_kinks_is_bit_identical_across_kernels(name, monkeypatch):
    """The piece loop (wave-level: lanes that are done ride along with h = 0) gives the same bits in the single-wave kernel, every
    pipelined shape and step-by-step through step_kernel."""
    import torch

    outs = []
    for env in ({"GEMX_PIPE": "0"}, {"GEMX_PIPE": "1", "GEMX_PIPE_SHAPE": "0"}, {"GEMX_PIPE": "1", "GEMX_PIPE_SHAPE": "1"},
                {"GEMX_PIPE": "1", "GEMX_PIPE_SHAPE": "2"}):
        for k in ("GEMX_PIPE", "GEMX_PIPE_SHAPE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _, meta, obs, done = _run_golden(name, "float32", solver="rk4k", n_envs=128)
        outs.append((obs, done))
    for o, dn in outs[1:]:
        assert np.array_equal(o, outs[0][0]) and np.array_equal(dn, outs[0][1])
    d, meta = _load(name)
    env = _make_from_meta(meta, 128, solver="rk4k", auto_reset=True)
    ps = env.physical_system
    acts = torch.as_tensor(np.repeat(d["actions"][:60].reshape(60, 1, -1), 128, axis=1)).cuda()
    for k in range(60):
        o = ps.simulate(acts[k])
        assert np.array_equal(o[0].double().cpu().numpy(), outs[0][0][k])
    assert ("step_kernel" in ps.last_launch()) == (os.environ.get("GEMX_STEP_KERNEL", "1") != "0")
    env.close()


def test_ref_data_npz_on_gpu():
    """The reference's own golden trajectory (tests/integration_tests/ref_data.npz), DP5 fp32 and fp64."""
    for dtype, tol in (("float32", 1e-4), ("float64", 1e-7)):
        d, meta, obs, done = _run_golden("refdata_cont_sc_permexdc_dopri5", dtype, solver="dp5")
        rel, _ = _rel_err(obs, d["states"], meta["state_names"])
        assert rel < tol, (dtype, rel)
        assert not done.any()


def test_fixed_step_rk4_matches_reference_solve_ivp_path():
    """BASELINE config 1's solver: ScipySolveIvpSolver (solvers.py:187-219).  At rtol 1e-10 / atol 1e-12 it is the exact solution to
    ~1e-9, so GPU RK4 / DP5 fp32 must agree within the 1e-4 contract over 10 k steps.  (With its DEFAULT tolerances the reference's
    solve_ivp path is itself 5e-4 off its own default solver -- rtol 1e-3 plus the aliased-RHS quirk restated in
    oracle/gemx_oracle.c:ivp_rk45 -- so that fixture pins the oracle, not the device.)"""
    for solver in ("rk4", "dp5"):
        d, meta, obs, done = _run_golden("permexdc_free_uniform_10k_ivp_tight", "float32", solver=solver)
        rel, _, col, _ = compare_trajectory(meta, d, obs, done)
        assert rel < 1e-4, (solver, rel, col)


@pytest.mark.parametrize("mode", ["pipe0", "shape0", "shape1", "shape2", "shape3"])
def test_bench_configuration_episodic_rk4_against_reference_default_solver(mode, monkeypatch):
    """The bench's own instantiation -- Finite-CC-PMSM-v0, tau 1e-4, RK4 through the one-step affine map + per-action voltage table,
    default constraint + in-kernel auto-reset, uniformly random switching -- against the reference's default solver (dopri5) over 6000
    steps / ~109 episodes, through every pipelined shape and the single-wave kernel: done masks with the margin guard, trajectories
    episode by episode (not just up to the first termination)."""
    if mode == "pipe0":
        monkeypatch.setenv("GEMX_PIPE", "0")
    else:
        monkeypatch.setenv("GEMX_PIPE", "1")
        monkeypatch.setenv("GEMX_PIPE_SHAPE", mode[-1])
    d, meta, obs, done = _run_golden("pmsm_epi_uniform_tau1e-4_dopri5", "float32", solver="rk4", n_envs=128)
    assert d["terminated"].sum() > 50
    rel, _, col, dmsg = compare_trajectory(meta, d, obs, done, min_fraction=0.5)
    assert rel < 1e-4, (rel, col, dmsg)


@pytest.mark.parametrize("env_id, n_envs, solver", [
    ("Cont-CC-PermExDc-v0", 4096, "euler"),   # BASELINE config 2
    ("Finite-CC-PMSM-v0", 16384, "rk4"),      # BASELINE config 3 (the bench headline: one-step map + voltage table + <12, 3> shape)
    ("Finite-CC-PMSM-v0", 32768, "rk4"),      # BASELINE config 5's per-GPU shard (8 x 32768): the <4, 2> shape
    ("Finite-CC-PMSM-v0", 32768, "default"),  # ... as bench.py's `configs.pmsm_32768` builds it: make() with no solver named, rate limiter on
    ("Cont-SC-SCIM-v0", 65536, "rk4"),        # BASELINE config 4 with the env's own PolynomialStaticLoad, plain RK4 (`scim_plain_rk4`)
    ("Cont-SC-SCIM-v0", 65536, "default"),    # ... as bench.py's `configs.scim` measures it: the solver make() hands out = RK4 + kink correction,
                                              #     <2, 2> shape under the rate limiter, against the oracle's restatement of that scheme (rk4_kink)
    ("Cont-SC-SCIM-v0:constspeed", 65536, "rk4"),  # BASELINE config 4 as BASELINE.json words it: + ConstantSpeedLoad (one-step map)
])
def test_full_size_configs_against_oracle(env_id, n_envs, solver):
    """BASELINE.json sizes exactly as bench.py runs them: default constraints + in-kernel auto-reset, tau = 1e-4, per-env random
    actions, K = 1000 control steps in ONE fused launch.  64 sampled envs (first / last lanes of workgroups, both halves of the
    grid) are checked step by step against the fp64 oracle with the SAME integrator -- trajectories episode by episode, done masks
    exactly (flips only within 1e-5 of the constraint boundary) -- all envs for finiteness and a plausible termination count, and
    step-by-step simulate() == the fused rollout bit for bit.  The kernel instantiation and shape the launcher picked are asserted
    from gemx_last_launch(): what is compared here IS what bench.py times."""
    _full_size_check(env_id, n_envs, solver, 1000)


def test_headline_ten_thousand_step_fused_launch_against_oracle():
    """The north star's horizon in ONE launch: BASELINE config 3 (Finite-CC-PMSM-v0, 16384 envs, RK4, tau 1e-4), 10 000 control steps
    fused (9.2 GB of observation rows), 64 sampled envs against the fp64 oracle over all 10 000 steps and ~180 episodes each."""
    _full_size_check("Finite-CC-PMSM-v0", 16384, "rk4", 10000, single_step_check=False)


def _full_size_check(env_id, n_envs, solver, K, single_step_check=True):
    import torch

    import gym_electric_motor_amd as ga
    from oracle import oracle as orc

    sol = {"euler": ga.EulerSolver(), "rk4": ga.RK4Solver(), "default": None}[solver]  # default: whatever make() hands out (bench.py: make_env)
    env_id, _, variant = env_id.partition(":")
    golden = {"Cont-CC-PermExDc-v0": "permexdc_epi_held_euler", "Finite-CC-PMSM-v0": "pmsm_epi_held_tau1e-4_euler",
              "Cont-SC-SCIM-v0": "scim_epi_uniform_euler"}[env_id]
    if variant == "constspeed":
        golden = "scim_constspeed_free_held_euler"
    _, meta = _load(golden)
    mkw = dict(load=ga.ConstantSpeedLoad(omega_fixed=meta["omega_fixed"])) if variant == "constspeed" else {}
    env = ga.make(env_id, n_envs=n_envs, ode_solver=sol, tau=1e-4, **mkw)
    ps = env.physical_system
    g = torch.Generator(device="cuda").manual_seed(1234)
    if ps._discrete:
        acts = torch.randint(0, 8, (K, n_envs), device="cuda", generator=g, dtype=torch.uint8)
    else:
        acts = torch.rand((K, n_envs, ps._n_act), device="cuda", generator=g) * 2 - 1
    obs, done = env.rollout(acts)
    torch.cuda.synchronize()
    # the kernel the bench measures (BASELINE config 2, a small batch of a DC machine behind a constant-speed load: dc_stream_kernel)
    ll = ps.last_launch()
    assert ("dc_stream_kernel" if "PermExDc" in env_id else "advance_pipe_kernel") in ll, ll
    assert "overrides" not in ll, ll  # no GEMX_* switch changed what ran
    if n_envs > 64 * 256:  # more workgroups than CUs: the large-batch rate limiter is part of the measured launch
        assert "rate limit" in ll or "limiter calibrat" in ll, ll
    want_shape = {("Finite-CC-PMSM-v0", 16384): "D=12", ("Finite-CC-PMSM-v0", 32768): "D=4", ("Cont-SC-SCIM-v0", 65536): "D=2"}.get((env_id, n_envs))
    if want_shape is not None and not variant:
        assert want_shape + ">" in ll, ll
    osol = _oracle_solver_for(dict(meta, env_id=env_id, tau=1e-4), ps._ode_solver)
    assert osol is not None and osol[1] == 1
    if solver == "default" and "SCIM" in env_id:
        assert osol[0] == "rk4_kink"
    assert torch.isfinite(obs).all()
    # single-step path must give the same bits as the fused path (incl. the auto-reset)
    if single_step_check:
        env2 = ga.make(env_id, n_envs=n_envs, ode_solver=sol, tau=1e-4, **mkw)
        for k in range(40):
            o = env2.physical_system.simulate(acts[k])
            assert torch.equal(o, obs[k]) and torch.equal(env2.physical_system.done, done[k])
        env2.close()
    meta = dict(meta, tau=1e-4)
    p = orc.params_from_meta(meta, solver=osol[0], episodic=True)
    names = meta["state_names"]
    rng = np.random.default_rng(7)
    sample = sorted(set([0, 1, 63, 64, 127, n_envs // 2 - 1, n_envs // 2, n_envs // 2 + 17, n_envs - 64, n_envs - 1]) |
                    set(int(x) for x in rng.integers(0, n_envs, 54)))
    assert len(sample) >= 60
    idx = torch.as_tensor(sample, device="cuda")
    a_host = acts[:, idx].cpu().numpy().astype(np.float64)
    o_host = obs[:, idx].double().cpu().numpy()
    d_host = done[:, idx].cpu().numpy().astype(bool)
    worst, n_term, n_flip, n_cmp = 0.0, 0, 0, 0
    for c, j in enumerate(sample):
        e = orc.OracleEnv(p)
        e.reset()
        ref, rdone = e.rollout(a_host[:, c], auto_reset=True)
        d = {"state_index": np.arange(K), "states": ref, "terminated": rdone}
        rel, _, col, dmsg = compare_trajectory(dict(meta, every=1, episodic=True), d, o_host[:, c], d_host[:, c])
        assert rel < 1e-4, (j, rel, col, dmsg)
        worst = max(worst, rel)
        n_term += int(rdone.sum())
        n_flip += "flip" in dmsg
    total_done = int(done.sum().item())
    env.close()
    assert n_term > len(sample)            # every sampled env terminated (and restarted) more than once on average
    assert n_flip <= len(sample) // 8      # boundary flips are the exception
    assert abs(total_done / n_envs - n_term / len(sample)) < 0.25 * n_term / len(sample)  # all envs: same termination rate as the sample
    print(f"{env_id} N={n_envs} {solver} (oracle {osol[0]}): worst rel err {worst:.2e} over {len(sample)} envs x {K} steps, {n_term} terminations, {n_flip} flips; {ll}")


@pytest.mark.parametrize("env_id, golden, til", [
    ("Cont-CC-ExtExDc-v0", "extex_cont_free_held_euler", 0.0), ("Cont-SC-ExtExDc-v0", "extex_cont_sc_free_held_euler", 2e-6),
    ("Finite-CC-ExtExDc-v0", "extex_fin_free_held_euler", 0.0), ("Finite-CC-ExtExDc-v0", "extex_fin_free_held_til_euler", 1e-6),
    ("Cont-CC-EESM-v0", "eesm_cont_free_held_euler", 0.0), ("Cont-SC-EESM-v0", "eesm_cont_sc_epi_held_euler", 0.0),
    ("Finite-CC-EESM-v0", "eesm_fin_free_held_euler", 0.0),
    ("Cont-CC-DFIM-v0", "dfim_cont_free_held_euler", 0.0), ("Cont-SC-DFIM-v0", "dfim_cont_sc_free_held_euler", 2e-6),
    ("Finite-CC-DFIM-v0", "dfim_fin_free_held_euler", 0.0), ("Finite-SC-DFIM-v0", "dfim_fin_sc_free_uniform_euler", 1e-6),
])
def test_multi_converter_envs_per_env_actions_against_oracle(env_id, golden, til):
    """ExtExDc (2 x 4QC), EESM (B6 + 4QC) and DFIM (2 x B6): every env gets its own random action stream (flat MultiDiscrete index for
    the finite converters); a sample of envs is checked against the fp64 oracle with the SAME integrator (RK4), and the
    single-step path, the single-wave and the pipelined fused kernels must agree bit for bit."""
    import torch

    import gym_electric_motor_amd as ga
    from oracle import oracle as orc

    K, n_envs = 160, 1024
    _, meta = _load(golden)
    fin = env_id.startswith("Finite")

    def conv():
        if not til:
            return None
        if "DFIM" in env_id:
            sub = ga.FiniteB6BridgeConverter if fin else ga.ContB6BridgeConverter
        else:
            sub = ga.FiniteFourQuadrantConverter if fin else ga.ContFourQuadrantConverter
        holder = ga.FiniteMultiConverter if fin else ga.ContMultiConverter
        return holder(subconverters=[sub(interlocking_time=til), sub(interlocking_time=til)])

    def mk():
        return ga.make(env_id, n_envs=n_envs, ode_solver=ga.RK4Solver(), constraints=(), converter=conv())

    env = mk()
    ps = env.physical_system
    g = torch.Generator(device="cuda").manual_seed(4321)
    if ps._discrete:
        nflat = int(np.prod(ps.action_space.nvec))
        acts = torch.randint(0, nflat, (K, n_envs), device="cuda", generator=g, dtype=torch.uint8)
    else:
        acts = torch.rand((K, n_envs, ps._n_act), device="cuda", generator=g) * 2 - 1
    obs, _ = env.rollout(acts)
    torch.cuda.synchronize()
    # (the ExtExDc envs here sit behind a ConstantSpeedLoad without dead time: a small batch of them takes dc_stream_kernel)
    assert ("dc_stream_kernel" if ("ExtExDc" in env_id and not til) else "advance_pipe_kernel") in ps.last_launch()
    assert torch.isfinite(obs).all()
    env2 = mk()
    for k in range(4):
        assert torch.equal(env2.physical_system.simulate(acts[k]), obs[k])
    env2.close()
    os.environ["GEMX_PIPE"] = "0"
    try:
        env3 = mk()
        obs3, _ = env3.rollout(acts)
        assert "advance_kernel" in env3.physical_system.last_launch()
        assert torch.equal(obs3, obs)
        env3.close()
    finally:
        del os.environ["GEMX_PIPE"]
    meta = dict(meta, interlocking_time=til)
    p = orc.params_from_meta(meta, solver="rk4", episodic=False)
    a_host = acts.cpu().numpy().astype(np.float64)
    if ps._discrete:  # flat index -> [a0, a1] as the reference's MultiDiscrete action
        n0 = int(ps.action_space.nvec[0])
        a_host = np.stack([a_host % n0, a_host // n0], axis=-1)
    o_host = obs.double().cpu().numpy()
    worst = 0.0
    for j in (0, 63, 64, 517, n_envs - 1):
        e = orc.OracleEnv(p)
        e.reset()
        ref, _ = e.rollout(a_host[:, j])
        rel, _ = _rel_err(o_host[:, j], ref, meta["state_names"])
        worst = max(worst, rel)
    env.close()
    assert worst < 1e-4, worst


@pytest.mark.parametrize("name", ["pmsm_free_uniform_euler", "pmsm_epi_held_tau1e-4_euler", "pmsm_free_held_til_euler",
                                  "scim_epi_uniform_euler", "scim_free_held_til_euler", "permexdc_epi_held_euler",
                                  "permexdc_free_held_til_euler", "pmsm_free_uniform_10k_euler",
                                  "extex_fin_free_held_til_euler", "extex_cont_epi_held_euler", "eesm_fin_epi_held_tau1e-4_euler",
                                  "eesm_cont_free_uniform_euler", "dfim_fin_free_uniform_til_euler", "dfim_fin_epi_held_tau1e-4_euler",
                                  "dfim_cont_sc_epi_held_euler",
                                  "param_pmsm_fin_cc_lim_u350_epi_uniform_tau5e-5_euler", "param_pmsm_reversed_cont_cc_free_held_euler",
                                  "param_scim_fin_cc_lim_epi_uniform_euler", "param_permexdc_fin_cc_lim_epi_uniform_euler", "param_shunt_cont_cc_epi_held_euler",
                                  "param_extex_fin_cc_til_free_held_euler", "param_eesm_fin_cc_epi_held_euler", "param_dfim_fin_cc_free_held_euler"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_two_wave_pipelined_kernel_matches_reference_and_single_wave_kernel(name, dtype, monkeypatch):
    """n_envs = 128 (full 64-env workgroups) takes the two-wave pipelined kernel; it must agree with the reference AND be
    bit-identical to the single-wave kernel (GEMX_PIPE=0) on the same inputs."""
    monkeypatch.setenv("GEMX_PIPE", "1")
    d, meta, obs_p, done_p = _run_golden(name, dtype, n_envs=128)
    monkeypatch.setenv("GEMX_PIPE", "0")
    _, _, obs_s, done_s = _run_golden(name, dtype, n_envs=128)
    assert np.array_equal(obs_p, obs_s) and np.array_equal(done_p, done_s)
    rel, ab = _rel_err(obs_p[d["state_index"]], d["states"], meta["state_names"])
    assert (rel < 1e-4) if dtype == "float32" else (ab < 1e-9)
    if meta["episodic"]:
        _check_done(meta, d, done_p)


def _variant_against_oracle(name, meta, solver, n=8):
    """One device rollout (fp32, n lanes, each on its own seeded random action stream) of a fixture's env rebuilt from `meta` -- a
    fixture's meta or a variant of it with other recorded overrides --, every lane checked against the fp64 oracle run of the SAME
    variant (_lanes_against_oracle: 1e-4).  Returns the observations in PHYSICAL units [K, n, S_out]."""
    import torch

    import gym_electric_motor_amd as ga

    d = _load(name)[0]
    K = d["actions"].shape[0]
    env = _make_from_meta(meta, n, solver=solver, auto_reset=True)
    ps = env.physical_system
    rng = np.random.default_rng(5)
    if ps._discrete:  # (MultiDiscrete actions stay [K, N, 2]: rollout() packs them into the flat index)
        nvec = [int(v) for v in ps.action_space.nvec] if hasattr(ps.action_space, "nvec") else [int(ps.action_space.n)]
        a_np = np.stack([rng.integers(0, nv, (K, n)) for nv in nvec], axis=2).astype(np.uint8)
        a = torch.as_tensor(a_np.reshape(K, n) if len(nvec) == 1 else a_np)
    else:
        a_np = rng.uniform(-1.0, 1.0, (K, n, ps._n_act))
        a = torch.as_tensor(a_np)
    obs, done = env.rollout(a.cuda())
    obs, done = obs.double().cpu().numpy(), done.cpu().numpy().astype(bool)
    lim = [float(x) for x in ps.limits]
    sol_obj = ps._ode_solver
    env.close()
    worst = _lanes_against_oracle(name, dict(meta, limits=lim), a_np, obs, done, list(range(n)), sol_obj, "float32", 1 if a_np.shape[2] == 1 and ps._discrete else 2)
    assert worst is not None
    return obs * np.asarray(lim), worst


@pytest.mark.parametrize("name", ["param_scim_cont_cc_free_held_euler", "param_dfim_cont_cc_free_held_euler", "param_scim_cont_sc_free_held_dopri5",
                                  "param_dfim_fin_cc_free_held_euler"])
def test_stator_rotor_leakage_swap_is_seen_at_the_recorded_points(name):
    """The reference's default induction machines have l_sigs == l_sigr, so a stator / rotor mix-up anywhere (host constants, torque
    coefficient, rotor-current reconstruction, the kernels' packed index tables) gives identical numbers at every default fixture.  At
    the recorded non-default sets the swap must MOVE the device trajectory by more than 100x the 1e-4 contract -- and the recorded set
    and the swapped one must each still match the fp64 oracle run of their own parameters."""
    _, meta = _load(name)
    mp = meta["overrides"]["motor"]["motor_parameter"]
    assert mp["l_sigs"] != mp["l_sigr"]
    sw = json.loads(json.dumps(meta))
    sw["overrides"]["motor"]["motor_parameter"].update(l_sigs=mp["l_sigr"], l_sigr=mp["l_sigs"])
    sw["motor_parameter"].update(l_sigs=mp["l_sigr"], l_sigr=mp["l_sigs"])
    solver = "euler" if name.endswith("euler") else "rk4k"
    a, wa = _variant_against_oracle(name, meta, solver)
    b, wb = _variant_against_oracle(name, sw, solver)
    scale = np.maximum(np.abs(a).max(axis=(0, 1)), 1e-30)
    moved = (np.abs(a - b).max(axis=(0, 1)) / scale)
    cols = [i for i, c in enumerate(meta["state_names"]) if c not in ("epsilon", "u_sup") and not c.startswith("u_")]
    assert moved[cols].max() > 100 * 1e-4, (dict(zip(meta["state_names"], moved.round(6))), wa, wb)


@pytest.mark.parametrize("name", ["param_scim_cont_sc_free_held_dopri5", "param_pmsm_cont_sc_free_held_dopri5", "param_permexdc_cont_sc_u80_free_held_dopri5",
                                  "param_synrm_cont_sc_free_held_dopri5", "param_dfim_cont_sc_free_held_dopri5", "param_series_cont_sc_free_held_dopri5"])
@pytest.mark.parametrize("solver", ["rk4k", "dp5k", "euler", "adaptive"])
def test_quadratic_load_term_is_seen_at_the_recorded_points(name, solver):
    """Every default speed-control env has c = 0 in its PolynomialStaticLoad, so the quadratic term c omega |omega| -- written out in
    the scalar load ODE, the packed RHS, the kink-side branch, the fp64 stage solver and the adaptive solver -- was never compared on
    the device.  At the recorded c != 0 points: switching the term off must move omega by more than 100x the 1e-4 contract, and both
    variants must match the fp64 oracle run of their own load (fixed steps with kink splitting, Euler, and the error-controlled
    solver, which the oracle restates as scipy's dopri5 at the same tolerance)."""
    import gym_electric_motor_amd as ga

    _, meta = _load(name)
    assert meta["load_parameter"]["c"] != 0
    off = json.loads(json.dumps(meta))
    off["overrides"]["load"]["load_parameter"]["c"] = 0.0
    off["load_parameter"]["c"] = 0.0
    sol = ga.ScipyOdeSolver() if solver == "adaptive" else solver
    a, _ = _variant_against_oracle(name, meta, sol)
    b, _ = _variant_against_oracle(name, off, sol if isinstance(sol, str) else ga.ScipyOdeSolver())
    w = meta["state_names"].index("omega")
    moved = np.abs(a[..., w] - b[..., w]).max() / np.abs(a[..., w]).max()
    assert moved > 100 * 1e-4, moved


@pytest.mark.parametrize("env_id, wrappers, control_space", [
    ("Cont-CC-PMSM-v0", ("dead2", "dq"), "abc"), ("Finite-CC-PMSM-v0", ("dead3",), "abc"), ("Cont-SC-SCIM-v0", ("dead1",), "dq"),
    ("Cont-CC-EESM-v0", ("dead1", "dq"), "abc"), ("Finite-CC-DFIM-v0", ("dead2",), "abc"), ("Cont-CC-PermExDc-v0", ("dead1",), "abc"),
    ("Cont-CC-SynRM-v0", ("dq",), "abc"), ("Finite-CC-PMSM-v0", ("rc",), "abc"), ("Cont-CC-DFIM-v0", ("rc", "dead1"), "abc"),
    ("Finite-SC-ExtExDc-v0", ("rc",), "abc"),
])
def test_action_stage_chunking_and_single_step_are_bit_identical(env_id, wrappers, control_space):
    """DeadTimeProcessor FIFO / dq action stage across launches: one K-step rollout == the same steps in uneven chunks ==
    step-by-step simulate() (the FIFO lives in HBM between launches), bit for bit, with per-env random actions, episodic
    (auto-reset refills the FIFO), odd env count (tail workgroup); and the oracle agrees on a sample of envs."""
    import torch

    import gym_electric_motor_amd as ga
    from oracle import oracle as orc

    K, n = 96, 200

    def mk():
        ws, kw = [], {}
        for w in wrappers:
            if w.startswith("dead"):
                ws.append(ga.DeadTimeProcessor(steps=int(w[4:])))
            elif w == "rc":  # RCVoltageSupply: the supply state lives in HBM between launches, like the FIFO
                kw["supply"] = ga.RCVoltageSupply(u_nominal=60.0 if "Dc" in env_id else 420.0, supply_parameter=dict(R=0.5, C=2e-3))
            else:
                ws.append(ga.DqToAbcActionProcessor.make("EESM" if "EESM" in env_id else "PMSM"))
        return ga.make(env_id, n_envs=n, ode_solver=ga.RK4Solver(), physical_system_wrappers=tuple(ws), control_space=control_space, **kw)

    env = mk()
    ps = env.physical_system
    g = torch.Generator(device="cuda").manual_seed(99)
    if ps._discrete:
        nflat = int(np.prod(ps.action_space.nvec)) if hasattr(ps.action_space, "nvec") else int(ps.action_space.n)
        acts = torch.randint(0, nflat, (K, n), device="cuda", generator=g, dtype=torch.uint8)
    else:
        acts = torch.rand((K, n, ps._n_act), device="cuda", generator=g) * 2 - 1
    obs, done = env.rollout(acts)
    e2 = mk()
    parts, k0 = [], 0
    for kk in (1, 7, 2, 30, 56):
        parts.append(e2.rollout(acts[k0:k0 + kk]))
        k0 += kk
    assert torch.equal(torch.cat([p[0] for p in parts]), obs) and torch.equal(torch.cat([p[1] for p in parts]), done)
    e3 = mk()
    for k in range(12):
        assert torch.equal(e3.physical_system.simulate(acts[k]), obs[k])
        assert torch.equal(e3.physical_system.done, done[k])
    # oracle (same integrator, same wrappers) on a few envs
    golden = {"PMSM": "pmsm_cont_dqproc_free_held_euler", "SCIM": "scim_cont_dqspace_free_held_euler", "EESM": "eesm_cont_dqproc_free_held_euler",
              "DFIM": "dfim_fin_free_held_euler", "PermExDc": "permexdc_free_held_euler", "SynRM": "synrm_cont_dqspace_free_held_euler",
              "ExtExDc": "extex_fin_free_held_euler"}
    key = env_id.split("-")[2]
    gname = golden[key] if not env_id.startswith("Finite-CC-PMSM") else "pmsm_free_held_euler"
    gname = {"Cont-CC-DFIM-v0": "dfim_cont_free_held_euler", "Finite-SC-ExtExDc-v0": "rc_extex_fin_free_held_euler"}.get(env_id, gname)
    _, meta = _load(gname)
    if "rc" in wrappers:
        lp = env.physical_system.mechanical_load
        meta = dict(meta, supply="RCVoltageSupply", supply_parameter=dict(R=0.5, C=2e-3), u_nominal=env.physical_system.supply.u_nominal,
                    limits=[float(x) for x in env.physical_system.limits], j_total=float(lp.j_total))
        if env_id == "Finite-SC-ExtExDc-v0":
            meta.update(load="PolynomialStaticLoad", load_parameter=dict(lp.load_parameter), tau_decay=lp.tau_decay)
            meta.pop("omega_fixed", None)
    meta = dict(meta, episodic=True, dead_time_steps=sum(int(w[4:]) for w in wrappers if w.startswith("dead")),
                action_frame="dq_processor" if "dq" in wrappers else ("dq" if control_space == "dq" else "abc"))
    p = orc.params_from_meta(meta, solver="rk4", episodic=True)
    a_host = acts.cpu().numpy().astype(np.float64)
    if ps._discrete and hasattr(ps.action_space, "nvec"):
        n0 = int(ps.action_space.nvec[0])
        a_host = np.stack([a_host % n0, a_host // n0], axis=-1)
    o_host, d_host = obs.double().cpu().numpy(), done.cpu().numpy().astype(bool)
    for j in (0, 64, n - 1):
        e = orc.OracleEnv(p)
        e.reset()
        ref, rdone = e.rollout(a_host[:, j], auto_reset=True)
        first = int(np.argmax(rdone != d_host[:, j])) if (rdone != d_host[:, j]).any() else K
        rel, _ = _rel_err(o_host[:first + 1, j], ref[:first + 1], meta["state_names"], scale_ref=ref)
        assert rel < 1e-4, (j, rel)
        assert first >= K or first > 0  # a done flip (fp32 vs fp64 at the limit) may end the comparison, never at step 0
    for e_ in (env, e2, e3):
        e_.close()


REWARD_CASES = [c for c in CASES if c.startswith("rw_")]


def _install_reward(ps, meta):
    rw = meta["reward"]
    names = meta["state_names"]
    return ps.set_reward(reward_weights=np.array(rw["weights"]), reward_power=np.array(rw["powers"]), bias=rw["bias"],
                         violation_reward=rw["violation_reward"],
                         referenced_states=[n for n, r in zip(names, rw["referenced_states"]) if r])


@pytest.mark.parametrize("name", REWARD_CASES)
@pytest.mark.parametrize("n_envs", [70, 128, -70])
def test_fused_reward_matches_reference_env_rewards(name, n_envs, monkeypatch):
    """WeightedSumOfErrors fused into the rollout (gemx_rollout_reward): rewards env.step() returned in the reference run, with
    the references its generator produced fed in as data.  fp32: |dr| <= 1e-4 * reward scale; the violation reward exact.
    n_envs = 128: the pipelined kernel's aligned paths (reward computed by the output waves); 70: its unaligned, partial-workgroup paths
    (round 5; the single-wave kernel's reward code is compared through GEMX_PIPE=0 elsewhere)."""
    import torch

    single_wave = n_envs < 0  # (-70: the same batch through the single-wave kernel, GEMX_PIPE=0)
    n_envs = abs(n_envs)
    if single_wave:
        monkeypatch.setenv("GEMX_PIPE", "0")
    d, meta = _load(name)
    env = _make_from_meta(meta, n_envs, dtype="float32", auto_reset=True)
    ps = env.physical_system
    _install_reward(ps, meta)
    K = d["actions"].shape[0]
    a = torch.as_tensor(np.repeat(d["actions"].reshape(K, 1, -1), n_envs, axis=1))
    if ps._discrete and d["actions"].ndim == 1:
        a = a.reshape(K, n_envs)
    cols = [i for i, r in enumerate(meta["reward"]["referenced_states"]) if r]
    refs = torch.as_tensor(np.repeat(d["references"][:, None, cols], n_envs, axis=1))
    obs, done, rew = ps.rollout(a.cuda(), references=refs.cuda())
    torch.cuda.synchronize()
    assert ("advance_kernel" if single_wave else "advance_pipe_kernel") in ps.last_launch()
    rew, done = rew.double().cpu().numpy(), done.cpu().numpy().astype(bool)
    assert np.array_equal(rew[:, 0], rew[:, n_envs - 1])
    ref_done = d["terminated"]
    first = int(np.argmax(done[:, 0] != ref_done)) if (done[:, 0] != ref_done).any() else K
    assert first > 100  # (a done flip at a < 1e-5 constraint margin ends the like-for-like comparison)
    scale = max(1.0, float(np.abs(d["rewards"][~ref_done]).max()))
    assert np.abs(rew[:first, 0] - d["rewards"][:first]).max() < 1e-4 * scale
    viol = np.float32(meta["reward"]["violation_reward"])
    assert (rew[:first, 0][ref_done[:first]] == viol).all() and ref_done[:first].sum() > 0
    # chunked launches and the no-reward rollout give the same bits
    env2 = _make_from_meta(meta, n_envs, dtype="float32", auto_reset=True)
    _install_reward(env2.physical_system, meta)
    o1, d1, r1 = env2.physical_system.rollout(a[:333].cuda(), references=refs[:333].cuda())
    o2, d2, r2 = env2.physical_system.rollout(a[333:].cuda(), references=refs[333:].cuda())
    assert np.array_equal(torch.cat([r1, r2]).double().cpu().numpy(), rew) and torch.equal(torch.cat([o1, o2]), obs)
    env3 = _make_from_meta(meta, n_envs, dtype="float32", auto_reset=True)
    o3, d3 = env3.physical_system.rollout(a.cuda())
    assert torch.equal(o3, obs)
    # closed-loop form: env.step(actions, references) -> (obs, reward, terminated, ...) with the same bits
    env4 = _make_from_meta(meta, n_envs, dtype="float32", auto_reset=True)
    _install_reward(env4.physical_system, meta)
    ac, rc_ = a.cuda(), refs.cuda().float()
    for k in range(6):
        o4, r4, t4, _, _ = env4.step(ac[k], references=rc_[k])
        assert torch.equal(o4, obs[k]) and np.array_equal(r4.double().cpu().numpy(), rew[k])
    env4.close()
    for e in (env, env2, env3):
        e.close()


def test_fused_reward_fp64_and_soa_layout():
    import torch

    name = "rw_eesm_cont_cc_pow_mixed_epi_held_euler"  # powers 1, 2 and 0.5
    d, meta = _load(name)
    K = d["actions"].shape[0]
    cols = [i for i, r in enumerate(meta["reward"]["referenced_states"]) if r]
    out = {}
    for layout in ("aos", "soa"):
        env = _make_from_meta(meta, 65, dtype="float64", auto_reset=True, obs_layout=layout)
        _install_reward(env.physical_system, meta)
        a = torch.as_tensor(np.repeat(d["actions"].reshape(K, 1, -1), 65, axis=1)).cuda()
        refs = torch.as_tensor(np.repeat(d["references"][:, None, cols], 65, axis=1)).cuda()
        obs, done, rew = env.physical_system.rollout(a, references=refs)
        out[layout] = rew.cpu().numpy()
        assert np.array_equal(done[:, 0].cpu().numpy().astype(bool), d["terminated"])
        assert np.abs(out[layout][:, 0] - d["rewards"]).max() < 1e-9
        env.close()
    assert np.array_equal(out["aos"], out["soa"])


INIT_SAMPLES = os.path.join(GOLDEN, "init_samples.npz")
INIT_SAMPLES_PARAMS = os.path.join(GOLDEN, "init_samples_params.npz")  # (non-default motor parameters, recorded with their make-kwargs)


def _init_env(case, n_envs, seed=7, **kw):
    """case: a case of init_samples.npz, or 'params:<case>' of init_samples_params.npz."""
    import gym_electric_motor_amd as ga

    path = INIT_SAMPLES
    if case.startswith("params:"):
        path, case = INIT_SAMPLES_PARAMS, case[7:]
    d = np.load(path)
    meta = json.loads(str(d[case + "_meta"]))
    motor_cls = {"PermanentMagnetSynchronousMotor": ga.PermanentMagnetSynchronousMotor, "DcExternallyExcitedMotor": ga.DcExternallyExcitedMotor,
                 "ExternallyExcitedSynchronousMotor": ga.ExternallyExcitedSynchronousMotor, "DcPermanentlyExcitedMotor": ga.DcPermanentlyExcitedMotor,
                 "SquirrelCageInductionMotor": ga.SquirrelCageInductionMotor, "DoublyFedInductionMotor": ga.DoublyFedInductionMotor}[meta["motor"]]
    mkw = json.loads(json.dumps(meta.get("overrides", {}).get("motor", {})))
    mk = dict(motor=motor_cls(motor_initializer=meta["motor_initializer"], **mkw), seed=seed, n_envs=n_envs, **kw)
    if meta["load_initializer"] is not None:
        mk["load"] = ga.PolynomialStaticLoad(load_parameter=meta["load_parameter"], load_initializer=meta["load_initializer"])
    elif meta["load"] == "ConstantSpeedLoad":
        mk["load"] = ga.ConstantSpeedLoad(omega_fixed=float(d[case + "_y"][0, 0]))
    return ga.make(meta["env_id"], **mk), meta, d[case + "_y"], d[case + "_obs"]


@pytest.mark.parametrize("case", ["pmsm_sc_uniform", "extex_cc_uniform_interval", "eesm_sc_uniform"])
def test_random_uniform_initialisers_match_reference_distribution(case):
    """Random initialisers: 4000 envs reset once on the GPU vs 4000 resets of the live reference -- same support
    (bounds from nominal values / state space / interval) and same distribution (two-sample KS per ODE state); the state ->
    reset-observation map is exact (oracle reset from the drawn state)."""
    import torch
    from scipy import stats

    from oracle import oracle as orc

    n = 4000
    env, meta, ref_y, ref_obs = _init_env(case, n)
    ps = env.physical_system
    obs = ps.reset().double().cpu().numpy()
    y = ps.get_state().double().cpu().numpy().T  # [N, S_ode]
    assert y.shape == ref_y.shape
    for j in range(y.shape[1]):
        lo, hi = ref_y[:, j].min(), ref_y[:, j].max()
        if hi - lo < 1e-12:
            assert np.allclose(y[:, j], lo, rtol=1e-6, atol=1e-9)
            continue
        span = hi - lo
        assert y[:, j].min() >= lo - 0.01 * span and y[:, j].max() <= hi + 0.01 * span
        assert y[:, j].max() - y[:, j].min() > 0.98 * span
        assert stats.ks_2samp(y[:, j], ref_y[:, j]).pvalue > 1e-3, j
        if j + 1 < y.shape[1]:  # independent draws per state
            assert abs(np.corrcoef(y[:, j], y[:, (j + 1) % y.shape[1]])[0, 1]) < 0.06 or ref_y[:, (j + 1) % y.shape[1]].std() < 1e-12
    # state -> reset observation: exact (fp32) against the oracle's reset from the same state
    gname = {"pmsm_sc_uniform": "pmsm_cont_dqspace_free_held_euler", "extex_cc_uniform_interval": "extex_cont_free_held_euler",
             "eesm_sc_uniform": "eesm_cont_sc_epi_held_euler"}[case]
    _, gmeta = _load(gname)
    gmeta = dict(gmeta, action_frame="abc", limits=[float(x) for x in ps.limits], u_nominal=float(ps.supply.u_nominal))
    p = orc.params_from_meta(gmeta, episodic=False)
    for i in (0, 1, 999, n - 1):
        for j in range(y.shape[1]):
            p.init[j] = y[i, j]
        e = orc.OracleEnv(p)
        assert np.abs(e.reset() - obs[i]).max() < 5e-6
    # and the reference's own (state, observation) pairs obey the same map
    for i in (0, 17):
        for j in range(y.shape[1]):
            p.init[j] = ref_y[i, j]
        assert np.abs(orc.OracleEnv(p).reset() - ref_obs[i]).max() < 1e-12
    env.close()


@pytest.mark.parametrize("case", ["scim_sc_uniform", "scim_cc_uniform", "scim_cc_negspeed_uniform", "dfim_cc_negspeed_interval_uniform",
                                  # init_samples_params.npz: p = 3, l_sigs != l_sigr, other l_m / r_s / r_r (oracle/make_golden.py:main_params)
                                  "params:scim_sc_uniform", "params:scim_cc_negspeed_uniform", "params:dfim_cc_negspeed_uniform"])
def test_induction_machine_random_initialisers_match_reference_distribution(case):
    """SURVEY 8f rank 4, induction machines (round 4): the MOTOR initialiser of a SCIM / DFIM re-derives its flux bounds at every reset
    from a random field angle (induction_motor.py:174-185, 250-285; squirrel_cage_induction_motor.py:146-157) -- psi_d_max = l_m
    i_sd,nominal while omega is 0, and from the PREVIOUS reset's stator currents otherwise (at the CC envs' +100 rad/s the reference's
    clip leaves psi_d_max = 0: every flux draw is exactly 0; the live branch is recorded at a negative speed).  4096 envs on the GPU,
    reset twice (the second reset reads the first one's currents), against 4000 resets of the live reference: per-state support and
    two-sample KS, the flux MAGNITUDE's distribution (joint structure: both components share one field angle), and the state ->
    reset-observation map against the oracle."""
    from scipy import stats

    from oracle import oracle as orc

    n = 4096
    env, meta, ref_y, ref_obs = _init_env(case, n)
    ps = env.physical_system
    ps.reset()
    obs = ps.reset().double().cpu().numpy()
    y = ps.get_state().double().cpu().numpy().T  # [N, S_ode]
    assert y.shape[1] == ref_y.shape[1] == 6
    for j in range(6):
        lo, hi = ref_y[:, j].min(), ref_y[:, j].max()
        if hi - lo < 1e-12:
            assert np.allclose(y[:, j], lo, rtol=1e-6, atol=1e-9), j
            continue
        span = hi - lo
        # (the flux columns' marginals thin out towards their extremes -- psi_d_max needs both previous currents AND the field angle
        # aligned --, so the sample range of 4000 draws is not the support: KS decides there, the bound is the theoretical one)
        slack = 0.03 * span if j not in (3, 4) else max(0.0, 0.9 * meta["motor_parameter"]["l_m"] * np.sqrt(2.0) * np.abs(ref_y[:, 1:3]).max() * 1.01 - hi)
        assert y[:, j].min() >= lo - slack and y[:, j].max() <= hi + slack, j
        assert y[:, j].max() - y[:, j].min() > 0.85 * span, j
        assert stats.ks_2samp(y[:, j], ref_y[:, j]).pvalue > 1e-3, j
    mag, ref_mag = np.hypot(y[:, 3], y[:, 4]), np.hypot(ref_y[:, 3], ref_y[:, 4])
    if ref_mag.max() > 0:
        assert stats.ks_2samp(mag, ref_mag).pvalue > 1e-3
        if case.endswith("scim_sc_uniform"):  # omega == 0: |psi| <= l_m i_sd,nominal (defaults: 0.14375 H x 3.9 A)
            psi_max = meta["motor_parameter"]["l_m"] * meta["nominal_state"][meta["state_names"].index("i_sd")]
            assert mag.max() <= psi_max * (1 + 1e-6) and mag.max() > 0.9 * psi_max
    else:
        assert mag.max() == 0.0
    # the first reset of an env reads the CONFIGURED currents (zeros): at omega != 0 that gives psi_d_max = 0.9 clip(., 0, |l_m 0|) = 0
    if "cc" in case:
        e1, _, _, _ = _init_env(case, 256)
        y1 = e1.physical_system.get_state().double().cpu().numpy().T
        assert np.abs(y1[:, 3:5]).max() == 0.0 and np.ptp(y1[:, 1]) > 1.0
        e1.close()
    gname = "scim_free_held_euler" if "scim" in case else "dfim_cont_free_held_euler"
    if case.startswith("params:"):  # (the state -> observation map reads the motor parameters: a fixture of the same set)
        gname = "param_scim_cont_cc_free_held_euler" if "scim" in case else "param_dfim_cont_cc_free_held_euler"
    _, gmeta = _load(gname)
    gmeta = dict(gmeta, action_frame="abc", limits=[float(x) for x in ps.limits], u_nominal=float(ps.supply.u_nominal), load=meta["load"])
    p = orc.params_from_meta(gmeta, episodic=False)
    for i in (0, 1, 999, n - 1):
        for j in range(6):
            p.init[j] = y[i, j]
        assert np.abs(orc.OracleEnv(p).reset() - obs[i]).max() < 5e-6
    for i in (1, 17):
        for j in range(6):
            p.init[j] = ref_y[i, j]
        assert np.abs(orc.OracleEnv(p).reset() - ref_obs[i]).max() < 1e-12
    env.close()


def test_induction_machine_random_initialiser_is_the_same_draw_in_every_kernel():
    """The per-reset flux bounds live in the draw itself (init_draw_all), so the in-kernel auto-reset of every kernel -- the single-wave
    kernel, the pipelined FULL instantiation, the K = 1 step kernel -- and gemx_reset give the same states bit for bit: one launch ==
    uneven chunks == step by step, with terminations (fresh draws) inside the launch; gaussian draws stay inside their bounds."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 200, 120

    def mk(dist="uniform"):
        mi = dict(random_init=dist) if dist == "uniform" else dict(random_init=dist, random_params=(None, 0.2))
        return ga.make("Cont-SC-SCIM-v0", n_envs=n, seed=11, motor=ga.SquirrelCageInductionMotor(motor_initializer=mi))

    e1, e2, e3 = mk(), mk(), mk()
    for e in (e1, e2, e3):
        e.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    acts = torch.rand((K, n, 3), device="cuda", generator=g) * 2 - 1
    obs, done = e1.rollout(acts)
    assert done.any() and not done.all()
    parts = [e2.rollout(acts[:7]), e2.rollout(acts[7:50]), e2.rollout(acts[50:])]
    assert torch.equal(torch.cat([p_[0] for p_ in parts]), obs) and torch.equal(torch.cat([p_[1] for p_ in parts]), done)
    for k in range(30):
        assert torch.equal(e3.physical_system.simulate(acts[k]), obs[k]), k
    assert torch.equal(e1.physical_system.get_state(), e2.physical_system.get_state())
    eg = mk("gaussian")
    eg.reset()
    yg = eg.physical_system.get_state().double().cpu().numpy()
    assert np.abs(yg[1:3]).max() <= 3.9 and np.hypot(yg[3], yg[4]).max() <= 0.14375 * 3.9 * (1 + 1e-6) and np.ptp(yg[3]) > 0.05
    for e in (e1, e2, e3, eg):
        e.close()


@pytest.mark.parametrize("env_id, golden", [("Cont-SC-SCIM-v0", "scim_free_held_euler"), ("Cont-SC-DFIM-v0", "dfim_cont_sc_free_held_euler")])
def test_induction_motor_random_load_initialiser_reset_rows(env_id, golden):
    """Induction-motor systems accept a random LOAD initialiser (omega); their reset observation is then written per env by
    reset_kernel (gemx_capi.hip:reset_obs_row) in the SCIM / DFIM layout -- u_abc = -0.5 u_sup per leg, dq columns in the rotor-flux
    frame -- and equals the oracle's reset from the drawn state, both from reset() and from a masked reset."""
    import torch

    import gym_electric_motor_amd as ga
    from oracle import oracle as orc

    n = 300
    _, meta = _load(golden)
    load = ga.PolynomialStaticLoad(load_parameter=meta["load_parameter"], load_initializer=dict(random_init="uniform", interval=[[-150.0, 220.0]]))
    env = ga.make(env_id, n_envs=n, load=load, seed=3)
    ps = env.physical_system
    obs = ps.reset().double().cpu().numpy()
    y = ps.get_state().double().cpu().numpy().T
    assert y[:, 0].min() >= -150.0 and y[:, 0].max() <= 220.0 and np.ptp(y[:, 0]) > 200.0 and np.abs(y[:, 1:]).max() == 0.0
    p = orc.params_from_meta(meta)
    for i in (0, 1, 63, 64, n - 1):
        p.init[0] = y[i, 0]
        assert np.abs(orc.OracleEnv(p).reset() - obs[i]).max() < 1e-6, i
    us = ps.state_positions["u_sup"]
    assert np.all(obs[:, us] == 1.0) and np.isfinite(obs).all()
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mask[5] = 1
    o2 = ps.reset(mask).double().cpu().numpy()
    y2 = ps.get_state().double().cpu().numpy().T
    assert y2[5, 0] != y[5, 0] and np.array_equal(np.delete(y2, 5, axis=0), np.delete(y, 5, axis=0))
    p.init[0] = y2[5, 0]
    assert np.abs(orc.OracleEnv(p).reset() - o2[5]).max() < 1e-6 and np.array_equal(np.delete(o2, 5, axis=0), np.delete(obs, 5, axis=0))
    env.close()


def test_dq_processor_angle_advance_beyond_half_a_turn():
    """DqToAbcActionProcessor's angle advance (0.5 + dead time) * tau * p * omega (dq_to_abc_action_processor.py:83-100) exceeds pi at
    8 dead-time steps, tau = 4e-4 and 400 rad/s (4.08 rad): the fp32 fixed-point angle must WRAP there (its float -> int conversion
    saturates at half a turn), as the fp64 path and the reference do.  GPU fp32 and fp64 against the oracle, same (RK4) integrator
    (explicit Euler is unstable at 0.48 rad of electrical rotation per step)."""
    import torch

    import gym_electric_motor_amd as ga
    from oracle import oracle as orc

    _, meta = _load("pmsm_cont_dqproc_dead2_free_held_euler")
    meta = dict(meta, tau=4e-4, dead_time_steps=8, omega_fixed=400.0)
    p = orc.params_from_meta(meta, solver="rk4", episodic=False)
    K, n = 300, 64
    rng = np.random.default_rng(3)
    acts = rng.uniform(-0.3, 0.3, (K, 2))
    e = orc.OracleEnv(p)
    e.reset()
    ref, _ = e.rollout(acts, auto_reset=False)
    for dtype, tol in (("float32", 1e-4), ("float64", 1e-9)):
        env = ga.make("Cont-CC-PMSM-v0", n_envs=n, dtype=dtype, tau=4e-4, ode_solver=ga.RK4Solver(), constraints=(),
                      load=ga.ConstantSpeedLoad(omega_fixed=400.0),
                      physical_system_wrappers=(ga.DeadTimeProcessor(steps=8), ga.DqToAbcActionProcessor.make("PMSM")))
        a = torch.as_tensor(np.repeat(acts[:, None, :], n, axis=1)).cuda()
        obs, _ = env.rollout(a)
        torch.cuda.synchronize()
        rel, ab = _rel_err(obs[:, 0].double().cpu().numpy(), ref, meta["state_names"])
        env.close()
        assert (rel if dtype == "float32" else ab) < tol, (dtype, rel, ab)


def test_single_env_random_initialiser_reset_returns_the_drawn_state():
    """n_envs == 1 (the instance handed to the reference's ElectricMotorEnvironment): with a random initialiser reset() returns the
    observation of the state the kernel just drew, not the constant initial state's."""
    env, meta, _, _ = _init_env("pmsm_sc_uniform", 1)
    ps = env.physical_system
    seen = []
    for _ in range(3):
        o = ps.reset()
        y = ps.get_state().double().cpu().numpy()[:, 0]
        assert isinstance(o, np.ndarray) and o.shape == (len(ps.state_names),)
        lim = ps.limits
        assert abs(o[ps.state_positions["omega"]] * lim[0] - y[0]) < 1e-3 * max(1.0, abs(y[0]))
        assert abs(o[ps.state_positions["i_sd"]] * lim[ps.state_positions["i_sd"]] - y[1]) < 1e-3 * max(1.0, abs(y[1]))
        seen.append(o.copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    env.close()


@pytest.mark.parametrize("case", ["pmsm_fin_til", "permexdc_rc", "pmsm_fin_rc", "dfim_fin_rc", "dfim_fin_til", "scim_dq", "pmsm_dead3", "pmsm_dqproc_dead2",
                                  "pmsm_random_init", "extex_fin_soa", "eesm_f64"])
def test_step_kernel_is_bit_identical_to_the_rollout_kernels(case, monkeypatch):
    """gemx_step launches step_kernel (one batch of loads, no LDS, rows stored from registers); GEMX_STEP_KERNEL=0 sends the same call
    through advance_kernel.  Same observations, done masks and final ODE / switching state, bit for bit, on a batch with a tail
    workgroup, for every feature the single step supports: converter dead time, RC supply, two-byte leg state, dq action frames,
    DeadTimeProcessor queue (+ its refill on auto-reset), random initialisers, SoA observations, fp64."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 200, 48
    kw, env_id, dtype = {}, "Finite-CC-PMSM-v0", "float32"
    if case == "pmsm_fin_til":
        kw = dict(converter=dict(interlocking_time=1e-6))
    elif case == "permexdc_rc":
        env_id, kw = "Cont-CC-PermExDc-v0", dict(supply=ga.RCVoltageSupply(u_nominal=60.0, supply_parameter=dict(R=0.05, C=4e-3)))
    elif case == "pmsm_fin_rc":  # finite converter behind an RC supply: leg states tracked by the dead-time-free code (Stepper::legs_of)
        kw = dict(supply=ga.RCVoltageSupply(u_nominal=420.0, supply_parameter=dict(R=0.5, C=2e-3)), tau=1e-4)
    elif case == "dfim_fin_rc":  # two bytes of leg state
        env_id, kw = "Finite-CC-DFIM-v0", dict(supply=ga.RCVoltageSupply(u_nominal=420.0, supply_parameter=dict(R=2.0, C=4e-3)))
    elif case == "dfim_fin_til":
        env_id = "Finite-CC-DFIM-v0"
        kw = dict(converter=ga.FiniteMultiConverter(subconverters=[ga.FiniteB6BridgeConverter(interlocking_time=1e-6), ga.FiniteB6BridgeConverter(interlocking_time=1e-6)]))
    elif case == "scim_dq":
        env_id, kw = "Cont-SC-SCIM-v0", dict(control_space="dq")
    elif case == "pmsm_dead3":
        kw = dict(physical_system_wrappers=(ga.DeadTimeProcessor(steps=3),), tau=1e-4)
    elif case == "pmsm_dqproc_dead2":
        env_id, kw = "Cont-SC-PMSM-v0", dict(physical_system_wrappers=(ga.DeadTimeProcessor(steps=2), ga.DqToAbcActionProcessor.make("PMSM")))
    elif case == "extex_fin_soa":
        env_id, kw = "Finite-CC-ExtExDc-v0", dict(obs_layout="soa")
    elif case == "eesm_f64":
        env_id, dtype = "Cont-CC-EESM-v0", "float64"

    def run(step_kernel):
        monkeypatch.setenv("GEMX_STEP_KERNEL", step_kernel)
        if case == "pmsm_random_init":
            env = _init_env("pmsm_sc_uniform", n, seed=5, ode_solver=ga.RK4Solver())[0]
        else:
            env = ga.make(env_id, n_envs=n, ode_solver=ga.RK4Solver(), dtype=dtype, **kw)
        ps = env.physical_system
        g = torch.Generator(device="cuda").manual_seed(11)
        if ps._discrete:
            nflat = int(np.prod(ps.action_space.nvec)) if hasattr(ps.action_space, "nvec") else int(ps.action_space.n)
            acts = torch.randint(0, nflat, (K, n), device="cuda", generator=g, dtype=torch.uint8)
        else:
            acts = (torch.rand((K, n, ps._n_act), device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(ps._tdtype)
        out = []
        for k in range(K):
            o = ps.simulate(acts[k])
            out.append((o.clone(), ps.done.clone()))
        assert ("step_kernel" in ps.last_launch()) == (step_kernel == "1")
        res = (torch.stack([o for o, _ in out]), torch.stack([d for _, d in out]), ps.get_state(), ps.get_switch_state())
        env.close()
        return res

    a, b = run("1"), run("0")
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    if case in ("permexdc_rc", "pmsm_fin_rc", "pmsm_dead3", "pmsm_random_init"):
        assert a[1].any()  # these terminate and auto-reset within the 48 steps: the reset path of both kernels is compared too


@pytest.mark.parametrize("name", ["rc_pmsm_fin_til_epi_uniform_tau1e-4_euler", "rc_permexdc_cont_free_held_euler", "rc_eesm_cont_epi_held_euler",
                                  "rc_dfim_fin_free_uniform_euler", "rc_scim_cont_sc_free_held_dopri5", "init:pmsm_sc_uniform", "init:extex_cc_uniform_interval"])
def test_full_pipelined_variant_matches_single_wave_kernel(name, monkeypatch):
    """RCVoltageSupply and random initialisers ride the pipelined kernel too (its FULL instantiation: per-lane supply voltage handed
    to the output waves, draws in the integrator's reset path): bit-identical to the single-wave kernel (GEMX_PIPE=0) on 128 envs --
    observations incl. the u_sup column, done masks, final ODE + supply state, and the random streams after in-kernel auto-resets."""
    import torch

    import gym_electric_motor_amd as ga

    n = 128

    def run(pipe):
        monkeypatch.setenv("GEMX_PIPE", pipe)
        if name.startswith("init:"):
            env = _init_env(name[5:], n, seed=9, ode_solver=ga.RK4Solver())[0]
            ps = env.physical_system
            g = torch.Generator(device="cuda").manual_seed(3)
            K = 300
            if ps._discrete:
                acts = torch.randint(0, 8, (K, n), device="cuda", generator=g, dtype=torch.uint8)
            else:
                acts = torch.rand((K, n, ps._n_act), device="cuda", generator=g) * 2 - 1
        else:
            d, meta = _load(name)
            env = _make_from_meta(meta, n, auto_reset=True)
            ps = env.physical_system
            acts = d["actions"]
            K = acts.shape[0]
            acts = torch.as_tensor(np.repeat(acts.reshape(K, 1, -1), n, axis=1))
            if ps._discrete and d["actions"].ndim == 1:
                acts = acts.reshape(K, n)
            acts = acts.cuda()
            # per-env variation, so that lanes differ: scale continuous actions / rotate discrete ones by the env index
            if ps._discrete and d["actions"].ndim == 1:
                acts = ((acts.long() + torch.arange(n, device="cuda").reshape(1, n)) % int(ps.action_space.n)).to(torch.uint8)
            elif not ps._discrete:
                acts = acts * torch.linspace(0.3, 1.0, n, device="cuda", dtype=acts.dtype).reshape(1, n, 1)
        obs, done = env.rollout(acts)
        kern = ps.last_launch()
        obs2, done2 = env.rollout(acts[:37])  # a second, shorter launch continues from the stored state (supply state / reset counters)
        res = (obs, done, obs2, done2, ps.get_state())
        env.close()
        return res, kern

    (a, ka), (b, kb) = run("1"), run("0")
    assert "advance_pipe_kernel" in ka and "advance_kernel" in kb
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    if name.startswith("init:") or "epi" in name:
        assert a[1].any()


def _varied_actions(d, ps, n):
    """A fixture's recorded action sequence for n envs, varied per env so that lanes differ (continuous: scaled by 0.3 .. 1; discrete:
    rotated by the env index)."""
    import torch

    acts = d["actions"]
    K = acts.shape[0]
    a = torch.as_tensor(np.repeat(acts.reshape(K, 1, -1), n, axis=1))
    if ps._discrete and acts.ndim == 1:
        a = a.reshape(K, n).cuda()
        return ((a.long() + torch.arange(n, device="cuda").reshape(1, n)) % int(ps.action_space.n)).to(torch.uint8)
    a = a.cuda()
    if not ps._discrete:
        a = a * torch.linspace(0.3, 1.0, n, device="cuda", dtype=a.dtype).reshape(1, n, 1)
    return a


PARTIAL_CASES = ["pmsm_epi_held_tau1e-4_euler",            # finite B6: voltage table, compact hand-off rows, one-step map
                 "scim_epi_uniform_euler",                 # continuous duty cycles (12 bytes per env-step through the loader), PolynomialStaticLoad
                 "permexdc_epi_held_euler",                # one-state DC machine (dc_stream_kernel wants whole workgroups: the pipelined kernel serves these)
                 "pmsm_free_uniform_til_euler",            # converter dead time: leg states loaded / stored per lane
                 "dfim_fin_epi_held_tau1e-4_euler",        # two bytes of leg state per env, 24-column rows
                 "pmsm_fin_dead1_til_free_uniform_euler",  # DeadTimeProcessor queue in HBM
                 "rc_pmsm_fin_til_epi_uniform_tau1e-4_euler",  # RCVoltageSupply: the FULL instantiation
                 "init:pmsm_sc_uniform",                   # random initialisers: reset counters per lane (FULL)
                 # non-default machines (oracle/make_golden.py:main_params): custom limits + tau 5e-5, a negative torque limit,
                 # l_sigs != l_sigr behind custom limits, a kink-band load with c != 0
                 "param_pmsm_fin_cc_lim_u350_epi_uniform_tau5e-5_euler", "param_pmsm_reversed_cont_cc_free_held_euler",
                 "param_scim_fin_cc_lim_epi_uniform_euler", "param_scim_cont_sc_free_held_dopri5"]


@pytest.mark.parametrize("name", PARTIAL_CASES)
@pytest.mark.parametrize("n", [16, 80, 208, 70, 7, 203])
def test_partial_last_workgroup_of_the_pipelined_kernel(name, n, monkeypatch):
    """A batch that is not a multiple of 64 envs no longer falls back to the single-wave kernel (round 4: 6-8 x slower, silently): the
    pipelined kernel's last workgroup takes the remaining envs (clamped loads, masked stores, lane-by-lane staging, row stores over
    the valid span), and batches whose rows are not 16-byte aligned (n = 70, 7, 203) take those general I/O paths in every workgroup.
    Every shape, bit for bit against the single-wave kernel: all observation rows and done bytes of all envs, a
    second launch from the stored state, and the final ODE / leg / supply state -- and the memory right behind every output tensor
    untouched (the partial workgroup's lanes beyond the batch store nothing)."""
    import torch

    import gym_electric_motor_amd as ga

    def run(pipe, shape):
        monkeypatch.setenv("GEMX_PIPE", pipe)
        if shape is None:
            monkeypatch.delenv("GEMX_PIPE_SHAPE", raising=False)
        else:
            monkeypatch.setenv("GEMX_PIPE_SHAPE", shape)
        if name.startswith("init:"):
            env = _init_env(name[5:], n, seed=9, ode_solver=ga.RK4Solver())[0]
            ps = env.physical_system
            g = torch.Generator(device="cuda").manual_seed(3)
            if ps._discrete:
                acts = torch.randint(0, 8, (150, n), device="cuda", generator=g, dtype=torch.uint8)
            else:
                acts = torch.rand((150, n, ps._n_act), device="cuda", generator=g) * 2 - 1
        else:
            d, meta = _load(name)
            env = _make_from_meta(meta, n, auto_reset=True)
            ps = env.physical_system
            acts = _varied_actions(d, ps, n)[:150]
        K = acts.shape[0]
        # outputs inside larger guarded buffers: [K * n * n_out] rows followed by a canary
        obuf = torch.full((K * n * ps._n_out + 64,), -7.0, device="cuda")
        dbuf = torch.full((K * n + 64,), 9, device="cuda", dtype=torch.uint8)
        obs = obuf[: K * n * ps._n_out].view(K, n, ps._n_out)
        done = dbuf[: K * n].view(K, n)
        env.rollout(acts, obs_out=obs, done_out=done)
        kern = ps.last_launch()
        assert (obuf[K * n * ps._n_out:] == -7.0).all() and (dbuf[K * n:] == 9).all()
        obs2, done2 = env.rollout(acts[:37])
        res = (obs.clone(), done.clone(), obs2, done2, ps.get_state(), ps.get_switch_state())
        env.close()
        return res, kern

    ref, kref = run("0", None)
    assert "advance_kernel" in kref
    shapes = (None,) if name.startswith(("rc_", "init:")) else (None, "0", "1", "2", "3")  # (FULL: one instantiation, shape <4, 2>)
    for shape in shapes:
        got, k = run("1", shape)
        assert "advance_pipe_kernel" in k, (shape, k)
        for x, y in zip(got, ref):
            assert torch.equal(x, y), (name, n, shape)
    if "epi" in name or name.startswith("init:"):
        assert ref[1].any()


CHECKPOINT_CASES = ["rc_pmsm_fin_til_epi_uniform_tau1e-4_euler",   # RCVoltageSupply rows + leg states (dead time)
                    "rc_permexdc_cont_free_held_euler",            # RC supply behind a continuous converter
                    "pmsm_fin_dead1_til_free_uniform_euler",       # DeadTimeProcessor queue + phase
                    "init:pmsm_sc_uniform",                        # random initialisers: per-env reset counters
                    "pmsm_epi_held_tau1e-4_euler",                 # nothing but ODE state (the aux blob is its header + the angle words)
                    "adaptive:scim_epi_uniform_euler"]             # error-controlled solver: the carried step size of every env


@pytest.mark.parametrize("name", CHECKPOINT_CASES)
@pytest.mark.parametrize("n", [128, 70])
def test_checkpoint_resumes_bit_for_bit(name, n):
    """A COMPLETE checkpoint (round 4 verdict: gemx_get_state moved the ODE rows and the angle only, so a handle with an RC supply, a
    DeadTimeProcessor or random initialisers could not be resumed): rollout K, save (state + leg states + aux blob + k), rollout K more
    == restore into a FRESH system, rollout K more -- observations, done bytes and the final state bit for bit; with K not a multiple
    of the DeadTimeProcessor's depth (the queue phase matters), through the pipelined kernel (n = 128) and the single-wave one (70).
    A blob from another configuration is refused."""
    import torch

    import gym_electric_motor_amd as ga

    def mk(nn=n):
        if name.startswith("init:"):
            env = _init_env(name[5:], nn, seed=11, ode_solver=ga.RK4Solver())[0]
            return env, None
        if name.startswith("adaptive:"):
            d, meta = _load(name[9:])
            return _make_from_meta(meta, nn, solver=ga.ScipyOdeSolver(), auto_reset=True), d
        d, meta = _load(name)
        return _make_from_meta(meta, nn, auto_reset=True), d

    env, d = mk()
    ps = env.physical_system
    K = 75
    if d is None:
        g = torch.Generator(device="cuda").manual_seed(5)
        acts = (torch.randint(0, 8, (2 * K, n), device="cuda", generator=g, dtype=torch.uint8) if ps._discrete
                else torch.rand((2 * K, n, ps._n_act), device="cuda", generator=g) * 2 - 1)
    else:
        acts = _varied_actions(d, ps, n)[: 2 * K]
    o1, d1 = env.rollout(acts[:K])
    ck = ps.get_checkpoint()
    assert ck["k"] == K and ck["aux"].numel() % 16 == 0
    ck = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ck.items()}
    o2, d2 = env.rollout(acts[K:])
    s2, sw2 = ps.get_state(), ps.get_switch_state()
    env.close()
    env_b, _ = mk()
    pb = env_b.physical_system
    pb.rollout(acts[:13])  # (a handle that has already moved: everything is overwritten)
    pb.set_checkpoint(ck)
    assert pb.k == K
    o3, d3 = env_b.rollout(acts[K:])
    assert torch.equal(o3, o2) and torch.equal(d3, d2)
    assert torch.equal(pb.get_state(), s2) and torch.equal(pb.get_switch_state(), sw2)
    if name.startswith("init:") or name == "pmsm_epi_held_tau1e-4_euler":
        assert d2.any()  # (episodes end -- and, with random initialisers, restart from the next draw -- after the restore too)
    env_b.close()
    other, _ = mk(n + 16)
    with pytest.raises(ValueError):
        other.physical_system.set_checkpoint(ck)
    bad = dict(ck, aux=torch.zeros(int(other.physical_system._L.gemx_aux_state_bytes(other.physical_system._handle)), dtype=torch.uint8, device="cuda"))
    bad["state"], bad["switch_state"] = other.physical_system.get_state(), other.physical_system.get_switch_state()
    with pytest.raises(ValueError):  # right size, not a blob
        other.physical_system.set_checkpoint(bad)
    other.close()


def test_random_initialiser_counters_after_create():
    """gemx_create leaves draw #1 in place with the counters at 1 (ABI 6): an env's first in-kernel auto-reset is draw #2 -- not draw #1
    again (advisor finding, round 4: a caller stepping with auto_reset and never calling reset started episodes 1 and 2 from the same
    state) -- and so is the user's first reset(); the construction-time observation rows ARE draw #1."""
    import torch

    import gym_electric_motor_amd as ga

    n = 128
    env = _init_env("pmsm_sc_uniform", n, seed=21, ode_solver=ga.RK4Solver())[0]
    ps = env.physical_system
    obs0 = ps._obs.clone()           # rows of draw #1 (gemx_reset_again at construction)
    s1 = ps.get_state()
    counters = lambda: ps.get_checkpoint()["aux"][128 : 128 + 4 * n].view(torch.int32)  # noqa: E731  (header | no RC rows | no queue | counters | angle words)
    assert (counters() == 1).all()
    r2 = env.reset()[0].clone()      # draw #2
    s2 = ps.get_state()
    assert not torch.equal(s1, s2) and not torch.equal(obs0, r2)
    assert (counters() == 2).all()
    env.close()
    env = _init_env("pmsm_sc_uniform", n, seed=21, ode_solver=ga.RK4Solver())[0]  # same seed: same draws
    assert torch.equal(env.physical_system.get_state(), s1) and torch.equal(env.physical_system._obs, obs0)
    env.reset()
    assert torch.equal(env.physical_system.get_state(), s2)
    env.close()


def test_the_single_wave_fallback_says_so_and_unaligned_batches_no_longer_take_it(capfd):
    """Since round 5 EVERY batch size runs the pipelined kernel (rows that are not 16-byte aligned -- n_envs not a multiple of 16 -- go
    lane by lane through its general I/O paths instead of falling back, 6-8 x slower, to the single-wave kernel), and so do custom
    constraint sets and solver sub-steps (its rolled copy of the step), and random initial states at any size (the loader wave prepares
    the draws).  What still lands on the fallback -- random initial states TOGETHER with a custom constraint set -- says so, once per
    handle, on stderr (GEMX_QUIET=1 silences it)."""
    import torch

    import gym_electric_motor_amd as ga

    for n in (70, 7, 1000):
        env = ga.make("Finite-CC-PMSM-v0", n_envs=n)
        env.rollout(torch.zeros((8, n), dtype=torch.uint8, device="cuda"))
        assert "advance_pipe_kernel" in env.physical_system.last_launch(), n
        env.close()
    for kw in (dict(constraints=("i_sq",)), dict(ode_solver=ga.RK4Solver(nsteps=3))):
        env = ga.make("Finite-CC-PMSM-v0", n_envs=128, **kw)
        env.rollout(torch.zeros((8, 128), dtype=torch.uint8, device="cuda"))
        assert "advance_pipe_kernel" in env.physical_system.last_launch(), kw
        env.close()
    assert "fallback" not in capfd.readouterr().err
    n = 65600  # 1025 workgroups: one more than 4 per CU (the FULL instantiation's old size rule)
    env = _init_env("pmsm_sc_uniform", n, seed=3)[0]
    acts = torch.zeros((8, n, env.physical_system._n_act), dtype=torch.float32, device="cuda")
    env.rollout(acts)
    assert "advance_pipe_kernel" in env.physical_system.last_launch()
    env.close()
    assert "fallback" not in capfd.readouterr().err
    env = _init_env("pmsm_sc_uniform", 128, seed=3, constraints=("i_sq",))[0]
    acts = torch.zeros((8, 128, env.physical_system._n_act), dtype=torch.float32, device="cuda")
    env.rollout(acts)
    env.rollout(acts)
    assert "advance_kernel" in env.physical_system.last_launch()
    env.close()
    err = capfd.readouterr().err
    assert err.count("single-wave fallback kernel") == 1 and "random initial states" in err


@pytest.mark.parametrize("case", ["pmsm_sc_uniform", "permexdc_sc_gauss", "extex_cc_uniform_interval", "eesm_sc_uniform", "scim_sc_uniform",
                                  "scim_cc_negspeed_uniform", "dfim_cc_negspeed_interval_uniform"])
@pytest.mark.parametrize("n", [70, 4096])
def test_prepared_draws_of_the_loader_wave_give_the_inline_draws_bits(case, n, monkeypatch):
    """Round 5: in the FULL pipelined kernel the loader wave computes every lane's NEXT random initial state ahead of time (a pure function
    of (env, reset count)); the integrator takes the prepared entry at a reset and draws inline only when a lane resets again before the
    loader's next pass.  Either way the bits are those of the single-wave kernel, which always draws inline: observations, terminations,
    states and reset counters, over launches with many terminations (held actions drive the currents into their limits)."""
    import torch

    import gym_electric_motor_amd as ga

    K = 400

    def run(pipe):
        monkeypatch.setenv("GEMX_PIPE", pipe)
        env = _init_env(case, n, seed=13)[0]
        ps = env.physical_system
        g = torch.Generator(device="cuda").manual_seed(23)
        acts = (torch.rand((K, n, ps._n_act), device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(ps._tdtype)
        acts[20:] = acts[20]  # held: every env runs into a limit again and again
        obs, done = env.rollout(acts)
        assert ("advance_pipe_kernel" in ps.last_launch()) == (pipe == "1"), ps.last_launch()
        obs2, done2 = env.rollout(acts[:37])  # (a launch whose last block is partial)
        res = (obs.clone(), done.clone(), obs2.clone(), done2.clone(), ps.get_state(), ps.get_checkpoint()["aux"].clone())  # (aux: the reset counters)
        env.close()
        return res

    a, b = run("1"), run("0")
    for x, y in zip(a, b):
        assert torch.equal(x.cpu(), y.cpu())
    per_env = a[1].sum(dim=0)
    assert int(per_env.max()) >= 3 and float((per_env > 0).float().mean()) > 0.2, "too few terminations to exercise the reset path"


@pytest.mark.parametrize("combo", ["dead_time", "rc_supply", "dead_time+rc_supply", "reward", "synthetic"])
def test_prepared_draws_beside_the_other_per_lane_features(combo, monkeypatch):
    """Random initial states (RINIT instantiation, prepared draws) together with what else lives in the FULL kernel or its loader wave: a
    DeadTimeProcessor queue (refilled at every reset), the RC supply's per-lane state, the fused reward's reference rows, synthetic
    actions generated by the same loader wave.  Bit for bit the single-wave kernel's results (synthetic actions: the same stream fed
    as a tensor)."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 200, 300

    def run(pipe):
        monkeypatch.setenv("GEMX_PIPE", pipe)
        kw = dict(motor=ga.PermanentMagnetSynchronousMotor(motor_initializer=dict(random_init="uniform")), seed=31, n_envs=n, ode_solver=ga.RK4Solver(), tau=1e-4)
        if "dead_time" in combo:
            kw["physical_system_wrappers"] = (ga.DeadTimeProcessor(steps=2),)
        if "rc_supply" in combo:
            kw["supply"] = ga.RCVoltageSupply(u_nominal=420.0, supply_parameter=dict(R=0.5, C=2e-3))
        env = ga.make("Cont-CC-PMSM-v0", **kw)
        ps = env.physical_system
        g = torch.Generator(device="cuda").manual_seed(41)
        acts = (torch.rand((K, n, ps._n_act), device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(ps._tdtype)
        acts[30:] = acts[30]
        extra = ()
        if combo == "reward":
            rc = ps.set_reward(reward_weights=dict(i_sd=0.5, i_sq=0.5), referenced_states=("i_sd", "i_sq"))
            refs = torch.rand((K, n, int(rc.n_ref)), device="cuda", generator=g) - 0.5
            rew = torch.empty((K, n), device="cuda")
            obs, done = ps.rollout(acts, references=refs, reward_out=rew)[:2]
            extra = (rew.clone(),)
        elif combo == "synthetic":
            if pipe == "1":
                obs, done = ps.rollout_synthetic(K, seed=5, step0=0)
            else:
                obs, done = ps.rollout(ps.synthetic_actions(K, seed=5, step0=0))
        else:
            obs, done = ps.rollout(acts)
        if pipe == "1":
            assert "advance_pipe_kernel" in ps.last_launch(), ps.last_launch()
        res = (obs.clone(), done.clone(), ps.get_state(), ps.get_checkpoint()["aux"].clone()) + extra
        env.close()
        return res

    a, b = run("1"), run("0")
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert int(a[1].sum()) > n, "too few terminations to exercise the reset path"


def test_rate_limiter_per_handle_switch_changes_the_launch_not_the_results():
    """gemx_set_rate_limiter / system.set_rate_limiter (advisor finding of round 4: a per-handle switch beside the environment variables):
    off, open loop, an explicit target, closed loop -- the launch line says what ran, the bits are the same."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 65536, 128
    acts = torch.randint(0, 8, (K, n), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    ref = None
    for mode, kw in (("off", {}), ("open", {}), ("open", dict(target_gbps=5000.0)), ("closed", {})):
        env = ga.make("Finite-CC-PMSM-v0", n_envs=n)
        ps = env.physical_system
        ps.set_rate_limiter(mode, **kw)
        obs, done = env.rollout(acts)
        line = ps.last_launch()
        if mode != "closed":  # (a closed-loop launch may be the bracket's unpaced candidate)
            assert ("rate limit" in line) == (mode == "open"), line
        assert ("limiter calibrat" in line) == (mode == "closed"), line
        if ref is None:
            ref = (obs.clone(), done.clone())
        else:
            assert torch.equal(obs, ref[0]) and torch.equal(done, ref[1])
        env.close()
    env = ga.make("Finite-CC-PMSM-v0", n_envs=64)
    with pytest.raises(ValueError):
        env.physical_system.set_rate_limiter("sometimes")
    env.close()


SLOW_STEP_CASES = [
    # (env id, make kwargs): custom constraint sets and solver sub-steps on the pipelined kernel's rolled copy of the step
    ("Finite-CC-PMSM-v0", dict(constraints=("i_sq",))),
    ("Finite-CC-PMSM-v0", dict(constraints=("i_sd", "omega"), solver="rk4x3")),
    ("Cont-CC-PMSM-v0", dict(solver="euler4")),
    ("Cont-SC-SCIM-v0", dict(constraints=("i_sa", "i_sb"), solver="rk4x2")),
    ("Finite-CC-DFIM-v0", dict(solver="rk4x2")),
    ("Cont-CC-ExtExDc-v0", dict(constraints=("i_a",), solver="dp5")),
    ("Finite-CC-ShuntDc-v0", dict(solver="euler4", delay=2)),
    ("Cont-CC-EESM-v0", dict(constraints=("i_e", "i_sq"), delay=1)),
    ("Cont-TC-SeriesDc-v0", dict(constraints=("i", "torque"), rc=True)),
    ("Cont-SC-PermExDc-v0", dict(solver="rk4x3", load="poly")),
]


@pytest.mark.parametrize("env_id, opts", SLOW_STEP_CASES, ids=[f"{e}-{'-'.join(f'{k}' for k in o)}" for e, o in SLOW_STEP_CASES])
@pytest.mark.parametrize("n", [128, 70])
def test_sub_steps_and_custom_constraints_on_the_pipelined_kernel_bit_for_bit(env_id, opts, n, monkeypatch):
    """Round 5: solver sub-steps (nsteps > 1) and custom constraint sets run the pipelined kernel (before: the single-wave fallback,
    6-8 x slower).  Its rolled copy of the step must give the single-wave kernel's bits: observations, terminations, auto-resets,
    final state -- through dead time, an RC supply, a kinked load, whole and partial workgroups."""
    import torch

    import gym_electric_motor_amd as ga

    K = 150
    sol = {"rk4x3": lambda: ga.RK4Solver(nsteps=3), "rk4x2": lambda: ga.RK4Solver(nsteps=2), "euler4": lambda: ga.EulerSolver(nsteps=4),
           "dp5": lambda: ga.DormandPrince5Solver(nsteps=2)}

    def run(pipe):
        monkeypatch.setenv("GEMX_PIPE", pipe)
        kw = dict(n_envs=n)
        if "constraints" in opts:
            kw["constraints"] = opts["constraints"]
        if "solver" in opts:
            kw["ode_solver"] = sol[opts["solver"]]()
        if opts.get("rc"):
            kw["supply"] = ga.RCVoltageSupply(u_nominal=420.0, supply_parameter=dict(R=0.05, C=4e-3))
        if opts.get("load") == "poly":
            kw["load"] = ga.PolynomialStaticLoad(load_parameter=dict(a=0.01, b=0.01, c=0.0, j_load=1e-4))
        if "delay" in opts:
            kw["physical_system_wrappers"] = (ga.DeadTimeProcessor(steps=opts["delay"]),)
        env = ga.make(env_id, **kw)
        ps = env.physical_system
        g = torch.Generator(device="cuda").manual_seed(17)
        if ps._discrete:
            nflat = int(np.prod(ps.action_space.nvec)) if hasattr(ps.action_space, "nvec") else int(ps.action_space.n)
            acts = torch.randint(0, nflat, (K, n), device="cuda", generator=g, dtype=torch.uint8)
        else:
            acts = (torch.rand((K, n, ps._n_act), device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(ps._tdtype)
        acts[40:] = acts[40]  # (held from step 40 on: the currents run into their limits, so that the constraint sets terminate episodes)
        obs, done = env.rollout(acts)
        assert ("advance_pipe_kernel" in ps.last_launch()) == (pipe == "1"), ps.last_launch()
        obs2, done2 = env.rollout(acts)  # a second launch: carried state, queue, supply
        res = (obs.clone(), done.clone(), obs2.clone(), done2.clone(), ps.get_state())
        env.close()
        return res

    a, b = run("1"), run("0")
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    if "constraints" in opts:
        assert a[1].any() or a[3].any(), "no termination in the run: the custom constraint set was not exercised"


@pytest.mark.parametrize("env_id, delay, kw", [
    ("Finite-CC-PMSM-v0", 3, dict(tau=1e-4)), ("Finite-CC-PMSM-v0", 8, dict(tau=1e-4)), ("Finite-CC-PMSM-v0", 1, dict(tau=1e-4)),
    ("Cont-CC-PermExDc-v0", 2, {}), ("Cont-SC-SCIM-v0", 1, dict(control_space="dq")), ("Finite-CC-DFIM-v0", 2, {}), ("Finite-CC-EESM-v0", 5, dict(tau=1e-4)),
    ("Finite-CC-ShuntDc-v0", 4, {}),
    # behind a DqToAbcActionProcessor the queue holds TRANSFORMED actions: a row buffer indexed by the step of the block
    ("Cont-CC-PMSM-v0", 1, dict(dqproc="PMSM")), ("Cont-CC-PMSM-v0", 2, dict(dqproc="PMSM", tau=1e-4)), ("Cont-CC-PMSM-v0", 8, dict(dqproc="PMSM")),
    ("Cont-SC-PMSM-v0", 3, dict(dqproc="PMSM")), ("Cont-CC-SynRM-v0", 2, dict(dqproc="PMSM")), ("Cont-CC-EESM-v0", 2, dict(dqproc="EESM")),
])
def test_delayed_read_deadtime_queue_matches_the_fifo_representation(env_id, delay, kw, monkeypatch):
    """DeadTimeProcessor in the pipelined kernel's deep shape: no queue, but the action row staged `delay` steps earlier, zeroed while
    fewer than `delay` steps have passed since the env's reset (table-driven, unrolled blocks stay).  Bit-identical to the single-wave
    kernel's explicit FIFO: one launch, uneven chunks (the ring in HBM hands the pending entries over, incl. K < delay and resets right
    before a launch boundary), and a continuation after the chunks; per-env random actions, default constraints + auto-reset."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 256, 173

    kw = dict(kw)
    dqproc = kw.pop("dqproc", None)
    wrappers = (ga.DeadTimeProcessor(steps=delay),) + ((ga.DqToAbcActionProcessor.make(dqproc),) if dqproc else ())

    def mk(pipe):
        monkeypatch.setenv("GEMX_PIPE", pipe)
        monkeypatch.setenv("GEMX_PIPE_SHAPE", "0")
        return ga.make(env_id, n_envs=n, ode_solver=ga.RK4Solver(), physical_system_wrappers=wrappers, **kw)

    env = mk("1")
    ps = env.physical_system
    g = torch.Generator(device="cuda").manual_seed(4)
    if ps._discrete:
        nflat = int(np.prod(ps.action_space.nvec)) if hasattr(ps.action_space, "nvec") else int(ps.action_space.n)
        acts = torch.randint(0, nflat, (K + 40, n), device="cuda", generator=g, dtype=torch.uint8)
    else:
        acts = torch.rand((K + 40, n, ps._n_act), device="cuda", generator=g) * 2 - 1
    obs, done = env.rollout(acts[:K])
    assert "advance_pipe_kernel" in ps.last_launch()
    if "DFIM" not in env_id and "EESM-v0" not in env_id:  # (their hand-off rows do not fit the deep shape: they keep the FIFO
        assert "D=12" in ps.last_launch()                   # representation, compared all the same)
    obs_c, done_c = env.rollout(acts[K:])  # continuation from the ring the launch left behind
    ref = mk("0")
    robs, rdone = ref.rollout(acts[:K])
    assert "advance_kernel" in ref.physical_system.last_launch()
    robs_c, rdone_c = ref.rollout(acts[K:])
    assert torch.equal(obs, robs) and torch.equal(done, rdone) and torch.equal(obs_c, robs_c) and torch.equal(done_c, rdone_c)
    e2 = mk("1")
    parts, k0 = [], 0
    for kk in (1, 7, 2, 30, 13, 24, 96):  # 1 and 2: fewer steps than some queues are deep; 24 = two full blocks; 96 = eight
        parts.append(e2.rollout(acts[k0:k0 + kk]))
        k0 += kk
    assert k0 == K
    assert torch.equal(torch.cat([p[0] for p in parts]), obs) and torch.equal(torch.cat([p[1] for p in parts]), done)
    o2, d2 = e2.rollout(acts[K:])
    assert torch.equal(o2, obs_c) and torch.equal(d2, done_c)
    if "PMSM" in env_id or "EESM" in env_id or "ShuntDc" in env_id or "PermExDc" in env_id:
        assert done.any()  # resets happened: the zero-action window after a reset was exercised
    for e in (env, ref, e2):
        e.close()


RESET_ACTION_CASES = ["pmsm_cont_dead2_reset_epi_held_euler", "pmsm_fin_dead3_reset_epi_uniform_tau1e-4_euler", "permexdc_cont_dead1_reset_epi_held_euler",
                      "pmsm_cont_dqproc_dead2_reset_epi_held_euler", "extex_fin_dead2_reset_epi_uniform_euler"]


@pytest.mark.parametrize("name", RESET_ACTION_CASES)
def test_custom_dead_time_reset_action_in_every_kernel(name, monkeypatch):
    """DeadTimeProcessor(steps, reset_action=...) (dead_time_processor.py:27-50; round 4): every reset -- gemx_reset and
    the in-kernel auto-reset -- refills the queue with a NON-zero action.  The five fixtures recorded from the reference with such a
    processor (continuous / discrete / MultiDiscrete actions, alone and inside the dq processor; episodic, so the refill happens inside
    the run) are compared by the Euler golden tests like every other fixture; here every representation of the queue must agree bit for
    bit: the pipelined kernel's deep shape (delayed reads / the row buffer of transformed actions), its <4, 2> shape (LDS FIFO), the
    single-wave kernel, uneven chunks (the ring in HBM between launches) and step-by-step simulate() (step_kernel) -- with per-env
    random actions and resets at different steps in different lanes."""
    import torch

    d, meta = _load(name)
    n, K = 192, 150

    def mk(pipe, shape=None):
        monkeypatch.setenv("GEMX_PIPE", pipe)
        if shape is None:
            monkeypatch.delenv("GEMX_PIPE_SHAPE", raising=False)
        else:
            monkeypatch.setenv("GEMX_PIPE_SHAPE", shape)
        return _make_from_meta(meta, n, solver="rk4", auto_reset=True)

    env = mk("1", "0")
    ps = env.physical_system
    assert any(ps._cfg.action_delay_reset[i] != 0.0 for i in range(6)) and ps._cfg.action_delay == meta["dead_time_steps"]
    g = torch.Generator(device="cuda").manual_seed(8)
    if ps._discrete:
        nflat = int(np.prod(ps.action_space.nvec)) if hasattr(ps.action_space, "nvec") else int(ps.action_space.n)
        acts = torch.randint(0, nflat, (K, n), device="cuda", generator=g, dtype=torch.uint8)
    else:
        acts = torch.rand((K, n, ps._n_act), device="cuda", generator=g) * 2 - 1
    obs, done = env.rollout(acts)
    assert done.any() and not done.all()
    for pipe, shape in (("1", "1"), ("0", None)):
        e = mk(pipe, shape)
        o, dn = e.rollout(acts)
        assert torch.equal(o, obs) and torch.equal(dn, done), (pipe, shape, e.physical_system.last_launch())
        e.close()
    e2 = mk("1", "0")
    parts, k0 = [], 0
    for kk in (1, 2, 9, 24, 50, 64):
        parts.append(e2.rollout(acts[k0:k0 + kk]))
        k0 += kk
    assert k0 == K and torch.equal(torch.cat([p_[0] for p_ in parts]), obs) and torch.equal(torch.cat([p_[1] for p_ in parts]), done)
    e3 = mk("1")
    for k in range(40):
        assert torch.equal(e3.physical_system.simulate(acts[k]), obs[k]) and torch.equal(e3.physical_system.done, done[k]), k
    # the reset action is what the converter sees right after a reset: a handle with the DEFAULT (zero) reset action differs
    m0 = dict(meta)
    m0.pop("dead_time_reset_action")
    monkeypatch.setenv("GEMX_PIPE", "1")
    e0 = _make_from_meta(m0, n, solver="rk4", auto_reset=True)
    o0, _ = e0.rollout(acts)
    assert not torch.equal(o0[0], obs[0])
    for e in (env, e2, e3, e0):
        e.close()


def test_random_initialisers_streams_and_auto_reset():
    """Counter-based Philox streams: same seed -> same states, other seed / env / reset -> other states; the in-kernel auto-reset
    draws a fresh state (inside the bounds) for exactly the envs that terminated; step-by-step == fused == chunked, bit for bit."""
    import torch

    n, K = 192, 64
    mk = lambda seed: _init_env("pmsm_sc_uniform", n, seed=seed, ode_solver=__import__("gym_electric_motor_amd").RK4Solver())[0]  # noqa: E731
    e1, e2, e3 = mk(11), mk(11), mk(12)
    y1, y2, y3 = (e.physical_system.get_state() for e in (e1, e2, e3))
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)
    assert len(torch.unique(y1[1])) > n - 3  # per-env draws
    e1.reset()
    assert not torch.equal(e1.physical_system.get_state(), y1)  # second reset of the same env: a new draw
    e2.reset()
    assert torch.equal(e1.physical_system.get_state(), e2.physical_system.get_state())
    g = torch.Generator(device="cuda").manual_seed(5)
    acts = torch.rand((K, n, 3), device="cuda", generator=g) * 2 - 1
    obs, done = e1.rollout(acts)
    assert done.any() and not done.all()
    parts = [e2.rollout(acts[:10]), e2.rollout(acts[10:33]), e2.rollout(acts[33:])]
    assert torch.equal(torch.cat([p_[0] for p_ in parts]), obs) and torch.equal(torch.cat([p_[1] for p_ in parts]), done)
    e4 = mk(11)
    e4.reset()
    for k in range(8):
        assert torch.equal(e4.physical_system.simulate(acts[k]), obs[k])
    # an env that terminated at step k starts step k+1 from a fresh draw: its currents jump away from the violating state
    ps = e1.physical_system
    isd, isq = ps.state_positions["i_sd"], ps.state_positions["i_sq"]
    k, j = [int(x[0]) for x in torch.nonzero(done[:-1], as_tuple=True)]
    assert (obs[k, j, isd] ** 2 + obs[k, j, isq] ** 2) > 1.0
    lim = ps.limits
    nom = ps.electrical_motor.nominal_values["i_sd"] / lim[isd]
    assert abs(float(obs[k + 1, j, isd])) < nom * 1.5 + 0.2
    for e in (e1, e2, e3, e4):
        e.close()


@pytest.mark.parametrize("n", [8192, 8192 + 2 * 37])  # (second: N/2 % 64 != 0 -- every half ends in a partial workgroup, and starts inside one of the whole)
@pytest.mark.parametrize("what", ["pmsm_sc_uniform", "scim_sc_uniform", "dfim_cc_negspeed_interval_uniform", "synthetic", "synthetic_cont", "wiener"])
def test_two_half_size_shards_equal_one_whole_bit_for_bit(what, n):
    """Every device-side random stream is keyed by the GLOBAL env index (gemx_config.env_base, ABI 7): two handles of N/2 envs with bases 0
    and N/2 produce, concatenated, exactly what one handle of N envs produces -- random initial states (uniform; the induction machines'
    flux mode with its look-back at the previous draw) through create, reset and the in-kernel auto-resets of a fused rollout (prepared
    draws of the loader wave), `rollout_synthetic`'s actions, and the Wiener reference generators.  Round 5 keyed them by the local index:
    every shard of a multi-GPU job replayed shard 0's draws (the reference: one seed-sequence branch per env object, core.py:373-385,
    physical_systems.py:164-169, random_component.py:60-87).  Also: a shard with another base draws OTHER states."""
    import torch

    import gym_electric_motor_amd as ga

    h = n // 2
    K = 192

    def cat(parts, dim):
        return torch.cat([p_.cpu() for p_ in parts], dim=dim)

    if what == "wiener":
        envs = [ga.make("Cont-CC-PMSM-v0", n_envs=m, env_base=b) for m, b in ((n, 0), (h, 0), (h, h))]
        gens = [ga.BatchedWienerProcessReferenceGenerator(reference_states=("i_sd", "i_sq"), seed=31).set_modules(e.physical_system) for e in envs]
        assert [int(g._cfg.env_base) for g in gens] == [0, 0, h]  # (taken from the physical system)
        for g in gens:
            g.reset()
        d = (torch.rand((K, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) < 0.01).to(torch.uint8)
        whole = gens[0].rollout(K, done=d)
        halves = cat([gens[1].rollout(K, done=d[:, :h].contiguous()), gens[2].rollout(K, done=d[:, h:].contiguous())], 1)
        assert torch.equal(whole.cpu(), halves)
        assert not torch.equal(whole[:, :h].cpu(), whole[:, h:].cpu())
        st = [g.state() for g in gens]
        for j in range(3):
            assert torch.equal(st[0][j].cpu(), cat([st[1][j], st[2][j]], 1))
        for e in envs:
            e.close()
        return
    if what.startswith("synthetic"):
        env_id = "Finite-CC-PMSM-v0" if what == "synthetic" else "Cont-SC-SCIM-v0"
        envs = [ga.make(env_id, n_envs=m, env_base=b, tau=1e-4) for m, b in ((n, 0), (h, 0), (h, h))]
        outs = []
        for e in envs:
            ps = e.physical_system
            a = ps.synthetic_actions(K, seed=9, step0=5)
            o, d = ps.rollout_synthetic(K, seed=9, step0=5)
            assert "advance_pipe_kernel" in ps.last_launch()
            outs.append((a.clone(), o.clone(), d.clone()))
        for j in range(3):
            assert torch.equal(outs[0][j].cpu(), cat([outs[1][j], outs[2][j]], 1)), j
        assert not torch.equal(outs[1][0].cpu(), outs[2][0].cpu())  # the second shard's actions are not the first shard's
        for e in envs:
            e.close()
        return
    envs = [_init_env(what, m, seed=13, env_base=b)[0] for m, b in ((n, 0), (h, 0), (h, h))]
    pss = [e.physical_system for e in envs]
    y = [ps.get_state() for ps in pss]  # draw #1 (create)
    assert torch.equal(y[0].cpu(), cat(y[1:], 1)) and not torch.equal(y[1].cpu(), y[2].cpu())
    r = [ps.reset() for ps in pss]  # draw #2
    assert torch.equal(r[0].cpu(), cat(r[1:], 0))
    g = torch.Generator(device="cuda").manual_seed(23)
    acts = (torch.rand((K, n, pss[0]._n_act), device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(pss[0]._tdtype)
    acts[20:] = acts[20]  # held: every env runs into a limit again and again (auto-resets: prepared and inline draws)
    res = []
    for ps, sl in zip(pss, (slice(0, n), slice(0, h), slice(h, n))):
        o, d = ps.rollout(acts[:, sl].contiguous())
        assert "advance_pipe_kernel" in ps.last_launch()
        res.append((o.clone(), d.clone(), ps.get_state(), ps.get_checkpoint()["aux"].clone()))
    assert torch.equal(res[0][0].cpu(), cat([res[1][0], res[2][0]], 1)) and torch.equal(res[0][1].cpu(), cat([res[1][1], res[2][1]], 1))
    assert torch.equal(res[0][2].cpu(), cat([res[1][2], res[2][2]], 1))
    per_env = res[0][1].sum(dim=0)
    assert int(per_env.max()) >= 3 and float((per_env > 0).float().mean()) > 0.2, "too few terminations to exercise the reset path"
    # the checkpoint blob names its shard: restoring shard 1's blob into shard 0's handle is refused
    with pytest.raises(ValueError, match="env_base"):
        pss[1].set_checkpoint(dict(pss[1].get_checkpoint(), aux=res[2][3]))
    for e in envs:
        e.close()


def test_random_gaussian_initialiser_is_a_truncated_normal():
    """random_init='gaussian': normal(mue, sigma) truncated to the bounds (scipy.stats.truncnorm, electric_motor.py:236-249).
    (The reference passes a CONSTANT random_state to truncnorm.rvs, so it returns the same draw at every reset -- visible in
    tests/golden/init_samples.npz -- which is not reproduced; the distribution it draws from is.)"""
    from scipy import stats

    n = 8000
    env, meta, ref_y, _ = _init_env("permexdc_sc_gauss", n)
    y = env.physical_system.get_state().double().cpu().numpy().T
    assert np.ptp(ref_y, axis=0).max() < 1e-12  # the reference quirk
    for j, (mu, sg, lo, hi) in enumerate([(100.0, 60.0, -300.0, 300.0), (30.0, 40.0, -50.0, 90.0)]):
        a, b = (lo - mu) / sg, (hi - mu) / sg
        assert y[:, j].min() >= lo - 1e-3 and y[:, j].max() <= hi + 1e-3
        assert stats.kstest(y[:, j], stats.truncnorm(a, b, loc=mu, scale=sg).cdf).pvalue > 1e-3, j
    env.close()


def test_device_wiener_reference_generator_matches_reference_distribution():
    """Device-side MultipleReferenceGenerator([Wiener(i_sd), Wiener(i_sq)]) (csrc/gemx_refgen.hip) vs samples of the live reference
    (tests/golden/wiener_samples.npz): margins equal; initial values, sub-episode sigmas and lengths, sigma-normalised increments
    pass two-sample KS tests; the walk is clipped to the margins; chunked == one-shot; terminations restart the generators; the
    tensor feeds the fused reward."""
    import torch
    from scipy import stats

    import gym_electric_motor_amd as ga

    w = np.load(os.path.join(GOLDEN, "wiener_samples.npz"))
    n, K = 4096, 700
    env = ga.make("Cont-CC-PMSM-v0", n_envs=n)
    ps = env.physical_system
    gen = ga.BatchedWienerProcessReferenceGenerator(reference_states=("i_sq", "i_sd"), seed=31).set_modules(ps)
    assert gen.reference_names == ("i_sd", "i_sq")  # state order of the physical system = column order of the reward's references
    assert np.allclose([[gen._cfg.margin_lo[j], gen._cfg.margin_hi[j]] for j in range(2)], w["margins"], rtol=1e-14)
    gen.reset()
    v0, _, _ = gen.state()
    for j in range(2):  # reset(): initial reference ~ U(initial_range = limit margin)
        assert stats.ks_2samp(v0[j].cpu().numpy(), w["initial_values"][:, j]).pvalue > 1e-3
    refs = gen.rollout(K)
    torch.cuda.synchronize()
    r = refs.double().cpu().numpy()
    lo, hi = w["margins"][0]
    assert r.min() >= lo - 1e-6 and r.max() <= hi + 1e-6 and (np.abs(r) > hi - 1e-6).any()  # clipped walk that does reach the margin
    twin = ga.BatchedWienerProcessReferenceGenerator(reference_states=("i_sd", "i_sq"), seed=31).set_modules(ps)
    twin.reset()
    parts = torch.cat([twin.rollout(1), twin.rollout(249), twin.rollout(450)])
    assert torch.equal(parts, refs)
    # first sub-episode of every (env, generator): sigma, length, increments
    g2 = ga.BatchedWienerProcessReferenceGenerator(reference_states=("i_sd", "i_sq"), seed=77).set_modules(ps)
    g2.reset()
    first = g2.rollout(1)
    _, sg, left = g2.state()
    rest = g2.rollout(450).double().cpu().numpy()
    sg, left = sg.cpu().numpy(), left.cpu().numpy()
    for j in range(2):
        assert stats.ks_2samp(np.log10(sg[j]), np.log10(w[f"sub_sigma_{j}"])).pvalue > 1e-3
        assert stats.ks_2samp((left[j] + 1).astype(float), w[f"sub_len_{j}"].astype(float)).pvalue > 1e-3
        assert left[j].min() + 1 >= 500 and left[j].max() + 1 < 2000
        seq = np.concatenate([first.double().cpu().numpy()[:, :, j], rest[:, :, j]])  # [451, N] all inside the first sub-episode (>= 500)
        dz = np.diff(seq, axis=0) / sg[j][None, :]
        inside = (seq[1:] > lo + 1e-4) & (seq[1:] < hi - 1e-4) & (seq[:-1] > lo + 1e-4) & (seq[:-1] < hi - 1e-4) & (sg[j][None, :] > 3e-3)
        z = dz[inside][:200000]  # (fp32 storage: keep sigmas whose steps are well above the rounding of values ~0.5)
        assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
        assert stats.ks_2samp(z[:20000], w[f"z_{j}"][:20000]).pvalue > 1e-3
    # terminations: the generators of a terminated env restart (new initial value, new sub-episode)
    done = torch.zeros((50, n), dtype=torch.uint8, device="cuda")
    done[20, ::2] = 1
    g3 = ga.BatchedWienerProcessReferenceGenerator(reference_states=("i_sd", "i_sq"), seed=5).set_modules(ps)
    g3.reset()
    r3 = g3.rollout(50, done=done).double().cpu().numpy()
    jump = np.abs(r3[21, :, 0] - r3[20, :, 0])
    assert np.median(jump[::2]) > 0.1 and np.median(jump[1::2]) < 0.05
    assert stats.kstest(r3[21, ::2, 0], stats.uniform(lo, hi - lo).cdf).pvalue > 1e-4  # ~ U(margin) + one small step
    # and the references drive the fused reward
    ps.set_reward(reward_weights=dict(i_sd=0.5, i_sq=0.5), referenced_states=gen.reference_names)
    acts = torch.rand((64, n, 3), device="cuda") * 2 - 1
    obs, dn, rew = env.rollout(acts, references=refs[:64])
    want = -(0.5 * (obs[..., ps.state_positions["i_sd"]] - refs[:64, :, 0]).abs() / 2 + 0.5 * (obs[..., ps.state_positions["i_sq"]] - refs[:64, :, 1]).abs() / 2)
    ok = dn == 0
    assert torch.allclose(rew[ok], want[ok], atol=2e-6)
    gen.apply_done(dn)
    for g_ in (gen, twin, g2, g3):
        g_.close()
    env.close()


def test_obs_layouts_agree_and_tail_block():
    import torch

    import gym_electric_motor_amd as ga

    for env_id in ("Cont-CC-PermExDc-v0", "Finite-CC-PMSM-v0", "Cont-SC-SCIM-v0", "Finite-CC-DFIM-v0", "Cont-CC-EESM-v0", "Finite-SC-ExtExDc-v0"):
        for n in (1, 3, 64, 65, 129):
            ea = ga.make(env_id, n_envs=n, obs_layout="aos")
            es = ga.make(env_id, n_envs=n, obs_layout="soa")
            ps = ea.physical_system
            g = torch.Generator(device="cuda").manual_seed(n)
            K = 20
            if ps._discrete:
                nflat = int(np.prod(ps.action_space.nvec)) if hasattr(ps.action_space, "nvec") else int(ps.action_space.n)
                acts = torch.randint(0, nflat, (K, n), device="cuda", generator=g, dtype=torch.uint8)
            else:
                acts = torch.rand((K, n, ps._n_act), device="cuda", generator=g) * 2 - 1
            oa, da = ea.rollout(acts)
            os_, ds = es.rollout(acts)
            assert torch.equal(oa, os_.transpose(1, 2)) and torch.equal(da, ds)
            # last_only returns the final row and the OR of the dones
            el = ga.make(env_id, n_envs=n)
            ol, dl = el.rollout(acts, last_only=True)
            assert torch.equal(ol, oa[-1])
            for e in (ea, es, el):
                e.close()


def test_single_env_numpy_contract_and_state_roundtrip():
    """n_envs == 1 behaves like the reference PhysicalSystem: numpy 1-D in/out, k counter, reset()."""
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make("Finite-CC-PMSM-v0", n_envs=1, constraints=())
    ps = env.physical_system
    s0 = ps.reset()
    assert isinstance(s0, np.ndarray) and s0.shape == (14,) and ps.k == 0
    s1 = ps.simulate(5)
    assert isinstance(s1, np.ndarray) and s1.shape == (14,) and s1.dtype == np.float64 and ps.k == 1
    with pytest.raises(AssertionError):
        ps.simulate(8)
    st = ps.get_state()
    assert st.shape == (4, 1)
    ps.simulate(3)
    s3a = ps.simulate(1)
    ps.set_state(st)
    ps.simulate(3)
    s3b = ps.simulate(1)
    assert np.array_equal(s3a, s3b)
    assert np.array_equal(ps.reset(), s0)
    env.close()
    dc = ga.make("Cont-CC-PermExDc-v0", n_envs=1).physical_system
    out = dc.simulate(np.array([0.3]))
    assert out.shape == (5,) and abs(out[3] - 0.3) < 1e-6  # u = action * u_sup / limit
    dc.close()


@pytest.mark.parametrize("name", ["extex_fin_free_held_til_euler", "eesm_fin_free_held_euler", "dfim_fin_free_uniform_til_euler",
                                  "dfim_cont_free_held_euler", "rc_pmsm_fin_free_held_euler", "pmsm_cont_dqproc_dead2_free_held_euler"])
def test_single_env_reference_contract_for_the_widened_systems(name):
    """n_envs == 1, numpy in / numpy out, exactly as the reference's PhysicalSystem is driven by ElectricMotorEnvironment.step
    (core.py:344): the golden trajectory reproduced step by step with the reference's own action objects (MultiDiscrete arrays,
    Box arrays), plus get_state / set_state / switching-state round trip and last_only rollouts."""
    import torch

    d, meta = _load(name)
    env = _make_from_meta(meta, 1, dtype="float64")
    ps = env.physical_system
    r = ps.reset()
    assert isinstance(r, np.ndarray) and np.abs(r - d["reset_state"]).max() < 1e-12
    K = 300
    for k in range(K):
        a = d["actions"][k]
        a = int(a) if np.ndim(a) == 0 else np.asarray(a)  # Discrete -> int, MultiDiscrete / Box -> array
        s = ps.simulate(a)
        assert isinstance(s, np.ndarray) and s.dtype == np.float64 and s.shape == (len(meta["state_names"]),)
        err = np.abs(s - d["states"][k])
        if "epsilon" in meta["state_names"]:
            i = meta["state_names"].index("epsilon")
            err[i] = min(err[i], 2.0 - err[i])
        assert err.max() < 1e-9, (k, err.max())
    assert ps.k == K
    env.close()
    # state round trip and last_only on a small batch (fp32)
    env = _make_from_meta(meta, 5, dtype="float32")
    ps = env.physical_system
    acts = torch.as_tensor(np.repeat(d["actions"][:40].reshape(40, 1, -1), 5, axis=1)).cuda()
    if ps._discrete and d["actions"].ndim == 1:
        acts = acts.reshape(40, 5)
    o1, _ = env.rollout(acts[:20])
    st, sw = ps.get_state(), ps.get_switch_state()
    o2, d2 = env.rollout(acts[20:])
    if meta["supply"] != "RCVoltageSupply" and not meta.get("dead_time_steps"):  # (supply state / action queue are not part of get_state)
        ps.set_state(st)
        ps.set_switch_state(sw)
        o3, _ = env.rollout(acts[20:])
        # (the fp32 path keeps the angle as a 32-bit turn fraction; get_state reports it in fp32 radians, i.e. rounded to ~1e-7 rad)
        assert torch.allclose(o2, o3, atol=2e-6, rtol=0)
        ps.set_state(st)
        ps.set_switch_state(sw)
        ol, dl = env.rollout(acts[20:], last_only=True)
        assert torch.equal(ol, o3[-1]) and torch.equal(dl.bool(), d2.bool().any(dim=0))
    env.close()


def test_episodic_auto_reset_matches_oracle_loop():
    """done -> restart from the reset state on the next step (`if terminated: env.reset()`), per env."""
    import torch

    import gym_electric_motor_amd as ga
    from oracle import oracle as orc

    n, K = 257, 400
    env = ga.make("Cont-CC-PermExDc-v0", n_envs=n, ode_solver=ga.EulerSolver())
    rng = np.random.default_rng(5)
    acts = rng.uniform(-1, 1, (K, n, 1)) * rng.uniform(0, 1, (1, n, 1))
    obs, done = env.rollout(torch.as_tensor(acts).cuda())
    torch.cuda.synchronize()
    obs, done = obs.double().cpu().numpy(), done.cpu().numpy().astype(bool)
    _, meta = _load("permexdc_epi_held_euler")
    p = orc.params_from_meta(meta, solver="euler", episodic=True)
    n_done = 0
    for j in (0, 5, 64, 200, 256):
        e = orc.OracleEnv(p)
        e.reset()
        ref, rdone = e.rollout(acts[:, j], auto_reset=True)
        margin = np.abs(np.abs(ref[:, 2]) - 1.0)
        if not np.array_equal(done[:, j], rdone):
            first = int(np.argmax(done[:, j] != rdone))
            assert margin[first] < 1e-5
            continue
        rel, _ = _rel_err(obs[:, j], ref, meta["state_names"])
        assert rel < 1e-4, rel
        n_done += int(rdone.sum())
    assert n_done > 10
    env.close()


def test_invalid_discrete_action_is_flagged():
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make("Finite-CC-PMSM-v0", n_envs=128)
    bad = torch.full((128,), 9, dtype=torch.uint8, device="cuda")
    env.physical_system.simulate(bad)
    with pytest.raises(AssertionError):
        env.physical_system.check_errors()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("where", [None, (0, 5), (17, 100), (29, 127)])
@pytest.mark.parametrize("shape", ["0", "1", "2"])
def test_invalid_discrete_action_in_a_rollout_is_flagged(where, shape, monkeypatch):
    """Pipelined kernels: the LOADER wave validates the staged action rows (first block, a middle block, the tail block)."""
    import torch

    import gym_electric_motor_amd as ga

    monkeypatch.setenv("GEMX_PIPE_SHAPE", shape)
    env = ga.make("Finite-CC-PMSM-v0", n_envs=128)
    g = torch.Generator(device="cuda").manual_seed(3)
    acts = torch.randint(0, 8, (30, 128), device="cuda", generator=g, dtype=torch.uint8)
    if where is not None:
        acts[where[0], where[1]] = 8 + 3 * where[0]
    env.rollout(acts)
    assert "advance_pipe_kernel" in env.physical_system.last_launch()
    if where is None:
        env.physical_system.check_errors()
    else:
        with pytest.raises(AssertionError):
            env.physical_system.check_errors()
    env.close()


def test_masked_reset():
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make("Cont-SC-SCIM-v0", n_envs=100, constraints=())
    ps = env.physical_system
    a = torch.rand((30, 100, 3), device="cuda") * 2 - 1
    env.rollout(a)
    mask = torch.zeros(100, dtype=torch.uint8, device="cuda")
    mask[::2] = 1
    last = ps.simulate(a[0]).clone()
    o = ps.reset(mask)
    st = ps.get_state().cpu().numpy()
    assert np.all(st[:, ::2] == 0.0) and np.any(st[:, 1::2] != 0.0)
    # returned observations: reset rows show the reset state, the others keep their last step's row
    ro = torch.as_tensor(ps.reset_observation, dtype=torch.float32, device="cuda")
    assert torch.equal(o[::2], ro.expand(50, -1)) and torch.equal(o[1::2], last[1::2])
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env_id, K", [("Finite-CC-PMSM-v0", 96), ("Cont-CC-PMSM-v0", 53), ("Finite-CC-EESM-v0", 48), ("Finite-CC-SCIM-v0", 40),
                                       # the map linmap_kernel builds from p and omega, at p = 5 / 3 and a negative speed
                                       ("Cont-CC-PMSM-v0:param_pmsm_cont_cc_negspeed_free_held_euler", 53),
                                       ("Finite-CC-PMSM-v0:param_pmsm_reversed_cont_cc_free_held_euler", 96),
                                       ("Finite-CC-SCIM-v0:param_scim_cont_cc_negspeed_free_held_euler", 40)])
def test_one_step_map_equals_stage_solver_and_is_dropped_when_omega_differs(env_id, K, monkeypatch):
    """ConstantSpeedLoad + RK4: the electrical subsystem is stepped by the precomputed affine map x1 = Phi x0 + S g (integrate<LIN>).
    (1) Same rollout with GEMX_LINMAP=0 (RK4 stage by stage): equal up to fp32 rounding of the same polynomial (<= 2e-5 of each
    column's scale).  (2) After set_state() moved omega away from init[0] in the first wave only, the
    map (built for init[0]) is not valid there: that wave must fall back by itself -- again equal to the stage solver."""
    import torch

    import gym_electric_motor_amd as ga

    env_id, _, golden = env_id.partition(":")
    mk = _param_overrides(golden, omega_fixed=True) if golden else {}

    def run(linmap, perturb):
        monkeypatch.setenv("GEMX_LINMAP", linmap)
        env = ga.make(env_id, n_envs=128, ode_solver=ga.RK4Solver(), constraints=(), **mk)
        ps = env.physical_system
        env.reset()
        g = torch.Generator(device="cuda").manual_seed(7)
        if ps._discrete:
            nflat = int(np.prod(ps.action_space.nvec)) if hasattr(ps.action_space, "nvec") else int(ps.action_space.n)
            acts = torch.randint(0, nflat, (K, 128), device="cuda", generator=g, dtype=torch.uint8)
        else:
            acts = torch.rand((K, 128, ps._n_act), device="cuda", generator=g) * 2 - 1
        if perturb:
            st = ps.get_state()
            st[0, :64] *= 0.5  # omega of the first wave
            ps.set_state(st)
        obs, _ = env.rollout(acts)
        first = obs.double().cpu().numpy()
        # chunked + single-step continuation stays bit-identical whichever solver the wave takes
        o2, _ = env.rollout(acts[:7])
        o3 = [ps.simulate(acts[7 + i]).clone() for i in range(3)]
        env.close()
        return first, o2.double().cpu().numpy(), torch.stack(o3).double().cpu().numpy()

    for perturb in (False, True):
        a, a2, a3 = run("1", perturb)
        b, b2, b3 = run("0", perturb)
        for x, y in ((a, b), (a2, b2), (a3, b3)):
            scale = np.maximum(np.abs(y).max(axis=(0, 1)), 1e-3)
            assert (np.abs(x - y) / scale).max() < 2e-5
        if perturb:  # the perturbation took: the first wave runs at half the (constant) speed of the untouched one
            assert abs(a[-1, 64, 0]) > 1e-3 and abs(a[-1, 0, 0] - 0.5 * a[-1, 64, 0]) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pmsm_epi_held_tau1e-4_euler", "scim_epi_uniform_euler", "permexdc_epi_held_euler", "eesm_fin_epi_held_tau1e-4_euler",
                                  "dfim_fin_epi_held_tau1e-4_euler", "extex_cont_epi_held_euler",
                                  "param_pmsm_fin_cc_lim_u350_epi_uniform_tau5e-5_euler", "param_pmsm_reversed_cont_cc_free_held_euler",
                                  "param_pmsm_nonsalient_fin_cc_free_held_euler", "param_synrm_fin_cc_free_held_euler", "param_scim_fin_cc_lim_epi_uniform_euler",
                                  "param_scim_cont_cc_negspeed_free_held_euler", "param_permexdc_fin_cc_lim_epi_uniform_euler", "param_shunt_cont_cc_epi_held_euler",
                                  "param_eesm_cont_cc_epi_held_euler", "param_dfim_cont_cc_free_held_euler", "param_dfim_fin_cc_free_held_euler"])
def test_all_pipelined_shapes_are_bit_identical(name, monkeypatch):
    """<12 steps, 3 output waves>, <4, 2> and <2, 2> (chosen by N in production, forced here with GEMX_PIPE_SHAPE) and the single-wave
    kernel give the same bits on the same inputs; K of the fixtures is not a multiple of any D, so every shape runs a tail block."""
    monkeypatch.setenv("GEMX_PIPE", "1")
    outs = []
    for shape in ("0", "1", "2", "3"):  # 3: <12 steps, 6 output waves>, the shape of launches with the fused reward
        monkeypatch.setenv("GEMX_PIPE_SHAPE", shape)
        _, _, obs, done = _run_golden(name, "float32", n_envs=128)
        outs.append((obs, done))
    monkeypatch.delenv("GEMX_PIPE_SHAPE")
    monkeypatch.setenv("GEMX_PIPE", "0")
    _, _, obs, done = _run_golden(name, "float32", n_envs=128)
    for o, d in outs:
        assert np.array_equal(o, obs) and np.array_equal(d, done)


@pytest.mark.gpu
def test_single_step_launches_replay_from_a_hip_graph_bit_identically():
    """simulate() enqueues one kernel on the current stream and never synchronises: a closed loop (policy -> step) captured with
    torch.cuda.CUDAGraph (hipGraph) and replayed continues the simulation exactly like the eager loop (examples/hip_graph_closed_loop.py)."""
    import torch

    import gym_electric_motor_amd as ga

    def make():
        env = ga.make("Cont-CC-PMSM-v0", n_envs=256, ode_solver=ga.RK4Solver())
        obs, _ = env.reset()
        return env, env.physical_system, obs

    gain = torch.tensor([[0.5, -0.25, 0.75]], device="cuda")
    cols = torch.tensor([5, 6, 2], device="cuda")

    def loop(ps, obs, action, steps, trace):
        for _ in range(steps):
            torch.mul(torch.tanh(obs.index_select(1, cols) * 3.0 + 0.1), gain, out=action)
            obs = ps.simulate(action)
            if trace is not None:
                trace.append(obs.clone())
        return obs

    env1, ps1, obs1 = make()
    a1 = torch.zeros((256, 3), device="cuda")
    eager = []
    loop(ps1, obs1, a1, 4 + 3 * 8, eager)
    env2, ps2, obs2 = make()
    a2 = torch.zeros((256, 3), device="cuda")
    loop(ps2, obs2, a2, 4, None)  # warm-up outside the capture (lazy one-time work of the handle)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loop(ps2, obs2, a2, 8, None)
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(obs2, eager[4 + 8 * (r + 1) - 1])
    env1.close()
    env2.close()


@pytest.mark.parametrize("env_id", ["Cont-CC-PermExDc-v0", "Finite-CC-PermExDc-v0", "Cont-CC-SeriesDc-v0", "Finite-SC-SeriesDc-v0", "Cont-CC-ShuntDc-v0",
                                    "Finite-CC-ShuntDc-v0", "Cont-CC-ExtExDc-v0", "Finite-CC-ExtExDc-v0",
                                    # the non-default DC machines of oracle/make_golden.py:main_params (motor parameters; PermExDc: custom limits)
                                    "Cont-CC-PermExDc-v0:param_permexdc_cont_cc_free_held_euler", "Finite-CC-PermExDc-v0:param_permexdc_fin_cc_lim_epi_uniform_euler",
                                    "Cont-CC-SeriesDc-v0:param_series_cont_cc_free_held_euler", "Finite-CC-ShuntDc-v0:param_shunt_cont_cc_epi_held_euler",
                                    "Cont-CC-ExtExDc-v0:param_extex_fin_cc_til_free_held_euler"])
@pytest.mark.parametrize("solver", ["euler", "rk4", "rk4_nolinmap", "dp5", "euler_epw64", "rk4_epw64"])
def test_dc_stream_kernel_is_bit_identical_to_the_pipelined_kernel(env_id, solver, monkeypatch):
    """Small batches of the DC machines behind a ConstantSpeedLoad take dc_stream_kernel (pre waves: converter + input term; integrator:
    the recurrence alone; output waves: observation row + done flag, stored from registers).  It calls the device functions the other
    kernels call on the same values: observations, done masks and the final state are bit-identical to advance_pipe_kernel's -- over
    launches with whole blocks, a tail block, fewer steps than a block, continuation across launches, and auto-resets (random actions
    drive the currents over their limits).  After gemx_set_state (omega may differ from its initial value) the general kernels serve
    the handle until the next full reset."""
    import torch

    import gym_electric_motor_amd as ga

    n = 192
    env_id, _, golden = env_id.partition(":")
    motor = _param_overrides(golden)["motor"] if golden else None
    # (`_epw64`: the form with one env per lane, which the launcher takes from 4097 to 8192 envs; default here: 32 envs per workgroup)
    if solver.endswith("_epw64"):
        monkeypatch.setenv("GEMX_DCS_EPW", "64")
        solver = solver[:-6]
    else:
        monkeypatch.delenv("GEMX_DCS_EPW", raising=False)
    sol = dict(euler=ga.EulerSolver, rk4=ga.RK4Solver, rk4_nolinmap=ga.RK4Solver, dp5=ga.DormandPrince5Solver)[solver]

    def run(stream):
        monkeypatch.setenv("GEMX_DC_STREAM", stream)
        if solver == "rk4_nolinmap":
            monkeypatch.setenv("GEMX_LINMAP", "0")
        else:
            monkeypatch.delenv("GEMX_LINMAP", raising=False)
        env = ga.make(env_id, n_envs=n, ode_solver=sol(), tau=1e-4, load=ga.ConstantSpeedLoad(omega_fixed=60.0), motor=json.loads(json.dumps(motor)))
        ps = env.physical_system
        env.reset()
        g = torch.Generator(device="cuda").manual_seed(23)
        outs, kernels = [], []
        for K in (120, 57, 24, 25, 7, 2):
            if ps._discrete:
                nflat = int(np.prod(ps.action_space.nvec)) if hasattr(ps.action_space, "nvec") else int(ps.action_space.n)
                acts = torch.randint(0, nflat, (K, n), device="cuda", generator=g, dtype=torch.uint8)
            else:
                acts = torch.rand((K, n, ps._n_act), device="cuda", generator=g, dtype=torch.float32) * 3 - 1.5  # (beyond the duty-cycle clip too)
            obs, done = env.rollout(acts)
            outs += [obs.cpu().numpy().copy(), done.cpu().numpy().copy()]
            kernels.append(ps.last_launch())
        outs.append(ps.get_state().cpu().numpy().copy())
        # omega moved away from its initial value: the general kernels until the next full reset
        y = ps.get_state().clone()
        y[0] += 1.0
        ps.set_state(y)
        acts = torch.zeros((30, n), device="cuda", dtype=torch.uint8) if ps._discrete else torch.zeros((30, n, ps._n_act), device="cuda")
        obs, done = env.rollout(acts)
        outs += [obs.cpu().numpy().copy(), done.cpu().numpy().copy()]
        kernels.append(ps.last_launch())
        env.reset()
        obs, done = env.rollout(acts)
        outs += [obs.cpu().numpy().copy(), done.cpu().numpy().copy()]
        kernels.append(ps.last_launch())
        env.close()
        return outs, kernels

    a, ka = run("1")
    b, kb = run("0")
    assert all("dc_stream_kernel" in k for k in ka[:6]) and "dc_stream_kernel" not in ka[6] and "dc_stream_kernel" in ka[7], ka
    assert all(("grid=3 x" in k) == (os.environ.get("GEMX_DCS_EPW") == "64") for k in ka[:6]), ka  # 192 envs: 3 workgroups of 64 or 6 of 32
    assert not any("dc_stream_kernel" in k for k in kb), kb
    if "PermExDc" in env_id:
        assert a[1].any(), "the rollout should contain terminations"
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (i, np.abs(x.astype(np.float64) - y.astype(np.float64)).max())


def test_dc_stream_kernel_flags_an_invalid_discrete_action():
    """the pre waves validate discrete action indices as the loader wave of the pipelined kernel does (converters.py:204-206)"""
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make("Finite-CC-PermExDc-v0", n_envs=128, ode_solver=ga.EulerSolver(), tau=1e-4)
    ps = env.physical_system
    env.reset()
    acts = torch.randint(0, 4, (50, 128), device="cuda", dtype=torch.uint8)
    env.rollout(acts)
    assert "dc_stream_kernel" in ps.last_launch()
    ps.check_errors()
    acts[37, 99] = 4
    env.rollout(acts)
    with pytest.raises(Exception):
        ps.check_errors()
    env.close()


DC_STREAM_GOLDEN = ["permexdc_epi_held_euler", "permexdc_epi_uniform_euler", "permexdc_free_uniform_10k_euler", "permexdc_free_held_euler",
                    "permexdc_fin_epi_held_euler", "permexdc_fin_free_held_euler", "extex_cont_epi_held_euler", "extex_cont_free_uniform_euler",
                    "extex_fin_epi_held_euler", "extex_fin_free_uniform_euler"]


@pytest.mark.parametrize("name", [c for c in DC_STREAM_GOLDEN if c in CASES])
def test_dc_stream_kernel_matches_reference_trajectories(name):
    """The reference's own recorded runs of the DC machines behind a ConstantSpeedLoad (same integrator: Euler), at a batch size that
    takes dc_stream_kernel: fp32 within 1e-4 of the reference, episode by episode, exact done masks (margin-guarded)."""
    import torch

    d, meta = _load(name)
    n_envs = 128
    env = _make_from_meta(meta, n_envs, dtype="float32", auto_reset=True)
    ps = env.physical_system
    acts = d["actions"]
    K = acts.shape[0]
    a = torch.as_tensor(np.repeat(acts.reshape(K, 1, -1), n_envs, axis=1))
    if ps._discrete and acts.ndim == 1:
        a = a.reshape(K, n_envs)
    obs, done = env.rollout(a.cuda())
    torch.cuda.synchronize()
    assert "dc_stream_kernel" in ps.last_launch(), ps.last_launch()
    obs = obs.double().cpu().numpy()
    done = done.cpu().numpy().astype(bool)
    env.close()
    assert np.array_equal(obs[:, 0], obs[:, n_envs - 1]) and np.array_equal(done[:, 0], done[:, 77])
    rel, ab, col, dmsg = compare_trajectory(meta, d, obs[:, 0], done[:, 0], min_fraction=0.5)
    assert rel < 1e-4, (rel, ab, col, dmsg)


# ------------------------------------------------------------------------------------------------ round 3: replayed graphs, device-side premises
def _capture(torch, fn):
    """fn() captured into a HIP graph on a side stream (after one eager warm-up call outside the capture)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    return g


@pytest.mark.timeout(120)
def test_a_replayed_graph_never_runs_dc_stream_kernel_on_a_moved_omega():
    """dc_stream_kernel is chosen on the HOST from what it knows about omega at enqueue time, so a captured launch must not be that kernel:
    a graph captured while every env sat at its initial speed, replayed after gemx_set_state moved omega, has to integrate the moved
    machine (the pipelined kernel decides on the device).  Replay == eager, bit for bit, before and after the state change."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 256, 96
    mk = lambda: ga.make("Cont-CC-PermExDc-v0", n_envs=n, ode_solver=ga.EulerSolver(), tau=1e-4)  # noqa: E731
    g0 = torch.Generator(device="cuda").manual_seed(5)
    acts = torch.rand((K, n, 1), device="cuda", generator=g0) * 2 - 1
    env_g, env_e = mk(), mk()
    pg, pe = env_g.physical_system, env_e.physical_system
    env_g.rollout(acts)  # warm-up (eager: the small-batch kernel)
    assert "dc_stream_kernel" in pg.last_launch()
    env_g.reset()
    obs_g = torch.empty((K, n, 5), device="cuda")
    done_g = torch.empty((K, n), dtype=torch.uint8, device="cuda")
    graph = _capture(torch, lambda: env_g.rollout(acts, obs_out=obs_g, done_out=done_g))
    assert "dc_stream_kernel" not in pg.last_launch(), pg.last_launch()
    env_g.reset()
    env_e.reset()
    graph.replay()
    o_e, d_e = env_e.rollout(acts)
    torch.cuda.synchronize()
    assert torch.equal(obs_g, o_e) and torch.equal(done_g, d_e)
    y = pe.get_state().clone()
    y[0] += 17.0
    pe.set_state(y)
    pg.set_state(y)
    graph.replay()
    o_e, d_e = env_e.rollout(acts)
    torch.cuda.synchronize()
    assert "dc_stream_kernel" not in pe.last_launch()
    assert torch.equal(obs_g, o_e) and torch.equal(done_g, d_e)
    assert abs(float(obs_g[0, 0, 0]) * 400.0 - (100.0 + 17.0)) < 1e-3  # the moved speed is what was integrated (until an env's next reset)
    pg.check_errors()
    env_g.close()
    env_e.close()


@pytest.mark.timeout(120)
def test_dc_stream_kernel_checks_its_premise_on_the_device(monkeypatch):
    """GEMX_DC_STREAM=3 takes dc_stream_kernel WITHOUT the host's knowledge that omega is at its initial value: the integrator wave's own
    check of the omega row must raise the sticky GEMX_ERRFLAG_OMEGA_MOVED bit (check_errors() raises), and stay silent when omega is fine."""
    import torch

    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd._lib import GemxError

    monkeypatch.setenv("GEMX_DC_STREAM", "3")
    env = ga.make("Cont-CC-PermExDc-v0", n_envs=192, ode_solver=ga.EulerSolver(), tau=1e-4)
    ps = env.physical_system
    acts = torch.zeros((40, 192, 1), device="cuda")
    env.rollout(acts)
    assert "dc_stream_kernel" in ps.last_launch()
    ps.check_errors()
    y = ps.get_state().clone()
    y[0, 100] += 1.0  # ONE env of the second workgroup
    ps.set_state(y)
    env.rollout(acts)
    assert "dc_stream_kernel" in ps.last_launch()
    with pytest.raises(GemxError):
        ps.check_errors()
    env.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("env_id, delay, K", [("Finite-CC-PMSM-v0", 3, 7), ("Cont-CC-PMSM-v0", 2, 5), ("Cont-CC-PermExDc-v0", 3, 1)])
def test_dead_time_queue_phase_survives_graph_replay(env_id, delay, K):
    """The DeadTimeProcessor FIFO's slot of a launch's first step (control steps so far mod delay) lives in DEVICE memory and is advanced
    by the kernels themselves, so a K-step launch replayed from a graph (K not a multiple of the delay) continues the queue where the
    previous replay left it: replay r == the r-th eager launch, bit for bit (a phase computed on the host would be frozen at capture)."""
    import torch

    import gym_electric_motor_amd as ga

    n, R = 192, 5
    mk = lambda: ga.make(env_id, n_envs=n, ode_solver=ga.RK4Solver(), tau=1e-4, physical_system_wrappers=(ga.DeadTimeProcessor(steps=delay),))  # noqa: E731
    env_g, env_e = mk(), mk()
    pg, pe = env_g.physical_system, env_e.physical_system
    g0 = torch.Generator(device="cuda").manual_seed(11)
    if pg._discrete:
        acts = torch.randint(0, 8, (K, n), device="cuda", generator=g0, dtype=torch.uint8)
    else:
        acts = torch.rand((K, n, pg._n_act), device="cuda", generator=g0) * 2 - 1
    nout = pg._n_out
    if K == 1:
        run_g = lambda: pg.simulate(acts[0])  # noqa: E731
        run_e = lambda: pe.simulate(acts[0]).clone()  # noqa: E731
        out_g = pg._obs
    else:
        out_g = torch.empty((K, n, nout), device="cuda")
        dn_g = torch.empty((K, n), dtype=torch.uint8, device="cuda")
        run_g = lambda: env_g.rollout(acts, obs_out=out_g, done_out=dn_g)  # noqa: E731
        run_e = lambda: env_e.rollout(acts)[0]  # noqa: E731
    run_g()  # warm-up outside the capture, then both sides from the reset state
    env_g.reset()
    env_e.reset()
    torch.cuda.synchronize()
    graph = _capture(torch, run_g)
    env_g.reset()
    for r in range(R):
        graph.replay()
        ref = run_e()
        torch.cuda.synchronize()
        assert torch.equal(out_g.reshape(ref.shape), ref), (r, float((out_g.reshape(ref.shape) - ref).abs().max()))
    env_g.close()
    env_e.close()


_RCCL_WORLD1 = r'''
import os, sys
sys.path.insert(0, %r)
import torch
import torch.distributed as dist
import gym_electric_motor_amd as ga
from gym_electric_motor_amd import distributed as gd

rank, world, local = gd.init_from_env(backend="nccl", timeout_s=120, force=True)
assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
n, K = 4096, 50
env = gd.make_sharded("Finite-CC-PMSM-v0", n, rank, world, device=local, ode_solver=ga.RK4Solver(), tau=1e-4)
assert env.shard == (0, n)
g = torch.Generator(device="cuda").manual_seed(3)
acts = torch.randint(0, 8, (K, n), device="cuda", generator=g, dtype=torch.uint8)
obs, done = env.rollout(acts)
# the batched-return path, forced down the collective branch although the world is one rank: RCCL moves the real rollout outputs
go, gdn = gd.gather_rollout(obs, done, force=True)
assert go.shape == (1, K, n, 14) and gdn.shape == (1, K, n) and go.data_ptr() != obs.data_ptr()
assert torch.equal(go[0], obs) and torch.equal(gdn[0], done)
o1 = env.physical_system.simulate(acts[0])
a1, d1 = gd.gather_observations(o1, env.physical_system.done, force=True)
assert a1.shape == (n, 14) and a1.data_ptr() != o1.data_ptr() and torch.equal(a1, o1) and torch.equal(d1, env.physical_system.done)
a2, _ = gd.gather_observations(o1, None, n_total=n, force=True)
assert torch.equal(a2, o1)
dist.barrier()
torch.cuda.synchronize()
env.close()
dist.destroy_process_group()
print("RCCL_WORLD1_OK", int(done.sum()))
'''


@pytest.mark.timeout(300)
def test_rccl_gather_of_real_rollout_outputs_in_a_world_of_one():
    """The multi-GPU path as far as ONE GPU allows: torch.distributed initialised with backend "nccl" (= RCCL) and a
    world of one rank, this rank's shard stepped by the kernels, and `gather_rollout` / `gather_observations` FORCED down their
    collective branch on the real rollout outputs -- RCCL's all-gather returns the shard bit for bit in a fresh tensor.  (Own
    process: the process group must not outlive the test.)"""
    import subprocess
    import sys

    from gym_electric_motor_amd.distributed import free_port

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([sys.executable, "-c", _RCCL_WORLD1 % repo], env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "RCCL_WORLD1_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.timeout(600)
def test_bench_multi_gpu_code_path_through_rccl_in_a_world_of_one():
    """The exact code path of the driver's scaling run (`torchrun ... bench.py --gpus N`: process group on `nccl`, barriers, the
    max-over-ranks all-reduce, the bounded `chunk` gather leg with its `rccl` record, `config5`) executed on ONE GPU: WORLD_SIZE=1 in the
    environment makes bench.py initialise torch.distributed exactly as for N > 1.  The line must carry value, roofline (one clock:
    value x bytes per env-step == roofline.achieved), rccl.world_seen / bytes_per_rank / GB_per_s, and the gathered chunk's own slot
    must be this rank's outputs bit for bit."""
    import json
    import subprocess
    import sys

    from gym_electric_motor_amd.distributed import free_port

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import tempfile

    side = os.path.join(tempfile.mkdtemp(prefix="gemx_bench_"), "extras.json")
    cmd = [sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--gather", "chunk", "--config5", "on",
           "--no-extras", "--no-pmc", "--settle-ms", "5", "--repeats", "1", "--steps-per-launch", "200", "--extras-file", side]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    last = r.stdout.rstrip("\n").splitlines()[-1]
    assert last.startswith("{") and len(last) < 6000, len(last)  # ONE compact line, last on stdout (round 5's 20 KB were not parsed)
    line = json.loads(last)
    full = json.load(open(side))  # the full record went to the side file
    assert full["value"] == line["value"] and "repeats" in full and "telemetry" in full and "repeats" not in line
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["config"]["backend"] == "nccl"
    rf = line["roofline"]
    # one clock: value (env-steps/s) x algorithmic bytes per env-step of a launch == roofline.achieved
    per_env_step = rf["algorithmic_bytes_per_launch"] / (16384 * 200)
    assert abs(line["value"] * per_env_step / 1e9 / rf["achieved"] - 1) < 1e-9
    rc = line["rccl"]
    assert "error" not in rc, rc
    assert rc["world_seen"] == 1 and rc["backend"] == "nccl" and rc["own_slot_bit_identical"] is True
    assert rc["bytes_per_rank"] == 16384 * 200 * 57 and rc["GB_per_s"] > 0 and rc["ms"] > 0
    assert line["gather"]["chunk"]["value"] > 0 and "error" not in line["config5"] and line["config5"]["envs_per_gpu"] == 32768
    assert line["overrides"] == {k: v for k, v in os.environ.items() if k.startswith("GEMX_") and k != "GEMX_COVERAGE_FILE"}


@pytest.mark.timeout(300)
def test_bench_plain_run_dumps_the_same_outputs_every_time():
    """A plain `bench.py` run (no --full) times its K launches once, prints the line with the contract's keys, writes no side file, and
    `--dump-outputs DIR` writes the last timed launch's outputs as float32 .npy files (< 64 MB) -- bit for bit the same in two runs with
    the same arguments (seeded actions, envs reset after the clock-bound settle launches), and equal to the launch's own rows."""
    import json
    import subprocess
    import sys
    import tempfile

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    tmp = tempfile.mkdtemp(prefix="gemx_dump_")
    dumps = []
    for i in range(2):
        d = os.path.join(tmp, str(i))
        cmd = [sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--steps-per-launch", "200",
               "--dump-outputs", d]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=140, cwd=tmp)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        line = json.loads(r.stdout.rstrip("\n").splitlines()[-1])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
        assert "extras_file" not in line and "legs" not in line and "cpu_baseline" not in line
        files = sorted(os.listdir(d))
        assert files == ["done_last.npy", "done_sample.npy", "obs_last.npy", "obs_sample.npy"], files
        arrs = {f: np.load(os.path.join(d, f)) for f in files}
        assert all(a.dtype == np.float32 for a in arrs.values()) and sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert arrs["obs_last.npy"].shape == (16384, 14) and arrs["obs_sample.npy"].shape == (200, 512, 14)
        assert np.isfinite(arrs["obs_sample.npy"]).all() and set(np.unique(arrs["done_last.npy"])) <= {0.0, 1.0}
        dumps.append(arrs)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


def test_rate_limiter_closed_loop_calibrates_and_never_changes_results(monkeypatch):
    """The large-batch rate limiter is closed loop since round 5: a handle's first paced launches take turns at the built-in target x
    {1, 0.93, 1.07, 0.86} and unpaced, each timed with HIP events on the launch stream, and the fastest is kept (gemx_last_launch() says
    `calibrating` / `calibrated` and at what factor).  The limiter only delays block starts, so every launch -- calibrating, calibrated,
    GEMX_PACE_CAL=0, GEMX_PACE_GBPS=0 -- produces the same bits; the calibration belongs to (workgroups, shape, reward / action source, and
    the CLASS of the launch length: < 256 steps | longer | the long launches at one workgroup per CU), so that a loop that varies K keeps it."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 32768, 128
    acts = torch.randint(0, 8, (K, n), device="cuda", dtype=torch.uint8, generator=torch.Generator(device="cuda").manual_seed(3))

    def run(env_kw, launches):
        for k, v in env_kw.items():
            monkeypatch.setenv(k, v)
        env = ga.make("Finite-CC-PMSM-v0", n_envs=n, tau=1e-4)
        ps = env.physical_system
        outs, descs = [], []
        o = torch.empty((K, n, ps._n_out), device="cuda")
        d = torch.empty((K, n), dtype=torch.uint8, device="cuda")
        for i in range(launches):
            env.reset()
            env.rollout(acts, obs_out=o, done_out=d)
            if i % 8 == 7:
                torch.cuda.synchronize()  # (completed launches are harvested at later launches)
            if i == 0:
                outs.append((o.clone(), d.clone()))
            else:  # (every launch -- whatever candidate it ran -- against the first: compared on the spot, 235 MB a piece)
                assert torch.equal(o, outs[0][0]) and torch.equal(d, outs[0][1]), i
            descs.append(ps.last_launch())
        torch.cuda.synchronize()
        env.rollout(acts[: K // 2])  # another length of the same class (< 256 steps): the calibration is kept (round 6)
        d_same = ps.last_launch()
        env.rollout(torch.cat([acts, acts, acts]))  # 384 steps: the other class -- a new calibration
        d2 = (d_same, ps.last_launch())
        env.close()
        for k in env_kw:
            monkeypatch.delenv(k)
        return outs, descs, d2

    outs, descs, d2 = run({}, 240)  # (30 launches per bracket, up to five brackets when the winner keeps sitting at an edge)
    assert "limiter calibrating" in descs[0] and "1.00 x" in descs[0]
    assert any("limiter calibrated" in d for d in descs), descs[-1]
    assert "limiter calibrated" in descs[-1]
    assert "limiter calibrated" in d2[0]  # K changed within its class (short launches): no new calibration -- a training loop may vary K
    assert "limiter calibrating" in d2[1]  # ... across the classes (K >= 256): fixed costs no longer weigh on the timings, a new one
    ref, rdesc, _ = run({"GEMX_PACE_CAL": "0"}, 2)
    assert "limiter" not in rdesc[0] and "rate limit" in rdesc[0]
    assert torch.equal(ref[0][0], outs[0][0]) and torch.equal(ref[0][1], outs[0][1])
    off, odesc, _ = run({"GEMX_PACE_GBPS": "0"}, 1)
    assert "rate limit" not in odesc[0] and torch.equal(off[0][0], outs[0][0])


@pytest.mark.timeout(900)
def test_two_ranks_on_two_gpus_through_rccl():
    """The first box with >= 2 GPUs runs the collective under pytest too (round 4 verdict: no RCCL collective had ever run between two
    ranks): `bench.py --gpus 2` spawns its own two ranks (one per GPU, `nccl` = RCCL over xGMI on 127.0.0.1), each steps its shard,
    and the bounded chunk-gather leg all-gathers one launch's observation rows.  Asserted: both ranks were seen by the collective,
    every rank's own slot of the gathered tensor is its own output bit for bit, the line carries the whole-job value (2 x the shard),
    and config 5's leg.  Skipped on a box with one GPU (the driver's GPU test tier)."""
    import json
    import subprocess
    import sys

    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible: the two-rank RCCL path needs two (world-of-one code path: the test above; gloo world of 2: tests/test_distributed_cpu.py)")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full", "--no-extras", "--no-pmc",
           "--settle-ms", "5", "--repeats", "1", "--steps-per-launch", "200"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=840)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["config"]["backend"] == "nccl" and line["scaling"] == "weak"
    assert line["config"]["envs_per_gpu"] == 16384 and not line["config"]["oversubscribed"]
    rc = line["rccl"]
    assert "error" not in rc, rc
    assert rc["world_seen"] == 2 and rc["backend"] == "nccl" and rc["own_slot_bit_identical"] is True
    assert rc["bytes_per_rank"] == 16384 * 200 * 57 and rc["GB_per_s"] > 0
    assert line["gather"]["chunk"]["value"] > 0
    assert "error" not in line["config5"] and line["config5"]["envs_total"] == 65536


def test_last_launch_names_every_active_override(monkeypatch):
    """A dozen GEMX_* environment switches change which kernel a PRODUCT call runs (A/B work); whatever was set when the handle was
    created is part of gemx_last_launch() -- and of bench.py's `overrides` field -- so a stray variable cannot silently change a
    benchmark; a clean environment adds nothing."""
    import torch

    import gym_electric_motor_amd as ga

    for k in [k for k in os.environ if k.startswith("GEMX_")]:
        monkeypatch.delenv(k)
    acts = torch.zeros((8, 128), dtype=torch.uint8, device="cuda")
    e = ga.make("Finite-CC-PMSM-v0", n_envs=128)
    e.rollout(acts)
    clean = e.physical_system.last_launch()
    e.close()
    assert "overrides" not in clean and "advance_pipe_kernel" in clean
    monkeypatch.setenv("GEMX_PIPE_SHAPE", "1")
    monkeypatch.setenv("GEMX_LINMAP", "0")
    e = ga.make("Finite-CC-PMSM-v0", n_envs=128)
    e.rollout(acts)
    forced = e.physical_system.last_launch()
    e.close()
    assert forced.endswith("overrides[GEMX_PIPE_SHAPE=1 GEMX_LINMAP=0]") and "D=4" in forced


@pytest.mark.parametrize("env_id,n_envs,K", [("Finite-CC-PMSM-v0", 51968, 96), ("Cont-CC-PMSM-v0", 32768, 96), ("Finite-CC-ShuntDc-v0", 33216, 96),
                                             ("Cont-SC-SCIM-v0", 65536, 96), ("Finite-CC-PMSM-v0", 16384, 1600), ("Cont-CC-PMSM-v0", 8192, 1536)])
def test_rate_limiter_changes_launch_time_only(monkeypatch, env_id, n_envs, K):
    """The large-batch rate limiter (advance_pipe_kernel: the integrator waits for its block's slot on the 100 MHz clock) holds
    workgroups back and does nothing else: limiter off (GEMX_PACE_GBPS=0), the built-in default and a target far too low give the same
    bits -- full rounds and a ragged last round (the pipelined kernel takes whole 64-env workgroups only) -- and gemx_last_launch() names the interval
    of a launch that was paced.  The last two cases: LONG launches at one workgroup per CU, which the launcher moves from <12, 6> to the paced
    <12, 3> on its own (`long_one`)."""
    import torch

    import gym_electric_motor_amd as ga

    for k in [k for k in os.environ if k.startswith("GEMX_")]:
        monkeypatch.delenv(k)
    g = torch.Generator(device="cuda").manual_seed(11)
    outs = {}
    for tag, val in (("off", "0"), ("default", None), ("slow", "900" if K < 1000 else "5000")):
        if val is None:
            monkeypatch.delenv("GEMX_PACE_GBPS", raising=False)
        else:
            monkeypatch.setenv("GEMX_PACE_GBPS", val)
        e = ga.make(env_id, n_envs=n_envs)
        ps = e.physical_system
        if tag == "off":
            acts = (torch.randint(0, int(ps.action_space.n), (K, n_envs), device="cuda", generator=g, dtype=torch.uint8) if ps._discrete
                    else torch.rand((K, n_envs, ps._n_act), device="cuda", generator=g) * 2 - 1)
        e.reset()
        obs, done = ps.rollout(acts)
        outs[tag] = (obs.clone(), done.clone(), ps.last_launch())
        e.close()
    assert "rate limit" not in outs["off"][2] and "GEMX_PACE_GBPS=0" in outs["off"][2]
    assert "rate limit" in outs["default"][2] and "overrides" not in outs["default"][2], outs["default"][2]
    if K < 1000:
        assert "rate limit" in outs["slow"][2]
    else:  # the long launches: five output waves' worth of threads = <12, 3>, against <12, 6> with the limiter off (finite-set converter)
        assert "D=12" in outs["default"][2] and "x 320 threads" in outs["default"][2], outs["default"][2]
    for tag in ("default", "slow"):
        assert torch.equal(outs[tag][0], outs["off"][0]) and torch.equal(outs[tag][1], outs["off"][1]), (tag, outs[tag][2])


def test_bind_step_is_simulate_without_the_argument_handling():
    """PhysicalSystem.bind_step(action_buffer): the closed loop's pre-bound FFI call.  Same launches as simulate() -- bit-identical
    observations and done flags, step counter advanced, the internal observation tensor returned -- and it refuses a buffer the kernel
    could not read as it is."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 192, 40
    g = torch.Generator(device="cuda").manual_seed(2)
    acts = torch.randint(0, 8, (K, n), device="cuda", generator=g, dtype=torch.uint8)
    e1 = ga.make("Finite-CC-PMSM-v0", n_envs=n, ode_solver=ga.RK4Solver(), tau=1e-4)
    e2 = ga.make("Finite-CC-PMSM-v0", n_envs=n, ode_solver=ga.RK4Solver(), tau=1e-4)
    e1.reset()
    e2.reset()
    p1, p2 = e1.physical_system, e2.physical_system
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    step, obs, done = p2.bind_step(buf)
    for k in range(K):
        o1 = p1.simulate(acts[k])
        buf.copy_(acts[k])
        o2 = step()
        assert o2 is obs and torch.equal(o1, o2) and torch.equal(p1._done, done), k
    assert p2.k == p1.k == K
    with pytest.raises(ValueError):
        p2.bind_step(torch.zeros(n, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        p2.bind_step(torch.zeros(2 * n, dtype=torch.uint8, device="cuda")[::2])
    e1.close()
    e2.close()
    with pytest.raises(ValueError):  # a stepper outliving its system: the C ABI's "null handle", not a stale pointer
        step()


@pytest.mark.parametrize("env_id", ["Finite-CC-PMSM-v0", "Cont-CC-PermExDc-v0"])
def test_bind_rollout_is_rollout_without_the_argument_handling(env_id):
    """PhysicalSystem.bind_rollout(actions, obs_out, done_out): the pre-bound fused launch (what bench.py's loops call).  Same launches as
    rollout() -- bit-identical observations and done flags over consecutive chunks, the step counter advanced, the caller's buffers
    returned -- it follows what the caller writes into the bound action tensor, and it refuses tensors the kernel could not use as they are."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 4096, 200
    e1, e2 = ga.make(env_id, n_envs=n), ga.make(env_id, n_envs=n)
    e1.reset()
    e2.reset()
    p1, p2 = e1.physical_system, e2.physical_system
    g = torch.Generator(device="cuda").manual_seed(3)
    mk = (lambda: torch.randint(0, int(p1.action_space.n), (K, n), device="cuda", generator=g, dtype=torch.uint8)) if p1._discrete else \
         (lambda: torch.rand((K, n, p1._n_act), device="cuda", generator=g) * 2 - 1)
    chunks = [mk() for _ in range(3)]
    buf = torch.empty_like(chunks[0])
    obs, done = torch.empty((K, n, p2._n_out), device="cuda"), torch.empty((K, n), dtype=torch.uint8, device="cuda")
    launch = e2.bind_rollout(buf, obs, done)
    for c in chunks:
        o1, d1 = p1.rollout(c)
        buf.copy_(c)
        o2, d2 = launch()
        assert o2 is obs and d2 is done and torch.equal(o1, o2) and torch.equal(d1, d2)
    assert p1.k == p2.k == 3 * K and p1.last_launch() == p2.last_launch()
    with pytest.raises(ValueError):
        p2.bind_rollout(buf.to(torch.float64) if not p1._discrete else buf.to(torch.float32), obs, done)
    with pytest.raises(ValueError):
        p2.bind_rollout(buf, obs[:-1], done)
    with pytest.raises(ValueError):
        p2.bind_rollout(buf, obs, done.to(torch.int32))
    with pytest.raises(ValueError):
        p2.bind_rollout(buf.cpu(), obs, done)
    e1.close()
    e2.close()
    with pytest.raises(ValueError):  # a launcher outliving its system: the C ABI's "null handle", not a stale pointer
        launch()


_DCS_WATCHDOG = r'''
import sys
sys.path.insert(0, %r)
import torch
import gym_electric_motor_amd as ga
launches = 0
for env_id in ("Cont-CC-PermExDc-v0", "Finite-CC-PermExDc-v0", "Cont-CC-SeriesDc-v0", "Finite-CC-ShuntDc-v0", "Cont-CC-ExtExDc-v0"):
    for n in (64, 4096):
        kw = {} if "PermExDc" in env_id else {"load": ga.ConstantSpeedLoad(omega_fixed=30.0)}
        env = ga.make(env_id, n_envs=n, ode_solver=ga.EulerSolver(), tau=1e-4, **kw)
        ps = env.physical_system
        g = torch.Generator(device="cuda").manual_seed(n)
        for K in (2, 3, 31, 32, 33, 64, 65, 96, 127, 1000, 1023):
            env.reset()
            if ps._discrete:
                a = torch.randint(0, int(ps.action_space.n) if hasattr(ps.action_space, "n") else 4, (K, n), device="cuda", generator=g, dtype=torch.uint8)
            else:
                a = torch.rand((K, n, ps._n_act), device="cuda", generator=g) * 2 - 1
            for _ in range(3):  # back to back: a workgroup of the next launch starts while one of the last still drains
                obs, done = ps.rollout(a)
            torch.cuda.synchronize()
            assert "dc_stream_kernel" in ps.last_launch(), ps.last_launch()
            assert bool(torch.isfinite(obs).all())
            launches += 3
        env.close()
print("DCS_WATCHDOG_OK", launches)
'''


@pytest.mark.timeout(200)
def test_dc_stream_kernel_finishes_under_a_watchdog():
    """dc_stream_kernel synchronises sixteen (eight) waves with different jobs through one s_barrier per block, and three (one) of
    them only exist to keep a SIMD free: every wave has to reach every barrier exactly as often as the others, for every block count
    -- whole blocks, tail blocks, fewer steps than one block -- or the workgroup hangs.  All of those shapes, every DC machine, in a
    child process that a watchdog kills: a hang fails this test after 150 s instead of stalling the suite (and the box)."""
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        r = subprocess.run([sys.executable, "-c", _DCS_WATCHDOG % repo], capture_output=True, text=True, timeout=150)
    except subprocess.TimeoutExpired as e:  # (subprocess.run has killed the child)
        pytest.fail(f"dc_stream_kernel did not finish within the watchdog's 150 s: {(e.stdout or b'')[-500:]!r}")
    assert r.returncode == 0 and "DCS_WATCHDOG_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("name", ["Cont-CC-PermExDc-v0", "Finite-CC-PMSM-v0", "Cont-SC-SCIM-v0", "Finite-CC-PMSM-v0_DeadTime2"])
def test_replay_of_the_reference_env_shell_transcript(name):
    """The contract of the drop-in seam, replayed: tests/golden/shell_*.json is the ordered list of everything the UNMODIFIED reference
    env shell (ElectricMotorEnvironment, core.py:197-371, with its reference generator, reward function, constraint monitor and
    dashboards) read from and called on its physical system over a seeded 200-step run with resets -- recorded in the build container by
    oracle/make_shell_transcript.py (the GPU box has no reference; the build container has no GPU).  `make(env_id, n_envs=1)`'s physical
    system answers the same sequence: metadata reads identically, `k` exactly, `reset()` to 1e-12, `simulate(action)` within the 1e-4
    contract of the reference's default solver (numpy in, 1-D numpy out, as core.py:328-371 consumes it)."""
    import gym_electric_motor_amd as ga
    from test_host_cpu import _decode, check_shell_get, shell_transcript

    doc = shell_transcript(name)
    wr = (ga.DeadTimeProcessor(steps=2),) if doc["wrappers"] else ()
    env = ga.make(doc["env_id"], n_envs=1, physical_system_wrappers=wr)
    ps = env.physical_system
    got, ref, n_sim, n_reset = [], [], 0, 0
    for e in doc["log"]:
        if e["op"] == "get":
            if e["name"] == "k":
                assert ps.k == e["value"], (ps.k, e["value"])
            else:
                check_shell_get(ps, e)
            continue
        args, ret = _decode(e["args"]), _decode(e["ret"])
        if e["name"] == "simulate":
            out = ps.simulate(*args)
            assert isinstance(out, np.ndarray) and out.ndim == 1 and out.dtype == np.float64 and out.shape == ret.shape
            got.append(out)
            ref.append(ret)
            n_sim += 1
        elif e["name"] == "reset":
            out = ps.reset(*args)
            assert isinstance(out, np.ndarray) and np.abs(out - ret).max() < 1e-12
            n_reset += 1
        elif e["name"] == "close":
            ps.close()
        else:
            raise AssertionError(f"the shell called {e['name']}: not part of the surface this test knows")
    assert n_sim == doc["steps"] and n_reset >= 1
    rel, ab = _rel_err(np.asarray(got), np.asarray(ref), list(ps.state_names))
    assert rel < 1e-4, (rel, ab)


@pytest.mark.parametrize("env_id, n", [("Cont-SC-SCIM-v0", 4096), ("Cont-CC-PMSM-v0", 200), ("Finite-CC-PMSM-v0", 16384), ("Finite-CC-DFIM-v0", 1000),
                                       ("Cont-CC-DFIM-v0", 70), ("Finite-CC-ExtExDc-v0", 4160), ("Cont-CC-PermExDc-v0", 8256)])
def test_synthetic_actions_generated_in_the_launch_equal_the_same_stream_from_a_tensor(env_id, n):
    """gemx_rollout_synthetic (actions generated on-device -- the loader wave computes every env's action of every step from
    (seed, env, step, component) and no action tensor is read) against gemx_rollout on the tensor gemx_synthetic_actions writes for the
    same stream: observations, done bytes and final state bit for bit, over two chunked launches that continue the stream, partial
    workgroups and unaligned batch sizes included; the stream itself is uniform (continuous: on (-1, 1), mean / variance / range;
    discrete: every index of the action set, equally often) and differs between envs, steps, components and seeds."""
    import torch

    import gym_electric_motor_amd as ga

    K1, K2, seed = 96, 37, 0xC0FFEE1234
    ea, eb = ga.make(env_id, n_envs=n), ga.make(env_id, n_envs=n)
    pa, pb = ea.physical_system, eb.physical_system
    acts = pb.synthetic_actions(K1 + K2, seed=seed, step0=0)
    o1, d1 = ea.rollout_synthetic(K1, seed=seed)
    assert "advance_pipe_kernel" in pa.last_launch()
    o2, d2 = ea.rollout_synthetic(K2, seed=seed)  # (step0 defaults to the step count: the stream continues)
    r1, q1 = eb.rollout(acts[:K1])
    r2, q2 = eb.rollout(acts[K1:])
    assert torch.equal(o1, r1) and torch.equal(d1, q1) and torch.equal(o2, r2) and torch.equal(d2, q2)
    assert torch.equal(pa.get_state(), pb.get_state()) and pa.k == pb.k == K1 + K2
    a = acts.double().cpu().numpy()
    if pa._discrete:
        nflat = int(np.prod(pa.action_space.nvec)) if hasattr(pa.action_space, "nvec") else int(pa.action_space.n)
        counts = np.bincount(a.astype(np.int64).ravel(), minlength=nflat)
        assert len(counts) == nflat and counts.min() > 0.9 * a.size / nflat and counts.max() < 1.1 * a.size / nflat
    else:
        assert -1.0 < a.min() < -1.0 + 20.0 / a.size and 1.0 - 20.0 / a.size < a.max() < 1.0
        assert abs(a.mean()) < 5.0 * 0.5774 / np.sqrt(a.size) + 1e-4 and abs(a.var() - 1.0 / 3.0) < 5.0 * 0.3 / np.sqrt(a.size) + 1e-4
        if a.shape[2] > 1:
            assert abs(np.corrcoef(a[..., 0].ravel(), a[..., 1].ravel())[0, 1]) < 5.0 / np.sqrt(a[..., 0].size)  # (5 sigma of an uncorrelated sample)
    assert abs(np.corrcoef(a[:-1].ravel(), a[1:].ravel())[0, 1]) < 5.0 / np.sqrt(a[1:].size)          # step to step
    assert abs(np.corrcoef(a[:, :-1].ravel(), a[:, 1:].ravel())[0, 1]) < 5.0 / np.sqrt(a[:, 1:].size)    # env to env
    other = pb.synthetic_actions(4, seed=seed + 1, step0=0)
    assert not torch.equal(other, acts[:4])
    assert torch.equal(pb.synthetic_actions(5, seed=seed, step0=K1), acts[K1:K1 + 5])
    ea.close(), eb.close()


def test_synthetic_rollout_refuses_what_the_pipelined_kernel_does_not_serve():
    import gym_electric_motor_amd as ga

    env = ga.make("Finite-CC-PMSM-v0", n_envs=128, constraints=("i_sq",))  # (a custom constraint set is served since round 5)
    env.rollout_synthetic(16)
    assert "advance_pipe_kernel" in env.physical_system.last_launch()
    env.close()
    env = ga.make("Finite-CC-PMSM-v0", n_envs=128, dtype="float64")
    with pytest.raises(ValueError, match="fp32"):
        env.rollout_synthetic(16)
    env.close()
