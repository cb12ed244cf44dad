"""Custom constraint sets: the cases, their action streams and their fp64 oracle runs, for tests/test_constraints_cpu.py (oracle alone,
on the CPU) and for device runs of the same cases against the oracle (test_gpu_parity._make_from_meta builds a case's env from its meta).

A set is data, as oracle/make_golden.py stores it in a fixture's meta["constraints"]:
    [{"kind": "limit" | "squared" | "name", "states": [...]}, ...]
("name": bare state names or "all_states", handed to make() as strings).  A case of the matrix is a recorded `default_*` fixture's meta
(what `make(env_id)` builds, read from the live reference) with a few entries replaced, plus such a set.
"""
import functools
import glob
import json
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURE_DIR = os.path.join(GOLDEN, "constraints")  # (a directory of its own: the tests that enrol tests/golden/*.npz apply the DEFAULT masks)
FIXTURES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(FIXTURE_DIR, "*.npz")))

N_ENVS, K_STEPS, HELD_FROM = 70, 300, 40  # one full wave plus a partial workgroup; random for 40 steps, then held
DONE_BAND = 1e-5                          # tests/parity_contract.py: DONE_MARGIN


def L(*s):
    return dict(kind="limit", states=list(s))


def S(*s):
    return dict(kind="squared", states=list(s))


def NAMES(*s):
    return dict(kind="name", states=list(s))


def load_fixture(name):
    d = np.load(os.path.join(FIXTURE_DIR, name + ".npz"))
    return d, json.loads(str(d["meta"]))


def build_constraints(spec, limit_cls, squared_cls):
    """A stored set -> what make(constraints=...) takes, from the given LimitConstraint / SquaredConstraint classes (the package's holders,
    or the reference's own classes when oracle/make_golden.py records)."""
    out = []
    for c in spec:
        if c["kind"] == "limit":
            out.append(limit_cls(tuple(c["states"])))
        elif c["kind"] == "squared":
            out.append(squared_cls(tuple(c["states"])))
        else:
            assert c["kind"] == "name", c
            out.extend(c["states"])
    return tuple(out)


def package_constraints(ga, spec):
    return build_constraints(spec, ga.LimitConstraint, ga.SquaredConstraint)


def term_values(meta, masks, rows):
    """The two sub-expressions of a set on normalised rows [..., S]: (max |x_i| over the limit mask, sum x_i^2 over the squared mask)."""
    n = len(meta["state_names"])
    li = [i for i in range(n) if masks[0] >> i & 1]
    si = [i for i in range(n) if masks[1] >> i & 1]
    rows = np.asarray(rows, dtype=np.float64)
    lim = np.abs(rows[..., li]).max(axis=-1) if li else np.zeros(rows.shape[:-1])
    sq = (rows[..., si] ** 2).sum(axis=-1) if si else np.zeros(rows.shape[:-1])
    return lim, sq


# ---------------------------------------------------------------------------------------------------------------------------------
# The matrix.  base: the `default_*` fixture whose meta describes the env id; meta: entries replaced in it (tau, dead time, supply,
# wrappers -- all read by both oracle.params_from_meta and test_gpu_parity._make_from_meta); solver: the device solver ("euler", "rk4x3",
# "scipy"); limit_values: the motor's limit_values make-kwarg (keys that ARE state names, or "u": every voltage column but u_sup), so that
# a term that the default limits leave dead inside 300 steps -- or on every row -- carries real episodes; default_bits: the set is the env's default written as objects and must give the bits of plain make(env_id).
RC = dict(supply="RCVoltageSupply", supply_parameter=dict(R=1.0, C=4e-3))
MATRIX = {
    # squared sets that are not the default
    "scim_sq_iabc": dict(base="cont_sc_scim", spec=[S("i_sa", "i_sb", "i_sc")]),
    "pmsm_sq_udq": dict(base="cont_cc_pmsm", spec=[S("u_sd", "u_sq")]),
    "eesm_sq_idq_ie": dict(base="cont_cc_eesm", spec=[S("i_sd", "i_sq", "i_e")]),
    "permexdc_poly_sq_i_omega": dict(base="cont_sc_permexdc", spec=[S("i", "omega")]),
    # mixed sets
    "pmsm_sc_sq_idq_lim_omega": dict(base="cont_sc_pmsm", limit_values=dict(omega=12.0), spec=[S("i_sd", "i_sq"), L("omega")]),
    "dfim_sq_idq_lim_ira_omega": dict(base="cont_sc_dfim", spec=[S("i_sd", "i_sq"), L("i_ra", "omega")]),
    "scim_sq_idq_lim_torque": dict(base="cont_sc_scim", limit_values=dict(torque=0.08), spec=[S("i_sd", "i_sq"), L("torque")]),
    # limit sets on derived columns
    "pmsm_lim_ia_ib_torque": dict(base="cont_cc_pmsm", spec=[L("i_a", "i_b", "torque")]),
    # (behind a finite B6 bridge a phase voltage is +-u_sup / 2 whatever the action: 210 V under the ideal 420 V supply, above its 150 V
    # limit on every row.  Behind an RC supply with the limit at 211 V it violates where a braking machine pumps the DC link above 422 V:
    # calm lanes on the zero vector draw no supply current and stay at 210 / 211)
    "pmsm_fin_rc_lim_ub": dict(base="finite_cc_pmsm", meta=dict(tau=1e-4, supply="RCVoltageSupply", supply_parameter=dict(R=0.5, C=1e-3)),
                               limit_values=dict(u=422.0), spec=[L("u_b")]),
    "series_lim_i_torque": dict(base="cont_cc_seriesdc", limit_values=dict(i=60.0, torque=4.0), spec=[L("i", "torque")]),
    # all states
    "permexdc_all_states": dict(base="cont_sc_permexdc", spec=[NAMES("all_states")]),
    "pmsm_all_states": dict(base="cont_cc_pmsm", spec=[L("all_states")]),
    # (300.2 V: fl32(300.2) * fl32(1 / 300.2) = 1 + 2^-23 -- the plain rounded reciprocal limit would terminate every env at once)
    "pmsm_all_states_300v2": dict(base="cont_cc_pmsm", u_nominal=300.2, spec=[L("all_states")]),
    # the default set written as objects
    "pmsm_default_as_objects": dict(base="cont_cc_pmsm", spec=[S("i_sq", "i_sd")], default_bits=True),
    "eesm_default_as_objects": dict(base="cont_cc_eesm", spec=[S("i_sq", "i_sd"), L("i_e")], default_bits=True),
    "shunt_default_as_objects": dict(base="cont_cc_shuntdc", spec=[L("i_a", "i_e")], default_bits=True),
    # beside other per-lane features that pass through the pipelined kernel's own copy of the expressions
    "pmsm_rc_supply_sq_idq_lim_ia": dict(base="cont_cc_pmsm", meta=RC, spec=[S("i_sd", "i_sq"), L("i_a", "torque")]),
    "pmsm_fin_dead_time_lim_ia_ib_ic": dict(base="finite_cc_pmsm", meta=dict(tau=1e-4, interlocking_time=1e-6), spec=[L("i_a", "i_b", "i_c")]),
    "pmsm_delay2_sq_idq_lim_torque": dict(base="cont_cc_pmsm", meta=dict(dead_time_steps=2), spec=[S("i_sd", "i_sq"), L("torque")]),
    "pmsm_rk4x3_lim_isq_torque": dict(base="cont_cc_pmsm", solver="rk4x3", spec=[L("i_sq", "torque")]),
    "pmsm_dq_space_sq_iab_lim_isd": dict(base="cont_cc_pmsm", meta=dict(action_frame="dq"), spec=[S("i_a", "i_b"), L("i_sd")]),
    "scim_scipy_sq_iabc_lim_torque": dict(base="cont_sc_scim", solver="scipy", limit_values=dict(torque=0.08), spec=[S("i_sa", "i_sb", "i_sc"), L("torque")]),
}


def case_meta(case_id):
    c = MATRIX[case_id]
    d = np.load(os.path.join(GOLDEN, f"default_{c['base']}_dopri5.npz"))
    meta = json.loads(str(d["meta"]))
    meta.update(c.get("meta", {}))
    if "u_nominal" in c:  # an ideal supply of another voltage: the u_sup column's limit is that voltage
        meta["u_nominal"] = meta["limits"][meta["state_names"].index("u_sup")] = float(c["u_nominal"])
        meta["overrides"] = dict(supply=dict(u_nominal=float(c["u_nominal"])))
    if "limit_values" in c:
        for key, v in c["limit_values"].items():
            # ("u": the motor's voltage limit; behind a B6 bridge the limit of every voltage column is half of it)
            for col in ([n for n in meta["state_names"] if n.startswith("u_") and n != "u_sup"] if key == "u" else [key]):
                meta["limits"][meta["state_names"].index(col)] = float(v) / 2 if key == "u" else float(v)
        meta["overrides"] = dict(motor=dict(limit_values=dict(c["limit_values"])))
    meta.update(name=case_id, episodic=True, every=1, constraints=c["spec"], solver={"scipy": "dopri5"}.get(c.get("solver", "euler"), c.get("solver", "euler")))
    return meta


def oracle_solver(case_id):
    """(oracle solver name, nsteps) of the case's integrator."""
    return {"euler": ("euler", 1), "rk4x3": ("rk4", 3), "scipy": ("dopri5", 1)}[MATRIX[case_id].get("solver", "euler")]


def n_actions(meta):
    if meta["converter"].startswith("Finite"):
        per = {"FiniteB6BridgeConverter": 8, "FiniteFourQuadrantConverter": 4}
        names = meta["converter"].split("[")[1].rstrip("]").split(",") if "[" in meta["converter"] else [meta["converter"]]
        return [per[n] for n in names]
    return None


def actions(case_id, meta, n_act, K=K_STEPS, n=N_ENVS):
    """[K, n, A] float64: random for HELD_FROM steps, then held, so that currents and speeds run into their limits; every third lane is
    calm instead -- its actions scaled to 2 %, or kept on the zero vector behind a finite converter -- and never terminates."""
    rng = np.random.default_rng(zlib.crc32(case_id.encode()))
    calm = np.arange(n) % 3 == 2
    nvec = n_actions(meta)
    if nvec is not None:
        a = np.stack([rng.integers(0, nv, (K, n)) for nv in nvec], axis=-1).astype(np.float64)
        a[HELD_FROM:] = a[HELD_FROM]
        a[:, calm] = 0.0
    else:
        a = rng.uniform(-1.0, 1.0, (K, n, n_act))
        a[HELD_FROM:] = a[HELD_FROM]
        a[:, calm] *= 0.02
    return a, calm


@functools.lru_cache(maxsize=None)
def oracle_run(case_id):
    """The fp64 oracle on every lane of the case, computed once: dict(meta, masks, actions [K,N,A], calm [N], rows [K,N,S], done [K,N])."""
    import ctypes as C

    from oracle import oracle as orc

    meta = case_meta(case_id)
    masks = orc.masks_from_spec(meta, meta["constraints"])
    name, nsteps = oracle_solver(case_id)
    p = orc.params_from_meta(meta, solver=name, masks=masks)
    p.nsteps = nsteps
    e = orc.OracleEnv(p)  # ONE oracle object for all lanes, initialised afresh for each
    a, calm = actions(case_id, meta, e.n_act)
    K, n = a.shape[:2]
    rows, done = np.zeros((K, n, e.n_out)), np.zeros((K, n), dtype=bool)
    for j in range(n):
        C.memset(e._env, 0, len(e._env))
        e.L.orc_init(C.byref(e.p), e._env)
        e.reset()
        rows[:, j], done[:, j] = e.rollout(a[:, j], auto_reset=True)
    return dict(meta=meta, masks=masks, actions=a, calm=calm, rows=rows, done=done)


def oracle_counts(run):
    """What the oracle alone says about a case: terminations, lanes without one, which terms fired, lane-steps within DONE_BAND of the
    boundary (each of them is a step where an fp32 device may decide `done` the other way)."""
    lim, sq = term_values(run["meta"], run["masks"], run["rows"])
    done = run["done"]
    assert np.array_equal(done, (lim > 1.0) | (sq > 1.0))  # (the oracle's own done IS the two sub-expressions)
    fired = dict(limit=bool((done & (lim > 1.0)).any()), squared=bool((done & (sq > 1.0)).any()))
    want = dict(limit=bool(run["masks"][0]), squared=bool(run["masks"][1]))
    near = int((np.abs(np.maximum(lim, sq) - 1.0) < DONE_BAND).sum())
    per_lane = done.sum(axis=0)
    return dict(terminations=int(done.sum()), lanes_without=int((per_lane == 0).sum()), lanes_repeated=int((per_lane >= 2).sum()), fired=fired, want=want,
                near=near, lane_steps=int(done.size))
