"""The smooth dynamics of every chain against a first-principles reference (tests/first_principles_oracle.py: dense projections of
rigid-body mechanics in numpy, no algorithm shared with the oracle or the kernels): the fp64 oracle (oracle/mjo_core.c) and the host
builds of the device engines (tests/host_harness, fp64 and fp32) at airborne states with no contact and no joint limit active, so that
body masses / COMs / inertia tensors, M(q), the Coriolis / centrifugal / gyroscopic / gravity bias, passive and actuator forces, the
unconstrained integrators and the humanoid's cinert / cvel / qfrc_actuator blocks are pinned by something their author did not write.

MEASURED (64 candidate states per case, `python tests/test_first_principles_host.py` prints this table).  Per quantity: the worst
oracle-vs-reference residual over all kinds and walker2d sizes, the reference's own error estimate, the smallest residual a flaw
switch that touches the quantity produces (over the kinds the flaw applies to), and the bound, which sits >= 100x above the first two
and >= 100x below the third:

    quantity                 residual   reference error   smallest flaw residual   bound
    body_mass      (rel)     5.3e-16   rounding          - (no flaw moves a mass)   1e-9
    body_ipos      (m)       1.7e-16   rounding          - (no flaw moves a COM)    1e-9
    body_inertia   (rel)     1.4e-15   rounding          5.3e-3 hemisphere_offset   1e-9
    M              (rel)     1.1e-15   rounding          4.3e-4 no_armature         1e-9
    bias           (rel)     6.6e-15   4.3e-12           2.3e-3 hemisphere_offset   1e-7
    qacc_smooth    (rel)     1.8e-13   4.3e-12           6.3e-3 hemisphere_offset   1e-7
    step qpos      (abs)     1.9e-14   4.3e-12           3.9e-5 hemisphere_offset   1e-8
    step qvel      (rel)     1.2e-13   4.3e-12           1.6e-3 hemisphere_offset   1e-7
    cinert         (rel)     2.4e-15   rounding          2.7e-4 no_gyroscopic       1e-9 at set_state, 1e-7 after a step
    cvel           (rel)     6.1e-15   4.3e-12           2.6e-2 no_gyroscopic       1e-7
    qfrc_actuator  (rel)     0         exact             6.0e-1 no_ctrl_clip        1e-9

The reference error of the constants and of M is rounding in closed forms (a few ulp, checked against quadrature and by symmetry);
that of everything velocity-dependent is `jdot_error`, the distance of the analytic J' v from Richardson-extrapolated central
differences of J (itself limited by the differences' own rounding, so an upper estimate).

fp32 host builds: the project's stated fp32 tolerances -- planar step |dqpos| <= 5e-5 and |dqvel| / (1 + |qvel|inf) <= 5e-4
(tests/test_gpu_pinned_constants.py), humanoid obs rel <= 2e-4 and qvel rel <= 5e-4 (tests/test_gpu_humanoid.py), forward-only
quantities (constants, M, the set_state observation) <= 2e-5.  An acceleration has no stated tolerance of its own; an error e_a held
over one env step of length T moves the end velocity by T e_a, so the bound that is consistent with the velocity tolerance is
|dqacc| <= 5e-4 (1 + |qvel|inf) / T.  Worst fp32 figures measured: constants 3.1e-7, M 9.7e-7 (humanoid),
planar step |dqpos| 4.5e-7 and qvel rel 1.3e-6, planar |dqacc| T / (1 + |qvel|inf) 3.5e-6 of 5e-4, humanoid step obs rel 1.3e-5 and
qvel rel 1.3e-5, humanoid |dqacc| T / (1 + |qvel|inf) 4.5e-4 of 5e-4 (its light arms under xi at the box corners)."""
import ctypes
import functools

import numpy as np
import pytest

import first_principles_oracle as fp
from oracle_bindings import (DIMS, _p, oracle_batch_step, oracle_constants, oracle_forward, oracle_humanoid_reset_obs,
                             oracle_humanoid_step)

WALKER_KEYS = sorted(fp.walker_sizes())
CASES = [("hopper", None), ("halfcheetah", None), ("humanoid", None)] + [("walker2d", k) for k in WALKER_KEYS]
CASE_IDS = [k or kind for kind, k in CASES]
N_CANDIDATES = 64

# fp64 bounds (see the table above)
BOUND = dict(body_mass=1e-9, body_ipos=1e-9, body_inertia=1e-9, M=1e-9, bias=1e-7, qacc_smooth=1e-7, step_qpos=1e-8, step_qvel=1e-7,
             cinert=1e-9, cvel=1e-7, qfrc_actuator=1e-9, cinert_step=1e-7, cvel_step=1e-7, qfrc_actuator_step=1e-9)
# the kinds on which a flaw changes anything: single-geom bodies have no parallel-axis term, only the half-cheetah sets a total mass,
# only the humanoid has a free joint, a principal-axis spin (planar chains turn about a principal axis: w x I w = 0) and a ctrlrange
# inside the action range
FLAW_KINDS = dict(hemisphere_offset=("hopper", "halfcheetah", "walker2d", "humanoid"), no_parallel_axis=("halfcheetah", "humanoid"),
                  no_armature=("hopper", "halfcheetah", "walker2d", "humanoid"), xi_scales_inertia=("hopper", "halfcheetah", "walker2d", "humanoid"),
                  totalmass_masses_only=("halfcheetah",), free_omega_world=("humanoid",), no_gyroscopic=("humanoid",), no_ctrl_clip=("humanoid",))
assert set(FLAW_KINDS) == set(fp.FLAWS)

# ---- the state generator ------------------------------------------------------------------------------------------------------
SPIN = dict(hopper=12.0, walker2d=12.0, halfcheetah=18.0, humanoid=8.0)      # root spin, rad/s
RATE = dict(hopper=8.0, walker2d=8.0, halfcheetah=4.0, humanoid=6.0)         # joint rates, rad/s
# what a joint can travel in one env step (rate x T plus what a saturated motor adds against armature, damping and spring), rad
TRAVEL = dict(hopper=0.15, walker2d=0.15, halfcheetah=0.5, humanoid=0.4)
HOPPER_FOLD_CAP = 1.5    # -(hip + knee) below this keeps the hopper's torso clear of its own leg and foot capsules


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def candidates(kind, n, seed, key=None):
    """Seeded airborne states inside the joint limits, fp32-representable: (qpos, qvel, action, xi)."""
    from random_envs_amd.specs import SPECS
    rng = np.random.RandomState(seed)
    b = np.array(SPECS[kind].search_bounds, dtype=np.float64)
    xi = rng.uniform(b[:, 0], b[:, 1], (n, len(b)))                          # the whole search box
    if kind == "walker2d":
        xi[:, 7:11] = fp.walker_sizes()[key]
    m = fp.model(key or kind)
    T = m.timestep * DIMS[kind]["frame_skip"]
    q = np.tile(m.qpos0, (n, 1)); v = np.zeros((n, m.nv))
    for d, (k, body, a0, an0, qa, ref) in enumerate(m.dofs):
        name = m.jnt_names[d]
        if k == "hinge" and name in m.range:
            lo, hi = m.range[name]
            tr = min(TRAVEL[kind], 0.45 * (hi - lo))
            q[:, qa] = rng.uniform(lo + tr, hi - tr, n); v[:, d] = rng.uniform(-RATE[kind], RATE[kind], n)
        elif k == "hinge":                                                   # the planar root pitch: any angle
            q[:, qa] = rng.uniform(-np.pi, np.pi, n); v[:, d] = rng.uniform(-SPIN[kind], SPIN[kind], n)
        elif k in ("slide", "lin"):
            v[:, d] = rng.uniform(-2, 2, n)
        else:
            v[:, d] = rng.uniform(-SPIN[kind], SPIN[kind], n)
    if kind == "humanoid":                                                   # full random root orientation
        qq = rng.randn(n, 4); q[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    if kind == "hopper":
        for _ in range(100):
            bad = -(q[:, 3] + q[:, 4]) > HOPPER_FOLD_CAP
            if not bad.any():
                break
            q[bad, 3:5] = rng.uniform(-2.6 + TRAVEL[kind], -TRAVEL[kind], (int(bad.sum()), 2))
    zi = 2 if kind == "humanoid" else 1
    q[:, zi] += rng.uniform(0.5, 1.0, n) + 2 * T - m.clearance(q)            # every geom at least 0.5 m + the fall of one step up
    a = rng.uniform(-1, 1, (n, m.nu))
    q, v, a, xi = _f32(q), _f32(v), _f32(a), _f32(xi)
    if kind == "walker2d":       # the lengths name a rendered table: they stay exact (the device rounds them to fp32, 3e-8 relative)
        xi[:, 7:11] = fp.walker_sizes()[key]
    return q, v, a, xi


def _oracle_step(kind, q, v, a, xi):
    return oracle_humanoid_step(q, v, a, xi) if kind == "humanoid" else oracle_batch_step(kind, q, v, a, xi)


@functools.lru_cache(maxsize=None)
def kept_states(kind, key=None, n=N_CANDIDATES, seed=7):
    """The candidates at which the ORACLE reports no contact and no constraint row at the start state and at the end state of its own
    step, with what the oracle computes there.  dict(q, v, a, xi, kept fraction, velocity / gravity bias ratio, oracle outputs)."""
    q, v, a, xi = candidates(kind, n, seed, key)
    st = _oracle_step(kind, q, v, a, xi)
    keep = np.zeros(n, bool); ratio = np.zeros(n); fw = []
    for i in range(n):
        f0 = oracle_forward(kind, q[i], v[i], a[i], xi[i]); f1 = oracle_forward(kind, st["qpos"][i], st["qvel"][i], a[i], xi[i])
        keep[i] = f0["ncon"] == 0 and f0["nefc"] == 0 and f1["ncon"] == 0 and f1["nefc"] == 0
        g = oracle_forward(kind, q[i], 0 * v[i], a[i], xi[i])["bias"]        # gravity's part of the bias
        ratio[i] = np.abs(f0["bias"] - g).max() / np.abs(g).max()
        fw.append(f0)
    out = dict(q=q[keep], v=v[keep], a=a[keep], xi=xi[keep], kept=keep.mean(), ratio=ratio[keep],
               M=np.array([f["M"] for f in fw])[keep], bias=np.array([f["bias"] for f in fw])[keep],
               qacc_smooth=np.array([f["qacc_smooth"] for f in fw])[keep], qpos=st["qpos"][keep], qvel=st["qvel"][keep])
    if kind == "humanoid":
        out["obs_step"] = st["obs"][keep]
        out["obs_reset"] = oracle_humanoid_reset_obs(out["q"], out["v"], out["xi"])[0]
    return out


# ---- residuals ----------------------------------------------------------------------------------------------------------------
def _rel(got, ref):
    """worst over states of max |got - ref| / (1 + max |ref|), both [N, ...]"""
    got = np.asarray(got).reshape(len(got), -1); ref = np.asarray(ref).reshape(len(ref), -1)
    return float((np.abs(got - ref).max(1) / (1 + np.abs(ref).max(1))).max())


def _blocks(obs):
    return dict(cinert=obs[:, 45 + 10:185], cvel=obs[:, 185 + 6:269], qfrc_actuator=obs[:, 269:292])     # (the world body's rows are zeros)


@functools.lru_cache(maxsize=None)
def reference_side(kind, key=None, flaw=None, step=True):
    """what the reference computes at the kept states of (kind, key)"""
    s = kept_states(kind, key)
    m = fp.model(key or kind, flaw=flaw)
    d = m.dynamics(s["q"], s["v"], s["a"], s["xi"])
    out = dict(model=m, M=d["M"], bias=d["bias"], qacc_smooth=d["qacc_smooth"])
    if kind == "humanoid":
        out["reset"] = m.com_blocks(s["q"], s["v"], None, s["xi"])           # reset / set_state: ctrl = 0
    if step:
        e = m.env_step(s["q"], s["v"], s["a"], s["xi"], DIMS[kind]["frame_skip"])
        out.update(qpos=e["qpos"], qvel=e["qvel"])
        if kind == "humanoid":
            out["step"] = m.com_blocks(e["qpos_stage4"], e["qvel_stage4"], s["a"], s["xi"])
    return out


def constants_residuals(m, mass, com_or_ipos, inertia, body_frame_is_world):
    """mass [nb], COM and inertia of a model under test against the reference model m.  Planar chains: body frames are world-aligned
    at qpos0, so the COM (body origin + ipos) and the full tensor compare directly; the humanoid's waist and pelvis frames are tilted
    by quaternions the tables do not carry, so |ipos| and the principal moments compare there (its cinert block at random orientations
    pins the tensors' axes and the COMs' directions)."""
    r = dict(body_mass=float(np.abs(mass - m.mass0).max() / m.mass0.max()))
    if body_frame_is_world:
        r["body_ipos"] = float(np.abs(m.body_pos0 + com_or_ipos - m.com0).max())
        r["body_inertia"] = float(np.abs(inertia - m.inertia0).max() / np.abs(m.inertia0).max())
    else:
        r["body_ipos"] = float(np.abs(np.linalg.norm(com_or_ipos, axis=1) - np.linalg.norm(m.com0 - m.body_pos0, axis=1)).max())
        ev = lambda I: np.sort(np.linalg.eigvalsh(I), axis=-1)
        r["body_inertia"] = float(np.abs(ev(inertia) - ev(m.inertia0)).max() / np.abs(m.inertia0).max())
    return r


def dynamics_residuals(kind, ref, got):
    """got: dict with any of M, bias, qacc_smooth, qpos, qvel, obs_reset, obs_step of a side under test, at the kept states"""
    r = {}
    if "M" in got:
        r["M"] = float((np.abs(got["M"] - ref["M"]).max((1, 2)) / np.abs(ref["M"]).max((1, 2))).max())
    for k in ("bias", "qacc_smooth"):
        if k in got:
            r[k] = _rel(got[k], ref[k])
    if "qpos" in got and "qpos" in ref:
        r["step_qpos"] = float(np.abs(got["qpos"] - ref["qpos"]).max())
        r["step_qvel"] = _rel(got["qvel"], ref["qvel"])
    for tag, sfx in (("reset", ""), ("step", "_step")):
        if "obs_" + tag in got and tag in ref:
            for k, blk in _blocks(got["obs_" + tag]).items():
                want = ref[tag][k]
                r[k + sfx] = _rel(blk, want.reshape(len(want), -1))
    return r


def oracle_residuals(kind, key=None, flaw=None, step=True):
    ref = reference_side(kind, key, flaw, step)
    oc = oracle_constants(kind, size=fp.walker_sizes()[key] if key else None)
    r = constants_residuals(ref["model"], oc["body_mass"][1:], oc["body_ipos"][1:], oc["body_inertia"][1:].reshape(-1, 3, 3), kind != "humanoid")
    r.update(dynamics_residuals(kind, ref, kept_states(kind, key)))
    return r


def _check(r, bounds, tag):
    print("%s: %s" % (tag, "  ".join("%s %.2e" % kv for kv in sorted(r.items()))))
    over = {k: (x, bounds[k]) for k, x in r.items() if not x <= bounds[k]}
    assert not over, (tag, over)


# ---- the reference's own tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,L", [(0.05, 0.4), (0.06, 0.39), (0.09, 0.14), (0.031, 0.2771), (0.075, 0.0)])
def test_reference_solids_against_quadrature(r, L):
    """closed-form capsule (cylinder + two hemispheres with their own centroid offset) and sphere against brute-force quadrature of
    the solid; the midpoint grid's own error is O(1 / n) at the curved boundary, 1e-3 relative at n = 400"""
    vol, it, ia = fp.solid_by_quadrature(r, L)
    if L == 0.0:
        m, diag = fp.sphere_solid(r, 1.0)
    else:
        m, diag = fp.capsule_solid(r, L, 1.0, capsule_volume="exact")
    e = max(abs(m / vol - 1), abs(diag[0] / it - 1), abs(diag[2] / ia - 1))
    print("r %.3f L %.3f: closed form vs quadrature %.2e" % (r, L, e))
    assert e < 2e-3
    if L:       # ... and the quadrature tells the hemisphere-offset misreading from the solid
        _, bad = fp.capsule_solid(r, L, 1.0, capsule_volume="exact", flaw="hemisphere_offset")
        assert abs(bad[0] / it - 1) > 10 * e


@pytest.mark.parametrize("kind,key", CASES, ids=CASE_IDS)
def test_reference_mass_matrix_is_symmetric_positive_definite(kind, key):
    M = reference_side(kind, key, step=False)["M"]
    assert np.abs(M - np.swapaxes(M, 1, 2)).max() <= 1e-13 * np.abs(M).max()
    assert np.linalg.eigvalsh(M).min() > 0


def test_reference_free_floating_humanoid_conserves_momentum_and_energy():
    """No gravity, no damping, no springs, no motors, and no armature (a rotor inertia on the joint axis alone carries no momentum of
    its own, so a model with armature does not conserve the bodies' momentum): the total linear and angular momentum of a spinning,
    flailing humanoid have zero time derivative at the reference's own accelerations, to rounding.  Over one env step (five RK4 steps
    of 3 ms) they and the energy drift by the integrator's truncation alone: little, and 4x less when the step is halved.  (Second
    order, not fourth: mj_RungeKutta advances the root quaternion by the WEIGHTED SUM of the stage rotation vectors, which drops the
    commutator of rotations about different axes.  That is convention 1 of the reference's header, not mechanics.)"""
    s = kept_states("humanoid")
    m = fp.Model("humanoid", flaw="no_armature")
    kw = dict(gravity=False, passive=False)
    d0 = m.dynamics(s["q"], s["v"], None, s["xi"], **kw)
    acc = np.einsum("nbkd,nd->nbk", d0["Jv"], d0["qacc_smooth"]) + d0["jdot_v"]
    alpha = np.einsum("nbkd,nd->nbk", d0["Jw"], d0["qacc_smooth"]) + d0["jdot_w"]
    mass = d0["mass"][..., None]
    pdot = (mass * acc).sum(1)
    Iw = d0["Iw"]; w = d0["w"]
    Ldot = (np.cross(d0["kin"]["com"], mass * acc) + np.einsum("nbij,nbj->nbi", Iw, alpha)
            + np.cross(w, np.einsum("nbij,nbj->nbi", Iw, w))).sum(1)
    scale = (mass * np.abs(acc)).sum(1).max(1)                              # the forces that cancel
    rate = max(float((np.abs(pdot).max(1) / scale).max()), float((np.abs(Ldot).max(1) / scale).max()))
    print("free-floating humanoid: |dp/dt|, |dL/dt| / cancelling forces %.2e" % rate)
    assert rate < 1e-11
    drift = []
    for halvings in (0, 1):
        m.timestep = 0.003 / 2 ** halvings
        e = m.env_step(s["q"], s["v"], None, s["xi"], DIMS["humanoid"]["frame_skip"] * 2 ** halvings, **kw)
        d1 = m.dynamics(e["qpos"], e["qvel"], None, s["xi"], **kw)
        drift.append({k: float((np.abs(d1[k] - d0[k]).reshape(len(s["q"]), -1).max(1) / np.abs(d0[k]).reshape(len(s["q"]), -1).max(1)).max())
                      for k in ("lin_momentum", "ang_momentum", "energy")})
        print("  relative drift over 15 ms at h = %.4f: %s" % (m.timestep, drift[-1]))
    for k in drift[0]:
        assert drift[0][k] < 1e-4 and drift[1][k] < drift[0][k] / 3, (k, drift)


@pytest.mark.parametrize("kind,key", CASES, ids=CASE_IDS)
def test_reference_jdot_error_estimate(kind, key):
    s = kept_states(kind, key)
    e = fp.model(key or kind).jdot_error(s["q"], s["v"]).max()
    print("%s: analytic J'v vs Richardson-extrapolated central differences %.2e" % (key or kind, e))
    assert e * 100 <= min(BOUND["bias"], BOUND["qacc_smooth"], BOUND["step_qvel"], BOUND["cvel"])


# ---- the state sample ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,key", CASES, ids=CASE_IDS)
def test_states_are_kept_and_fast(kind, key):
    s = kept_states(kind, key)
    fast = float((s["ratio"] >= 1).mean())
    print("%s: %.0f %% of the candidates kept, velocity part of the bias >= gravity's part in %.0f %% of them (median ratio %.2f)"
          % (key or kind, 100 * s["kept"], 100 * fast, np.median(s["ratio"])))
    assert s["kept"] >= 0.9
    assert fast >= 0.5
    if kind == "humanoid":       # the +-0.4 ctrlrange clips
        assert (np.abs(s["a"]) > 0.4).mean() > 0.3


# ---- oracle vs reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,key", CASES, ids=CASE_IDS)
def test_oracle_matches_first_principles(kind, key):
    _check(oracle_residuals(kind, key), BOUND, "oracle %s" % (key or kind))


@pytest.mark.parametrize("flaw", fp.FLAWS)
def test_every_flaw_fails_the_oracle_comparison(flaw):
    """each named misreading, switched on in the reference, misses the oracle by >= 100x a bound on every kind it applies to"""
    for kind in FLAW_KINDS[flaw]:
        key = "walker2d_size_2" if kind == "walker2d" else None
        r = oracle_residuals(kind, key, flaw)
        worst = max(r, key=lambda k: r[k] / BOUND[k])
        print("%s on %s: %s off by %.2e = %.0fx its bound" % (flaw, key or kind, worst, r[worst], r[worst] / BOUND[worst]))
        assert r[worst] >= 100 * BOUND[worst], (flaw, kind, r)


# ---- host builds of the device engines vs reference ---------------------------------------------------------------------------
I32 = ctypes.POINTER(ctypes.c_int); UB = ctypes.POINTER(ctypes.c_ubyte)


def fp32_bounds(kind):
    T = fp.model(kind).timestep * DIMS[kind]["frame_skip"]
    if kind == "humanoid":
        return dict(body_mass=2e-5, body_ipos=2e-5, body_inertia=2e-5, M=2e-5, step_qvel=5e-4, cinert=2e-5, cvel=2e-5, qfrc_actuator=2e-5,
                    cinert_step=2e-4, cvel_step=2e-4, qfrc_actuator_step=2e-4, qacc_T=5e-4 / T)
    return dict(body_mass=2e-5, body_inertia=2e-5, M=2e-5, step_qpos=5e-5, step_qvel=5e-4, qacc_T=5e-4 / T)


def _qacc_T(got, s):
    """|dqacc| / (1 + |qvel|inf): compared with 5e-4 / T (module header)"""
    return float((np.abs(got["qacc_smooth"] - got["_ref_qacc"]).max(1) / (1 + np.abs(s["v"]).max(1))).max())


@pytest.mark.parametrize("f32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind,key", [c for c in CASES if c[0] != "humanoid"], ids=[i for i, c in zip(CASE_IDS, CASES) if c[0] != "humanoid"])
def test_planar_host_engine_matches_first_principles(kind, key, f32):
    """ph_constants, ph_forward and ph_step (planar_engine.hpp compiled for the host): walker2d derives its geometry from the xi lengths
    the way the device does"""
    from host_harness.build import host_constants, host_forward, host_step
    s = kept_states(kind, key); ref = reference_side(kind, key); m = ref["model"]
    c = host_constants(kind, bool(f32), size=fp.walker_sizes()[key] if key else None)
    r = dict(body_mass=float(np.abs(c["mass"] - m.mass0).max() / m.mass0.max()),
             body_inertia=float(np.abs(c["iyy"] - m.inertia0[:, 1, 1]).max() / np.abs(m.inertia0).max()))
    fw = [host_forward(kind, bool(f32), s["q"][i], s["v"][i], s["a"][i], s["xi"][i]) for i in range(len(s["q"]))]
    assert all(it == 0 for _, _, it in fw)                                   # no row, no solver iteration
    qo, vo, cap = host_step(kind, bool(f32), s["q"], s["v"], s["a"], s["xi"], DIMS[kind]["frame_skip"])
    assert not cap.any()
    got = dict(M=np.array([f[1] for f in fw]), qacc_smooth=np.array([f[0] for f in fw]), qpos=qo, qvel=vo)
    r.update(dynamics_residuals(kind, ref, got))
    if f32:
        got["_ref_qacc"] = ref["qacc_smooth"]; r["qacc_T"] = _qacc_T(got, s); del r["qacc_smooth"]
    _check(r, fp32_bounds(kind) if f32 else BOUND, "planar host %s %s" % (key or kind, "fp32" if f32 else "fp64"))


def _hum_step(lib, name, f32, s):
    n = len(s["q"])
    qs, vs, as_, xs = [np.ascontiguousarray(x.T) for x in (s["q"], s["v"], s["a"], s["xi"])]
    qo = np.zeros_like(qs); vo = np.zeros_like(vs); obs = np.zeros((376, n)); r = np.zeros(n); d = np.zeros(n, dtype=np.uint8)
    xo = np.zeros((14, n)); ov = np.zeros(n, dtype=np.int32); nr = np.zeros(n, dtype=np.int32)
    args = [f32, n, _p(qs), _p(vs), _p(as_), _p(xs), None, _p(qo), _p(vo), _p(obs), _p(r), d.ctypes.data_as(UB), _p(xo), ov.ctypes.data_as(I32)]
    if name == "hp_step":
        args.append(nr.ctypes.data_as(I32))
    assert getattr(lib, name)(*args) == 0 and ov.sum() == 0 and nr.sum() == 0
    return dict(qpos=qo.T.copy(), qvel=vo.T.copy(), obs_step=obs.T.copy())


@pytest.mark.parametrize("f32", [0, 1], ids=["fp64", "fp32"])
def test_humanoid_host_engines_match_first_principles(f32):
    """hh_constants, hh_forward, hh_step (humanoid_engine.hpp) and hp_step (humanoid_pair.hpp, the two-lanes-per-env step kernel's math)"""
    from host_harness.build import build_so
    hh = ctypes.CDLL(build_so("humanoid_host", "humanoid_host.cpp"))
    hp = ctypes.CDLL(build_so("humanoid_pair_host", "humanoid_pair_host.cpp", ["-pthread"]))
    s = kept_states("humanoid"); ref = reference_side("humanoid"); m = ref["model"]
    tag = "humanoid host %s" % ("fp32" if f32 else "fp64")
    bounds = fp32_bounds("humanoid") if f32 else BOUND
    if not f32:      # (the model is built once, in fp64, and converted)
        mass = np.zeros(14); ib = np.zeros(28); idf = np.zeros(23); ipos = np.zeros(42); inr = np.zeros(84); npair = ctypes.c_int()
        hh.hh_constants(_p(mass), _p(ib), _p(idf), _p(ipos), _p(inr), ctypes.byref(npair))
        i6 = inr.reshape(14, 6)[1:]
        I = np.array([[[a[0], a[3], a[4]], [a[3], a[1], a[5]], [a[4], a[5], a[2]]] for a in i6])
        _check(constants_residuals(m, mass[1:], ipos.reshape(14, 3)[1:], I, False), bounds, tag + " constants")
    n = len(s["q"]); qa = np.zeros((n, 23)); M = np.zeros((n, 23, 23))
    for i in range(n):
        info = np.zeros(4, dtype=np.int32)
        hh.hh_forward(f32, _p(s["q"][i]), _p(s["v"][i]), _p(s["a"][i]), _p(s["xi"][i]), _p(qa[i]), _p(M[i]), info.ctypes.data_as(I32))
        assert not info.any(), (i, info)                                     # no contact, no row, no sweep, nothing dropped
    got = dict(M=M, qacc_smooth=qa)
    r = dynamics_residuals("humanoid", ref, got)
    if f32:
        got["_ref_qacc"] = ref["qacc_smooth"]; r["qacc_T"] = _qacc_T(got, s); del r["qacc_smooth"]
    _check(r, bounds, tag + " hh_forward")
    for lib, name in ((hh, "hh_step"), (hp, "hp_step")):
        r = dynamics_residuals("humanoid", ref, _hum_step(lib, name, f32, s))
        if f32:
            del r["step_qpos"]      # (the project states no fp32 qpos tolerance for the humanoid: its qpos rides in the observation)
        _check(r, bounds, "%s %s" % (tag, name))


# ---- the table of the module header -------------------------------------------------------------------------------------------
if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    worst, err, flawed = {}, 0.0, {}
    for kind, key in CASES:
        for k, x in oracle_residuals(kind, key).items():
            worst[k] = max(worst.get(k, 0.0), x)
        s = kept_states(kind, key)
        err = max(err, float(fp.model(key or kind).jdot_error(s["q"], s["v"]).max()))
    for flaw in fp.FLAWS:
        for kind in FLAW_KINDS[flaw]:
            key = "walker2d_size_2" if kind == "walker2d" else None
            clean = oracle_residuals(kind, key)
            for k, x in oracle_residuals(kind, key, flaw).items():
                if x > 1e3 * max(clean[k], 1e-16):                           # the flaw touches this quantity
                    flawed.setdefault(k, []).append((x, flaw, kind))
    print("jdot_error (reference's own error estimate of everything velocity-dependent): %.1e" % err)
    for k in BOUND:
        lo = min(flawed.get(k, [(np.nan, "-", "-")]))
        print("%-20s residual %.1e   smallest flaw residual %.1e (%s, %s)   bound %.0e" % (k, worst.get(k, np.nan), lo[0], lo[1], lo[2], BOUND[k]))
