"""Collision, constraint rows and the constrained solve against a second, independent reading (tests/contact_reference.py: numpy, an
active-set solve of the dual LCP with its own KKT certificate; nothing shared with oracle/ or the kernels): the fp64 oracle
(oracle/mjo_core.c through the row probe mjo_probe_rows) and the host builds of the device engines (tests/host_harness, fp64 and fp32)
at states WITH contacts and joint limits.

Samples (inputs rounded to fp32; `python tests/test_contact_reference_host.py` prints every figure quoted here):
  planar    box_states(kind, 256, "uniform" | "corners", seed=3) over the whole xi box; walker2d keeps the first 96 of those 256 (every
            walker2d state has its own lengths, hence its own reference model: 96 keep the module's run time down, no class is lost)
  folded    hopper, 512 states with the leg folded against the torso: the capsule-capsule rows
  humanoid  the three generators of tests/test_gpu_humanoid.py (standing, crouched, pile-ups), 128 states each
Every sample is ordered round-robin by class (floor contact only, limit only, both, partly active pyramid, two feet, each capsule-capsule
pair, each humanoid row-count class), so that its first 33 states already hold every class it has: the GPU module steps the first 33 / 65.
One env step is taken from the first N_STEP states of a sample.

MEASURED.  Residual: worst oracle-vs-reference distance over all samples.  Reference error: for geometry the spread between the
candidate enumeration and brute-force sampling of the two segments (41 x 41 points, zoomed 14 times on the best cell), for rows
rounding, for everything behind the solve the reference's KKT certificate.  Flaw: the smallest residual a flaw switch that touches the
quantity produces.  Bound: >= 100x above the first two, >= 100x below the third.

    quantity       residual   reference error             smallest flaw residual         bound
    dist           1.4e-15    6e-16 (segment sampling)    7.2e-2 capsule_ends_only       1e-10
    pos            1.3e-15    rounding                    1.3e-2 contact_on_geom2        1e-10
    normal         8.8e-14    rounding                    1.1    capsule_ends_only       1e-10
    J              2.9e-14    rounding                    2.6e-2 contact_on_geom2        1e-10
    pos - margin   1.4e-15    rounding                    7.2e-2 capsule_ends_only       1e-10
    diagApprox     5.2e-13    rounding                    1.7e-2 invweight_at_q          1e-9    (relative, row by row)
    R              4.4e-12    rounding                    1.7e-2 invweight_at_q          1e-9    (relative, row by row)
    aref           4.4e-13    rounding                    1.3e-3 impedance_no_margin     1e-9
    invweight0     4.6e-14    rounding                    1.7e-2 (seen in diagApprox)    1e-9    (oracle, ph_constants, hh_constants)
    meaninertia    8.9e-16    rounding                    -                              1e-9
    qacc           7.5e-13    1.6e-11 (KKT certificate)   3.5e-3 invweight_at_q          1e-8
    step qpos      2.6e-14    1.6e-11                     9.1e-6 invweight_at_q          1e-8
    step qvel      1.3e-13    1.6e-11                     7.5e-4 invweight_at_q          1e-8
Both halves of the 100x rule hold for every quantity.  Each flaw is shown on the sample where it can show: a margin in the impedance
argument matters only where dmin != dmax and margin != 0 (the humanoid), the tangent rule only off the plane (the humanoid).  The
complementarity residual of the reference is at most 4e-13 (relative); its active-set solve needs at most 8 pivot rounds.  NOTHING
FAILED in the oracle or in the fp64 host engines: contacts, rows in their order, the Newton kinds' minimiser, the humanoid's 50-sweep
PGS iterate and one env step all agree with the second reading.  fp64 host engines: humanoid within the same bounds (qacc 6.4e-14, step
2.4e-15 / 1.3e-14); the planar engines stop their Newton iteration by the model's tolerance of 1e-8 on the scaled gradient, not at
1e-12, and are held to HOST64 = 100x that tolerance (measured: hopper 5.8e-14; half-cheetah qacc 7.7e-9, step 2.4e-9 / 1.2e-8;
walker2d 8.3e-9, 7.2e-11 / 1.4e-9), still 100x under the weakest flaw.

WHAT FAILED, and was fixed: the fp32 planar engine on the folded hopper.  Where two capsule axes CROSS in the plane the two closest
points coincide, and MuJoCo's rule gives the normal (1, 0, 0) when their distance is below 1e-15.  In fp64 the crossing point comes out
1e-17 apart; in fp32 1e-8 apart, so the engine normalised rounding noise: 31 of the first 128 folded states missed the 5e-4 gate with
|dqvel|rel up to 1.4 in every solver form, none explained by the oracle's conditioning.  planar_contacts.hpp::capsule_capsule_2d now
says it geometrically: non-parallel axes in one plane whose stationary point lies inside both segments CROSS there, and the two
closest points are taken as one point (no threshold, no dependence on the crossing angle).  With it the worst folded lane is 3.3e-7 /
3.9e-6 and no lane of any sample needs the explained clause.

Oracle's Newton iteration cap: at tolerance 1e-12 the oracle runs into its 200-iteration cap in about 2 % of walker2d corner states (its
gradient test sits below rounding level there); `test_oracle_iteration_cap_is_not_a_wrong_answer` holds two such states to the qacc
bound and prints the reference's certificate.

Humanoid: the oracle and the engines are held to the reference's 50-sweep PGS iterate, not to the minimiser.  Distance between the two,
|dqacc| / (1 + |qacc|inf), max / median per family (test_humanoid_pgs_distance_to_the_minimiser): standing 4.1e-3 / 6.6e-7, crouched
2.5e-2 / 1.1e-6, pile-ups 2.2e-1 / 1.1e-4; 74, 63 and 100 of 128 states use all 50 sweeps.

Run time: 74 cases, 70 to 130 s on one core, by the machine.

fp32 host builds: the project's per-lane gates (planar |dqpos| 2e-5 and |dqvel|rel 2e-4 with caps 5e-4 / 2e-2; folded hopper 5e-5 /
5e-4; humanoid 2e-4 / 5e-4 with caps 2e-2 / 5e-2 -- the 2e-4 is the project's relative gate on the observation, whose position block is
qpos[2:], applied here to |dqpos| itself, which is the stricter form; crouched and pile-ups qvel 1e-4 with K = 256) on BOTH |dqpos| and
|dqvel|rel through parity_util.assert_lanes_explained.  Worst fp32 figures, |dqpos| / |dqvel|rel over the solver forms: hopper 1.6e-7 /
5.8e-6, folded 3.3e-7 / 3.9e-6; half-cheetah 7.9e-6 / 4.0e-5; walker2d 3.6e-7 / 4.7e-6; humanoid hh_step / hp_step standing 7.3e-7 /
4.0e-6, crouched 6.6e-7 / 1.5e-6, pile-ups 6.6e-7 / 1.4e-6; at most 1 % of the lanes may pass
by the explained clause, whose conditioning estimate is oracle_sensitivity (the comparison itself is against the reference)."""
import ctypes
import functools

import numpy as np
import pytest

import contact_reference as cr
from oracle_bindings import (DIMS, _p, box_states, oracle_batch_step, oracle_constants, oracle_humanoid_step, oracle_rows,
                             oracle_sensitivity)
from parity_util import assert_lanes_explained

PLANAR = ("hopper", "halfcheetah", "walker2d")
N_PLANAR = dict(hopper=256, halfcheetah=256, walker2d=96)
N_FOLDED, N_HUM = 512, 128
N_STEP = {"hopper": 128, "halfcheetah": 128, "walker2d": 66, "folded": 128, "standing": 33, "crouched": 33, "pileup": 66}
SAMPLES = ["%s-%s" % (k, m) for k in PLANAR for m in ("uniform", "corners")] + ["hopper-folded"] + \
          ["humanoid-%s" % f for f in ("standing", "crouched", "pileup")]
NEAR_MARGIN = 1e-9          # a contact this close to its margin may be in one list and not in the other ...
MAX_LEFT_OUT = 0.01         # ... in at most this fraction of a sample's states
MAX_EXPLAINED = 0.01

# fp64 bounds (the table above)
BOUND = dict(dist=1e-10, pos=1e-10, normal=1e-10, J=1e-10, posm=1e-10, diagApprox=1e-9, R=1e-9, aref=1e-9, invweight0=1e-9,
             meaninertia=1e-9, qacc=1e-8, step_qpos=1e-8, step_qvel=1e-8)


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ---- samples ------------------------------------------------------------------------------------------------------------------
def _raw(name):
    from random_envs_amd.specs import SPECS
    kind, fam = name.split("-")
    if fam in ("uniform", "corners"):
        n = N_PLANAR[kind]
        q, v, xi = [x[:n] for x in box_states(kind, 256, fam, seed=3)]
        a = np.random.RandomState(5).uniform(-1.2, 1.2, (256, DIMS[kind]["nu"]))[:n]
    elif fam == "folded":
        n = N_FOLDED; rng = np.random.RandomState(3)
        q = np.zeros((n, 6)); q[:, 0] = rng.uniform(-1, 1, n); q[:, 1] = rng.uniform(0.3, 1.4, n); q[:, 2] = rng.uniform(-1, 1, n)
        q[:, 3:5] = rng.uniform(-2.7, 0.05, (n, 2)); q[:, 5] = rng.uniform(-0.8, 0.8, n)
        v = rng.uniform(-3, 3, (n, 6)); xi = np.array(SPECS["hopper"].nominal_task) * rng.uniform(0.5, 1.5, (n, 4))
        a = rng.uniform(-1.2, 1.2, (n, 3))
    else:
        n = N_HUM; nom = np.array(SPECS["humanoid"].nominal_task)
        q = np.tile(np.array([0, 0, 1.4, 1, 0, 0, 0] + [0] * 17, dtype=float), (n, 1))
        if fam == "standing":                            # tests/test_gpu_humanoid.py::_states
            rng = np.random.RandomState(3)
            q = q + rng.uniform(-.01, .01, (n, 24)); q[:, 7:] += rng.uniform(-.3, .3, (n, 17)); q[:, 2] = rng.uniform(1.0, 1.45, n)
            v = rng.uniform(-1, 1, (n, 23)); a = rng.uniform(-.5, .5, (n, 17)); xi = nom * rng.uniform(.8, 1.2, (n, 30))
        else:                                            # ::test_crouched_states_every_sweep_layout, ::test_pile_up_states_all_solver_paths
            rng = np.random.RandomState(11 if fam == "crouched" else 5)
            spread, zlo, zhi, tilt = (0.9, 0.3, 1.3, 0.5) if fam == "crouched" else (1.2, 0.05, 0.6, 1.0)
            q[:, 7:] += rng.uniform(-spread, spread, (n, 17)); q[:, 2] = rng.uniform(zlo, zhi, n)
            qq = np.array([1, 0, 0, 0]) + rng.uniform(-tilt, tilt, (n, 4)); q[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
            v = rng.uniform(-1, 1, (n, 23)); a = rng.uniform(-.4, .4, (n, 17)); xi = nom * rng.uniform(.9, 1.1, (n, 30))
    return kind, [_f32(x) for x in (q, v, a, xi)]


def ref_forward(kind, q, v, a, xi, flaw=None, solver=None):
    """per-state records of what the reference computes (walker2d: one reference model per set of lengths)"""
    n = len(q); rec = [None] * n
    keys = [cr.walker_table_key(x[7:11]) for x in xi] if kind == "walker2d" else [kind] * n
    for key in dict.fromkeys(keys):
        idx = np.array([i for i in range(n) if keys[i] == key])
        cm = cr.contact_model(key, flaw)
        F = cm.forward(q[idx], v[idx], a[idx], xi[idx], solver)
        r, c = F["rows"], F["contacts"]
        for k, i in enumerate(idx):
            s = slice(F["start"][k], F["start"][k + 1]); cs = c["state"] == k
            rec[i] = dict(J=r["J"][s], posm=(r["pos"] - r["margin"])[s], diagApprox=r["diagApprox"][s], R=r["R"][s], aref=r["aref"][s],
                          type=r["type"][s], contact=r["contact"][s], force=F["force"][s], qacc=F["qacc"][k], cert=F["certificate"][k],
                          comp=F["complementarity"][k], rounds=F["rounds"][k], g=np.stack([c["g1"][cs], c["g2"][cs]], 1),
                          dist=c["dist"][cs], pos=c["pos"][cs], normal=c["frame"][cs][:, 0], condim=c["condim"][cs],
                          margin=c["margin"][cs], gname=cm.gname,
                          pair_margin={(pr["g1"], pr["g2"]): pr["margin"] - pr["gap"] for pr in cm.pairs})
    return rec


def classes(kind, r):
    """the classes one state belongs to, from the reference's own rows"""
    out = set()
    lim, con = (r["type"] == 0).any(), (r["type"] > 0).any()
    floor = r["g"][:, 0] == 0 if len(r["g"]) else np.zeros(0, bool)
    if con and not lim:
        out.add("contact only")
    if lim and not con:
        out.add("limit only")
    if lim and con:
        out.add("both")
    if len(r["force"]) and (r["force"] > 0).any() and (r["force"] == 0).any():
        out.add("partly active")
    if kind != "humanoid" and len(set(r["g"][floor][:, 1])) >= 2:
        out.add("two feet")
    for g1, g2 in r["g"][~floor]:
        out.add("%s-%s" % (r["gname"][g1], r["gname"][g2]) if kind != "humanoid" else "body-body")
    if kind == "humanoid":
        ne = len(r["type"])
        if floor.any():
            out.add("floor")
        out.update(c for c, lo, hi in (("rows 1-16", 1, 16), ("rows 17-21", 17, 21), ("rows 22-64", 22, 64), ("rows > 64", 65, 10 ** 6)) if lo <= ne <= hi)
    return out


def round_robin(cls):
    """order in which the states' classes take turns: every class a sample has is among its first few states"""
    names = sorted(set().union(*cls)); left = list(range(len(cls))); order = []
    while left:
        took = False
        for c in names + [None]:
            for i in left:
                if c is None or c in cls[i]:
                    order.append(i); left.remove(i); took = True
                    break
            if not left:
                break
        assert took
    return np.array(order)


@functools.lru_cache(maxsize=None)
def sample(name):
    kind, (q, v, a, xi) = _raw(name)
    rec = ref_forward(kind, q, v, a, xi, solver="exact" if kind != "humanoid" else None)
    o = round_robin([classes(kind, r) for r in rec])
    out = dict(kind=kind, q=q[o], v=v[o], a=a[o], xi=xi[o])
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, flaw=None, solver=None):
    s = sample(name)
    return ref_forward(s["kind"], s["q"], s["v"], s["a"], s["xi"], flaw, solver)


@functools.lru_cache(maxsize=None)
def oracle(name):
    s = sample(name)                 # the humanoid's PGS stops by the model's own tolerance; the Newton kinds are solved to 1e-12
    return [oracle_rows(s["kind"], s["q"][i], s["v"][i], s["a"][i], s["xi"][i], tolerance=0.0 if s["kind"] == "humanoid" else 1e-12)
            for i in range(len(s["q"]))]


def n_step(name):
    return N_STEP[name.split("-")[1] if name.split("-")[1] not in ("uniform", "corners") else name.split("-")[0]]


@functools.lru_cache(maxsize=None)
def reference_step(name, flaw=None):
    """the reference's env step from the first n_step states of the sample"""
    s = sample(name); n = n_step(name); kind = s["kind"]
    keys = [cr.walker_table_key(x[7:11]) for x in s["xi"][:n]] if kind == "walker2d" else [kind] * n
    qo = np.zeros((n, DIMS[kind]["nq"])); vo = np.zeros((n, DIMS[kind]["nv"]))
    for key in dict.fromkeys(keys):
        idx = np.array([i for i in range(n) if keys[i] == key])
        e = cr.contact_model(key, flaw).env_step(s["q"][idx], s["v"][idx], s["a"][idx], s["xi"][idx], DIMS[kind]["frame_skip"])
        qo[idx] = e["qpos"]; vo[idx] = e["qvel"]
    qo.setflags(write=False); vo.setflags(write=False)
    return dict(qpos=qo, qvel=vo)


def _oracle_step(kind, q, v, a, xi):
    return oracle_humanoid_step(q, v, a, xi) if kind == "humanoid" else oracle_batch_step(kind, q, v, a, xi)


@functools.lru_cache(maxsize=None)
def oracle_step(name):
    """the oracle's env step from the same states, and its sensitivity to fp32-sized input changes (the `explained` clause's estimate)"""
    s = sample(name); n = n_step(name)
    return oracle_sensitivity(lambda *x: _oracle_step(s["kind"], *x), [s[k][:n] for k in ("q", "v", "a", "xi")], ["qpos", "qvel"], trials=2)


# ---- residuals ----------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.abs(a - b).max() / (1 + np.abs(b).max())) if np.size(b) else 0.0


def state_residuals(o, r):
    """oracle record (oracle_rows) against reference record, one state.  None: the two lists differ by a contact within NEAR_MARGIN of
    its margin (left out).  An `inf` entry: they differ otherwise."""
    oc = o["contacts"]
    ok = sorted(range(len(oc)), key=lambda i: (oc[i, 0], oc[i, 1])); rk = sorted(range(len(r["g"])), key=lambda i: tuple(r["g"][i]))
    og = [(int(oc[i, 0]), int(oc[i, 1])) for i in ok]; rg = [tuple(int(x) for x in r["g"][i]) for i in rk]
    if og != rg:                  # only the contacts that are in one list and not in the other are looked at, each against its pair's margin
        from collections import Counter
        extra_o, extra_r = Counter(og) - Counter(rg), Counter(rg) - Counter(og)
        near = []
        for extra, keys, dist in ((extra_o, og, oc[ok, 2]), (extra_r, rg, r["dist"][rk])):
            for g, cnt in extra.items():            # (two ends of one capsule share a pair: the `cnt` nearest to the margin are the candidates)
                d = sorted(abs(x - r["pair_margin"][g]) for k, x in zip(keys, dist) if k == g)[:cnt]
                near += [x < NEAR_MARGIN for x in d]
        return None if near and all(near) else dict(contacts=np.inf)
    out = {}
    if len(og):
        out = dict(dist=float(np.abs(oc[ok, 2] - r["dist"][rk]).max()), pos=float(np.abs(oc[ok, 3:6] - r["pos"][rk]).max()),
                   normal=float(np.abs(oc[ok, 6:9] - r["normal"][rk]).max()))
        if not np.array_equal(oc[ok, 9], r["condim"][rk]):
            out["contacts"] = np.inf
    if o["nefc"] != len(r["type"]) or not np.array_equal(o["efc_type"], r["type"]):
        out["rows"] = np.inf
        return out
    if o["nefc"]:
        out.update(J=float(np.abs(o["efc_J"] - r["J"]).max()), posm=float(np.abs(o["efc_pos"] - o["efc_margin"] - r["posm"]).max()),
                   diagApprox=float(np.abs(o["efc_diagApprox"] / r["diagApprox"] - 1).max()), R=float(np.abs(o["efc_R"] / r["R"] - 1).max()),
                   aref=_rel(o["efc_aref"], r["aref"]))
    out["qacc"] = _rel(o["qacc"], r["qacc"])
    return out


def sample_residuals(name, flaw=None, solver=None):
    """(worst residual per quantity over the sample, fraction of states left out)"""
    worst, left = {}, 0
    for o, r in zip(oracle(name), reference(name, flaw, solver)):
        x = state_residuals(o, r)
        if x is None:
            left += 1
            continue
        for k, e in x.items():
            worst[k] = max(worst.get(k, 0.0), e)
    return worst, left / len(oracle(name))


def step_residuals(name, flaw=None):
    ref, (orc, _) = reference_step(name, flaw), oracle_step(name)
    ok = np.isfinite(orc["qvel"]).all(1) & np.isfinite(orc["qpos"]).all(1)
    assert ok.mean() >= 0.9, (name, "the oracle's step is finite in only %.0f %% of the lanes" % (100 * ok.mean()))
    return dict(step_qpos=float(np.abs(orc["qpos"] - ref["qpos"])[ok].max()),
                step_qvel=float((np.abs(orc["qvel"] - ref["qvel"]).max(1) / (1 + np.abs(ref["qvel"]).max(1)))[ok].max()))


def _check(r, bounds, tag):
    print("%s: %s" % (tag, "  ".join("%s %.2e" % kv for kv in sorted(r.items()))))
    over = {k: (x, bounds.get(k, 0.0)) for k, x in r.items() if not x <= bounds.get(k, 0.0)}
    assert not over, (tag, over)


# ---- the reference's own tests ------------------------------------------------------------------------------------------------
def geometry_spread(n=48):
    """the enumeration's closest distance against brute-force sampling of the two segments, on the folded hopper's capsule pairs"""
    s = sample("hopper-folded"); cm = cr.contact_model("hopper")
    kin = cm.m.kinematics(s["q"][:n]); worst = 0.0; below = 0.0
    for pr in cm.pairs:
        if cm.gtype[pr["g1"]] != 3:
            continue
        c1, a1, l1 = cm._capsule(kin, pr["g1"]); c2, a2, l2 = cm._capsule(kin, pr["g2"])
        ss, tt, _ = cr.segment_closest(c1, a1, l1, c2, a2, l2)
        d = np.linalg.norm(c1 + ss[:, None] * a1 - c2 - tt[:, None] * a2, axis=1)
        for i in range(n):
            b = cr.segment_distance_brute(c1[i], a1[i], l1[i], c2[i], a2[i], l2[i])
            worst = max(worst, b - d[i]); below = max(below, d[i] - b)
    return worst, below


def test_reference_segment_enumeration_against_brute_force():
    """the sampled minimum (41 x 41 points, zoomed 14 times on the best cell) can only lie above the true one; the enumeration must never
    lie above the sampled minimum by more than rounding"""
    above, below = geometry_spread()
    print("segment-segment: brute-force minimum above the enumeration by at most %.2e, below it by at most %.2e" % (above, below))
    assert below <= 1e-14 and above * 100 <= BOUND["dist"]


@pytest.mark.parametrize("name", SAMPLES)
def test_reference_certificate(name):
    """the reference's own error estimate of everything behind the solve: its KKT certificate and complementarity residual"""
    ref = reference(name, solver="exact")
    cert = max(r["cert"] for r in ref); comp = max(r["comp"] for r in ref); rounds = max(r["rounds"] for r in ref)
    print("%s: certificate %.2e, complementarity %.2e, at most %d pivot rounds" % (name, cert, comp, rounds))
    assert cert * 100 <= BOUND["qacc"] and comp * 100 <= BOUND["qacc"]


# ---- coverage conditions (the reference's own counts) -------------------------------------------------------------------------
def _frac(name, pred):
    ref = reference(name)
    return float(np.mean([bool(pred(r)) for r in ref]))


@pytest.mark.parametrize("name", [s for s in SAMPLES if s.split("-")[1] in ("uniform", "corners")])
def test_planar_samples_cover_contacts_limits_and_partial_pyramids(name):
    kind = sample(name)["kind"]
    con = _frac(name, lambda r: (r["type"] > 0).any()); lim = _frac(name, lambda r: (r["type"] == 0).any())
    part = _frac(name, lambda r: "partly active" in classes(kind, r))
    print("%s: contact row in %.0f %%, limit row in %.0f %%, partly active in %.0f %% of the states" % (name, 100 * con, 100 * lim, 100 * part))
    assert con >= 0.30 and lim >= 0.15 and part >= 0.10
    first = set().union(*[classes(kind, r) for r in reference(name)[:33]])
    assert first == set().union(*[classes(kind, r) for r in reference(name)]), "the first 33 states hold every class"


def test_folded_sample_covers_every_capsule_capsule_pair():
    ref = reference("hopper-folded")
    cc = _frac("hopper-folded", lambda r: (r["g"][:, 0] > 0).any())
    pairs = {}
    for r in ref:
        for g1, g2 in r["g"][r["g"][:, 0] > 0]:
            pairs[(r["gname"][g1], r["gname"][g2])] = pairs.get((r["gname"][g1], r["gname"][g2]), 0) + 1
    print("folded hopper: capsule-capsule contact in %.0f %% of the states, per pair %s" % (100 * cc, pairs))
    assert cc >= 0.10 and len(pairs) == 3
    assert {c for r in ref[:33] for c in classes("hopper", r)} >= {"%s-%s" % p for p in pairs}


def test_humanoid_pile_ups_cover_every_row_count_class():
    ref = reference("humanoid-pileup")
    con = _frac("humanoid-pileup", lambda r: len(r["g"]) > 0)
    ne = np.array([len(r["type"]) for r in ref])
    print("humanoid pile-ups: contact in %.0f %% of the states, rows max %d median %d" % (100 * con, ne.max(), np.median(ne)))
    assert con >= 0.80
    assert any((r["condim"] == 3).any() for r in ref) and any((r["condim"] == 1).any() for r in ref)
    want = {"rows 1-16", "rows 17-21", "rows 22-64", "rows > 64", "floor", "body-body"}
    assert {c for r in ref[:33] for c in classes("humanoid", r)} >= want


# ---- constants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PLANAR + ("humanoid",))
def test_invweight0_and_meaninertia(kind):
    """from their definition at qpos0 with the reference's own M, against the oracle's compile step, ph_constants and hh_constants"""
    import first_principles_oracle as fp
    from host_harness.build import build_so, host_constants
    keys = sorted(fp.walker_sizes()) if kind == "walker2d" else [kind]
    for key in keys:
        size = fp.walker_sizes()[key] if kind == "walker2d" else None
        c = cr.contact_model(key).constants(); oc = oracle_constants(kind, size=size)
        r = dict(invweight0=max(float(np.abs(oc["body_invweight0"][1:] / c["body_invweight0"][1:] - 1).max()),
                                float(np.abs(oc["dof_invweight0"] / c["dof_invweight0"] - 1).max())))
        if kind != "walker2d":                            # (the row probe reports the meaninertia of the model it built)
            r["meaninertia"] = abs(oracle("humanoid-standing" if kind == "humanoid" else kind + "-uniform")[0]["meaninertia"] / c["meaninertia"] - 1)
        if kind != "humanoid":
            for f32 in (False, True):
                h = host_constants(kind, f32, size=size)
                e = dict(invweight0=max(float(np.abs(h["tran_invw"] / c["body_invweight0"][1:, 0] - 1).max()),
                                        float(np.abs(h["dof_invw"][1:] / c["dof_invweight0"][3:] - 1).max())),
                         meaninertia=abs(h["meaninertia"] / c["meaninertia"] - 1))
                cm = cr.contact_model(key); tc = max(0.02, 2 * cm.m.timestep)
                dmax = cm.pairs[0]["solimp"][1]; dl = cm.limits[0][5][1]
                e["sol"] = max(abs(h["con_K"] * (dmax * tc) ** 2 - 1), abs(h["con_B"] * dmax * tc / 2 - 1), abs(h["lim_K"] * (dl * tc) ** 2 - 1),
                               abs(h["lim_B"] * dl * tc / 2 - 1))
                _check(e, dict(invweight0=2e-5, meaninertia=2e-5, sol=2e-5) if f32 else dict(BOUND, sol=1e-9), "%s ph_constants %s" % (key, "fp32" if f32 else "fp64"))
        else:
            hh = ctypes.CDLL(build_so("humanoid_host", "humanoid_host.cpp"))
            mass = np.zeros(14); ib = np.zeros(28); idf = np.zeros(23); ipos = np.zeros(42); inr = np.zeros(84); npair = ctypes.c_int()
            hh.hh_constants(_p(mass), _p(ib), _p(idf), _p(ipos), _p(inr), ctypes.byref(npair))
            e = dict(invweight0=max(float(np.abs(ib.reshape(14, 2)[1:] / c["body_invweight0"][1:] - 1).max()), float(np.abs(idf / c["dof_invweight0"] - 1).max())))
            assert npair.value == len(cr.contact_model(key).pairs), (npair.value, len(cr.contact_model(key).pairs))
            _check(e, BOUND, "humanoid hh_constants")
        _check(r, BOUND, "%s oracle constants" % key)


# ---- oracle vs reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SAMPLES)
def test_oracle_contacts_and_rows_match_the_reference(name):
    """contacts by geom pair, rows in order (their order is a convention only PGS depends on, and it matches); the oracle's qacc against
    the minimiser (Newton kinds) or the 50-sweep PGS iterate (humanoid)"""
    r, left = sample_residuals(name)
    print("%s: %.1f %% of the states left out (a contact within %.0e of its margin)" % (name, 100 * left, NEAR_MARGIN))
    assert left <= MAX_LEFT_OUT
    _check(r, BOUND, "oracle rows %s" % name)
    capped = [i for i, o in enumerate(oracle(name)) if o["solver_iter"] >= 200]
    if capped:
        ref = reference(name)
        print("  the oracle's Newton hit its 200-iteration cap in states %s; reference certificate there %.2e, |dqacc| rel %.2e"
              % (capped, max(ref[i]["cert"] for i in capped), max(_rel(oracle(name)[i]["qacc"], ref[i]["qacc"]) for i in capped)))


def test_oracle_iteration_cap_is_not_a_wrong_answer():
    """lanes 26 and 77 of box_states("walker2d", 128, "corners", seed=3): the oracle's Newton runs its 200 iterations at tolerance 1e-12
    and still returns the minimiser"""
    q, v, xi = [_f32(x) for x in box_states("walker2d", 128, "corners", seed=3)]
    for i in (26, 77):
        o = oracle_rows("walker2d", q[i], v[i], np.zeros(6), xi[i], tolerance=1e-12)
        r = ref_forward("walker2d", q[i:i + 1], v[i:i + 1], np.zeros((1, 6)), xi[i:i + 1])[0]
        e = _rel(o["qacc"], r["qacc"])
        print("lane %d: oracle iterations %d, |dqacc| rel %.2e, reference certificate %.2e" % (i, o["solver_iter"], e, r["cert"]))
        assert e <= BOUND["qacc"] and r["cert"] * 100 <= BOUND["qacc"]


@pytest.mark.parametrize("name", SAMPLES)
def test_oracle_env_step_matches_the_reference(name):
    _check(step_residuals(name), BOUND, "oracle step %s (%d states)" % (name, n_step(name)))


@pytest.mark.parametrize("fam", ["standing", "crouched", "pileup"])
def test_humanoid_pgs_distance_to_the_minimiser(fam):
    """humanoid.xml asks for PGS capped at 50 sweeps: its contact dynamics are defined by that algorithm, not by the minimiser"""
    name = "humanoid-" + fam
    pg, ex = reference(name), reference(name, solver="exact")
    d = np.array([_rel(p["qacc"], e["qacc"]) for p, e in zip(pg, ex)]); sweeps = np.array([p["rounds"] for p in pg])
    print("%s: 50-sweep PGS vs the minimiser, |dqacc| / (1 + |qacc|inf): max %.2e median %.2e; %d of %d states use all 50 sweeps"
          % (name, d.max(), np.median(d), int((sweeps >= 50).sum()), len(d)))
    assert np.isfinite(d).all()
    if fam == "pileup":
        assert d.max() > 100 * BOUND["qacc"], "the two targets are told apart"


# ---- misreadings --------------------------------------------------------------------------------------------------------------
# where each flaw shows: (sample, quantities it has to move); the rest of the samples is not looked at
FLAW_SAMPLES = dict(contact_on_geom2=("hopper-uniform", ("pos", "J")), impedance_no_margin=("humanoid-standing", ("R", "aref")),
                    no_pyramid_2mu2=("hopper-uniform", ("R",)), diag_rot_for_slide=("halfcheetah-uniform", ("diagApprox", "R")),
                    aref_no_damping=("hopper-uniform", ("aref",)), limit_sign=("hopper-uniform", ("J",)),
                    capsule_ends_only=("hopper-folded", ("dist", "contacts", "rows")), tangent_default=("humanoid-pileup", ("J",)),
                    invweight_at_q=("hopper-uniform", ("diagApprox", "R")), pgs_warm=("humanoid-pileup", ("qacc",)))
assert set(FLAW_SAMPLES) == set(cr.FLAWS)


def flaw_residuals(flaw):
    name, keys = FLAW_SAMPLES[flaw]
    r, _ = sample_residuals(name, flaw)
    return name, {k: r.get(k, 0.0) for k in keys}, r


@pytest.mark.parametrize("flaw", cr.FLAWS)
def test_every_flaw_fails_the_oracle_comparison(flaw):
    """each named misreading, switched on in the reference, misses the oracle by >= 100x the bound of a quantity it touches"""
    name, r, full = flaw_residuals(flaw)
    worst = max(r, key=lambda k: r[k] / BOUND.get(k, 1.0))
    print("%s on %s: %s off by %.2e = %.0fx its bound; qacc off by %.2e" % (flaw, name, worst, r[worst], r[worst] / BOUND.get(worst, 1.0), full.get("qacc", np.nan)))
    assert r[worst] >= 100 * BOUND.get(worst, 1.0), (flaw, r)


# ---- host builds of the device engines ----------------------------------------------------------------------------------------
I32 = ctypes.POINTER(ctypes.c_int); UB = ctypes.POINTER(ctypes.c_ubyte)
FORMS = {"hopper": [(1, 0), (0, 0), (0, 2), (0, 1)], "halfcheetah": [(1, 0), (0, 0), (0, 2)], "walker2d": [(1, 0), (0, 0), (0, 2)]}     # tests/test_planar_box_host.py
PLANAR_SAMPLES = [s for s in SAMPLES if not s.startswith("humanoid")]
# per-lane fp32 gates of each state family: (tol qpos, cap qpos, tol qvel rel, cap qvel rel, K)
GATES = {"uniform": (2e-5, 5e-4, 2e-4, 2e-2, 64.0), "corners": (2e-5, 5e-4, 2e-4, 2e-2, 64.0), "folded": (5e-5, 5e-4, 5e-4, 2e-2, 64.0),
         "standing": (2e-4, 2e-2, 5e-4, 5e-2, 64.0), "crouched": (2e-4, 2e-2, 1e-4, 5e-1, 256.0), "pileup": (2e-4, 2e-2, 1e-4, 5e-1, 256.0)}
# fp64 engine builds stop their Newton iteration by the model's tolerance (1e-8 on the scaled gradient), not at 1e-12: see HOST64 below
HOST64 = dict(qacc=1e-6, step_qpos=1e-8, step_qvel=1e-6)


def gate_lanes(name, qpos, qvel, label, idx=None):
    """the family's per-lane gates against the REFERENCE's step (lane i holds state idx[i] of the sample; default: the first n_step
    states in order); returns (worst |dqpos|, worst |dqvel|rel, lanes that passed as explained)"""
    ref, (orc, sens) = reference_step(name), oracle_step(name)
    idx = np.arange(len(ref["qpos"])) if idx is None else np.asarray(idx)
    tq, cq, tv, cv, K = GATES[name.split("-")[1]]
    ok = np.isfinite(ref["qvel"][idx]).all(1) & np.isfinite(orc["qvel"][idx]).all(1)
    assert ok.mean() >= 0.9, (label, ok.mean())
    vs = 1 + np.abs(ref["qvel"][idx]).max(1)
    ev = np.abs(qvel - ref["qvel"][idx]).max(1) / vs
    eq = np.abs(qpos - ref["qpos"][idx]).max(1)
    print("%s: worst |dqpos| %.2e, worst |dqvel|rel %.2e over %d lanes" % (label, eq[ok].max(), ev[ok].max(), int(ok.sum())))
    assert_lanes_explained(ev[ok], (sens["qvel"][idx] / vs)[ok], tv, cv, K=K, label=label + " |dqvel|rel")
    assert_lanes_explained(eq[ok], sens["qpos"][idx][ok], tq, cq, K=K, label=label + " |dqpos|")
    over = (ev > tv) | (eq > tq)
    explained = int(over[ok].sum())
    assert explained <= MAX_EXPLAINED * len(idx), (label, explained, len(idx))
    return float(eq[ok].max()), float(ev[ok].max()), explained


@pytest.mark.parametrize("name", PLANAR_SAMPLES)
def test_planar_host_engine_fp64_matches_the_reference(name):
    """ph_forward and ph_step (planar_engine.hpp for the host, fp64) in every form of the solver"""
    from host_harness.build import host_forward, host_step, set_fast, set_rolled
    s = sample(name); kind = s["kind"]; ref = reference(name); n = n_step(name); st = reference_step(name)
    for fast, rolled in FORMS[kind]:
        set_fast(fast); set_rolled(rolled)
        try:
            qa = np.array([host_forward(kind, False, s["q"][i], s["v"][i], s["a"][i], s["xi"][i])[0] for i in range(len(ref))])
            qo, vo, cap = host_step(kind, False, s["q"][:n], s["v"][:n], s["a"][:n], s["xi"][:n], DIMS[kind]["frame_skip"])
        finally:
            set_fast(1); set_rolled(0)
        assert cap.sum() == 0
        r = dict(qacc=max(_rel(qa[i], ref[i]["qacc"]) for i in range(len(ref))), step_qpos=float(np.abs(qo - st["qpos"]).max()),
                 step_qvel=float((np.abs(vo - st["qvel"]).max(1) / (1 + np.abs(st["qvel"]).max(1))).max()))
        _check(r, HOST64, "planar host fp64 %s fast=%d rolled=%d" % (name, fast, rolled))


@pytest.mark.parametrize("name", PLANAR_SAMPLES)
def test_planar_host_engine_fp32_within_the_per_lane_gates(name):
    from host_harness.build import host_step, set_fast, set_rolled
    s = sample(name); kind = s["kind"]; n = n_step(name)
    for fast, rolled in FORMS[kind]:
        set_fast(fast); set_rolled(rolled)
        try:
            qo, vo, cap = host_step(kind, True, s["q"][:n], s["v"][:n], s["a"][:n], s["xi"][:n], DIMS[kind]["frame_skip"])
        finally:
            set_fast(1); set_rolled(0)
        assert cap.sum() == 0
        gate_lanes(name, qo, vo, "planar host fp32 %s fast=%d rolled=%d" % (name, fast, rolled))


def _hum_step(lib, fn, f32, s, n):
    qs, vs, as_, xs = [np.ascontiguousarray(s[k][:n].T) for k in ("q", "v", "a", "xi")]
    qo = np.zeros_like(qs); vo = np.zeros_like(vs); obs = np.zeros((376, n)); r = np.zeros(n); d = np.zeros(n, dtype=np.uint8)
    xo = np.zeros((14, n)); ov = np.zeros(n, dtype=np.int32); nr = np.zeros(n, dtype=np.int32)
    args = [f32, n, _p(qs), _p(vs), _p(as_), _p(xs), None, _p(qo), _p(vo), _p(obs), _p(r), d.ctypes.data_as(UB), _p(xo), ov.ctypes.data_as(I32)]
    if fn == "hp_step":
        args.append(nr.ctypes.data_as(I32))
    assert getattr(lib, fn)(*args) == 0 and ov.sum() == 0
    return qo.T.copy(), vo.T.copy()


@pytest.mark.parametrize("fam", ["standing", "crouched", "pileup"])
def test_humanoid_host_engines_match_the_reference(fam):
    """hh_forward (qacc against the 50-sweep PGS iterate), hh_contacts (bodies, distance, dim, height of the contact point), hh_step and
    hp_step in fp64; the fp32 builds of the two steps within the family's per-lane gates"""
    from host_harness.build import build_so
    hh = ctypes.CDLL(build_so("humanoid_host", "humanoid_host.cpp"))
    hp = ctypes.CDLL(build_so("humanoid_pair_host", "humanoid_pair_host.cpp", ["-pthread"]))
    name = "humanoid-" + fam; s = sample(name); ref = reference(name); n = n_step(name); st = reference_step(name)
    cm = cr.contact_model("humanoid"); worst = dict(qacc=0.0, dist=0.0, pos=0.0); left = 0
    hmargin = cm.pairs[0]["margin"] - cm.pairs[0]["gap"]
    assert all(pr["margin"] - pr["gap"] == hmargin for pr in cm.pairs)     # (one margin for every pair of this model)
    for i, r in enumerate(ref):
        qa = np.zeros(23); M = np.zeros((23, 23)); info = np.zeros(4, dtype=np.int32); con = np.zeros(5 * 96)
        hh.hh_forward(0, _p(s["q"][i]), _p(s["v"][i]), _p(s["a"][i]), _p(s["xi"][i]), _p(qa), _p(M), info.ctypes.data_as(I32))
        nc = hh.hh_contacts(_p(con), 96); con = con.reshape(96, 5)[:nc]
        con = con[con[:, 2] < hmargin]                                    # (the engine lists what is within the margin)
        if nc != len(r["g"]) and len(con) != len(r["g"]):
            near = any(abs(d - m) < NEAR_MARGIN for d, m in zip(r["dist"], r["margin"])) or any(abs(c[2] - hmargin) < NEAR_MARGIN for c in con)
            assert near, (i, nc, len(r["g"]))
            left += 1
            continue
        b = np.sort(np.array(cm.gbody)[r["g"]], axis=1)
        key_r = sorted(range(len(b)), key=lambda k: (b[k, 0], b[k, 1], r["dist"][k]))
        key_h = sorted(range(len(con)), key=lambda k: (min(con[k, 0], con[k, 1]), max(con[k, 0], con[k, 1]), con[k, 2]))
        if len(con):
            hb = np.sort(con[key_h][:, :2], axis=1)
            assert np.array_equal(hb, b[key_r]) and np.array_equal(con[key_h][:, 3], r["condim"][key_r]), i
            worst["dist"] = max(worst["dist"], float(np.abs(con[key_h][:, 2] - r["dist"][key_r]).max()))
            worst["pos"] = max(worst["pos"], float(np.abs(con[key_h][:, 4] - r["pos"][key_r][:, 2]).max()))
        worst["qacc"] = max(worst["qacc"], _rel(qa, r["qacc"]))
    assert left <= MAX_LEFT_OUT * len(ref)
    _check(worst, BOUND, "humanoid host fp64 %s hh_forward / hh_contacts" % fam)
    for lib, fn in ((hh, "hh_step"), (hp, "hp_step")):
        qo, vo = _hum_step(lib, fn, 0, s, n)
        ok = np.isfinite(st["qvel"]).all(1)
        r = dict(step_qpos=float(np.abs(qo - st["qpos"])[ok].max()), step_qvel=float((np.abs(vo - st["qvel"]).max(1) / (1 + np.abs(st["qvel"]).max(1)))[ok].max()))
        _check(r, BOUND, "humanoid host fp64 %s %s" % (fam, fn))
        qo, vo = _hum_step(lib, fn, 1, s, n)
        gate_lanes(name, qo, vo, "humanoid host fp32 %s %s" % (fam, fn))


# ---- the table of the module header -------------------------------------------------------------------------------------------
if __name__ == "__main__":
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t0 = time.time(); worst, cert, flawed = {}, 0.0, {}
    for name in SAMPLES:
        r, left = sample_residuals(name); r.update(step_residuals(name))
        cert = max(cert, max(x["cert"] for x in reference(name, solver="exact")))
        for k, x in r.items():
            worst[k] = max(worst.get(k, 0.0), x)
        print(name, "left out %.3f" % left, {k: "%.1e" % x for k, x in r.items()})
    for flaw in cr.FLAWS:
        name, r, full = flaw_residuals(flaw); clean, _ = sample_residuals(name)
        for k, x in full.items():
            if x > 1e3 * max(clean.get(k, 0.0), 1e-16):
                flawed.setdefault(k, []).append((x, flaw, name))
        print(flaw, name, {k: "%.1e" % x for k, x in full.items()})
    print("certificate %.1e, geometry spread (above, below) %s" % (cert, geometry_spread()))
    for k in BOUND:
        lo = min(flawed.get(k, [(np.nan, "-", "-")]))
        print("%-12s residual %.1e   smallest flaw residual %.1e (%s, %s)   bound %.0e" % (k, worst.get(k, np.nan), lo[0], lo[1], lo[2], BOUND[k]))
    print("%.0f s" % (time.time() - t0))
