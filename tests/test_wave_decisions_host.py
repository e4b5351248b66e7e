"""The wave-uniform decisions of the Newton solvers (planar_newton.hpp: solve_newton, planar_newton_list.hpp: solve_newton_list, planar_newton_common.hpp: CorrPlan, corr_step) were thinned out:
the correction plan is formed without short circuits and early returns, both ballots of the correction block are taken ahead of the one branch
into it, the pair exchange of its pivot check no longer sits behind a divergent branch, and one place at the end of a pass decides whether
the wave iterates on and only then brings Ma up to date (rebuilt after a correction trip -- the `ma_dirty` test at the top of every pass is
gone -- or carried after a pass that did not search).  Control flow only: every floating-point operation keeps its operands and its order,
so the fp32 host build must reproduce, word for word, what the code before the change gave -- also on the paths forward() dispatches to when
a wave is not on the warm feet-only path, which a later change of that dispatch will have to keep.

tests/golden/planar_decisions_bits.npz was recorded from that earlier code (tests/golden/record_decisions_bits.py: 32 envs per kind with
reset-neighbourhood lanes, lanes 1 m up in free flight, lanes pitched about 1.2 rad at low height that lie down on every capsule, for
the hopper a folded leg whose self pairs pass the cull; 16 env-steps; corr 0 / 1 / 2, warm start off, `fast` off, the list and the rolled
solver, three line-search schedules).  It adds the decisions that tests/golden/planar_fp32_bits.npz (reset neighbourhood, default corr and
warm) never takes the other way."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import record_decisions_bits as rec  # noqa: E402

DT = {"hopper": 0.008, "walker2d": 0.008, "halfcheetah": 0.05}   # env-step length (timestep x frame_skip)
GRAVITY = 9.81
# recorded step at which free flight is judged: the last one (0.128 s, 8 cm of fall); the half-cheetah's first (0.2 s, 20 cm: at its last, 0.8 s, a
# root started 1 m up has landed)
REC_AT = {"hopper": rec.N_STEPS // rec.EVERY - 1, "walker2d": rec.N_STEPS // rec.EVERY - 1, "halfcheetah": 0}


@pytest.fixture(scope="module")
def fixture():
    return np.load(rec.PATH)


@pytest.fixture(scope="module")
def replayed(fixture):
    """every kind replayed once, shared by the tests below"""
    f = fixture
    return {kind: rec.replay(kind, f[kind + "_q0"], f[kind + "_v0"], f[kind + "_xi"], f[kind + "_act"]) for kind in rec.KINDS}


def test_fixture_is_small():
    assert os.path.getsize(rec.PATH) < os.path.getsize(os.path.join(os.path.dirname(rec.PATH), "planar_fp32_bits.npz"))


@pytest.mark.parametrize("kind", rec.KINDS)
def test_fixture_bits_are_reproduced(fixture, replayed, kind):
    f = fixture
    qb, vb, modes, capped = replayed[kind]
    want_q, want_v = rec.unpack(f[kind + "_qbits"]), rec.unpack(f[kind + "_vbits"])
    assert qb.shape == want_q.shape == (len(rec.CASES), rec.N_STEPS // rec.EVERY, rec.N_ENVS, rec.NQ[kind])
    dq, dv = qb != want_q, vb != want_v
    per_case = (dq.sum(axis=(1, 2, 3)) + dv.sum(axis=(1, 2, 3))).tolist()
    print(kind, "differing words per case:", per_case)
    assert int(dq.sum()) + int(dv.sum()) == 0, (kind, per_case)
    assert capped == 0, (kind, capped)
    # the solver instantiation forward() enters at every step's start state is part of the record
    assert np.array_equal(modes, f[kind + "_mode"]), (kind, int((modes != f[kind + "_mode"]).sum()))


@pytest.mark.parametrize("kind", rec.KINDS)
def test_fixture_has_free_flight_and_floor_held_lanes(fixture, kind):
    """A condition on the inputs.  Without a contact force the centre of mass falls 0.5 g t^2 whatever the motors do (the root's own offset
    from it moves by a centimetre or two in this time).  Per case, at the recorded step REC_AT: every lane started 1 m up (zero action: no limb swings)
    is within a quarter of the fall of that parabola: no floor force has acted on it; and of the other lanes some have lost less than half of the free fall
    (the floor held them up)."""
    f = fixture
    z0 = f[kind + "_q0"][:, 1].astype(np.float64)
    q = rec.unpack(f[kind + "_qbits"]).view(np.float32).astype(np.float64)   # [case, rec, env, nq]
    r = REC_AT[kind]
    t = (r + 1) * rec.EVERY * DT[kind]
    fall = 0.5 * GRAVITY * t * t
    ground = np.ones(rec.N_ENVS, bool); ground[rec.FREE] = False
    for ci, case in enumerate(rec.CASES):
        z = q[ci, r, :, 1]
        free = np.abs(z[rec.FREE] - (z0[rec.FREE] - fall)) < 0.25 * fall
        held = z[ground] > z0[ground] - 0.5 * fall
        print(kind, case, "free-flight lanes:", int(free.sum()), "held up by the floor:", int(held.sum()))
        assert free.all(), (kind, case)
        assert held.any(), (kind, case)


@pytest.mark.parametrize("kind", rec.KINDS)
def test_fixture_reaches_every_mode(fixture, kind):
    """the recorded start states enter: no rows (0), the general instantiation (1), the feet-only one (3), and for the hopper the general
    instantiation with self rows (2); with `fast` off nothing enters mode 3"""
    m = fixture[kind + "_mode"]
    for ci, case in enumerate(rec.CASES):
        n = np.bincount(m[ci].ravel(), minlength=4)
        assert n[0] > 0 and n[1] > 0, (kind, case, n)
        assert (n[3] > 0) == (case[0] != 0), (kind, case, n)
        assert (n[2] > 0) == (kind == "hopper"), (kind, case, n)
