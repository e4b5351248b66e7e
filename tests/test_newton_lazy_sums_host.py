"""The Newton solvers compute the line-search sums and the carry of Ma only on the paths that read them (planar_newton.hpp, planar_newton_list.hpp: LAZY):
the same operations on the same values, so the fp32 host build must reproduce, word for word, what the eager code gave.

tests/golden/planar_fp32_bits.npz was recorded from the eager solvers (tests/golden/record_planar_bits.py: seeded reset states,
xi nominal +-20 %, 24 env-steps of random actions, 128 envs per kind; feet-only solver on / off / off with the list solver;
five line-search schedules, of which the default and (1, 4) are lazy in the first four passes of a solve, (3, 24) in every pass,
(3, 2) lazy then searching within one solve, (3, 0) searching throughout).  The harness is plain x86-64 g++ -O2 (no FMA contraction) with
the engine's own sincos_poly, so the bits do not depend on the machine."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import record_planar_bits as rec  # noqa: E402

# env-step length (timestep x frame_skip) and gravity of the three models: a root in free flight falls 0.5 g t^2
DT = {"hopper": 0.008, "walker2d": 0.008, "halfcheetah": 0.05}
GRAVITY = 9.81


@pytest.fixture(scope="module")
def fixture():
    return np.load(rec.PATH)


@pytest.mark.parametrize("kind", rec.KINDS)
def test_fixture_bits_are_reproduced(fixture, kind):
    f = fixture
    qb, vb, capped = rec.replay(kind, f[kind + "_q0"], f[kind + "_v0"], f[kind + "_xi"], f[kind + "_act"])
    want_q, want_v = rec.unpack(f[kind + "_qbits"]), rec.unpack(f[kind + "_vbits"])
    assert qb.shape == want_q.shape == (len(rec.MODES), len(rec.SCHEDULES), rec.N_STEPS // rec.EVERY, rec.N_ENVS, rec.NQ[kind])
    dq, dv = qb != want_q, vb != want_v
    per_case = (dq.sum(axis=(2, 3, 4)) + dv.sum(axis=(2, 3, 4))).tolist()   # [mode][schedule]
    print(kind, "differing words per (mode, schedule):", per_case)
    assert int(dq.sum()) + int(dv.sum()) == 0, (kind, per_case)
    assert capped == 0, (kind, capped)


@pytest.mark.parametrize("kind", rec.KINDS)
def test_fixture_is_not_free_flight(fixture, kind):
    """Per mode, the last recorded step has lanes that the floor held up: without a contact force the centre of mass falls 0.5 g t^2
    whatever the motors do (the root's own offset from it moves by centimetres at most in this time), so a root that has lost less than
    half of that by the last recorded step (0.19 s: 9 cm of 18; the half-cheetah 1.2 s) was standing on something."""
    f = fixture
    z0 = f[kind + "_q0"][:, 1].astype(np.float64)
    q = rec.unpack(f[kind + "_qbits"]).view(np.float32).astype(np.float64)   # [mode, schedule, rec, env, nq]
    for mi in range(len(rec.MODES)):
        t = rec.N_STEPS * DT[kind]
        held = q[mi, 0, -1, :, 1] > z0 - 0.25 * GRAVITY * t * t
        print(kind, rec.MODES[mi], "lanes held up by the floor:", int(held.sum()))
        assert held.any(), (kind, rec.MODES[mi])
