"""Self-consistency of the fp64 physics oracle (oracle/mjo_core.c): recalled public model constants, conservation laws and force
balance.  What the oracle computes for the SMOOTH dynamics -- body masses, COMs and inertia tensors, M(q), the bias, passive and
actuator forces, unconstrained integration, the humanoid's cinert / cvel -- is pinned independently of its author by
tests/test_first_principles_host.py (a numpy restatement of rigid-body mechanics from the rendered MJCF tables).  What stays pinned
to the oracle alone, MuJoCo being absent and the reference holding no numeric tests: collision, the constraint rows and the solvers,
and the 2.1.0 compiler's split of a capsule's mass between cylinder and caps."""
import numpy as np
import pytest

from oracle_bindings import (oracle_batch_step, oracle_constants, oracle_energy_drift, oracle_forward)
from random_envs_amd.specs import SPECS


def test_compiled_masses_match_public_mujoco_py_constants():
    """body_mass of the mujoco-py-era gym models (recalled public constants)."""
    hop = oracle_constants("hopper")
    assert np.allclose(hop["body_mass"][1:], [3.53429174, 3.92699082, 2.71433605, 5.0893801], atol=5e-9)
    che = oracle_constants("halfcheetah")
    assert np.allclose(che["body_mass"][1:], [6.36031332, 1.53524804, 1.58093995, 1.0691906, 1.42558747,
                                              1.17885117, 0.84986945], atol=5e-9)
    assert abs(che["body_mass"].sum() - 14.0) < 1e-12          # settotalmass, half_cheetah.xml:54
    wal = oracle_constants("walker2d")
    assert np.allclose(wal["body_mass"][1:], [3.53429174, 3.92699082, 2.71433605, 2.94053072] + [3.92699082, 2.71433605, 2.94053072], atol=5e-9)
    for k in ("hopper", "halfcheetah", "walker2d"):
        assert np.allclose(oracle_constants(k)["body_mass"][1:], SPECS[k].nominal_task[:len(oracle_constants(k)["body_mass"]) - 1], rtol=1e-12)


def test_model_dimensions():
    assert [oracle_constants("hopper")[k] for k in ("nbody", "nq", "nv", "ngeom", "nu", "npair")] == [5, 6, 6, 5, 3, 7]
    assert [oracle_constants("walker2d")[k] for k in ("nbody", "nq", "nv", "ngeom", "nu", "npair")] == [8, 9, 9, 8, 6, 7]
    assert [oracle_constants("halfcheetah")[k] for k in ("nbody", "nq", "nv", "ngeom", "nu", "npair")] == [8, 9, 9, 9, 6, 8]
    assert list(oracle_constants("hopper")["qpos0"]) == [0, 1.25, 0, 0, 0, 0]


# the humanoid's row: airborne and spinning (random root orientation, root spin and joint rates up to 2 rad/s); measured drift over 100
# steps 3.8e-8, 4.1e-8 and 7.0e-7 relative (joint springs kept).  Its root quaternion is advanced by the weighted sum of the RK4 stage
# rotation vectors (mj_RungeKutta), which is second order in the step for a body whose spin axis moves.  tests/test_humanoid_host.py holds the same drift to 1e-6 at
# rates up to 1 rad/s; a second-order term grows with the square of the rates, so at 2 rad/s the bound is 4e-6, rounded up to 5e-6.
@pytest.mark.parametrize("kind,nq,tol", [("hopper", 6, 1e-11), ("walker2d", 9, 1e-9), ("halfcheetah", 9, 1e-3), ("humanoid", 24, 5e-6)])
def test_energy_conservation(kind, nq, tol):
    """M(q) and c(q,v) are consistent: a conservative copy of the model keeps KE+PE under RK4."""
    rng = np.random.RandomState(0)
    for _ in range(3):
        if kind == "humanoid":
            q = np.array([0, 0, 3.0, 1, 0, 0, 0] + [0] * 17, dtype=float); q[7:] += rng.uniform(-.5, .5, 17)
            qq = rng.randn(4); q[3:7] = qq / np.linalg.norm(qq); v = rng.uniform(-2, 2, 23)
        else:
            q = rng.uniform(-.5, .5, nq); q[1] += 3; v = rng.uniform(-2, 2, nq)
        e0, e1 = oracle_energy_drift(kind, 100, q, v)
        print("%s: relative energy drift over 100 steps %.1e" % (kind, (e1 - e0) / abs(e0)))
        assert abs(e1 - e0) <= tol * abs(e0)
    if kind == "halfcheetah":   # the residual there is RK4 truncation on the stiff joint springs
        e0, e1 = oracle_energy_drift(kind, 100, q, v, keep_springs=False)
        assert abs(e1 - e0) <= 1e-8 * abs(e0)


def test_free_fall_and_weight_balance():
    xi = np.array(SPECS["hopper"].nominal_task)
    out = oracle_forward("hopper", [0, 1.25, 0, 0, 0, 0], np.zeros(6), np.zeros(3), xi)
    assert out["ncon"] == 0 and np.allclose(out["qacc"], [0, -9.81, 0, 0, 0, 0], atol=1e-12)
    # half-cheetah dropped from qpos0 settles on both feet: contact forces carry the weight
    xi = np.array(SPECS["halfcheetah"].nominal_task)
    q = np.zeros((1, 9)); v = np.zeros((1, 9))
    for _ in range(80):
        o = oracle_batch_step("halfcheetah", q, v, np.zeros((1, 6)), xi[None], nthreads=1, tolerance=0.0)
        q, v = o["qpos"], o["qvel"]
    f = oracle_forward("halfcheetah", q[0], v[0], np.zeros(6), xi)
    assert abs(f["force"].sum() - 14 * 9.81) < 0.05 and np.abs(v).max() < 1e-3


def test_xi_changes_mass_not_inertia():
    """set_task writes body_mass only.  Doubling every mass with gravity-free,
    contact-free state must NOT simply halve accelerations (inertia stays nominal)."""
    xi = np.array(SPECS["hopper"].nominal_task)
    q = [0, 3.0, 0.1, -0.3, -0.2, 0.1]; v = np.zeros(6); a = np.array([1.0, -0.5, 0.3])
    a1 = oracle_forward("hopper", q, v, a, xi)["qacc"]; a2 = oracle_forward("hopper", q, v, a, 2 * xi)["qacc"]
    M1 = oracle_forward("hopper", q, v, a, xi)["M"]; M2 = oracle_forward("hopper", q, v, a, 2 * xi)["M"]
    assert not np.allclose(M2, 2 * M1) and np.allclose(M2[0, 0], 2 * M1[0, 0])
    assert not np.allclose(a2[3:], a1[3:] / 2, rtol=1e-3)


def test_unmodeled_variants_oracle_semantics():
    """Unmodeled ids: frozen 0.8x prefix, reduced task; Walker2d loses the 0.8x mass
    scaling at the first set_task because the model is rebuilt."""
    import ctypes
    from oracle_bindings import lib, KINDS, _p
    L = lib()
    from random_envs_amd.specs import SPECS, UNMODELED_SPECS
    rng = np.random.RandomState(0)
    # hopper: stepping the unmodeled env with xi_r == stepping the regular env with [0.8*m0, xi_r]
    q = rng.uniform(-.01, .01, (8, 6)); q[:, 1] += 1.25; v = rng.uniform(-.5, .5, (8, 6)); a = rng.uniform(-1, 1, (8, 3))
    xr = np.array(UNMODELED_SPECS["hopper"].nominal_task) * rng.uniform(.8, 1.2, (8, 3))
    full = np.concatenate([np.full((8, 1), 0.8 * SPECS["hopper"].nominal_task[0]), xr], 1)
    o1 = oracle_batch_step("hopper", q, v, a, xr, variant=1); o0 = oracle_batch_step("hopper", q, v, a, full)
    assert np.allclose(o1["qvel"], o0["qvel"], rtol=1e-12, atol=1e-12)
    # cheetah
    q = rng.uniform(-.1, .1, (8, 9)); v = rng.uniform(-.5, .5, (8, 9)); a = rng.uniform(-1, 1, (8, 6))
    xr = np.array(UNMODELED_SPECS["halfcheetah"].nominal_task) * rng.uniform(.8, 1.2, (8, 5))
    full = np.concatenate([np.tile(0.8 * np.array(SPECS["halfcheetah"].nominal_task[:3]), (8, 1)), xr], 1)
    o1 = oracle_batch_step("halfcheetah", q, v, a, xr, variant=1); o0 = oracle_batch_step("halfcheetah", q, v, a, full)
    assert np.allclose(o1["qvel"], o0["qvel"], rtol=1e-12, atol=1e-12)
    # walker: after set_task the frozen masses are the geometry masses of (0.32, thighsize, legsize) -- NOT 0.8x
    q = rng.uniform(-.005, .005, (4, 9)); q[:, 1] += 1.25; v = rng.uniform(-.5, .5, (4, 9)); a = rng.uniform(-1, 1, (4, 6))
    xr = np.tile(np.array(UNMODELED_SPECS["walker2d"].nominal_task), (4, 1)); xr[:, 4] = [0.45, 0.5, 0.4, 0.45]
    geo = [oracle_constants("walker2d", size=[0.32, xr[i, 4], xr[i, 5], xr[i, 6]])["body_mass"][1:4] for i in range(4)]
    full = np.concatenate([np.array(geo), xr[:, :4], np.full((4, 1), 0.32), xr[:, 4:]], 1)
    o1 = oracle_batch_step("walker2d", q, v, a, xr, variant=1); o0 = oracle_batch_step("walker2d", q, v, a, full)
    assert np.allclose(o1["qvel"], o0["qvel"], rtol=1e-12, atol=1e-12)
    # ... and before any set_task they ARE 0.8x (NaN xi keeps the fresh model)
    geo0 = oracle_constants("walker2d", size=[0.32, 0.45, 0.6, 0.2])["body_mass"][1:]
    full0 = np.concatenate([0.8 * geo0[:3], geo0[3:], [0.32, 0.45, 0.6, 0.2, 0.9, 1.9]])[None].repeat(4, 0)
    o1 = oracle_batch_step("walker2d", q, v, a, np.full((4, 9), np.nan), variant=1)
    o0 = oracle_batch_step("walker2d", q, v, a, full0)
    assert np.allclose(o1["qvel"], o0["qvel"], rtol=1e-12, atol=1e-12)
