"""The two-lanes-per-env humanoid engine (random-envs_amd/csrc/humanoid_pair.hpp: the step kernel's math) compiled for the host
-- the two lanes of a pair as two lock-stepped threads, the env's LDS column as shared memory -- against the independent
fp64 oracle: a whole env step (20 forward evaluations, RK4), the 376-dim observation, reward, done; standing, crouched and
piled-up states (all three solver paths); fp64 pins the algorithm, fp32 sets the GPU tolerance."""
import ctypes

import numpy as np
import pytest

from host_harness.build import build_so
from oracle_bindings import _p, oracle_humanoid_reset_obs, oracle_humanoid_step
from random_envs_amd.specs import SPECS

UB = ctypes.POINTER(ctypes.c_ubyte); I = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def hp():
    return ctypes.CDLL(build_so("humanoid_pair_host", "humanoid_pair_host.cpp", ["-pthread"]))


def _step(hp, f32, q, v, a, xi, xprev=None):
    n = q.shape[0]
    qs, vs, as_, xs = [np.ascontiguousarray(x.T) for x in (q, v, a, xi)]
    xp = None if xprev is None else np.ascontiguousarray(xprev.T)
    qo = np.zeros_like(qs); vo = np.zeros_like(vs); obs = np.zeros((376, n)); r = np.zeros(n); d = np.zeros(n, dtype=np.uint8)
    xo = np.zeros((14, n)); ov = np.zeros(n, dtype=np.int32); nr = np.zeros(n, dtype=np.int32)
    hp.hp_step(f32, n, _p(qs), _p(vs), _p(as_), _p(xs), _p(xp), _p(qo), _p(vo), _p(obs), _p(r), d.ctypes.data_as(UB), _p(xo),
               ov.ctypes.data_as(I), nr.ctypes.data_as(I))
    return dict(qpos=qo.T, qvel=vo.T, obs=obs.T, reward=r, done=d.astype(bool), xipos_x=xo.T, overflow=ov, nrows=nr)


def _states(n, seed, spread=0.3):
    rng = np.random.RandomState(seed)
    nom = np.array(SPECS["humanoid"].nominal_task)
    q = np.tile(np.array([0, 0, 1.4, 1, 0, 0, 0] + [0] * 17, dtype=float), (n, 1)) + rng.uniform(-.01, .01, (n, 24))
    q[:, 7:] += rng.uniform(-spread, spread, (n, 17)); q[:, 2] = rng.uniform(1.0, 1.45, n)
    v = rng.uniform(-1, 1, (n, 23)); a = rng.uniform(-.5, .5, (n, 17)); xi = nom * rng.uniform(.8, 1.2, (n, 30))
    return q, v, a, xi


def test_side_bodies_have_no_orientation_offset(hp):
    assert hp.hp_check_model() == 1


def test_env_step_vs_oracle(hp):
    n = 96
    q, v, a, xi = _states(n, 1)
    ref = oracle_humanoid_step(q, v, a, xi)
    for f32, tv, to in ((0, 1e-10, 1e-10), (1, 1e-4, 2e-5)):
        out = _step(hp, f32, q, v, a, xi)
        ev = np.abs(out["qvel"] - ref["qvel"]).max(1) / (1 + np.abs(ref["qvel"]).max(1))
        eo = np.abs(out["obs"] - ref["obs"]).max(1) / (1 + np.abs(ref["obs"]).max(1))
        assert ev.max() < tv and eo.max() < to and out["overflow"].sum() == 0, (f32, ev.max(), eo.max())
        assert np.abs(out["reward"] - ref["reward"]).max() < (1e-9 if not f32 else 1e-4)
        assert np.array_equal(out["done"], ref["done"])
        assert np.abs(out["xipos_x"] - ref["xipos_x"]).max() < (1e-12 if not f32 else 1e-5)
    # second step: mass_center() "before" from the xipos the first step left behind
    a2 = np.random.RandomState(3).uniform(-.4, .4, (n, 17))
    out1 = _step(hp, 0, q, v, a, xi)
    ref2 = oracle_humanoid_step(ref["qpos"], ref["qvel"], a2, xi, xipos_x_prev=ref["xipos_x"])
    out2 = _step(hp, 0, out1["qpos"], out1["qvel"], a2, xi, xprev=out1["xipos_x"])
    assert np.abs(out2["reward"] - ref2["reward"]).max() < 1e-8


def test_pile_ups_all_solver_paths(hp):
    """lying / crumpled humanoids with hinges past their limits: <= 16 rows, 17..21 rows and the scratch-row PGS (> 21)"""
    n = 64; rng = np.random.RandomState(5)
    nom = np.array(SPECS["humanoid"].nominal_task)
    q = np.tile(np.array([0, 0, 1.4, 1, 0, 0, 0] + [0] * 17, dtype=float), (n, 1))
    q[:, 7:] += rng.uniform(-1.2, 1.2, (n, 17)); q[:, 2] = rng.uniform(0.05, 0.6, n)
    qq = np.array([1, 0, 0, 0]) + rng.uniform(-1, 1, (n, 4)); q[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    v = rng.uniform(-1, 1, (n, 23)); a = rng.uniform(-.4, .4, (n, 17)); xi = nom * rng.uniform(.9, 1.1, (n, 30))
    ref = oracle_humanoid_step(q, v, a, xi)
    out = _step(hp, 0, q, v, a, xi)
    ok = np.isfinite(ref["qvel"]).all(1)
    ev = np.abs(out["qvel"] - ref["qvel"]).max(1) / (1 + np.abs(ref["qvel"]).max(1))
    assert out["overflow"].sum() == 0 and ok.sum() > n // 2
    assert (out["nrows"] > 21).sum() >= 3 and (out["nrows"] <= 16).sum() >= 1, np.sort(out["nrows"])
    assert ev[ok].max() < 1e-7, ev[ok].max()



# humanoid.xml's own orders, written out independently of the code under test: bodies 1 torso, 2 lwaist, 3 pelvis, 4-6 right thigh / shin /
# foot, 7-9 left, 10-11 right upper / lower arm, 12-13 left; dofs 0-5 root, 6-8 abdomen z / y / x, 9-12 right hip x / z / y + knee, 13-16
# left, 17-19 right shoulder 1 / 2 + elbow, 20-22 left; motors (:106-122) abdomen y, z, x, right leg, left leg, right arm, left arm
BODY = ([1, 2, 3, 4, 5, 6, 10, 11], [1, 2, 3, 7, 8, 9, 12, 13])
DOF = (list(range(9)) + [9, 10, 11, 12, 17, 18, 19], list(range(9)) + [13, 14, 15, 16, 20, 21, 22])
MOTOR = ([1, 0, 2, 3, 4, 5, 6, 11, 12, 13], [1, 0, 2, 7, 8, 9, 10, 14, 15, 16])
QPOS0 = np.array([0, 0, 1.4, 1, 0, 0, 0] + [0] * 17, dtype=float)


def test_load_store_round_trip(hp):
    """load_lane then store_lane with nothing between (the kernel's own layout code): every state row comes back where it was, from
    exactly one lane; every xi and action row reaches the lane(s) that use it."""
    n = 3
    rows = dict(qpos=24, qvel=23, act=17, xi=30, aux=14)
    src = {}
    for j, (k, r) in enumerate(rows.items()):
        src[k] = 1000.0 * (j + 1) + np.arange(r * n, dtype=float).reshape(r, n)     # distinct over all blocks, rows and envs
    out = {k: np.full((rows[k], n), np.nan) for k in ("qpos", "qvel", "aux")}
    lane = np.full((2, 34, n), np.nan)
    hp.hp_roundtrip(n, _p(src["qpos"]), _p(src["qvel"]), _p(src["act"]), _p(src["xi"]), _p(src["aux"]),
                    _p(out["qpos"]), _p(out["qvel"]), _p(out["aux"]), _p(lane))
    assert np.array_equal(out["qpos"], src["qpos"]) and np.array_equal(out["qvel"], src["qvel"])
    assert np.array_equal(out["aux"][1:], src["aux"][1:]) and np.all(out["aux"][0] == 0)
    assert not any(np.isnan(o).any() for o in out.values()) and not np.isnan(lane).any()
    used = set()
    for s in (0, 1):
        assert np.array_equal(lane[s, :8], src["xi"][[b - 1 for b in BODY[s]]])                     # body_mass[1:] = xi[:13]
        assert np.all(lane[s, 8:14] == 0) and np.array_equal(lane[s, 14:24], src["xi"][[13 + d - 6 for d in DOF[s][6:]]])
        assert np.array_equal(lane[s, 24:], src["act"][MOTOR[s]])
        used |= set(MOTOR[s])
    assert used == set(range(17))                                                                   # each of the 17 action rows is consumed


@pytest.fixture(scope="module")
def reset64(hp):
    """hp_reset (reset_lane + emit_obs + store_lane, the kernel's fused auto-reset) at n = 64 in both precisions, with its inputs"""
    n = 64; rng = np.random.RandomState(7)
    draws = rng.uniform(0, 1, (47, n)).astype(np.float32).astype(np.float64)        # (fp32-representable: both precisions see the same uniforms)
    xi = np.array(SPECS["humanoid"].nominal_task) * rng.uniform(.8, 1.2, (n, 30))
    xs = np.ascontiguousarray(xi.T)
    res = {}
    for f32 in (0, 1):
        qo = np.full((24, n), np.nan); vo = np.full((23, n), np.nan); obs = np.full((376, n), np.nan); xo = np.full((14, n), np.nan)
        hp.hp_reset(f32, n, _p(draws), _p(xs), _p(qo), _p(vo), _p(obs), _p(xo))
        res[f32] = dict(qpos=qo.T.copy(), qvel=vo.T.copy(), obs=obs.T.copy(), xipos_x=xo.T.copy())
    return dict(draws=draws, xi=xi, out=res)


def test_reset_vs_oracle(reset64):
    draws, xi = reset64["draws"], reset64["xi"]
    q = (QPOS0[:, None] + 0.01 * (2 * (1 - draws[:24]) - 1)).T                       # random_humanoid.py:220-229, NQ draws then NV
    v = (0.01 * (2 * (1 - draws[24:]) - 1)).T
    for f32, tq, to, tx in ((0, 0.0, 1e-10, 1e-12), (1, 1.2e-7, 2e-5, 1e-5)):
        out = reset64["out"][f32]
        eq = max(np.abs(out["qpos"] - q).max(), np.abs(out["qvel"] - v).max())
        ref, xip = oracle_humanoid_reset_obs(out["qpos"], out["qvel"], xi)
        eo = (np.abs(out["obs"] - ref).max(1) / (1 + np.abs(ref).max(1))).max()
        ex = np.abs(out["xipos_x"] - xip).max()
        print("hp_reset f32=%d: |dq| %.2e, obs rel %.2e, xipos %.2e" % (f32, eq, eo, ex))
        assert eq <= tq and eo < to and ex < tx, (f32, eq, eo, ex)


def test_reset_then_step(hp, reset64):
    """the reset leaves the xipos that the next mass_center() reads"""
    out, xi = reset64["out"][0], reset64["xi"]
    a = np.random.RandomState(8).uniform(-.4, .4, (64, 17))
    _, xip = oracle_humanoid_reset_obs(out["qpos"], out["qvel"], xi)
    ref = oracle_humanoid_step(out["qpos"], out["qvel"], a, xi, xipos_x_prev=xip)
    got = _step(hp, 0, out["qpos"], out["qvel"], a, xi, xprev=out["xipos_x"])
    assert np.abs(got["reward"] - ref["reward"]).max() < 1e-8
