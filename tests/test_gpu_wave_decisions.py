"""The wave-uniform decisions of forward() (planar_engine.hpp) and of the Newton solvers (planar_newton.hpp, planar_newton_list.hpp) on the device, with waves whose lanes disagree.

Host builds have one-lane "waves" (REX_WAVE_ANY(x) is x), so only the device can get a ballot wrong: which solver instantiation a wave
enters (forward(): none, feet-only, general, general + self rows), the one exit test at the end of a Newton pass (does any lane iterate on,
was it the last pass) with the update of Ma behind it, and the two ballots ahead of the one branch into the correction block (some lane can
correct; some pair couples two groups).  The smallest batches at which that can happen: 33 envs in the two-lanes-per-env shape (one full
wave and a wave holding a single env) and 65 envs pinned to one lane per env (one full wave and a wave with a single lane; those kernels
share forward() and the correction plan).

Start states are mixed WITHIN the first wave: lanes from the reset distribution, lanes pitched about +-1.2 rad at low height (they lie down
on every capsule: the general solver modes; the hopper's last four with a folded leg, whose self pairs pass the cull) and four lanes 1 m
above the reset height -- so the wave's decision is taken for lanes that disagree.  The lone env of the second wave also starts 1 m up
with zero action: that wave has no row until it lands (forward() mode 0), then only its feet touch (mode 3); its root z is held to the
free-fall parabola over the first steps, so a step of this test really had a wave without rows.  64 free-running env-steps without
auto-reset under six knob sets -- the default, REX_FAST=0, REX_CORR=0, REX_CORR=1, REX_WARM=0, REX_LS_FREE=0 -- take every one of these
decisions both ways.

Every step of every lane is held to the fp64 oracle's step from the same (fp32) state, with the tolerances and per-lane gates of
tests/test_gpu_newton_lazy_sums.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDS = {"hopper": "RandomHopper-v0", "walker2d": "RandomWalker2d-v0", "halfcheetah": "RandomHalfCheetah-v0"}
TOL_QPOS, CAP_QPOS = 5e-5, 2e-3
TOL_QVEL_REL, CAP_QVEL_REL = 5e-4, 5e-2
STEPS = 64
KNOBS = (dict(), dict(REX_FAST=0), dict(REX_CORR=0), dict(REX_CORR=1), dict(REX_WARM=0), dict(REX_LS_FREE=0))
SHAPES = {"pair": (33, dict(pair=True)), "one_lane": (65, dict(pair=False))}
DT = {"hopper": 0.008, "walker2d": 0.008, "halfcheetah": 0.05}   # env-step length (timestep x frame_skip)
# env-steps over which the lone env's free fall is judged: 0.128 s = 8 cm (it lands after 0.45 s); the half-cheetah 0.2 s = 20 cm
FALL_STEPS = {"hopper": 16, "walker2d": 16, "halfcheetah": 4}
GRAVITY = 9.81


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def _inputs(kind, B):
    """fp32 start states, xi = nominal * U(0.9, 1.1) and one action sequence, the same for every knob set.  Of the first wave's envs (32 in the
    pair shape, 64 at one lane per env): the last quarter + 4 pitched at low height, the 4 before them 1 m up; the last env of the batch (alone in
    the second wave) 1 m up with zero action."""
    from oracle_bindings import DIMS
    from random_envs_amd.specs import SPECS
    d = DIMS[kind]; rng = np.random.RandomState(91)
    xi = np.array(SPECS[kind].nominal_task) * rng.uniform(0.9, 1.1, (B, d["nx"]))
    if kind == "halfcheetah":
        q = rng.uniform(-0.1, 0.1, (B, d["nq"])); v = 0.1 * rng.randn(B, d["nv"])
        low = -0.35    # root z is an offset from the model's 0.7
    else:
        q = rng.uniform(-0.005, 0.005, (B, d["nq"])); v = rng.uniform(-0.005, 0.005, (B, d["nv"]))
        q[:, 1] += 1.25
        low = 0.45
    W = B - 1                      # envs of the first wave
    lying = np.arange(W - W // 4 - 4, W); up = np.arange(lying[0] - 4, lying[0]); lone = B - 1
    q[up, 1] += 1.0
    q[lying, 1] = low + rng.uniform(-0.05, 0.05, lying.size)
    q[lying, 2] = np.where(np.arange(lying.size) % 2 == 0, 1.0, -1.0) * (1.2 + rng.uniform(-0.1, 0.1, lying.size))
    if kind == "hopper":   # folded leg: thigh and knee at about -115 deg bring the foot to the torso (a self row from the first step on)
        q[lying[-4:], 3] = rng.uniform(-2.05, -1.95, 4); q[lying[-4:], 4] = rng.uniform(-2.05, -1.95, 4)
    a = rng.uniform(-1, 1, (STEPS, B, d["nu"]))
    # the lone env: at rest, every joint inside its range (the reset pose has the hopper's and the walker's leg joints AT their upper limit 0)
    v[lone] = 0.0; q[lone, 3:] = 0.0 if kind == "halfcheetah" else -0.05
    q[lone, 1] += 1.0; a[:, lone] = 0.0
    return [x.astype(np.float32) for x in (q, v, xi, a)]


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join("%s=%s" % kv for kv in sorted(k.items())) or "default")
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("kind", sorted(IDS))
def test_mixed_waves_match_the_oracle(torch_mod, kind, shape, knobs):
    import random_envs_amd as rex
    from oracle_bindings import oracle_batch_step, oracle_sensitivity
    from parity_util import assert_lanes_explained, create_knobs
    torch = torch_mod
    B, pin = SHAPES[shape]
    if kind == "hopper" and shape == "one_lane":
        pin = dict(pin, rolled=False)
    q0, v0, xi, act = _inputs(kind, B)
    with create_knobs(**knobs):
        env = rex.make(IDS[kind], batch=B, autoreset=False)
    got = env.set_launch_shape(**pin)
    assert got["pair"] == pin["pair"], got
    env.set_task(xi); env.set_state(q0.astype(np.float64), v0.astype(np.float64))
    qs, vs = [], []
    for t in range(STEPS):
        q, v = env.get_state()
        qs.append(q.cpu().numpy().astype(np.float64)); vs.append(v.cpu().numpy().astype(np.float64))
        env.step(torch.as_tensor(act[t]))
    q, v = env.get_state()
    qs.append(q.cpu().numpy().astype(np.float64)); vs.append(v.cpu().numpy().astype(np.float64))
    c = env.counters()
    env.close()
    tag = "%s %s B=%d %s" % (kind, shape, B, knobs or "default")
    assert c["solver_capped"] == 0 and c["nonfinite"] == 0 and c["overflow"] == 0, (tag, c)
    assert np.array_equal(qs[0], q0.astype(np.float64)) and np.array_equal(vs[0], v0.astype(np.float64)), tag
    # the lone env of the second wave is in free flight over the first steps: that wave had no row
    n = FALL_STEPS[kind]; t = n * DT[kind]; fall = 0.5 * GRAVITY * t * t
    z = qs[n][B - 1, 1]; z_free = qs[0][B - 1, 1] + vs[0][B - 1, 1] * t - fall
    print(tag, "lone env: z after %d steps %.5f, free fall %.5f (fell %.4f)" % (n, z, z_free, fall))
    assert abs(z - z_free) < 0.25 * fall, (tag, z, z_free)
    qin, vin = np.concatenate(qs[:-1]), np.concatenate(vs[:-1])
    qout, vout = np.concatenate(qs[1:]), np.concatenate(vs[1:])
    ain = act.reshape(STEPS * B, -1).astype(np.float64); xin = np.tile(xi.astype(np.float64), (STEPS, 1))
    ref, sens = oracle_sensitivity(lambda q_, v_, a_, x_: oracle_batch_step(kind, q_, v_, a_, x_), [qin, vin, ain, xin],
                                   ["qpos", "qvel"], trials=2)
    eq = np.abs(qout - ref["qpos"]).max(1)
    scale = 1 + np.abs(ref["qvel"]).max(1)
    ev = np.abs(vout - ref["qvel"]).max(1) / scale
    assert_lanes_explained(eq, sens["qpos"], TOL_QPOS, CAP_QPOS, label=tag + " |dqpos|")
    assert_lanes_explained(ev, sens["qvel"] / scale, TOL_QVEL_REL, CAP_QVEL_REL, label=tag + " |dqvel|rel")
