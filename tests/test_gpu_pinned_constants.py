"""The wave-uniform model block as the step kernels' evaluation reads it (planar_kernels.hpp: pin_uniform).

The two-lanes-per-env hopper kernel copies the fields of `ugeom` into per-lane registers once per launch and every evaluation of the step
reads the copies, and it takes the solver parameters as a copy by value; a wrong, stale or swapped copy moves the dynamics (armature,
damping, stiffness, inertia, anchors in the mass matrix and the force vector; capsule ends and radii in the floor tests; K, B and the
impedance widths in every row).  All three planar kinds run in both launch shapes so that the kernels this left alone are held to the same
figures: 33 envs in the two-lanes-per-env shape (one full wave and a wave holding a lone env) and 65 envs at one lane per env.

64 free-running env-steps from a reset, auto-reset on and xi resampled from a uniform distribution at every reset (the fused reset runs
behind the same launch), under the default knobs and under REX_FAST=0, REX_WARM=0 and REX_LS_FREE=0 -- the general solver path, the cold
start and the searching passes read the parameter fields the default path reads least.  One more hopper case draws xi from the whole search
range and starts every env AT a search bound (alternating lower / upper per mass).

Every step of every lane is held to the fp64 oracle's step from the same (fp32) state, action and xi: the end-of-step observation (the
terminal observation of a lane that finished: qpos[1:] and qvel) and, for the lanes that went on, the root x of the next state, with the
tolerances and per-lane gates of tests/test_gpu_newton_lazy_sums.py.

On the parent of the change that added pin_uniform all 25 cases pass (3.9 s) with no lane-step above the tolerances: worst |dqpos| 1.3e-5
and worst relative |dqvel| 1.1e-4 (half-cheetah, pair shape); hopper 2.2e-7 / 1.5e-6, walker2d 3.6e-6 / 3.8e-5."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDS = {"hopper": "RandomHopper-v0", "walker2d": "RandomWalker2d-v0", "halfcheetah": "RandomHalfCheetah-v0"}
TOL_QPOS, CAP_QPOS = 5e-5, 2e-3
TOL_QVEL_REL, CAP_QVEL_REL = 5e-4, 5e-2
STEPS = 64
KNOBS = (dict(), dict(REX_FAST=0), dict(REX_WARM=0), dict(REX_LS_FREE=0))
SHAPES = {"pair": (33, dict(pair=True)), "one_lane": (65, dict(pair=False))}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def _actions(kind, B):
    from oracle_bindings import DIMS
    return np.random.RandomState(58).uniform(-1, 1, (STEPS, B, DIMS[kind]["nu"])).astype(np.float32)


def _run_and_check(torch, kind, shape, knobs, lo, hi, xi0, tag):
    """auto-reset + resampling run of STEPS env-steps; xi ~ U(lo, hi) at every reset (xi0, when given, is the first episode's task)"""
    import random_envs_amd as rex
    from oracle_bindings import oracle_batch_step, oracle_sensitivity
    from parity_util import assert_lanes_explained, create_knobs
    B, pin = SHAPES[shape]
    if kind == "hopper" and shape == "one_lane":
        pin = dict(pin, rolled=False)
    act = _actions(kind, B)
    with create_knobs(**knobs):
        env = rex.make(IDS[kind], batch=B, seed=11)
    assert env.autoreset
    got = env.set_launch_shape(**pin)
    assert got["pair"] == pin["pair"], got
    env.set_dr_distribution("uniform", np.stack([lo, hi], 1).ravel().tolist())
    env.set_dr_training(True)
    env.reset()
    if xi0 is not None:
        env.set_task(xi0.astype(np.float32))
    f64 = lambda x: x.cpu().numpy().astype(np.float64)
    qs, vs, xs, terms, dones = [], [], [], [], []
    for t in range(STEPS):
        q, v = env.get_state()
        qs.append(f64(q)); vs.append(f64(v)); xs.append(f64(env.get_task()))
        _, _, d, info = env.step(torch.as_tensor(act[t]))
        terms.append(f64(info["terminal_observation"])); dones.append(d.cpu().numpy().astype(bool))
    q, v = env.get_state()
    qs.append(f64(q))
    c = env.counters()
    env.close()
    assert c["solver_capped"] == 0 and c["nonfinite"] == 0 and c["overflow"] == 0, (tag, c)
    done = np.concatenate(dones)
    xin = np.concatenate(xs)
    assert (xin >= lo * (1 - 1e-6)).all() and (xin <= hi * (1 + 1e-6)).all(), tag
    if kind != "halfcheetah":   # (the half-cheetah has no termination rule; its episodes end at the time limit only)
        resets = int(done.sum()); redrawn = int((xs[-1] != xs[0]).any(1).sum())
        print("%s: %d resets in %d lane-steps, %d of %d envs ended on another xi than they began with" % (tag, resets, done.size, redrawn, B))
        assert resets > 0 and redrawn > 0, (tag, resets, redrawn)   # (the fused reset and its xi draw ran behind some step)
    qin, vin = np.concatenate(qs[:-1]), np.concatenate(vs)
    term = np.concatenate(terms); xnext = np.concatenate(qs[1:])[:, 0]
    ain = act.reshape(STEPS * B, -1).astype(np.float64)
    assert qin.shape[0] == vin.shape[0] == ain.shape[0] == xin.shape[0] == term.shape[0] == STEPS * B, tag
    ref, sens = oracle_sensitivity(lambda q_, v_, a_, x_: oracle_batch_step(kind, q_, v_, a_, x_), [qin, vin, ain, xin],
                                   ["qpos", "qvel"], trials=2)
    nq = qin.shape[1]
    eq = np.abs(term[:, :nq - 1] - ref["qpos"][:, 1:]).max(1)
    eq = np.maximum(eq, np.where(done, 0.0, np.abs(xnext - ref["qpos"][:, 0])))
    scale = 1 + np.abs(ref["qvel"]).max(1)
    ev = np.abs(term[:, nq - 1:] - ref["qvel"]).max(1) / scale
    print("%s: worst |dqpos| %.3e, worst relative |dqvel| %.3e" % (tag, eq.max(), ev.max()))
    assert_lanes_explained(eq, sens["qpos"], TOL_QPOS, CAP_QPOS, label=tag + " |dqpos|")
    assert_lanes_explained(ev, sens["qvel"] / scale, TOL_QVEL_REL, CAP_QVEL_REL, label=tag + " |dqvel|rel")


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join("%s=%s" % kv for kv in sorted(k.items())) or "default")
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("kind", sorted(IDS))
def test_autoreset_rollout_matches_the_oracle(torch_mod, kind, shape, knobs):
    from random_envs_amd.specs import SPECS
    nom = np.array(SPECS[kind].nominal_task)
    _run_and_check(torch_mod, kind, shape, knobs, 0.9 * nom, 1.1 * nom, None,
                   "%s %s %s" % (kind, shape, knobs or "default"))


def test_hopper_xi_at_the_search_bounds(torch_mod):
    from random_envs_amd.specs import SPECS
    b = np.array(SPECS["hopper"].search_bounds, dtype=np.float64)
    lo, hi = b[:, 0], b[:, 1]
    B = SHAPES["pair"][0]
    pick = (np.arange(B)[:, None] + np.arange(lo.size)[None, :]) % 2 == 0   # env i, mass k: lower bound when i + k is even
    xi0 = np.where(pick, lo, hi)
    _run_and_check(torch_mod, "hopper", "pair", dict(), lo, hi, xi0, "hopper pair xi at the search bounds")
