"""The Newton solvers' lazily computed line-search sums (planar_newton.hpp: solve_newton, planar_newton_list.hpp: solve_newton_list; LAZY) on the device.

An iteration that does not search skips M sr, phi'(0), the curvature and the phi' / phi'' sums, and carries Ma only where a further
iteration reads it; which of the two forms an iteration takes is a wave-uniform scalar branch on (iteration, ls_free, ls_max), and the
"is any lane still iterating" decision moved from the top of the iteration to its end.  The smallest batches at which those branches can
go wrong: 33 envs in the two-lanes-per-env shape (one full wave and a wave holding a single env) and 65 envs pinned to one lane per env
(one full wave and a wave with a single lane; those kernels keep the eager sums but share the loop control).  Each runs 64 env-steps without
auto-reset under three schedules: the default (ls_free 4: practically every pass lazy), REX_LS_FREE=0 (every pass searches) and
REX_LS_FREE=1 (the first pass of a solve lazy, later passes search: both forms and the hand-over of Ma between them in one solve).

Every step of every lane is held to the fp64 oracle's step from the same (fp32) state, with the per-lane gates of
tests/test_gpu_planar.py::test_hopper_contact_rich_and_limit_states (a free-running env leaves the reset neighbourhood: feet, joint limits
and, once it has fallen, every capsule on the floor)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDS = {"hopper": "RandomHopper-v0", "walker2d": "RandomWalker2d-v0", "halfcheetah": "RandomHalfCheetah-v0"}
TOL_QPOS, CAP_QPOS = 5e-5, 2e-3
TOL_QVEL_REL, CAP_QVEL_REL = 5e-4, 5e-2
STEPS = 64
SCHEDULES = (dict(), dict(REX_LS_FREE=0), dict(REX_LS_FREE=1))
SHAPES = {"pair": (33, dict(pair=True)), "one_lane": (65, dict(pair=False))}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _inputs(kind, B):
    """reset-distribution states, xi = nominal * U(0.9, 1.1), one action sequence -- fp32 values, the same for every schedule"""
    from oracle_bindings import DIMS
    from random_envs_amd.specs import SPECS
    d = DIMS[kind]; rng = np.random.RandomState(77)
    xi = np.array(SPECS[kind].nominal_task) * rng.uniform(0.9, 1.1, (B, d["nx"]))
    if kind == "halfcheetah":
        q = rng.uniform(-0.1, 0.1, (B, d["nq"])); v = 0.1 * rng.randn(B, d["nv"])
    else:
        q = rng.uniform(-0.005, 0.005, (B, d["nq"])); v = rng.uniform(-0.005, 0.005, (B, d["nv"]))
        q[:, 1] += 1.25
    a = rng.uniform(-1, 1, (STEPS, B, d["nu"]))
    return [x.astype(np.float32) for x in (q, v, xi, a)]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("kind", sorted(IDS))
def test_lazy_and_searching_passes_match_the_oracle(torch_mod, kind, shape):
    import random_envs_amd as rex
    from oracle_bindings import oracle_batch_step, oracle_sensitivity
    from parity_util import assert_lanes_explained, create_knobs
    torch = torch_mod
    B, pin = SHAPES[shape]
    if kind == "hopper" and shape == "one_lane":
        pin = dict(pin, rolled=False)
    q0, v0, xi, act = _inputs(kind, B)
    for knobs in SCHEDULES:
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
        tag = "%s %s B=%d %s" % (kind, shape, B, knobs or "default schedule")
        assert c["solver_capped"] == 0 and c["nonfinite"] == 0 and c["overflow"] == 0, (tag, c)
        assert np.array_equal(qs[0], q0.astype(np.float64)) and np.array_equal(vs[0], v0.astype(np.float64)), tag
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
