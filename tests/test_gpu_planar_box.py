"""The planar HIP kernels against the fp64 oracle over the WHOLE search box of the task xi (the box `set_dr_distribution("uniform", ...)` and
the inference loops roam), not a band around nominal: xi ~ U(box) and xi at the box's corners, states from oracle rollouts that honour the
done rule (oracle_bindings.box_states).  Same path, gates, tolerances and caps as tests/test_gpu_planar.py::test_step_parity_on_rollout_states;
in addition at most 1 % of the lanes may pass by the `explained` clause of parity_util.assert_lanes_explained.  The CPU twin of these tests
(the fp32 host instantiation of the same engine) is tests/test_planar_box_host.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ["hopper", "halfcheetah", "walker2d"]
IDS = {"hopper": "RandomHopper-v0", "walker2d": "RandomWalker2d-v0", "halfcheetah": "RandomHalfCheetah-v0"}
TOL_QPOS, CAP_QPOS = 2e-5, 5e-4            # tests/test_gpu_planar.py's own
TOL_QVEL_REL, CAP_QVEL_REL = 2e-4, 2e-2
TOL_REWARD, CAP_REWARD = 5e-3, 1e-1
SEEDS = {"hopper": 51, "halfcheetah": 52, "walker2d": 53}
N = 2048


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _f32(*xs):
    return [x.astype(np.float32).astype(np.float64) for x in xs]


def _done_margin(kind, qpos):
    """distance of the reference end state to the nearest threshold of the done rule (the half-cheetah never terminates)"""
    z, th = qpos[:, 1], qpos[:, 2]
    if kind == "hopper":
        return np.minimum(np.abs(z - 0.7), np.abs(np.abs(th) - 0.2))
    if kind == "walker2d":
        return np.minimum.reduce([np.abs(z - 0.8), np.abs(z - 2.0), np.abs(th - 1.0), np.abs(th + 1.0)])
    return np.full(len(z), np.inf)


@functools.lru_cache(maxsize=None)
def _reference(kind, mode):
    """fp32-rounded inputs (what the kernels see), the oracle's step from them and its sensitivity: once per (kind, mode), read-only"""
    from oracle_bindings import DIMS, box_states, oracle_batch_step, oracle_sensitivity
    d = DIMS[kind]
    q, v, xi = _f32(*box_states(kind, N, mode, SEEDS[kind] + (100 if mode == "corners" else 0)))
    a, = _f32(np.random.RandomState(5).uniform(-1.2, 1.2, (N, d["nu"])))
    ref, sens = oracle_sensitivity(lambda q_, v_, a_, x_: oracle_batch_step(kind, q_, v_, a_, x_), [q, v, a, xi], ["qpos", "qvel", "reward"])
    for x in [q, v, xi, a] + [ref[k] for k in ("qpos", "qvel", "reward", "done")] + list(sens.values()):
        x.setflags(write=False)
    return q, v, xi, a, ref, sens


def _check_step(kind, tag, n, out, ref, sens, counters):
    """every lane of one step (obs, reward, done, qpos, qvel of the first n reference lanes) against the oracle; <= 1 % explained"""
    from parity_util import assert_done_explained, assert_lanes_explained
    obs, r, dn, qq, vv = out
    assert qq.shape[0] == n and np.isfinite(qq).all() and np.isfinite(vv).all()
    rq, rv, rr = ref["qpos"][:n], ref["qvel"][:n], ref["reward"][:n]
    eq = np.abs(qq - rq).max(1)
    vs = 1 + np.abs(rv).max(1)
    ev = np.abs(vv - rv).max(1) / vs
    er = np.abs(r - rr)
    assert_lanes_explained(eq, sens["qpos"][:n], TOL_QPOS, CAP_QPOS, label=tag + " |dqpos|")
    assert_lanes_explained(ev, sens["qvel"][:n] / vs, TOL_QVEL_REL, CAP_QVEL_REL, label=tag + " |dqvel|rel")
    assert_lanes_explained(er, sens["reward"][:n], TOL_REWARD, CAP_REWARD, label=tag + " |dreward|")
    explained = int(((eq > TOL_QPOS) | (ev > TOL_QVEL_REL) | (er > TOL_REWARD)).sum())
    print("%s: %d of %d lanes pass by the explained clause (at most %d)" % (tag, explained, n, n // 100))
    assert explained <= n // 100, (tag, explained)
    assert np.array_equal(obs, np.concatenate([qq[:, 1:], vv], 1))          # obs = concat(qpos[1:], qvel), bitwise
    assert_done_explained(dn, ref["done"][:n], _done_margin(kind, rq), 2e-5, label=tag)
    assert counters["solver_capped"] == 0 and counters["nonfinite"] == 0, (tag, counters)


def _step_from(env, torch, q, v, xi, a):
    env.set_task(np.asarray(xi, dtype=np.float32))
    env.set_state(np.array(q), np.array(v))          # (copies: the shared reference arrays are read-only)
    obs, r, d, _ = env.step(torch.as_tensor(np.array(a), dtype=torch.float32))
    qq, vv = env.get_state()
    return obs.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), qq.cpu().numpy(), vv.cpu().numpy()


SHAPES = {"default": dict(), "one_lane": dict(REX_PAIR=0), "rolled": dict(REX_ROLLED=1, REX_PAIR=0)}
STEP_CASES = [(k, m, s) for k in KINDS for m in ("uniform", "corners") for s in SHAPES if s != "rolled" or k == "hopper"]


@pytest.mark.parametrize("kind,mode,shape", STEP_CASES)
def test_step_parity_over_the_search_box(torch_mod, kind, mode, shape):
    """set_task, set_state, one step, get_state in the default launch shape (two lanes per env), with one lane per env, and for the hopper in
    the rolled two-waves-per-SIMD kernel."""
    import random_envs_amd as rex
    from parity_util import create_knobs
    q, v, xi, a, ref, sens = _reference(kind, mode)
    with create_knobs(**SHAPES[shape]):
        env = rex.make(IDS[kind], batch=N, autoreset=False)
    ls = env.launch_shape()
    assert ls["pair"] == (shape == "default") and ls["rolled"] == (shape == "rolled"), ls
    out = _step_from(env, torch_mod, q, v, xi, a)
    _check_step(kind, "%s %s %s" % (kind, mode, shape), N, out, ref, sens, env.counters())
    env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_general_solver_over_the_box(torch_mod, kind):
    """REX_FAST=0 beside REX_PAIR=1: every evaluation of every lane on the LIST solver of the two-lanes-per-env kernels; corners."""
    import random_envs_amd as rex
    from parity_util import create_knobs
    n = 1024
    q, v, xi, a, ref, sens = _reference(kind, "corners")
    with create_knobs(REX_FAST=0, REX_PAIR=1):
        env = rex.make(IDS[kind], batch=n, autoreset=False)
    out = _step_from(env, torch_mod, q[:n], v[:n], xi[:n], a[:n])
    _check_step(kind, "%s corners list solver" % kind, n, out, ref, sens, env.counters())
    env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_device_box_draws_then_step(torch_mod, kind):
    """xi drawn ON THE DEVICE from U(search box), 25 auto-reset steps, then one step of every lane against the oracle on the device's own
    (qpos, qvel, xi): tests/test_gpu_configs.py's C4 pattern over the whole box."""
    import random_envs_amd as rex
    from oracle_bindings import DIMS, oracle_batch_step, oracle_sensitivity
    from random_envs_amd.specs import SPECS
    torch = torch_mod
    d = DIMS[kind]
    lo, hi = np.array(SPECS[kind].search_bounds, dtype=np.float64).T
    env = rex.make(IDS[kind], batch=N, seed=SEEDS[kind])
    env.set_dr_distribution("uniform", np.stack([lo, hi], 1).ravel().tolist())
    env.set_dr_training(True); env.reset()
    g = torch.Generator().manual_seed(7)
    for _ in range(25):
        env.step(torch.rand(N, d["nu"], generator=g) * 2 - 1)
    q, v = env.get_state(); xi = env.get_task()
    q, v, xi = [z.cpu().double().numpy() for z in (q, v, xi)]
    assert (xi >= lo - 1e-6).all() and (xi <= hi + 1e-6).all()
    # the draw really spans the box: every component's extremes within 2 % of the box width of the bounds
    assert ((xi.min(0) - lo) <= 0.02 * (hi - lo)).all() and ((hi - xi.max(0)) <= 0.02 * (hi - lo)).all(), (xi.min(0), xi.max(0))
    a = torch.rand(N, d["nu"], generator=g) * 2 - 1
    env.autoreset = False; env._push_flags()
    obs, r, dn, _ = env.step(a)
    qq, vv = env.get_state()
    ref, sens = oracle_sensitivity(lambda q_, v_, a_, x_: oracle_batch_step(kind, q_, v_, a_, x_), [q, v, a.double().numpy(), xi],
                                   ["qpos", "qvel", "reward"])
    out = (obs.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy(), qq.cpu().numpy(), vv.cpu().numpy())
    _check_step(kind, "%s device box draws" % kind, N, out, ref, sens, env.counters())
    env.close()


@pytest.mark.parametrize("mode", ["uniform", "corners"])
def test_walker2d_unmodeled_over_its_box(torch_mod, mode):
    """RandomWalker2dUnmodeled-v0: the reduced task over its own box (UNMODELED_SPECS); observations as in test_unmodeled_ids."""
    import random_envs_amd as rex
    from oracle_bindings import DIMS, UNMODELED_NX, box_states, oracle_batch_step, oracle_sensitivity
    from parity_util import assert_lanes_explained
    kind, eid, n = "walker2d", "RandomWalker2dUnmodeled-v0", 512
    d = DIMS[kind]
    q, v, xi = _f32(*box_states(kind, n, mode, 61 + (100 if mode == "corners" else 0), variant=1))
    assert xi.shape == (n, UNMODELED_NX[kind])
    a, = _f32(np.random.RandomState(6).uniform(-1, 1, (n, d["nu"])))
    env = rex.make(eid, batch=n, seed=3, autoreset=False)
    env.set_task(xi.astype(np.float32)); env.set_state(q, v)
    obs, r, dn, _ = env.step(torch_mod.as_tensor(a, dtype=torch_mod.float32))
    ref, sens = oracle_sensitivity(lambda q_, v_, a_, x_: oracle_batch_step(kind, q_, v_, a_, x_, variant=1), [q, v, a, xi], ["obs"])
    os_ = 1 + np.abs(ref["obs"]).max(1)
    e = np.abs(obs.cpu().numpy() - ref["obs"]).max(1) / os_
    tag = "%s %s" % (eid, mode)
    over = assert_lanes_explained(e, sens["obs"] / os_, 2e-4, 2e-2, label=tag + " |dobs|rel")
    print("%s: %d of %d lanes pass by the explained clause (at most %d)" % (tag, over, n, n // 100))
    assert over <= n // 100, (tag, over)
    c = env.counters()
    assert c["solver_capped"] == 0 and c["nonfinite"] == 0, (tag, c)
    env.close()
