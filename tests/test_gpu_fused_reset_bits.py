"""The auto-reset fused into the planar step kernel against the explicit masked reset, bit for bit.

Two handles with the same seed and the same actions: `fused` steps with auto-reset on (finished lanes restart inside the step launch:
their next episode's state, observation and xi come from Philox blocks evaluated in registers), `split` steps with auto-reset off
and calls the masked `reset()` after every step (planar_reset_kernel: rocRAND's engine).  The two paths share no RNG code, so equal
bits after every step hold the fused tail to the engine's streams draw by draw: init noise, the xi resample of every DR type
(uniform through the unrolled sampler; truncnorm / gaussian / fullgaussian, whose redraw rules consume a data-dependent number of
words, through the register word stream), the observation noise of the Noisy id, walker2d's re-derive from the new lengths, and the
single set of state stores (qpos, qvel, t, done, episode, xi, obs) plus the terminal observation kept from the stepped values.

tests/test_gpu_reset_dr.py pins the distributions of these draws and tests/test_gpu_launch_shapes.py the walker2d re-derive against
the oracle; neither compares the fused path with the reset kernel, and neither looks at t / episode / done or at the noisy reset
observation.

The half-cheetah ends only at the time limit (500 steps, no setter): its envs start with t = 499 - (i mod 48), so every env is
truncated once inside the 64 steps -- the same thing as a limit below 64.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, STEPS = 256, 64
SHAPES = {"pair": dict(lanes=64, pair=True, rolled=False), "one-lane": dict(lanes=64, pair=False, rolled=False)}


def _dr(env, mode):
    nom = np.asarray(env.original_task, dtype=np.float64)
    if mode == "uniform":
        env.set_dr_distribution("uniform", np.stack([0.9 * nom, 1.1 * nom], 1).ravel().tolist())
    elif mode == "truncnorm":
        env.set_dr_distribution("truncnorm", np.stack([nom, 0.1 * nom], 1).ravel().tolist())
    elif mode == "gaussian":      # wide enough that the redraw rule (< 0.1) fires on the light bodies
        env.set_dr_distribution("gaussian", np.stack([nom, 0.4 * nom], 1).ravel().tolist())
    elif mode == "fullgaussian":
        d = env.task_dim
        A = np.random.RandomState(0).randn(d, d) * 0.1
        env.set_dr_distribution("fullgaussian", {"mean": np.full(d, 2.0), "cov": A @ A.T + 0.05 * np.eye(d)})
    else:
        raise AssertionError(mode)
    env.set_dr_training(True)


def _make(torch, eid, mode, shape, autoreset):
    import random_envs_amd as rex
    env = rex.make(eid, batch=B, seed=11, autoreset=autoreset)
    got = env.set_launch_shape(**SHAPES[shape])
    assert got["pair"] == SHAPES[shape]["pair"] and got["lanes"] == 64 and not got["rolled"], got
    _dr(env, mode)
    env.reset()
    if "HalfCheetah" in eid:
        st = env.get_full_state()
        st["t"] = (499 - torch.arange(B, dtype=torch.int32) % 48).to(st["t"].device)
        env.set_full_state(st)
    return env


def _state(env):
    st = env.get_full_state()
    return {k: st[k].clone() for k in ("qpos", "qvel", "task", "t", "episode", "done")}


CASES = [("RandomHopper-v0", "uniform"), ("RandomHopper-v0", "truncnorm"), ("RandomHopper-v0", "gaussian"), ("RandomHopper-v0", "fullgaussian"),
         ("RandomWalker2d-v0", "uniform"), ("RandomWalker2d-v0", "truncnorm"), ("RandomHalfCheetahNoisy-v0", "uniform")]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("eid,mode", CASES)
def test_fused_reset_equals_step_then_masked_reset(eid, mode, shape):
    import torch
    fused = _make(torch, eid, mode, shape, True)
    split = _make(torch, eid, mode, shape, False)
    a0, b0 = _state(fused), _state(split)
    for k in a0:
        assert torch.equal(a0[k], b0[k]), (eid, mode, shape, "start", k)
    g = torch.Generator().manual_seed(5)
    finished = torch.zeros(B, dtype=torch.bool)
    resets = 0
    for step in range(STEPS):
        a = torch.rand(B, fused.dims.act_dim, generator=g) * 2 - 1
        tag = (eid, mode, shape, "step %d" % step)
        obs_f, r_f, d_f, info_f = fused.step(a)
        obs_f, r_f, d_f, term_f = obs_f.clone(), r_f.clone(), d_f.clone(), info_f["terminal_observation"].clone()
        obs_s, r_s, d_s, info_s = split.step(a)
        pre = obs_s.clone()                                    # the stepped observation of every env, finished ones included
        assert torch.equal(info_s["terminal_observation"], pre), tag
        assert torch.equal(d_f, d_s) and torch.equal(r_f.view(torch.int32), r_s.view(torch.int32)), tag
        assert torch.equal(info_f["TimeLimit.truncated"], info_s["TimeLimit.truncated"]), tag
        assert torch.equal(term_f.view(torch.int32), pre.view(torch.int32)), tag + ("terminal_observation",)
        if d_s.any():
            obs_s = split.reset(mask=d_s.to(torch.uint8)).clone()
        finished |= d_s.cpu(); resets += int(d_s.sum())
        assert torch.equal(obs_f.view(torch.int32), obs_s.view(torch.int32)), tag + ("obs",)
        sf, ss = _state(fused), _state(split)
        for k in sf:
            x, y = sf[k], ss[k]
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), tag + (k,)
    print("%s %s %s: %d of %d envs finished at least once, %d resets" % (eid, mode, shape, int(finished.sum()), B, resets))
    assert int(finished.sum()) >= B // 4, (eid, mode, shape, int(finished.sum()))   # on the path this comparison takes as given
    fused.close(); split.close()
