"""The HIP step kernels against the first-principles reference (tests/first_principles_oracle.py), never the oracle: the airborne,
spinning, constraint-free states of tests/test_first_principles_host.py through rex.make(..., autoreset=False), set_task, set_state, one
step, get_state, at the smallest shapes that reach every step kernel -- planar kinds at 33 envs two lanes per env (a full wave plus a lone
env) and 65 envs one lane per env, the hopper's rolled kernel, walker2d with per-lane xi lengths from every rendered size in the pair
kernel, the one-lane kernel and the one-lane kernel with REX_FUSED_DERIVE=0; the humanoid at 33 envs in its pair shape, 65 envs with
REX_HUM_PAIR=0 and 65 envs in 64-lane blocks, plus rex_get_obs after set_state for the cinert / cvel blocks.

The project's own fp32 tolerances, EVERY lane, no lane left out, no conditioning escape (no constraint is active, nothing is
ill-conditioned): planar |dqpos| <= 5e-5 and |dqvel| / (1 + |qvel|inf) <= 5e-4; humanoid obs rel <= 2e-4 and qvel rel <= 5e-4; the
forward-only observation <= 2e-5.

Worst errors measured on an MI355X (over the shapes of each kind): hopper |dqpos| 3.7e-7, qvel rel 2.1e-7; walker2d 3.3e-7,
1.1e-6; half-cheetah 4.5e-7, 3.9e-7; humanoid set_state obs rel 5.4e-7, step obs rel 2.9e-6, qvel rel 1.4e-5.  11 cases, 4 s."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDS = {"hopper": "RandomHopper-v0", "walker2d": "RandomWalker2d-v0", "halfcheetah": "RandomHalfCheetah-v0", "humanoid": "RandomHumanoid-v0"}
TOL_QPOS, TOL_QVEL_REL = 5e-5, 5e-4
TOL_HUM_OBS, TOL_HUM_QVEL, TOL_FORWARD_OBS = 2e-4, 5e-4, 2e-5


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_CACHE = {}


def _sample(kind):
    """kept states of `kind` and the reference's step from them (walker2d: every rendered size, interleaved so that neighbouring lanes
    carry different lengths); computed once"""
    if kind not in _CACHE:
        from test_first_principles_host import WALKER_KEYS, kept_states, reference_side
        keys = WALKER_KEYS if kind == "walker2d" else [None]
        parts = []
        for key in keys:
            s, ref = kept_states(kind, key), reference_side(kind, key)
            parts.append(dict(q=s["q"], v=s["v"], a=s["a"], xi=s["xi"], qpos=ref["qpos"], qvel=ref["qvel"],
                              **({"reset": ref["reset"], "step": ref["step"]} if kind == "humanoid" else {})))
        n = min(len(p["q"]) for p in parts)
        order = np.arange(n * len(parts)).reshape(len(parts), n).T.ravel()         # size 0 state 0, size 1 state 0, ...
        _CACHE[kind] = {k: np.concatenate([p[k][:n] for p in parts])[order] for k in ("q", "v", "a", "xi", "qpos", "qvel")}
        if kind == "humanoid":
            _CACHE[kind].update(reset=parts[0]["reset"], step=parts[0]["step"])
    return _CACHE[kind]


def _hum_obs(qpos, qvel, blocks):
    """the 376-dim observation from the reference's quantities (random_humanoid.py:207-216; the world body's rows and cfrc_ext are zeros)"""
    n = len(qpos)
    return np.concatenate([qpos[:, 2:], qvel, np.zeros((n, 10)), blocks["cinert"].reshape(n, -1), np.zeros((n, 6)),
                           blocks["cvel"].reshape(n, -1), blocks["qfrc_actuator"], np.zeros((n, 84))], 1)


def _make(kind, B, knobs):
    import random_envs_amd as rex
    from parity_util import create_knobs
    with create_knobs(**knobs):
        return rex.make(IDS[kind], batch=B, autoreset=False)


PLANAR_CASES = [(k, 33, dict(pair=True), {}) for k in ("hopper", "walker2d", "halfcheetah")] + \
               [("hopper", 65, dict(pair=False, rolled=False), {}), ("hopper", 65, dict(pair=False, rolled=True), {}),
                ("walker2d", 65, dict(pair=False), {}), ("walker2d", 65, dict(pair=False), dict(REX_FUSED_DERIVE=0)),
                ("halfcheetah", 65, dict(pair=False), {})]


@pytest.mark.parametrize("kind,B,shape,knobs", PLANAR_CASES,
                         ids=["%s-%d-%s%s" % (k, B, "-".join("%s%d" % kv for kv in sorted(s.items())), "-fused_derive0" if kn else "") for k, B, s, kn in PLANAR_CASES])
def test_planar_step_matches_first_principles(torch_mod, kind, B, shape, knobs):
    torch = torch_mod
    s = _sample(kind)
    idx = np.arange(B) % len(s["q"])
    env = _make(kind, B, knobs)
    got = env.set_launch_shape(**shape)
    assert all(got[k] == v for k, v in shape.items()), (shape, got)
    env.set_task(s["xi"][idx].astype(np.float32)); env.set_state(s["q"][idx], s["v"][idx])
    env.step(torch.as_tensor(s["a"][idx], dtype=torch.float32))
    qq, vv = [x.cpu().numpy().astype(np.float64) for x in env.get_state()]
    c = env.counters()
    env.close()
    eq = np.abs(qq - s["qpos"][idx]).max(1)
    ev = np.abs(vv - s["qvel"][idx]).max(1) / (1 + np.abs(s["qvel"][idx]).max(1))
    print("%s B=%d %s %s: worst |dqpos| %.2e, worst relative |dqvel| %.2e over %d lanes" % (kind, B, got, knobs, eq.max(), ev.max(), B))
    assert c["nonfinite"] == 0 and c["overflow"] == 0 and c["solver_capped"] == 0, c
    assert np.isfinite(eq).all() and np.isfinite(ev).all()
    assert eq.max() <= TOL_QPOS, np.where(eq > TOL_QPOS)[0]
    assert ev.max() <= TOL_QVEL_REL, np.where(ev > TOL_QVEL_REL)[0]


HUM_CASES = [("pair", 33, dict(hum_pair=True), {}), ("one_lane", 65, dict(hum_pair=False), dict(REX_HUM_PAIR=0)),
             ("lanes64", 65, dict(lanes=64), dict(REX_LANES=64))]


@pytest.mark.parametrize("tag,B,expect,knobs", HUM_CASES, ids=[c[0] for c in HUM_CASES])
def test_humanoid_step_and_observation_match_first_principles(torch_mod, tag, B, expect, knobs):
    torch = torch_mod
    from random_envs_amd import _native
    s = _sample("humanoid")
    idx = np.arange(B) % len(s["q"])
    env = _make("humanoid", B, knobs)
    sh = env.launch_shape()
    assert all(sh[k] == v for k, v in expect.items()), (expect, sh)
    env.set_task(s["xi"][idx].astype(np.float32)); env.set_state(s["q"][idx], s["v"][idx])
    # set_state -> forward -> observation: cinert / cvel (and qfrc_actuator = 0) with nothing integrated
    of = torch.empty(376, B, device="cuda")
    _native.check(_native.lib().rex_get_obs(env._h, ctypes.c_void_p(of.data_ptr()), env._stream()))
    of = of.t().cpu().numpy().astype(np.float64)
    want = _hum_obs(s["q"], s["v"], s["reset"])[idx]
    ef = np.abs(of - want).max(1) / (1 + np.abs(want).max(1))
    # one step
    obs = env.step(torch.as_tensor(s["a"][idx], dtype=torch.float32))[0].cpu().numpy().astype(np.float64)
    qq, vv = [x.cpu().numpy().astype(np.float64) for x in env.get_state()]
    c = env.counters()
    env.close()
    want = _hum_obs(s["qpos"], s["qvel"], s["step"])[idx]
    eo = np.abs(obs - want).max(1) / (1 + np.abs(want).max(1))
    ev = np.abs(vv - s["qvel"][idx]).max(1) / (1 + np.abs(s["qvel"][idx]).max(1))
    print("humanoid %s B=%d %s: set_state obs rel %.2e, step obs rel %.2e, qvel rel %.2e over %d lanes" % (tag, B, sh, ef.max(), eo.max(), ev.max(), B))
    assert c["nonfinite"] == 0 and c["overflow"] == 0 and c["solver_capped"] == 0, c
    assert np.isfinite(ef).all() and np.isfinite(eo).all() and np.isfinite(ev).all()
    assert ef.max() <= TOL_FORWARD_OBS, np.where(ef > TOL_FORWARD_OBS)[0]
    assert eo.max() <= TOL_HUM_OBS, np.where(eo > TOL_HUM_OBS)[0]
    assert ev.max() <= TOL_HUM_QVEL, np.where(ev > TOL_HUM_QVEL)[0]
