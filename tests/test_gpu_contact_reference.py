"""The HIP step kernels against the contact reference's env step (tests/contact_reference.py through tests/test_contact_reference_host.py),
never the oracle: states WITH floor contacts, joint limits, partly active friction pyramids, two feet on the floor, the hopper's three
capsule-capsule pairs and the humanoid's row-count classes (1-16, 17-21, 22-64, > 64 rows), through rex.make(..., autoreset=False),
set_task, set_state, one step, get_state.  Every sample is ordered round-robin by class, so the first 33 states of each hold every class.

Shapes, the smallest that reach every step kernel: planar kinds at 33 envs two lanes per env and 65 envs one lane per env; the hopper
also rolled, and with REX_FAST=0 beside REX_PAIR=1 (every evaluation through the LIST solver); walker2d also with REX_FUSED_DERIVE=0;
the humanoid at 33 envs in its pair shape, 65 envs with REX_HUM_PAIR=0 and 65 envs in 64-lane blocks.

Gates: the project's per-lane gates of each state family (test_contact_reference_host.GATES: planar box 2e-5 / 2e-4, folded hopper 5e-5 /
5e-4, humanoid |dqpos| 2e-4 and qvel 5e-4, crouched and pile-ups qvel 1e-4 with K = 256), on |dqpos| and |dqvel|rel alike, through parity_util.assert_lanes_explained, at most 1 % of the lanes by
the explained clause.  Its conditioning estimate is oracle_sensitivity (the CPU module holds the oracle to the reference on these same
states); the comparison itself is against the reference.

Worst errors measured on an MI355X, |dqpos| / |dqvel|rel over the shapes of each sample: hopper uniform 1.6e-7 / 4.0e-7, corners 1.5e-7 /
5.8e-6, folded 3.3e-7 / 1.5e-6; walker2d uniform 2.0e-7 / 4.7e-6, corners 3.6e-7 / 7.7e-7; half-cheetah uniform 1.2e-6 / 5.6e-6, corners
5.6e-6 / 1.1e-5; humanoid standing 9.9e-7 / 4.1e-6, crouched 5.2e-7 / 1.5e-6, pile-ups 6.5e-7 / 1.9e-6.  No lane above its tolerance, none
explained.  12 cases, 14 s.  (Before capsule_capsule_2d took the closest points of crossing axes as one point, the folded sample missed its gate in
a quarter of its lanes: tests/test_contact_reference_host.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDS = {"hopper": "RandomHopper-v0", "walker2d": "RandomWalker2d-v0", "halfcheetah": "RandomHalfCheetah-v0", "humanoid": "RandomHumanoid-v0"}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _make(kind, B, knobs):
    import random_envs_amd as rex
    from parity_util import create_knobs
    with create_knobs(**knobs):
        return rex.make(IDS[kind], batch=B, autoreset=False)


def _step(torch, env, name, B):
    """lane i steps state i mod n_step of the sample; (qpos, qvel, counters, idx)"""
    from test_contact_reference_host import n_step, sample
    s = sample(name); idx = np.arange(B) % n_step(name)
    env.set_task(s["xi"][idx].astype(np.float32)); env.set_state(s["q"][idx], s["v"][idx])
    env.step(torch.as_tensor(s["a"][idx], dtype=torch.float32))
    qq, vv = [x.cpu().numpy().astype(np.float64) for x in env.get_state()]
    return qq, vv, env.counters(), idx


PLANAR_CASES = [(k, 33, dict(pair=True), {}) for k in ("hopper", "walker2d", "halfcheetah")] + \
               [("hopper", 33, dict(pair=True), dict(REX_FAST=0, REX_PAIR=1)),
                ("hopper", 65, dict(pair=False, rolled=False), {}), ("hopper", 65, dict(pair=False, rolled=True), {}),
                ("walker2d", 65, dict(pair=False), {}), ("walker2d", 65, dict(pair=False), dict(REX_FUSED_DERIVE=0)),
                ("halfcheetah", 65, dict(pair=False), {})]


@pytest.mark.parametrize("kind,B,shape,knobs", PLANAR_CASES,
                         ids=["%s-%d-%s%s" % (k, B, "-".join("%s%d" % kv for kv in sorted(s.items())), "".join("-%s%s" % kv for kv in sorted(kn.items()))) for k, B, s, kn in PLANAR_CASES])
def test_planar_step_matches_the_contact_reference(torch_mod, kind, B, shape, knobs):
    from test_contact_reference_host import gate_lanes
    for fam in ("uniform", "corners") + (("folded",) if kind == "hopper" else ()):
        name = "%s-%s" % (kind, fam)
        env = _make(kind, B, knobs)
        got = env.set_launch_shape(**shape)
        assert all(got[k] == v for k, v in shape.items()), (shape, got)
        qq, vv, c, idx = _step(torch_mod, env, name, B)
        env.close()
        assert c["nonfinite"] == 0 and c["overflow"] == 0 and c["solver_capped"] == 0, c
        gate_lanes(name, qq, vv, "%s B=%d %s %s" % (name, B, got, knobs), idx)


HUM_CASES = [("pair", 33, dict(hum_pair=True), {}), ("one_lane", 65, dict(hum_pair=False), dict(REX_HUM_PAIR=0)),
             ("lanes64", 65, dict(lanes=64), dict(REX_LANES=64))]


@pytest.mark.parametrize("tag,B,expect,knobs", HUM_CASES, ids=[c[0] for c in HUM_CASES])
def test_humanoid_step_matches_the_contact_reference(torch_mod, tag, B, expect, knobs):
    from test_contact_reference_host import gate_lanes, reference_step
    for fam in ("standing", "crouched", "pileup"):
        name = "humanoid-" + fam
        env = _make("humanoid", B, knobs)
        sh = env.launch_shape()
        assert all(sh[k] == v for k, v in expect.items()), (expect, sh)
        qq, vv, c, idx = _step(torch_mod, env, name, B)
        env.close()
        bad_ref = int((~np.isfinite(reference_step(name)["qvel"][idx]).all(1)).sum())
        assert c["overflow"] == 0 and c["nonfinite"] <= bad_ref, c          # (as the oracle tests of these families)
        if fam == "standing":
            assert c["nonfinite"] == 0 and c["solver_capped"] == 0, c
        gate_lanes(name, qq, vv, "%s %s B=%d %s" % (name, tag, B, sh), idx)
