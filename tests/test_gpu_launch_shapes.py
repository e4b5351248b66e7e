"""Every launch shape the public API accepts, and the three walker2d derive paths of the auto-reset under DR, against the fp64 oracle.

The step kernels' arithmetic depends on the launch shape (which envs share a wave, which solver instantiation the wave enters, the
XCD-transposed block order of the narrow two-lanes-per-env blocks, the LDS column of the list solver), so each shape is pinned with
`set_launch_shape` and held to the oracle on every lane.  Oracle references and their sensitivities are computed once per chain (module
cache) and tiled over the batch with a period that is a multiple of the envs per wave: every copy in a whole wave must then be
bit-identical to the first, which a block order that skips or doubles an env group cannot fake.

Walker2d under DR re-derives a finished env's geometry from its newly drawn lengths in one of three places: inline in the pair kernel
(path 1, the default up to 32 768 envs), as a call from the one-lane kernel (path 2, up to 524 287 envs) or in a derive launch behind a
separate reset launch (path 3, `fused_derive` off: 524 288 envs and up).  Resets are forced on known lanes, and the step after the reset is
checked against the oracle, which compiles the geometry from xi itself: stale device geometry fails there."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDS = {"hopper": "RandomHopper-v0", "walker2d": "RandomWalker2d-v0", "halfcheetah": "RandomHalfCheetah-v0"}
# per-lane gates (parity_util.assert_lanes_explained), the same as tests/test_gpu_planar.py
TOL_QPOS, CAP_QPOS = 2e-5, 5e-4
TOL_QVEL_REL, CAP_QVEL_REL = 2e-4, 2e-2
TOL_REWARD, CAP_REWARD = 5e-3, 1e-1
# ... and tests/test_gpu_humanoid.py
TOL_OBS, CAP_OBS = 2e-4, 2e-2
TOL_REW, CAP_REW = 2e-3, 2e-1

P_PLANAR, P_HUM = 512, 256     # oracle-checked states per chain: multiples of every envs-per-wave count (4 .. 64)
LANES = (8, 16, 32, 64)
# planar batches: 2 045 envs give 8 m two-lanes-per-env blocks at every width (the XCD transpose active below 64 lanes) with a ragged
# last block; 2 049 give an odd block count (transpose off), again ragged
B_XCD, B_ODD = 2045, 2049
B_HUM = 4 * P_HUM - 3


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _done_margin(kind, qpos):
    """distance of the reference end state to the nearest threshold of the done rule (random_hopper.py:92, random_walker2d.py:124-125)"""
    z, th = qpos[:, 1], qpos[:, 2]
    if kind == "hopper":
        return np.minimum(np.abs(z - 0.7), np.abs(np.abs(th) - 0.2))
    if kind == "walker2d":
        return np.minimum.reduce([np.abs(z - 0.8), np.abs(z - 2.0), np.abs(th - 1.0), np.abs(th + 1.0)])
    return np.full(len(z), np.inf)


def _obs_parts(nq):
    """oracle step returning the observation split into its qpos and qvel parts (separate gates)"""
    def split(out):
        out = dict(out)
        out["oq"], out["ov"] = out["obs"][:, :nq - 1], out["obs"][:, nq - 1:]
        return out
    return split


_CACHE = {}


def _planar_ref(kind):
    """P_PLANAR rollout states, actions and the oracle's step from them with its sensitivity (computed once per chain)"""
    if kind not in _CACHE:
        from oracle_bindings import DIMS, oracle_batch_step, oracle_sensitivity, rollout_states
        q, v, xi = rollout_states(kind, P_PLANAR, steps_max=60, seed=31)
        q, v, xi = _f32(q), _f32(v), _f32(xi)
        a = _f32(np.random.RandomState(32).uniform(-1.2, 1.2, (P_PLANAR, DIMS[kind]["nu"])))
        ref, sens = oracle_sensitivity(lambda q_, v_, a_, x_: oracle_batch_step(kind, q_, v_, a_, x_), [q, v, a, xi], ["qpos", "qvel", "reward"])
        _CACHE[kind] = (q, v, a, xi, ref, sens)
    return _CACHE[kind]


def _hum_ref():
    if "humanoid" not in _CACHE:
        from oracle_bindings import oracle_humanoid_reset_obs, oracle_humanoid_step, oracle_sensitivity
        from random_envs_amd.specs import SPECS
        rng = np.random.RandomState(33); n = P_HUM
        nom = np.array(SPECS["humanoid"].nominal_task)
        q = np.tile(np.array([0, 0, 1.4, 1, 0, 0, 0] + [0] * 17, dtype=float), (n, 1)) + rng.uniform(-.01, .01, (n, 24))
        q[:, 7:] += rng.uniform(-.3, .3, (n, 17)); q[:, 2] = rng.uniform(1.0, 1.45, n)
        v = rng.uniform(-1, 1, (n, 23)); a = rng.uniform(-.5, .5, (n, 17)); xi = nom * rng.uniform(.8, 1.2, (n, 30))
        q, v, a, xi = _f32(q), _f32(v), _f32(a), _f32(xi)
        ref, sens = oracle_sensitivity(lambda q_, v_, a_, x_: oracle_humanoid_step(q_, v_, a_, x_), [q, v, a, xi], ["obs", "reward"], trials=2)
        # a second state for the set_state -> forward observation
        q2 = q.copy(); q2[:, 7:] += rng.uniform(-.4, .4, (n, 17)); q2 = _f32(q2); v2 = _f32(rng.uniform(-2, 2, (n, 23)))
        obs2, _ = oracle_humanoid_reset_obs(q2, v2, xi)
        _CACHE["humanoid"] = (q, v, a, xi, ref, sens, q2, v2, obs2)
    return _CACHE["humanoid"]


def _pin(env, **shape):
    got = env.set_launch_shape(**shape)
    assert env.launch_shape() == got and all(got[k] == bool(w) if k != "lanes" else got[k] == w for k, w in shape.items()), (shape, got)
    return got


def _planar_case(torch, kind, B, shape, knobs=None):
    """One step of B envs tiled from the chain's oracle-checked states under the pinned `shape`: every lane against the oracle, whole waves
    bit-identical to the first copy, obs = concat(qpos[1:], qvel), done explained, no non-finite lane, no capped solve."""
    import random_envs_amd as rex
    from parity_util import assert_done_explained, assert_lanes_explained, create_knobs
    q, v, a, xi, ref, sens = _planar_ref(kind)
    idx = np.arange(B) % P_PLANAR
    with create_knobs(**(knobs or {})):
        env = rex.make(IDS[kind], batch=B, autoreset=False)
    sh = _pin(env, **shape)
    env.set_task(xi[idx].astype(np.float32)); env.set_state(q[idx], v[idx])
    obs, r, dn, _ = env.step(torch.as_tensor(a[idx], dtype=torch.float32))
    qq, vv = env.get_state()
    obs, r, dn, qq, vv = [x.cpu().numpy() for x in (obs, r, dn, qq, vv)]
    c = env.counters()
    env.close()
    tag = "%s B=%d %s" % (kind, B, sh)
    assert c["nonfinite"] == 0 and c["solver_capped"] == 0, (tag, c)
    assert np.array_equal(obs, np.concatenate([qq[:, 1:], vv], 1)), tag
    eq = np.abs(qq - ref["qpos"][idx]).max(1)
    vs = 1 + np.abs(ref["qvel"][idx]).max(1)
    ev = np.abs(vv - ref["qvel"][idx]).max(1) / vs
    assert_lanes_explained(eq, sens["qpos"][idx], TOL_QPOS, CAP_QPOS, label=tag + " |dqpos|")
    assert_lanes_explained(ev, sens["qvel"][idx] / vs, TOL_QVEL_REL, CAP_QVEL_REL, label=tag + " |dqvel|rel")
    assert_lanes_explained(np.abs(r - ref["reward"][idx]), sens["reward"][idx], TOL_REWARD, CAP_REWARD, label=tag + " |dreward|")
    assert_done_explained(dn, ref["done"][idx], _done_margin(kind, ref["qpos"])[idx], 2e-5, label=tag)
    # every env stepped exactly once: a lane in a whole wave sits in a wave of the same envs as its first copy does
    epw = sh["lanes"] // 2 if sh["pair"] else sh["lanes"]
    full = (B // epw) * epw
    for x in (qq, vv, r):
        bad = np.where((x[:full] != x[:P_PLANAR][idx[:full]]).reshape(full, -1).any(1))[0]
        assert bad.size == 0, (tag, "lanes differ from their first copy", bad[:10])
    return qq, vv, r


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("kind", ["hopper", "walker2d", "halfcheetah"])
def test_pair_shapes_match_the_oracle(torch_mod, kind, lanes):
    """two lanes per env at 8 / 16 / 32 / 64 lanes per block: 8 m blocks with a ragged last one (XCD-transposed order below 64 lanes)
    and an odd block count (launch order)"""
    for B in (B_XCD, B_ODD):
        blocks = -(-2 * B // lanes)
        assert (blocks % 8 == 0) == (B == B_XCD) and (2 * B) % lanes != 0
        _planar_case(torch_mod, kind, B, dict(lanes=lanes, pair=True))


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("kind", ["hopper", "walker2d", "halfcheetah"])
def test_one_lane_shapes_match_the_oracle(torch_mod, kind, lanes):
    shape = dict(lanes=lanes, pair=False)
    if kind == "hopper":
        shape["rolled"] = False
    _planar_case(torch_mod, kind, B_XCD, shape)


@pytest.mark.parametrize("lanes", [32, 64])
def test_rolled_shapes_match_the_oracle(torch_mod, lanes):
    """the hopper's two-waves-per-SIMD kernel (rolled general solver)"""
    _planar_case(torch_mod, "hopper", B_XCD, dict(lanes=lanes, pair=False, rolled=True))


@pytest.mark.parametrize("kind", ["hopper", "walker2d", "halfcheetah"])
def test_one_lane_widths_are_lane_independent_without_the_fast_path(torch_mod, kind):
    """REX_FAST=0 (one solver instantiation for every wave): a lane's arithmetic does not depend on its wave, so the one-lane kernel gives
    the same bits at every block width"""
    outs = []
    for lanes in LANES:
        shape = dict(lanes=lanes, pair=False)
        if kind == "hopper":
            shape["rolled"] = False
        outs.append(_planar_case(torch_mod, kind, B_XCD, shape, knobs=dict(REX_FAST=0)))
    for lanes, o in zip(LANES[1:], outs[1:]):
        for x, x0 in zip(o, outs[0]):
            assert np.array_equal(x, x0), (kind, lanes)


def _hum_case(torch, shape):
    import ctypes
    import random_envs_amd as rex
    from random_envs_amd import _native
    from oracle_bindings import oracle_humanoid_reset_obs
    from parity_util import assert_done_explained, assert_lanes_explained
    q, v, a, xi, ref, sens, q2, v2, obs2 = _hum_ref()
    B = B_HUM
    idx = np.arange(B) % P_HUM
    env = rex.make("RandomHumanoid-v0", batch=B, autoreset=False)
    sh = _pin(env, **shape)
    tag = "humanoid B=%d %s" % (B, sh)
    env.set_task(xi[idx].astype(np.float32)); env.set_state(q[idx], v[idx])
    obs, r, dn, _ = env.step(torch.as_tensor(a[idx], dtype=torch.float32))
    o = obs.cpu().numpy().astype(np.float64); r = r.cpu().numpy().astype(np.float64); dn = dn.cpu().numpy()
    qq, _ = env.get_state(); qq = qq.cpu().numpy()
    os_ = 1 + np.abs(ref["obs"][idx]).max(1)
    assert_lanes_explained(np.abs(o - ref["obs"][idx]).max(1) / os_, sens["obs"][idx] / os_, TOL_OBS, CAP_OBS, label=tag + " |dobs|rel")
    assert_lanes_explained(np.abs(r - ref["reward"][idx]), sens["reward"][idx], TOL_REW, CAP_REW, label=tag + " |dreward|")
    z = ref["qpos"][:, 2]
    assert_done_explained(dn, ref["done"][idx], np.minimum(np.abs(z - 1.0), np.abs(z - 2.0))[idx], 2e-5, label=tag)
    epw = 32 if sh["hum_pair"] else sh["lanes"]
    full = (B // epw) * epw
    for x in (o, r, qq):
        bad = np.where((x[:full] != x[:P_HUM][idx[:full]]).reshape(full, -1).any(1))[0]
        assert bad.size == 0, (tag, "lanes differ from their first copy", bad[:10])
    # set_state -> sim.forward() -> _get_obs (humanoid_forward_kernel at this block width)
    env.set_state(q2[idx], v2[idx])
    of = torch.empty(376, B, device="cuda")
    _native.check(_native.lib().rex_get_obs(env._h, ctypes.c_void_p(of.data_ptr()), env._stream()))
    of = of.t().cpu().numpy().astype(np.float64)
    e = np.abs(of - obs2[idx]).max(1) / (1 + np.abs(obs2[idx]).max(1))
    assert e.max() < 2e-5, (tag, "set_state obs", e.max())
    # reset() (humanoid_reset_kernel at this block width): the new state's observation with the task in force
    ro = env.reset().cpu().numpy().astype(np.float64)
    qr, vr = env.get_state()
    qr, vr = qr.cpu().numpy().astype(np.float64), vr.cpu().numpy().astype(np.float64)
    ref_r, _ = oracle_humanoid_reset_obs(qr, vr, xi[idx])
    e = np.abs(ro - ref_r).max(1) / (1 + np.abs(ref_r).max(1))
    assert e.max() < 2e-5, (tag, "reset obs", e.max())
    c = env.counters()
    env.close()
    assert c["nonfinite"] == 0 and c["overflow"] == 0, (tag, c)


@pytest.mark.parametrize("lanes", LANES)
def test_humanoid_one_lane_shapes_match_the_oracle(torch_mod, lanes):
    _hum_case(torch_mod, dict(lanes=lanes, hum_pair=False))


def test_humanoid_pair_with_narrow_reset_and_forward_blocks(torch_mod):
    """the pair step kernel always runs 64-lane blocks; the reset and forward kernels run `lanes`"""
    _hum_case(torch_mod, dict(lanes=16, hum_pair=True))


# ------------------------------------------------------------------------------------------- walker2d auto-reset under DR
QPOS0_WALKER = np.array([0, 1.25, 0, 0, 0, 0, 0, 0, 0], dtype=float)
# a forced reset: torso height 0.7 < 0.8 with both legs folded inside their joint ranges, so that no foot reaches the floor at any length
# the DR draws (no contact rows: a deep penetration of straight legs is an fp32-ill-conditioned state, not a test of the reset)
FORCED_POSE = np.array([0, 0.7, 0, -1.0, -1.5, 0, -1.0, -1.5, 0])


def _walker_env(eid, B, path=None, seed=3, env_offset=0):
    """walker2d under truncnorm DR over every task parameter (lengths included), training on, auto-reset on.  path 1: the pair kernel,
    2: the one-lane kernel, 3: REX_FUSED_DERIVE=0 on the one-lane kernel; None: what rex_create picks."""
    import random_envs_amd as rex
    from parity_util import create_knobs
    with create_knobs(REX_FUSED_DERIVE=0 if path == 3 else None):
        env = rex.make(eid, batch=B, seed=seed, env_offset=env_offset)
    if path is not None:
        _pin(env, pair=path == 1)
    mean = np.array(env.spec.nominal_task); std = 0.1 * mean
    env.set_dr_distribution("truncnorm", np.stack([mean, std], 1).ravel().tolist()); env.set_dr_training(True)
    return env, mean, std


def _split_gates(tag, obs, ref, sens, nq):
    """end-of-step observation against the oracle: its qpos part absolutely, its qvel part relatively"""
    from parity_util import assert_lanes_explained
    oq, ov = obs[:, :nq - 1], obs[:, nq - 1:]
    vs = 1 + np.abs(ref["ov"]).max(1)
    assert_lanes_explained(np.abs(oq - ref["oq"]).max(1), sens["oq"], TOL_QPOS, CAP_QPOS, label=tag + " |dqpos|")
    assert_lanes_explained(np.abs(ov - ref["ov"]).max(1) / vs, sens["ov"] / vs, TOL_QVEL_REL, CAP_QVEL_REL, label=tag + " |dqvel|rel")


def _lengths(xi, variant):
    """columns of the task that are lengths: full task xi[7:11]; Unmodeled xi[4:7] (its torso length is frozen)"""
    return slice(4, 7) if variant else slice(7, 11)


def _forced_reset_and_next_step(torch, env, mean, std, variant, forced, check, seed, tag):
    """Force the `forced` lanes to finish (FORCED_POSE; the oracle agrees they are done), step, check the `check` lanes
    against the oracle from the snapshot taken before the step, the reset lanes' new task and state, then step again and check the
    `check` lanes against the oracle from the new (q, v, xi).  Returns every device output in order, for bit comparisons."""
    from oracle_bindings import oracle_batch_step, oracle_sensitivity
    from parity_util import assert_done_explained, assert_lanes_explained
    B = env.batch; nq = 9
    step = lambda q_, v_, a_, x_: _obs_parts(nq)(oracle_batch_step("walker2d", q_, v_, a_, x_, variant=variant))
    rng = np.random.RandomState(seed)
    outs = []
    q, v = env.get_state()
    q = q.cpu().numpy().astype(np.float64); v = v.cpu().numpy().astype(np.float64)
    v = _f32(v + rng.uniform(-0.5, 0.5, v.shape))
    q[forced] = FORCED_POSE
    xi0 = env.get_task().cpu().numpy().astype(np.float64)
    env.set_state(q, v)
    a = _f32(rng.uniform(-1, 1, (B, 6)))
    ref, sens = oracle_sensitivity(step, [q[check], v[check], a[check], xi0[check]], ["oq", "ov", "reward"], trials=2)
    fpos = np.searchsorted(check, forced)
    assert np.array_equal(check[fpos], forced) and ref["done"][fpos].all(), tag
    obs, r, d, info = env.step(torch.as_tensor(a, dtype=torch.float32))
    outs += [obs.clone(), r.clone(), d.clone(), info["terminal_observation"].clone()]
    obs, r, d = obs.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
    term = info["terminal_observation"].cpu().numpy().astype(np.float64)
    assert d[forced].all(), tag
    assert_done_explained(d[check], ref["done"], _done_margin("walker2d", ref["qpos"]), 2e-5, label=tag + " step 1")
    same = d[check] == ref["done"]
    # every lane's end-of-step observation (the terminal observation of a finished lane) and reward
    _split_gates(tag + " step 1", term[check][same], {k: ref[k][same] for k in ("oq", "ov")}, {k: sens[k][same] for k in ("oq", "ov")}, nq)
    assert_lanes_explained(np.abs(r[check] - ref["reward"])[same], sens["reward"][same], TOL_REWARD, CAP_REWARD, label=tag + " step 1 |dreward|")
    # the lanes that went on: state = the step's end state
    q1, v1 = env.get_state()
    q1 = q1.cpu().numpy().astype(np.float64); v1 = v1.cpu().numpy().astype(np.float64)
    xi1 = env.get_task().cpu().numpy().astype(np.float64)
    outs += [torch.as_tensor(q1), torch.as_tensor(v1), torch.as_tensor(xi1)]
    live = ~d
    assert np.array_equal(obs[live], np.concatenate([q1[live, 1:], v1[live]], 1)) and np.array_equal(term[live], obs[live]), tag
    assert np.array_equal(xi1[live], xi0[live]), tag
    # the lanes that finished: a redrawn task inside +-2 std, the reset state inside the init noise, its observation returned
    fin = np.where(d)[0]
    assert fin.size >= forced.size
    assert (xi1[fin] != xi0[fin]).any(1).all(), tag
    assert np.abs((xi1[fin] - mean) / std).max() <= 2 + 1e-4, tag
    assert np.abs(q1[fin] - QPOS0_WALKER).max() <= 0.005 + 1e-6 and np.abs(v1[fin]).max() <= 0.005 + 1e-7, tag
    assert np.array_equal(obs[fin], np.concatenate([q1[fin, 1:], v1[fin]], 1)), tag
    # the next step from the new (q, v, xi): the oracle compiles each lane's geometry (and, for the Unmodeled id, the frozen masses
    # 1..3 derived from the new lengths, random_walker2d_unmodeled.py:109-116) from xi
    a2 = _f32(rng.uniform(-1, 1, (B, 6)))
    ref2, sens2 = oracle_sensitivity(step, [q1[check], v1[check], a2[check], xi1[check]], ["oq", "ov", "reward"], trials=2)
    obs2, r2, d2, info2 = env.step(torch.as_tensor(a2, dtype=torch.float32))
    outs += [obs2.clone(), r2.clone(), d2.clone(), info2["terminal_observation"].clone()]
    term2 = info2["terminal_observation"].cpu().numpy().astype(np.float64)[check]
    r2 = r2.cpu().numpy()[check]
    _split_gates(tag + " step 2", term2, ref2, sens2, nq)
    assert_lanes_explained(np.abs(r2 - ref2["reward"]), sens2["reward"], TOL_REWARD, CAP_REWARD, label=tag + " step 2 |dreward|")
    # ... and the check has teeth: the reset lanes stepped with their OLD lengths land far from the device
    fc = np.intersect1d(fin, check)
    fcpos = np.searchsorted(check, fc)
    xs = xi1[fc].copy(); ls = _lengths(xs, variant); xs[:, ls] = xi0[fc][:, ls]
    stale = step(q1[fc], v1[fc], a2[fc], xs)
    vs = 1 + np.abs(stale["ov"]).max(1)
    miss = np.maximum(np.abs(term2[fcpos, :nq - 1] - stale["oq"]).max(1) / TOL_QPOS,
                      np.abs(term2[fcpos, nq - 1:] - stale["ov"]).max(1) / vs / TOL_QVEL_REL)
    print("%s: stale-length oracle misses the device by %.0fx the tolerance (median over %d reset lanes)" % (tag, np.median(miss), fc.size))
    assert np.median(miss) > 100, (tag, np.median(miss))
    if variant:   # stale frozen masses (the geometry-derived ones of the OLD lengths) miss as well
        from oracle_bindings import oracle_constants
        full = np.empty((fc.size, 13))
        for j, k in enumerate(fc):
            full[j, 0:3] = oracle_constants("walker2d", size=[0.32] + list(xi0[k, 4:7]))["body_mass"][1:4]
        full[:, 3:7] = xi1[fc, 0:4]; full[:, 7] = 0.32; full[:, 8:11] = xi1[fc, 4:7]; full[:, 11:13] = xi1[fc, 7:9]
        sm = _obs_parts(nq)(oracle_batch_step("walker2d", q1[fc], v1[fc], a2[fc], full))
        vs = 1 + np.abs(sm["ov"]).max(1)
        miss_m = np.abs(term2[fcpos, nq - 1:] - sm["ov"]).max(1) / vs / TOL_QVEL_REL
        print("%s: stale-mass oracle misses the device by %.0fx the tolerance (median)" % (tag, np.median(miss_m)))
        assert np.median(miss_m) > 5, (tag, np.median(miss_m))
    c = env.counters()
    assert c["nonfinite"] == 0 and c["solver_capped"] == 0, (tag, c)
    return outs


WALKER_DR_IDS = [("RandomWalker2d-v0", 0), ("RandomWalker2dUnmodeled-v0", 1)]


@pytest.mark.parametrize("eid,variant", WALKER_DR_IDS)
def test_walker_autoreset_under_dr_on_every_derive_path(torch_mod, eid, variant):
    """Paths 1 (inline in the pair kernel), 2 (a call from the one-lane kernel) and 3 (reset launch + derive launch) against the oracle;
    paths 2 and 3 differ only in where the derivation runs, so they give the same bits"""
    torch = torch_mod
    B = 4096
    forced = np.arange(5, B, 7)
    check = np.arange(B)
    outs = {}
    for path in (1, 2, 3):
        env, mean, std = _walker_env(eid, B, path)
        env.reset()
        outs[path] = _forced_reset_and_next_step(torch, env, mean, std, variant, forced, check, 40 + variant, "%s path %d" % (eid, path))
        env.close()
    for k, (x2, x3) in enumerate(zip(outs[2], outs[3])):
        assert torch.equal(x2.cpu(), x3.cpu()), (eid, "paths 2 and 3 differ in output", k)


def test_walker_autoreset_under_dr_at_the_fused_derive_threshold(torch_mod):
    """524 288 envs, default create (separate reset and derive launches): the forced lanes and a sample of the others against the oracle"""
    torch = torch_mod
    B = 524288
    env, mean, std = _walker_env("RandomWalker2d-v0", B)
    assert env.launch_shape() == dict(lanes=64, pair=False, rolled=False, hum_pair=False)
    env.reset()
    forced = np.arange(100, B, 509)
    rng = np.random.RandomState(7)
    check = np.union1d(forced, rng.choice(B, 2048, replace=False))
    _forced_reset_and_next_step(torch, env, mean, std, 0, forced, check, 50, "walker2d B=%d" % B)
    env.close()


# ------------------------------------------------------------------------------------------- pinned shards vs the single-GPU run
@pytest.mark.parametrize("eid,G", [("RandomWalker2d-v0", 524288), ("RandomWalker2d-v0", 16384), ("RandomHalfCheetah-v0", 16384)])
def test_pinned_shard_reproduces_the_single_gpu_run(torch_mod, eid, G):
    """Shard 1 of shard_strong(G, 1, 2) with pin_global_shape against the G-env run, in lockstep over 20 auto-reset steps under DR with
    forced resets: bit for bit.  Walker2d at 524 288 envs: the global run derives in a separate launch, the 262 144-env shard inside the
    step kernel; at 16 384 envs the global batch runs 32-lane pair blocks while an 8 192-env shard picks 16 lanes by itself."""
    import random_envs_amd as rex
    from random_envs_amd import sharding
    torch = torch_mod
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    off, n = sharding.shard_strong(G, 1, 2)
    kind = {"RandomWalker2d-v0": "walker2d", "RandomHalfCheetah-v0": "halfcheetah"}[eid]
    envs = []
    for o, b in ((0, G), (off, n)):
        env = rex.make(eid, batch=b, seed=9, env_offset=o)
        if o:
            native = env.launch_shape()
            sharding.pin_global_shape(env, G)
            assert env.launch_shape() == envs[0].launch_shape() == sharding.shape_for_batch(kind, G, simds)
            if G == 16384 and simds == 1024:
                assert native["lanes"] == 16 and env.launch_shape()["lanes"] == 32
        mean = np.array(env.spec.nominal_task)
        env.set_dr_distribution("truncnorm", np.stack([mean, 0.1 * mean], 1).ravel().tolist()); env.set_dr_training(True)
        envs.append(env)
    full, shard = envs
    sl = slice(off, off + n)
    assert torch.equal(full.reset()[sl], shard.reset())
    g = torch.Generator().manual_seed(4)
    nact = full.dims.act_dim
    resets = 0
    for t in range(20):
        if t in (0, 10) and kind == "walker2d":   # force resets on every 61st env of the shard
            q, v = full.get_state()
            q = q.clone(); q[off + 3:off + n:61] = torch.as_tensor(FORCED_POSE, dtype=q.dtype, device=q.device)
            full.set_state(q, v); shard.set_state(q[sl], v[sl])
        a = (torch.rand(G, nact, generator=g) * 2 - 1).cuda()
        o1, r1, d1, i1 = full.step(a)
        o2, r2, d2, i2 = shard.step(a[sl])
        assert torch.equal(o1[sl], o2) and torch.equal(r1[sl], r2) and torch.equal(d1[sl], d2), (eid, G, t)
        assert torch.equal(i1["terminal_observation"][sl], i2["terminal_observation"]), (eid, G, t)
        resets += int(d2.sum())
    assert torch.equal(full.get_task()[sl], shard.get_task())
    if kind == "walker2d":
        assert resets >= 2 * len(range(3, n, 61)), resets
    for env in envs:
        assert env.counters()["nonfinite"] == 0
        env.close()
