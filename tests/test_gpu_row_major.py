"""The gym surface in the caller's row-major layout (`make(id, row_major=True)`; rex_rows_enable / rex_reset_rows / rex_step_rows) against
the SoA path of a twin env, BIT FOR BIT.

The SoA path is held to the oracle by the rest of the suite; a comparison here never crosses kernel shapes (both twins are pinned to the
same launch shape), so any differing bit means the row-major instantiation of a kernel computed something else than its SoA twin, or
put it somewhere else.  The batches are the smallest at which the new indexing can go wrong: 1, 67 (a ragged last wave and, on the
two-lanes-per-env kernels, a half-used last block) and 64 at 16-lane pair blocks (8 blocks: the XCD block remap is active).  Every twin run
asserts that it has seen truncated and (where the kind can) terminated lanes."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOPPER, CHEETAH, WALKER, HUMANOID, CARTPOLE = ("RandomHopper-v0", "RandomHalfCheetahNoisy-v0", "RandomWalker2d-v0", "RandomHumanoid-v0",
                                               "RandomCartPole-v0")
SENTINEL = -7.25


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _bits(torch, x, y, what):
    """identical dtype, shape and bits (NaN == NaN, -0 != 0)"""
    assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape), (what, x.dtype, y.dtype, tuple(x.shape), tuple(y.shape))
    xb, yb = x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)
    if not torch.equal(xb, yb):
        bad = (xb != yb).reshape(x.shape[0], -1).any(1).nonzero().flatten()[:8].tolist()
        raise AssertionError("%s: bits differ in rows %s" % (what, bad))


def _make(eid, B, row_major, shape=None, knobs=None, **kw):
    """one env of a twin pair: seed 5, the pinned launch shape, DR on -- truncnorm over all 13 parameters for walker2d (as _walker_env of
    test_gpu_launch_shapes.py sets it up), uniform +-10 % of the nominal task elsewhere"""
    import random_envs_amd as rex
    from parity_util import create_knobs
    with create_knobs(**(knobs or {})):
        env = rex.make(eid, batch=B, seed=5, row_major=row_major, **kw)
    if shape:
        got = env.set_launch_shape(**shape)
        assert all(got[k] == v for k, v in shape.items()), (shape, got)
    nom = np.array(env.spec.nominal_task, dtype=np.float64)
    if env.kind == "walker2d":
        env.set_dr_distribution("truncnorm", np.stack([nom, 0.1 * nom], 1).ravel().tolist())
    else:
        env.set_dr_distribution("uniform", np.stack([0.9 * nom, 1.1 * nom], 1).ravel().tolist())
    env.set_dr_training(True)
    return env


def _actions(torch, env, g):
    B = env.batch
    if env.dims.discrete_action:
        return torch.randint(0, 2, (B,), generator=g, dtype=torch.int32).cuda()
    return ((torch.rand(B, env.dims.act_dim, generator=g) * 2 - 1) * float(env.dims.act_high)).cuda()


def _near_time_limit(envs, lanes):
    """t = 498 on `lanes` of every env, through set_full_state: the second step from here truncates them"""
    for env in envs:
        st = env.get_full_state()
        st["t"][lanes] = 498
        env.set_full_state(st)


def _force_termination(envs, lanes):
    """a state on `lanes` that the done rule of the kind rejects after one step (random_hopper.py:92, random_walker2d.py:124-125,
    random_humanoid.py:178-179, random_cartpole.py:198-203); the half-cheetah has no such rule"""
    kind = envs[0].kind
    if kind == "halfcheetah":
        return False
    for env in envs:
        q, v = env.get_state()
        q = q.clone()
        if kind == "hopper":
            q[lanes, 2] = 0.5        # torso pitch past 0.2
        elif kind == "walker2d":
            q[lanes, 2] = 1.5        # torso pitch past 1.0
        elif kind == "humanoid":
            q[lanes, 2] = 2.5        # torso above 2.0 (free fall: no contact)
        else:
            q[lanes, 0] = 3.0        # cart past 2.4
        env.set_state(q, v.clone())
    return True


def _compare_step(torch, tag, soa_out, row_out):
    o1, r1, d1, i1 = soa_out
    o2, r2, d2, i2 = row_out
    _bits(torch, o2, o1, tag + " obs")
    _bits(torch, r2, r1, tag + " reward")
    _bits(torch, d2, d1, tag + " done")
    _bits(torch, i2["TimeLimit.truncated"], i1["TimeLimit.truncated"], tag + " truncated")
    assert sorted(i1) == sorted(i2), (tag, sorted(i1), sorted(i2))
    for k in i1:
        if k not in ("TimeLimit.truncated", "terminal_observation"):
            _bits(torch, i2[k], i1[k], tag + " info " + k)
    dn = d1.nonzero().flatten()
    _bits(torch, i2["terminal_observation"][dn], i1["terminal_observation"][dn], tag + " terminal_observation on the done rows")
    tr = i1["TimeLimit.truncated"]
    return int(tr.sum()), int((d1 & ~tr).sum())


def _compare_end_state(torch, tag, a, r):
    s1, s2 = a.get_full_state(), r.get_full_state()
    assert sorted(s1) == sorted(s2)
    for k in s1:
        _bits(torch, s2[k], s1[k], tag + " full state " + k)
    _bits(torch, r.get_task(), a.get_task(), tag + " task")
    assert a.counters() == r.counters() and a.step_count() == r.step_count(), (tag, a.counters(), r.counters(), a.step_count(), r.step_count())


def _twin_run(torch, eid, B, shape=None, knobs=None, steps=8, **kw):
    """Two envs of one id, seed, DR and launch shape, one per layout, through reset, `steps` auto-reset steps with a time-limit truncation
    (every third lane from 0) and a forced termination (every third lane from 1; lane 0 of a single env) on the way."""
    a = _make(eid, B, False, shape, knobs, **kw)
    r = _make(eid, B, True, shape, knobs, **kw)
    assert a.launch_shape() == r.launch_shape()
    tag = "%s B=%d %s %s" % (eid, B, a.launch_shape(), knobs or "")
    _bits(torch, r.reset(), a.reset(), tag + " reset obs")
    _near_time_limit((a, r), slice(0, None, 3))
    g = torch.Generator().manual_seed(7)
    ntrunc = nterm = 0
    forced = False
    for k in range(steps):
        if k == 3:
            forced = _force_termination((a, r), slice(1, None, 3) if B > 1 else slice(0, 1))
        act = _actions(torch, a, g)
        tr, te = _compare_step(torch, "%s step %d" % (tag, k), a.step(act), r.step(act))
        ntrunc += tr; nterm += te
    assert ntrunc >= len(range(0, B, 3)), (tag, "truncated lanes seen", ntrunc)
    assert nterm >= (len(range(1, B, 3)) if B > 1 else 1) if forced else nterm == 0, (tag, "terminated lanes seen", nterm)
    _compare_end_state(torch, tag, a, r)
    a.close(); r.close()


# ------------------------------------------------------------------------------------------------- 1. twins, bit for bit
@pytest.mark.parametrize("B", [1, 67])
@pytest.mark.parametrize("eid", [CARTPOLE, HOPPER, CHEETAH, WALKER, HUMANOID])
def test_twins_agree_bit_for_bit(torch_mod, eid, B):
    _twin_run(torch_mod, eid, B)


@pytest.mark.parametrize("eid", [HOPPER, CHEETAH, WALKER])
def test_twins_agree_under_the_xcd_block_remap(torch_mod, eid):
    """64 envs in 16-lane two-lanes-per-env blocks: 8 blocks, taken in XCD-transposed order"""
    _twin_run(torch_mod, eid, 64, shape=dict(lanes=16, pair=True))


# ------------------------------------------------------------------------------------------------- 2. every launch shape
PLANAR_SHAPES = [dict(lanes=16, pair=True), dict(lanes=32, pair=True), dict(lanes=64, pair=True), dict(lanes=32, pair=False), dict(lanes=64, pair=False)]


@pytest.mark.parametrize("shape", PLANAR_SHAPES, ids=lambda s: "%s%d" % ("pair" if s["pair"] else "one", s["lanes"]))
@pytest.mark.parametrize("eid", [HOPPER, CHEETAH, WALKER])
def test_every_planar_launch_shape(torch_mod, eid, shape):
    if eid == HOPPER and not shape["pair"]:
        shape = dict(shape, rolled=False)
    _twin_run(torch_mod, eid, 67, shape=shape)


def test_hopper_rolled_launch_shape(torch_mod):
    _twin_run(torch_mod, HOPPER, 67, shape=dict(lanes=64, pair=False, rolled=True))


@pytest.mark.parametrize("hum_pair", [True, False])
def test_humanoid_launch_shapes(torch_mod, hum_pair):
    """hum_pair off: the one-lane step kernel with its separate masked reset launch, both into the staging"""
    _twin_run(torch_mod, HUMANOID, 67, shape=dict(hum_pair=hum_pair))


# ------------------------------------------------------------------------------------------------- 3. unfused auto-reset in rows
def test_walker_unfused_derive_resets_in_rows(torch_mod):
    """REX_FUSED_DERIVE=0 on the one-lane kernel: the step launch, the masked reset launch (which writes the reset lanes' rows) and the derive launch"""
    _twin_run(torch_mod, WALKER, 67, shape=dict(pair=False), knobs=dict(REX_FUSED_DERIVE=0))


def test_cartpole_resets_in_rows_behind_every_step(torch_mod):
    _twin_run(torch_mod, CARTPOLE, 67, steps=12)


@pytest.mark.parametrize("eid", [HOPPER, HUMANOID, CARTPOLE])
def test_without_autoreset_done_rows_keep_the_stepped_observation(torch_mod, eid):
    torch = torch_mod
    B = 67
    a, r = _make(eid, B, False, autoreset=False), _make(eid, B, True, autoreset=False)
    _bits(torch, r.reset(), a.reset(), eid + " reset obs")
    _near_time_limit((a, r), slice(0, None, 3))
    g = torch.Generator().manual_seed(11)
    seen = 0
    for k in range(3):
        if k == 1:
            _force_termination((a, r), slice(1, None, 3))
        act = _actions(torch, a, g)
        out = r.step(act)
        _compare_step(torch, "%s no autoreset step %d" % (eid, k), a.step(act), out)
        dn = out[2].nonzero().flatten()
        seen += dn.numel()
        _bits(torch, out[0][dn], out[3]["terminal_observation"][dn], "done rows hold the stepped observation")
    assert seen >= len(range(0, B, 3))
    _compare_end_state(torch, eid + " no autoreset", a, r)
    a.close(); r.close()


# ------------------------------------------------------------------------------------------------- 4. masked reset
@pytest.mark.parametrize("eid", [CARTPOLE, HOPPER, WALKER, HUMANOID])
def test_masked_reset_writes_the_masked_rows_only(torch_mod, eid):
    torch = torch_mod
    B = 67
    a, r = _make(eid, B, False), _make(eid, B, True)
    buf = r.reset(); a.reset()
    g = torch.Generator().manual_seed(3)
    for _ in range(2):
        act = _actions(torch, a, g)
        a.step(act); r.step(act)
    mask = torch.rand(B, generator=g) < 0.5
    assert 0 < int(mask.sum()) < B
    buf.fill_(SENTINEL)
    want = torch.full((B, a.dims.obs_dim), SENTINEL, device="cuda")
    o1 = a.reset(mask)
    o2 = r.reset(mask)
    assert o2.data_ptr() == buf.data_ptr()
    m = mask.cuda()
    _bits(torch, o2[m], o1[m], eid + " masked rows")
    _bits(torch, o2[~m], want[~m], eid + " unmasked rows keep the sentinel")
    act = _actions(torch, a, g)
    _compare_step(torch, eid + " step after the masked reset", a.step(act), r.step(act))
    _compare_end_state(torch, eid + " masked reset", a, r)
    a.close(); r.close()


# ------------------------------------------------------------------------------------------------- 5. mixed use
@pytest.mark.parametrize("eid", [HOPPER, HUMANOID, CARTPOLE])
def test_soa_and_row_major_steps_interleave_on_one_env(torch_mod, eid):
    torch = torch_mod
    B = 67
    a, m = _make(eid, B, False), _make(eid, B, True)
    _bits(torch, m.reset(), a.reset(), eid + " reset obs")
    _near_time_limit((a, m), slice(0, None, 3))
    g = torch.Generator().manual_seed(13)
    for k in range(6):
        act = _actions(torch, a, g)
        o1, r1, d1, i1 = a.step(act)
        if k % 2 == 0:
            soa = act if a.dims.discrete_action else act.t().contiguous()
            if k % 4 == 0:
                o2, r2, d2 = m.step_soa(soa)
            else:
                o2, r2, d2, t2, term2 = m.step_soa_full(soa)
                _bits(torch, t2.bool(), i1["TimeLimit.truncated"], "%s step %d truncated" % (eid, k))
            _bits(torch, o2.t(), o1, "%s step %d obs (step_soa on the row-major env)" % (eid, k))
            _bits(torch, r2, r1, "%s step %d reward" % (eid, k)); _bits(torch, d2.bool(), d1, "%s step %d done" % (eid, k))
        else:
            _compare_step(torch, "%s step %d" % (eid, k), (o1, r1, d1, i1), m.step(act))
    _compare_end_state(torch, eid + " mixed", a, m)
    q1, v1 = a.get_state(); q2, v2 = m.get_state()
    _bits(torch, q2, q1, "get_state qpos"); _bits(torch, v2, v1, "get_state qvel")
    a.close(); m.close()


# ------------------------------------------------------------------------------------------------- 6. surface contract
@pytest.mark.parametrize("eid", [HOPPER, CARTPOLE, HUMANOID])
def test_returned_tensors_are_the_envs_own_contiguous_buffers(torch_mod, eid):
    torch = torch_mod
    B = 67
    r = _make(eid, B, True)
    o0 = r.reset()
    g = torch.Generator().manual_seed(1)
    ptrs = None
    for _ in range(3):
        obs, rew, done, info = r.step(_actions(torch, r, g))
        ts = dict(obs=obs, reward=rew, done=done, truncated=info["TimeLimit.truncated"], terminal_observation=info["terminal_observation"])
        assert all(t.is_contiguous() and t.is_cuda for t in ts.values())
        assert obs.dtype == torch.float32 and tuple(obs.shape) == (B, r.dims.obs_dim) and tuple(ts["terminal_observation"].shape) == (B, r.dims.obs_dim)
        assert rew.dtype == torch.float32 and tuple(rew.shape) == (B,)
        assert done.dtype == torch.bool and ts["truncated"].dtype == torch.bool and tuple(done.shape) == (B,)
        assert int(done.view(torch.uint8).max()) <= 1
        for name in r.INFO_TERMS[r.kind]:
            assert tuple(info[name].shape) == (B,) and info[name].dtype == torch.float32
        now = {k: t.data_ptr() for k, t in ts.items()}
        assert ptrs is None or now == ptrs
        ptrs = now
    assert o0.data_ptr() == ptrs["obs"]
    r.close()


@pytest.mark.parametrize("eid", [HOPPER, CARTPOLE])
def test_a_contiguous_device_action_is_read_in_place(torch_mod, eid):
    """the caller's tensor is overwritten between two calls: the second call reads the new values (a twin stepped with them agrees), and the
    env's own action buffer is never written"""
    torch = torch_mod
    B = 67
    a, r = _make(eid, B, False), _make(eid, B, True)
    a.reset(); r.reset()
    g = torch.Generator().manual_seed(17)
    act = _actions(torch, a, g)
    own = r._act_rows.clone()
    _compare_step(torch, eid + " first", a.step(act.clone()), r.step(act))
    new = _actions(torch, a, g)
    assert not torch.equal(new, act)
    act.copy_(new)
    _compare_step(torch, eid + " second", a.step(new), r.step(act))
    assert torch.equal(r._act_rows, own)
    a.close(); r.close()


@pytest.mark.parametrize("eid", [HOPPER, CARTPOLE])
def test_other_action_types_give_the_bits_of_the_pass_through_path(torch_mod, eid):
    torch = torch_mod
    B = 67
    p, n = _make(eid, B, True), _make(eid, B, True)
    p.reset(); n.reset()
    g = torch.Generator().manual_seed(19)
    discrete = bool(p.dims.discrete_action)
    forms = [lambda x: x.cpu().numpy(), lambda x: x.to(torch.int64 if discrete else torch.float64),
             lambda x: x.cpu().numpy().tolist(), lambda x: x.cpu()]
    if not discrete:
        forms.append(lambda x: x.t().contiguous().t())     # [B, act_dim] with transposed strides
    for k, form in enumerate(forms):
        act = _actions(torch, p, g)
        other = form(act)
        if isinstance(other, torch.Tensor) and other.is_cuda and not discrete and k == len(forms) - 1:
            assert not other.is_contiguous()
        _compare_step(torch, "%s action form %d" % (eid, k), p.step(act), n.step(other))
    _compare_end_state(torch, eid + " action forms", p, n)
    p.close(); n.close()


def test_sb3_adapter_over_either_layout(torch_mod):
    torch = torch_mod
    from random_envs_amd.sb3_adapter import SB3VecEnvAdapter
    B = 8
    a, r = _make(HOPPER, B, False), _make(HOPPER, B, True)
    a.reset(); r.reset()
    _near_time_limit((a, r), slice(0, None, 3))
    va, vr = SB3VecEnvAdapter(a), SB3VecEnvAdapter(r)
    st = a.get_full_state()
    rng = np.random.RandomState(2)
    ndone = 0
    for k in range(20):
        act = rng.uniform(-1, 1, (B, 3)).astype(np.float32)
        o1, r1, d1, i1 = va.step(act)
        o2, r2, d2, i2 = vr.step(act)
        for x, y in ((o1, o2), (r1, r2), (d1, d2)):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
        for e in range(B):
            assert sorted(i1[e]) == sorted(i2[e])
            if d1[e]:
                ndone += 1
                assert i1[e]["terminal_observation"].tobytes() == i2[e]["terminal_observation"].tobytes()
                assert i1[e]["TimeLimit.truncated"] == i2[e]["TimeLimit.truncated"]
    assert ndone >= 3 and int(st["t"][0]) == 498
    va.close(); vr.close()


def test_the_normaliser_refuses_a_row_major_env(torch_mod):
    from random_envs_amd import NormalizedVecRandomEnv
    r = _make(HOPPER, 4, True)
    with pytest.raises(ValueError, match="row_major"):
        NormalizedVecRandomEnv(r)
    r.close()


# ------------------------------------------------------------------------------------------------- 7. raw ABI errors
def _raw_step_rows(env, bufs, skip=None):
    from random_envs_amd import _native
    L = _native.lib()
    p = [None if k == skip else ctypes.c_void_p(bufs[k].data_ptr()) for k in ("action", "obs", "reward", "done", "trunc", "term")]
    rc = L.rex_step_rows(env._h, *p, env._stream())
    return rc, L.rex_last_error().decode()


@pytest.mark.parametrize("eid", [HOPPER, CARTPOLE])
def test_null_required_buffers_are_refused_and_the_handle_steps_on(torch_mod, eid):
    torch = torch_mod
    B = 5
    a, r = _make(eid, B, False), _make(eid, B, True)
    a.reset(); r.reset()
    g = torch.Generator().manual_seed(23)
    act = _actions(torch, a, g)
    bufs = dict(action=act, obs=r._obs_rows, reward=r._reward, done=r._done_b, trunc=r._trunc_b, term=r._term_rows)
    before = r.step_count()
    for missing in ("action", "obs", "reward", "done"):
        rc, msg = _raw_step_rows(r, bufs, skip=missing)
        assert rc == -1 and "rex_step_rows" in msg and "null" in msg, (missing, rc, msg)
    from random_envs_amd import _native
    rc = _native.lib().rex_reset_rows(r._h, None, None, r._stream())
    assert rc == -1 and "rex_reset_rows" in _native.lib().rex_last_error().decode()
    assert r.step_count() == before                       # nothing was launched or counted
    for skip in ("trunc", "term", None):                  # the optional buffers may be null
        rc, msg = _raw_step_rows(r, bufs, skip=skip)
        assert rc == 0, (skip, msg)
        o1, r1, d1, _ = a.step(act)
        _bits(torch, r._obs_rows, o1, "raw call obs"); _bits(torch, r._reward, r1, "raw call reward"); _bits(torch, r._done_b, d1, "raw call done")
    _compare_end_state(torch, eid + " raw calls", a, r)
    a.close(); r.close()


def test_a_humanoid_handle_needs_rows_enable_first(torch_mod):
    torch = torch_mod
    from random_envs_amd import _native
    B = 5
    a, h = _make(HUMANOID, B, False), _make(HUMANOID, B, False)        # h: a default-mode env, so nothing has enabled the rows on its handle
    a.reset(); h.reset()
    g = torch.Generator().manual_seed(29)
    act = _actions(torch, a, g)
    f32 = dict(dtype=torch.float32, device="cuda")
    bufs = dict(action=act, obs=torch.zeros(B, 376, **f32), reward=torch.zeros(B, **f32), done=torch.zeros(B, dtype=torch.bool, device="cuda"),
                trunc=torch.zeros(B, dtype=torch.bool, device="cuda"), term=torch.zeros(B, 376, **f32))
    rc, msg = _raw_step_rows(h, bufs)
    assert rc == -3 and "rex_rows_enable" in msg, (rc, msg)
    L = _native.lib()
    rc = L.rex_reset_rows(h._h, None, ctypes.c_void_p(bufs["obs"].data_ptr()), h._stream())
    assert rc == -3 and "rex_rows_enable" in L.rex_last_error().decode()
    assert h.step_count() == 0
    o1, r1, d1, _ = a.step(act)
    o2, r2, d2, _ = h.step(act)                           # the handle steps normally afterwards
    _bits(torch, o2, o1, "obs after the refused call"); _bits(torch, r2, r1, "reward"); _bits(torch, d2, d1, "done")
    assert L.rex_rows_enable(h._h) == 0 and L.rex_rows_enable(h._h) == 0      # idempotent
    bufs["action"] = _actions(torch, a, g)
    rc, msg = _raw_step_rows(h, bufs)
    assert rc == 0, msg
    o1, r1, d1, _ = a.step(bufs["action"])
    _bits(torch, bufs["obs"], o1, "rows obs"); _bits(torch, bufs["reward"], r1, "rows reward"); _bits(torch, bufs["done"], d1, "rows done")
    _compare_end_state(torch, "humanoid raw calls", a, h)
    a.close(); h.close()
