"""Automatic domain randomisation on the device (rex_adr_*, AutoDR) against the numpy / Python-int restatement of its contract
(tests/adr_oracle.py).  Box, tallies, counters, lane state and the tasks stored into the env are held to IDENTICAL BITS: the layer forms
fp64 sums in a stated order, fp32 draws that are not contracted, and copies everything else.  The env runs feed the oracle the RAW device
reward / done of every step, so the physics plays no part."""
import ctypes

import numpy as np
import pytest

import adr_oracle as oracle
from adr_oracle import assert_same_bits, assert_snapshots_equal

pytestmark = pytest.mark.gpu

REX_ERR_ARG, REX_ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _make(env_id, B, seed=5, **kw):
    import random_envs_amd as rex
    return rex.make(env_id, batch=B, seed=seed, **kw)


def _settings(env, act=None, p_b=0.5, m=oracle.M_SCENARIO, t_lo=oracle.T_LO, t_hi=oracle.T_HI, width=None):
    """oracle.settings over the env's nominal task and search bounds; width: the initial box as centre * (1 -+ width) instead of zero width"""
    lo, hi = env.get_task_search_bounds()
    cfg = oracle.settings(np.asarray(env.original_task, np.float32), lo, hi, list(range(env.task_dim)) if act is None else act, p_b)
    cfg.update(m=m, t_lo=t_lo, t_hi=t_hi)
    if width is not None:
        cfg["init_lo"] = (cfg["centre"] * np.float32(1 - width)).astype(np.float32)
        cfg["init_hi"] = (cfg["centre"] * np.float32(1 + width)).astype(np.float32)
    return cfg


def _layer(env, cfg):
    import random_envs_amd as rex
    return rex.AutoDR(env, cfg["t_lo"], cfg["t_hi"], cfg["delta"], p_boundary=cfg["p_b"], buffer_size=cfg["m"], dims=cfg["act"], init_low=cfg["init_lo"],
                      init_high=cfg["init_hi"], centre=cfg["centre"], limit_low=cfg["lim_lo"], limit_high=cfg["lim_hi"], seed=cfg["seed"])


def _ref(env, cfg):
    return oracle.Box(env.batch, task=_np(env.get_task()).T, env_offset=0, **cfg)


class Device:
    """the views tests/adr_oracle.snapshot reads, over an AutoDR and its env"""

    def __init__(self, env, adr):
        self.env, self.adr = env, adr

    def state(self):
        return self.adr.state()

    def lane_state(self):
        ls = {k: _np(v) for k, v in self.adr.lane_state().items()}
        ls["ep"] = ls["ep"].view(np.uint32)
        return ls

    @property
    def task(self):
        return np.ascontiguousarray(_np(self.env.get_task()).T)


# ------------------------------------------------------------------------------------------------- 1. the scenario through record_buffers
def _synthetic_run(torch, env_id, B, ops=None, snaps=None):
    env = _make(env_id, B)
    cfg = _settings(env)
    adr = _layer(env, cfg)
    dev_view = Device(env, adr)
    if ops is None:
        ops, snaps = oracle.scenario(_ref(env, cfg), B, B)
    keep = []

    class Impl:
        def record(self, reward, done, apply):
            r, d = torch.from_numpy(reward).to(env.device), torch.from_numpy(done).to(env.device)
            keep.append((r, d))
            adr.record_buffers(r, d, apply)
        update = staticmethod(adr.update)
        assign = staticmethod(adr.assign)

    def after(j, op):
        if snaps is not None:
            assert_snapshots_equal(oracle.snapshot(dev_view), snaps[j], "%s B=%d behind operation %d (%s)" % (env_id, B, j, op[0]))
    oracle.replay(Impl(), ops, after)
    final = oracle.snapshot(dev_view)
    env.close()
    return ops, snaps, final


@pytest.mark.parametrize("env_id,B", [("RandomHopper-v0", 1), ("RandomHopper-v0", 63), ("RandomHopper-v0", 64), ("RandomHopper-v0", 257),
                                      ("RandomHopper-v0", 4097), ("RandomHopperUnmodeled-v0", 63), ("RandomCartPole-v0", 63), ("RandomHumanoid-v0", 65)])
def test_scenario_equals_the_oracle_and_repeats_bit_for_bit(torch_mod, env_id, B):
    ops, snaps, final = _synthetic_run(torch_mod, env_id, B)
    assert_snapshots_equal(final, snaps[-1], "%s B=%d" % (env_id, B))
    _, _, again = _synthetic_run(torch_mod, env_id, B, ops, None)
    assert_snapshots_equal(again, final, "second run")


# ------------------------------------------------------------------------------------------------- 2 / 3. an auto-resetting hopper run
def _actions(torch, env, gen):
    return torch.rand(env.batch, env.dims.act_dim, generator=gen) * 2 - 1


def _late_in_the_episode(env):
    st = env.get_full_state()
    st["t"][::3] = 497                                # every third lane meets the time limit inside the window
    env.set_full_state(st)


def _hopper_run(torch, with_log):
    import random_envs_amd as rex
    B = 4097
    env = _make("RandomHopper-v0", B, autoreset=True)
    env.reset()
    cfg = _settings(env, m=16, t_lo=0.5, t_hi=1.0, width=0.05)
    adr = _layer(env, cfg)
    adr.assign()
    ref = _ref(env, cfg)
    ref.assign(None)
    log = rex.EpisodeLog(env, 4 * B) if with_log else None
    _late_in_the_episode(env)                          # (set_full_state re-stores the task the layer just assigned)
    if log:
        log.sync()
    gen = torch.Generator().manual_seed(0)
    expected, n_trunc, n_done = [], 0, 0               # ledger rows as the oracle implies them: (task the episode ran under, bnd, tallied return or None)
    for c in range(9):
        _, reward, done, info = env.step(_actions(torch, env, gen))
        adr.record()
        if log:
            log.record(truncated=True)
        r, d = _np(env._reward), _np(env._done)
        n_trunc += int(_np(info["TimeLimit.truncated"]).sum()); n_done += int((d != 0).sum())
        task_before, bnd_before, first = ref.task.copy(), ref.bnd.copy(), len(ref.tallied)
        ref.record(r, d, True)
        tallied = {lane: ret for _, lane, _, ret in ref.tallied[first:]}
        for i in np.flatnonzero(d):
            expected.append((task_before[:, i], int(bnd_before[i]), tallied.get(int(i)), int(i), c))
    return env, adr, ref, log, expected, n_trunc, n_done


def test_end_to_end_hopper_autoreset(torch_mod):
    env, adr, ref, _, _, n_trunc, n_done = _hopper_run(torch_mod, False)
    ev = ref.events
    print("end to end: %d truncations, %d other finished episodes, events %s" % (n_trunc, n_done - n_trunc, ev))
    assert n_trunc >= 64 and n_done - n_trunc >= 32, "the run must contain time-limit AND other finished episodes (%d, %d)" % (n_trunc, n_done - n_trunc)
    assert ev["boundary_episodes"] >= 64 and ev["expand"] + ev["shrink"] + ev["hold"] >= 1
    assert_snapshots_equal(oracle.snapshot(Device(env, adr)), oracle.snapshot(ref), "hopper end to end")
    lo, hi, entropy = adr.box()
    w = (hi.astype(np.float64) - lo.astype(np.float64))
    assert entropy == float(np.mean(np.log(w[w > 0])))
    env.close()


def test_ledger_behind_the_layer_carries_the_task_each_episode_ran_under(torch_mod):
    env, adr, ref, log, expected, _, _ = _hopper_run(torch_mod, True)
    d = log.drain()
    assert d["dropped"] == 0 and len(d["env"]) == len(expected) >= 96
    task, ret, lane, step = _np(d["task"]), _np(d["episode_return"]), _np(d["env"]), _np(d["step"])
    assert_same_bits(lane, np.array([e[3] for e in expected], np.int64), "ledger env"); assert_same_bits(step, np.array([e[4] for e in expected], np.int64), "ledger step")
    assert_same_bits(task, np.array([e[0] for e in expected], np.float32), "ledger task against the task the oracle assigned to that episode")
    pinned = [j for j, e in enumerate(expected) if e[1] >= 0]
    assert len(pinned) >= 32 and all(expected[j][2] is not None for j in pinned)
    assert_same_bits(ret[pinned], np.array([expected[j][2] for j in pinned], np.float64), "ledger return of the pinned episodes against the tallied value")
    assert_snapshots_equal(oracle.snapshot(Device(env, adr)), oracle.snapshot(ref), "with a ledger behind it")
    env.close()


# ------------------------------------------------------------------------------------------------- 4. walker2d: the masked derive
def test_walker2d_geometry_follows_the_reassigned_lengths(torch_mod):
    torch = torch_mod
    B = 65
    env = _make("RandomWalker2d-v0", B, autoreset=True)
    env.reset()
    cfg = _settings(env, act=list(range(11)), width=0.1)          # masses and lengths
    adr = _layer(env, cfg)
    adr.assign()
    st = env.get_full_state()
    st["t"][::2] = 499                                 # every second lane finishes in the next step
    env.set_full_state(st)
    gen = torch.Generator().manual_seed(0)
    before = _np(env.get_task()).copy()
    _, _, done, _ = env.step(_actions(torch, env, gen))
    adr.record()
    after, d = _np(env.get_task()), _np(done)
    assert d[::2].all() and not d.all()
    assert (before[d, 7:11] != after[d, 7:11]).any(axis=1).all() and (before[~d] == after[~d]).all()    # new lengths on exactly the finished lanes
    twin = _make("RandomWalker2d-v0", B, autoreset=True)
    twin.reset()
    twin.set_task(env.get_task())                      # derives every lane's geometry from its lengths
    twin.set_full_state(env.get_full_state())
    a = _actions(torch, env, gen)
    out, ref = env.step(a), twin.step(a)
    for k, name in enumerate(("obs", "reward", "done")):
        assert_same_bits(_np(out[k]), _np(ref[k]), "one further step: %s" % name)
    q, v = env.get_state(); q2, v2 = twin.get_state()
    assert_same_bits(_np(q), _np(q2), "qpos"); assert_same_bits(_np(v), _np(v2), "qvel")
    env.close(); twin.close()


# ------------------------------------------------------------------------------------------------- 5. resume
def test_resume_from_state_and_lane_state_is_exact(torch_mod):
    torch = torch_mod
    B = 257

    def prepared():
        env = _make("RandomHopper-v0", B, autoreset=True)
        env.reset()
        cfg = _settings(env, m=4, t_lo=0.5, t_hi=1.0, width=0.05)
        return env, _layer(env, cfg)

    def late(env):
        st = env.get_full_state()
        st["t"][::3] = 497                             # finishes inside the first five steps
        st["t"][1::3] = 493                            # finishes inside the last four
        env.set_full_state(st)
    gen = torch.Generator().manual_seed(0)
    acts = [torch.rand(B, 3, generator=gen) * 2 - 1 for _ in range(9)]
    env, adr = prepared()
    adr.assign(); late(env)
    for a in acts:
        env.step(a); adr.record()
    whole, obs_whole = oracle.snapshot(Device(env, adr)), _np(env._obs).copy()
    env.close()
    env, adr = prepared()
    adr.assign(); late(env)
    for a in acts[:5]:
        env.step(a); adr.record()
    saved, lanes, full = adr.state(), adr.lane_state(), env.get_full_state()
    assert saved["counters"].sum() >= 1 and (_np(lanes["ep"]) >= 2).any()
    env.close()
    env, adr = prepared()                              # a fresh env + layer
    env.set_full_state(full)
    adr.load_state(saved); adr.load_lane_state(lanes)
    for a in acts[5:]:
        env.step(a); adr.record()
    assert_snapshots_equal(oracle.snapshot(Device(env, adr)), whole, "resumed run against the uninterrupted one")
    assert_same_bits(_np(env._obs), obs_whole, "observations")
    env.close()


# ------------------------------------------------------------------------------------------------- 6. argument and state errors
def test_errors_are_returned_with_nothing_launched(torch_mod):
    torch = torch_mod
    import random_envs_amd as rex
    from random_envs_amd import _native
    B = 63
    env = _make("RandomHopper-v0", B)
    L, h, dev = env._L, env._h, env.device
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    reward, done = torch.zeros(B, device=dev), torch.ones(B, dtype=torch.uint8, device=dev)
    ret, ln, bnd, ep = (torch.zeros(B, dtype=dt, device=dev) for dt in (torch.float64, torch.int32, torch.int32, torch.int32))
    h_lo, h_hi, h_n, h_s, h_c = np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(8, np.int64), np.zeros(8, np.float64), np.zeros(24, np.int64)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    every = lambda: [L.rex_adr_record(h, p(reward), p(done), 1, env._stream()), L.rex_adr_assign(h, None, env._stream()), L.rex_adr_update(h, env._stream()),
                     L.rex_adr_get_state(h, hp(h_lo), hp(h_hi), hp(h_n), hp(h_s), hp(h_c)), L.rex_adr_set_state(h, hp(h_lo), hp(h_hi), hp(h_n), hp(h_s), hp(h_c)),
                     L.rex_adr_get_lane_state(h, p(ret), p(ln), p(bnd), p(ep), env._stream()), L.rex_adr_set_lane_state(h, p(ret), p(ln), p(bnd), p(ep), env._stream())]
    task0 = _np(env.get_task()).copy()
    assert every() == [REX_ERR_STATE] * 7 and b"rex_adr_enable" in L.rex_last_error()
    cfg = _settings(env, width=0.05)

    def enable(handle=h, **kw):
        c = dict(cfg, **kw)
        arrs = {k: np.ascontiguousarray(c[k], np.float32) for k in ("delta", "lim_lo", "lim_hi", "centre", "init_lo", "init_hi")}
        act = np.ascontiguousarray(c["act"], np.int32)
        ptr = lambda k: None if c.get("null") == k else hp(arrs[k])
        desc = _native.RexAdrConfig(c.get("n_act", len(act)), None if c.get("null") == "act" else hp(act), c["p_b"], c["m"], c["t_lo"], c["t_hi"], ptr("delta"),
                                    ptr("lim_lo"), ptr("lim_hi"), ptr("centre"), ptr("init_lo"), ptr("init_hi"), c["seed"])
        return L.rex_adr_enable(handle, ctypes.byref(desc)), L.rex_last_error().decode()
    scaled = lambda name, s: {name: (cfg["centre"] * np.float32(s)).astype(np.float32)}
    bad_delta = cfg["delta"].copy(); bad_delta[3] = 0
    refused = [(dict(null=k), "pointer") for k in ("act", "delta", "lim_lo", "lim_hi", "centre", "init_lo", "init_hi")] + [
        (dict(n_act=0), "n_act"), (dict(n_act=5), "n_act"), (dict(act=[1, 0, 2, 3]), "act"), (dict(act=[0, 1, 2, 4]), "act"), (dict(act=[0, 1, 1, 2]), "act"),
        (dict(m=0), "m must"), (dict(p_b=-0.25), "p_b"), (dict(p_b=1.5), "p_b"), (dict(p_b=float("nan")), "p_b"), (dict(t_lo=2.0, t_hi=1.0), "t_lo"),
        (dict(delta=bad_delta), "delta"), (dict(delta=-cfg["delta"]), "delta"), (scaled("lim_lo", 1.5), "lim_lo <= lo"), (scaled("lim_hi", 0.5), "lim_lo <= lo"),
        (scaled("init_lo", 1.25), "lim_lo <= lo"), (scaled("init_hi", 0.75), "lim_lo <= lo"), (scaled("init_hi", 50.0), "lim_lo <= lo")]
    for kw, word in refused:
        rc, msg = enable(**kw)
        assert rc == REX_ERR_ARG and word in msg, (kw, rc, msg)
    assert L.rex_adr_enable(h, None) == REX_ERR_ARG and enable(handle=None)[0] == REX_ERR_ARG
    assert every() == [REX_ERR_STATE] * 7              # a refused enable enabled nothing
    assert_same_bits(_np(env.get_task()), task0, "tasks behind the refused calls")
    env.reset()
    obs, _, _, _ = env.step(torch.zeros(B, 3))
    assert torch.isfinite(obs).all()                   # the handle still steps
    adr = _layer(env, cfg)                             # rex_adr_enable through the Python object
    rc, msg = enable()
    assert rc == REX_ERR_STATE and "already enabled" in msg
    view = Device(env, adr)
    view.adr.assign()
    held = oracle.snapshot(view)
    assert (held["ep"] == 1).all() and not (held["task"] == task0.T).all()
    assert L.rex_adr_record(h, None, p(done), 1, env._stream()) == REX_ERR_ARG and L.rex_adr_record(h, p(reward), None, 1, env._stream()) == REX_ERR_ARG
    env.set_dr_training(True)
    assert L.rex_adr_record(h, p(reward), p(done), 1, env._stream()) == REX_ERR_STATE and b"dr_training" in L.rex_last_error()
    env.set_dr_training(False)
    assert L.rex_adr_get_state(h, None, hp(h_hi), hp(h_n), hp(h_s), hp(h_c)) == REX_ERR_ARG
    assert L.rex_adr_get_lane_state(h, p(ret), None, p(bnd), p(ep), env._stream()) == REX_ERR_ARG
    assert L.rex_adr_set_lane_state(h, p(ret), p(ln), p(bnd), None, env._stream()) == REX_ERR_ARG
    assert L.rex_adr_get_state(h, hp(h_lo), hp(h_hi), hp(h_n), hp(h_s), hp(h_c)) == 0
    outside = h_lo.copy(); outside[0] = np.float32(0.25)                               # below the limit
    assert L.rex_adr_set_state(h, hp(outside), hp(h_hi), hp(h_n), hp(h_s), hp(h_c)) == REX_ERR_ARG
    negative = h_n.copy(); negative[3] = -1
    assert L.rex_adr_set_state(h, hp(h_lo), hp(h_hi), hp(negative), hp(h_s), hp(h_c)) == REX_ERR_ARG
    assert_snapshots_equal(oracle.snapshot(view), held, "state, lanes and tasks behind the refused calls")
    assert L.rex_adr_record(h, p(reward), p(done), 1, env._stream()) == 0
    assert (oracle.snapshot(view)["ep"] == 2).all()
    env.close()
    # the Python object
    env = _make("RandomHopper-v0", B)
    with pytest.raises(ValueError, match="outside the limits"):
        rex.AutoDR(env, 0.0, 1.0, 0.1, limit_low=np.full(4, 4.0))
    with pytest.raises(ValueError, match="one value per task index"):
        rex.AutoDR(env, 0.0, 1.0, [0.1, 0.2])
    with pytest.raises(ValueError, match="n_act"):
        rex.AutoDR(env, 0.0, 1.0, 0.1, dims=[])
    adr = rex.AutoDR(env, 0.0, 1.0, 0.1)
    assert adr.buffer_size == 240 and adr.box()[2] == float("-inf")                    # the zero-width start
    with pytest.raises(ValueError):
        adr.record_buffers(reward[:-1], done[:-1])
    with pytest.raises(ValueError):
        adr.assign(torch.ones(B + 1))
    env.close()
