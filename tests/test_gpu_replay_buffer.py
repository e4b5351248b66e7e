"""Device-side replay buffer (rex_rbuf_*, ReplayBuffer) against the numpy / Python-int oracle of tests/replay_buffer_oracle.py, under the criteria
test_replay_buffer_host.py states and shares: stored arrays, drawn ids and every copied output to IDENTICAL BITS (also with the host harness),
normalised outputs bit for bit with what rex_norm_step writes for the same values under the same frozen statistics and within 1 fp32 ulp of
the oracle.  The end-to-end run feeds the oracle the RAW device outputs of every step, so the physics plays no part."""
import ctypes

import numpy as np
import pytest

import replay_buffer_oracle as oracle
from host_harness import rbuf as host
from test_replay_buffer_host import FIELDS, SHAPES, replay_step
from test_rollout_host import assert_same_bits
from test_vecnorm_host import assert_f32_within_one_ulp

pytestmark = pytest.mark.gpu

SEED = 0   # actions of the end-to-end run: the shape and seed of test_gpu_rollout.py, whose header records that the reference physics alone drops
           # 87 of 4097 hoppers within 9 steps on this input


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _make(env_id, B, seed=5, dr=False, **kw):
    import random_envs_amd as rex
    env = rex.make(env_id, batch=B, seed=seed, **kw)
    if dr:
        nom = np.array(env.original_task)
        env.set_dr_distribution("uniform", np.stack([0.9 * nom, 1.1 * nom], 1).ravel().tolist())
        env.set_dr_training(True)
    return env


def _dev(torch, env, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(env.device)


def _stored(buf):
    return {k: _np(getattr(buf, k)) for k in FIELDS}


def _assert_outputs(got, ref, what, keys=("obs", "next_obs", "action", "reward", "done")):
    for k in keys:
        g = _np(got[k]) if not isinstance(got[k], np.ndarray) else got[k]
        assert_same_bits(g, np.ascontiguousarray(ref[k]).astype(g.dtype, copy=False), "%s %s" % (what, k))


def _add_step(torch, env, buf, step, with_term=True, with_trunc=True):
    d = {k: _dev(torch, env, v) for k, v in step.items()}
    buf.add(d["obs"], d["action"], d["reward"], d["done"], d["next_obs"], d["terminal_obs"] if with_term else None, d["truncated"] if with_trunc else None)


# ------------------------------------------------------------------------------------------------- synthetic tensors through the C-ABI
CASES = [("RandomHopper-v0", T, B) for T, B in SHAPES] + [("RandomCartPole-v0", T, B) for T, B in SHAPES] + [("RandomHumanoid-v0", 3, 63)]


@pytest.mark.parametrize("env_id,T,B", CASES)
def test_add_gather_sample_equal_the_oracle(torch_mod, env_id, T, B):
    torch = torch_mod
    import random_envs_amd as rex
    env = _make(env_id, B)
    D, A = env.dims.obs_dim, env.dims.act_dim
    discrete = bool(env.dims.discrete_action)
    buf = rex.ReplayBuffer(env, T, seed=11)
    assert buf.action.dtype == (torch.int32 if discrete else torch.float32) and len(buf) == 0
    with pytest.raises(RuntimeError):
        buf.sample(4)
    rng = np.random.default_rng(T * 100 + B)
    ref = oracle.empty_buffers(T, B, D, A, np.int32 if discrete else np.float32)
    for t in range(T):
        step = replay_step(rng, B, D, A, discrete=discrete, p_done=(0.0, 0.1, 1.0)[t % 3])
        if discrete:
            step["action"] = (step["action"] * np.int32(0x7fffff01) - np.int32(5)).astype(np.int32)       # any 32-bit pattern must survive
        plain = t % 2 == 1
        if t == T - 1 and T > 1:
            # ---- the ring holds T - 1 slots: no draw may reach the last one
            out = buf.sample(500)
            assert len(buf) == (T - 1) * B and int(out["index"].max()) < (T - 1) * B
            sub = oracle.sample(ref, T - 1, 500, 11, 0)
            assert np.array_equal(_np(out["index"]), sub["index"])
            _assert_outputs(out, sub, "size < T")
        _add_step(torch, env, buf, step, not plain, not plain)
        oracle.add(ref, t, step["obs"], step["action"], step["reward"], step["done"], step["next_obs"], None if plain else step["terminal_obs"],
                   None if plain else step["truncated"])
    assert buf.full and buf.pos == 0 and len(buf) == T * B
    got = _stored(buf)
    for k in FIELDS:
        assert_same_bits(got[k], ref[k], "%s stored (T=%d B=%d)" % (k, T, B))
    # ---- gather of all ids in a shuffled order, and of a run with ids out of range
    N = T * B
    idx = rng.permutation(N)
    out = buf.gather(_dev(torch, env, idx.astype(np.int64)))
    _assert_outputs(out, oracle.gather(ref, idx)[0], "all ids")
    assert buf.bad_indices() == 0
    idx = np.concatenate([rng.integers(0, N, size=30), [-1, N, 2 ** 62], rng.integers(0, N, size=30)]).astype(np.int64)
    out = buf.gather(_dev(torch, env, idx))
    wanted, bad = oracle.gather(ref, idx)
    _assert_outputs(out, wanted, "ids out of range")
    assert bad == 3 and buf.bad_indices() == 3 and buf.bad_indices() == 0
    for k in ("obs", "next_obs", "action", "reward", "done"):
        assert not _np(out[k])[30:33].any(), k
    # ---- sample: ids and outputs against the oracle and the host harness; a second call with the same (seed, draw) gives the same bits
    for n in (1, 9, 1000):
        draw = buf.draws
        out = buf.sample(n)
        assert buf.draws == draw + 1
        wanted = oracle.sample(ref, T, n, 11, draw)
        assert np.array_equal(_np(out["index"]), wanted["index"])
        _assert_outputs(out, wanted, "sample n=%d" % n)
        rc, hosted, _ = host.sample(ref, n, size=T, seed=11, draw=draw)
        assert rc == 0 and np.array_equal(_np(out["index"]), hosted["index"])
        _assert_outputs(out, hosted, "sample n=%d (host)" % n)
        buf.draws = draw
        again = buf.sample(n)
        _assert_outputs(again, {k: _np(v) for k, v in out.items()}, "second call", keys=tuple(out))
    a, b = buf.sample(64), buf.sample(64)
    assert N == 1 or not torch.equal(a["index"], b["index"])
    env.close()


def test_abi_error_paths(torch_mod):
    torch = torch_mod
    from random_envs_amd import _native
    T, B = 4, 64
    env = _make("RandomHopper-v0", B)
    L, h = env._L, env._h
    f32 = dict(dtype=torch.float32, device=env.device)
    u8 = dict(dtype=torch.uint8, device=env.device)
    t = dict(obs=torch.zeros(T, B, 11, **f32), next_obs=torch.zeros(T, B, 11, **f32), action=torch.zeros(T, B, 3, **f32), reward=torch.zeros(T, B, **f32),
             done=torch.zeros(T, B, **u8), timeout=torch.zeros(T, B, **u8))
    desc = _native.RexRbufBuffers(*[t[k].data_ptr() for k in FIELDS], T)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    s_obs, s_act, s_rew, s_done = torch.zeros(11, B, **f32), torch.zeros(3, B, **f32), torch.zeros(B, **f32), torch.zeros(B, **u8)
    o_obs, o_rew, o_idx = torch.zeros(8, 11, **f32), torch.zeros(8, **f32), torch.zeros(8, dtype=torch.int64, device=env.device)
    out1 = ctypes.c_int64()

    def add(slot, d=desc):
        return L.rex_rbuf_add(h, ctypes.byref(d) if d is not None else None, slot, p(s_obs), p(s_act), p(s_rew), p(s_done), p(s_obs), None, None, env._stream())

    def sample(size, normalise=0, n=8):
        return L.rex_rbuf_sample(h, ctypes.byref(desc), size, n, 1, 0, normalise, p(o_obs), None, None, p(o_rew), None, p(o_idx), env._stream())

    def gather(normalise=0):
        return L.rex_rbuf_gather(h, ctypes.byref(desc), p(o_idx), 8, normalise, p(o_obs), None, None, p(o_rew), None, env._stream())

    calls = [lambda: add(0), lambda: sample(T), gather, lambda: L.rex_rbuf_read_bad_indices(h, ctypes.byref(out1), 0)]
    for c in calls:
        assert c() == -3                              # REX_ERR_STATE before rex_rbuf_enable
    assert "rex_rbuf_enable" in L.rex_last_error().decode()
    assert L.rex_rbuf_enable(h) == 0
    for c in calls:
        assert c() == 0
    assert add(T) == -1 and add(-1) == -1 and add(T - 1) == 0         # REX_ERR_ARG outside [0, T)
    assert add(0, None) == -1                                         # a NULL struct pointer
    assert sample(0) == -1 and sample(T + 1) == -1 and sample(-1) == -1 and sample(1) == 0 and sample(T) == 0
    assert sample(T, n=-1) == -1 and sample(T, n=0) == 0
    assert sample(T, normalise=1) == -3 and gather(normalise=1) == -3                    # normalise without rex_norm_enable
    assert "rex_norm_enable" in L.rex_last_error().decode()
    assert L.rex_norm_enable(h, None) == 0
    assert sample(T, normalise=1) == 0 and gather(normalise=1) == 0
    torch.cuda.synchronize()
    env.close()


# ------------------------------------------------------------------------------------------------- normalised sampling
def _norm_step_rows(torch, w, obs_soa, reward, done):
    """what rex_norm_step writes for one raw SoA step under the wrapper's (frozen) statistics"""
    env = w.env
    B, D = env.batch, env.dims.obs_dim
    nobs, nrew = torch.full((D, B), float("nan"), device=env.device), torch.full((B,), float("nan"), device=env.device)
    er, el = torch.zeros(B, dtype=torch.float64, device=env.device), torch.zeros(B, dtype=torch.int32, device=env.device)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    assert w._L.rex_norm_step(w._h, p(obs_soa), p(reward), p(done), None, p(nobs), p(nrew), None, p(er), p(el), env._stream()) == 0
    return nobs, nrew


@pytest.mark.parametrize("norm_obs", [True, False])
def test_normalised_sampling_equals_rex_norm_step_under_frozen_statistics(torch_mod, norm_obs):
    torch = torch_mod
    import random_envs_amd as rex
    T, B = 3, 257
    env = _make("RandomHopper-v0", B, dr=True)
    D, A = env.dims.obs_dim, env.dims.act_dim
    w = rex.NormalizedVecRandomEnv(env, norm_obs=norm_obs)
    w.reset()
    gen = torch.Generator().manual_seed(2)
    for _ in range(5):                               # the statistics leave their initial values
        w.step_soa((torch.rand(A, B, generator=gen) * 2 - 1).to(env.device))
    w.set_training(False)
    st = w.stats()
    assert st["count"][D] > 1 and abs(st["var"][D] - 1.0) > 1e-3
    buf = rex.ReplayBuffer(w, T)
    rng = np.random.default_rng(3)
    steps = []
    for t in range(T):
        step = replay_step(rng, B, D, A, p_done=0.2)
        step["obs"] = (step["obs"] * 1e-2).astype(np.float32)       # part of the values inside the clip
        steps.append(step)
        _add_step(torch, env, buf, step)
    ref = _stored(buf)
    idx = _dev(torch, env, np.arange(T * B, dtype=np.int64))
    out = buf.gather(idx)                            # normalize=None: yes, the env is a NormalizedVecRandomEnv
    raw = buf.gather(idx, normalize=False)
    _assert_outputs(raw, oracle.gather(ref, np.arange(T * B))[0], "normalize=False")
    zero = torch.zeros(B, dtype=torch.uint8, device=env.device)
    for t in range(T):
        rows = slice(t * B, (t + 1) * B)
        for k in ("obs", "next_obs"):
            soa = buf.views()[k][t].t().contiguous()
            nobs, nrew = _norm_step_rows(torch, w, soa, buf.reward[t].contiguous(), zero)
            if norm_obs:
                assert torch.equal(out[k][rows].view(torch.int32), nobs.t().contiguous().view(torch.int32)), "%s slot %d" % (k, t)
            else:
                assert torch.equal(out[k][rows].view(torch.int32), raw[k][rows].view(torch.int32)), "%s stays raw" % k
            assert torch.equal(out["reward"][rows].view(torch.int32), nrew.view(torch.int32)), "reward slot %d" % t
    assert w.stats()["count"][D] == st["count"][D]   # frozen
    norm = dict(mean=st["mean"], var=st["var"], norm_obs=norm_obs, norm_reward=True, epsilon=w.epsilon, clip_obs=w.clip_obs, clip_reward=w.clip_reward)
    wanted, _ = oracle.gather(ref, np.arange(T * B), norm)
    for k, clip in (("obs", w.clip_obs), ("next_obs", w.clip_obs), ("reward", w.clip_reward)):
        worst = assert_f32_within_one_ulp(_np(out[k]), wanted[k], clip, k)
        print("normalised %s: %d ulp from the oracle" % (k, worst))
    _assert_outputs(out, wanted, "copied outputs", keys=("action", "done"))
    s = buf.sample(300)                              # the sample path normalises the same way
    g = buf.gather(s["index"])
    for k in ("obs", "next_obs", "reward", "action", "done"):
        assert torch.equal(s[k].view(torch.int32), g[k].view(torch.int32)), k
    env.close()


# ------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_hopper_collect_and_wrap(torch_mod):
    torch = torch_mod
    import random_envs_amd as rex
    steps, B, T_small = 9, 4097, 4
    env = _make("RandomHopper-v0", B, dr=True, autoreset=True)
    env.reset()
    st = env.get_full_state()
    st["t"][::3] = 497                                # every third lane meets the time limit inside the window
    env.set_full_state(st)
    big, small = rex.ReplayBuffer(env, steps), rex.ReplayBuffer(env, T_small)
    D, A = env.dims.obs_dim, env.dims.act_dim
    gen = torch.Generator().manual_seed(SEED)
    log = []
    for t in range(steps):
        prev_obs = env._obs.clone()
        a_soa = (torch.rand(B, 3, generator=gen) * 2 - 1).t().contiguous().to(env.device)
        obs, reward, done, trunc, term = env.step_soa_full(a_soa)
        big.add(prev_obs, a_soa, reward, done, obs, term, trunc)
        small.add(prev_obs, a_soa, reward, done, obs, term, trunc)
        log.append({k: _np(x).copy() for k, x in dict(obs=prev_obs, action=a_soa, reward=reward, done=done, next_obs=obs, terminal_obs=term,
                                                       truncated=trunc).items()})
    ref = oracle.empty_buffers(steps, B, D, A)
    for t, s in enumerate(log):
        oracle.add(ref, t, s["obs"], s["action"], s["reward"], s["done"], s["next_obs"], s["terminal_obs"], s["truncated"])
    trunc = np.stack([s["truncated"] for s in log]).astype(bool); done = np.stack([s["done"] for s in log]).astype(bool)
    ended = done & ~trunc
    print("end to end: %d truncations, %d other dones" % (trunc.sum(), ended.sum()))
    assert trunc.any() and ended.any() and np.all(done[trunc])        # not vacuous
    got = _stored(big)
    for k in FIELDS:
        assert_same_bits(got[k], ref[k], k + " stored")
    assert big.full and big.pos == 0
    for t, s in enumerate(log):                      # next_obs: the terminal observation on the finished lanes, the step output elsewhere
        fin = s["done"] != 0
        assert_same_bits(got["next_obs"][t][fin], np.ascontiguousarray(s["terminal_obs"].T[fin]), "terminal rows of step %d" % t)
        assert_same_bits(got["next_obs"][t][~fin], np.ascontiguousarray(s["next_obs"].T[~fin]), "other rows of step %d" % t)
    assert any((s["terminal_obs"].T[s["done"] != 0] != s["next_obs"].T[s["done"] != 0]).any() for s in log)
    out = big.gather(torch.arange(steps * B, device=env.device), normalize=False)
    _assert_outputs(out, oracle.gather(ref, np.arange(steps * B))[0], "all ids")
    d_out = _np(out["done"]).reshape(steps, B)
    assert (d_out[trunc] == 0).all() and (d_out[ended] == 1).all() and (d_out[~done] == 0).all()
    # ---- the ring of T = 4 after 9 adds: pos 1, full, the last four steps
    assert small.full and small.pos == steps % T_small and len(small) == T_small * B
    got = _stored(small)
    for step in range(steps - T_small, steps):
        for k in FIELDS:
            assert_same_bits(got[k][step % T_small], ref[k][step], "%s of step %d in the ring" % (k, step))
    out = small.sample(512)
    assert np.array_equal(_np(out["index"]), oracle.sample_ids(0, 0, T_small, B, 512))
    _assert_outputs(out, oracle.gather(got, _np(out["index"]))[0], "sample of the ring")
    env.close()


def test_state_dict_round_trip_continues_the_sample_stream(torch_mod):
    torch = torch_mod
    import random_envs_amd as rex
    T, B = 5, 64
    env, env2 = _make("RandomHopper-v0", B), _make("RandomHopper-v0", B, seed=9)
    a, b = rex.ReplayBuffer(env, T, seed=77), rex.ReplayBuffer(env2, T, seed=1)
    rng = np.random.default_rng(8)
    for t in range(T + 2):
        _add_step(torch, env, a, replay_step(rng, B, 11, 3))
    a.sample(100); a.sample(100)
    state = a.state_dict()
    b.load_state_dict(state)
    assert (b.pos, b.full, b.seed, b.draws, len(b)) == (2, True, 77, 2, T * B)
    x, y = a.sample(100), b.sample(100)
    assert torch.equal(x["index"], y["index"]) and not torch.equal(x["index"], a.sample(100)["index"])
    for k in ("obs", "next_obs", "action", "reward", "done"):
        assert torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), k
    _add_step(torch, env, a, replay_step(rng, B, 11, 3))              # the state is a copy, not a view
    assert torch.equal(b.obs, state["obs"]) and not torch.equal(a.obs, state["obs"])
    env.close(); env2.close()
