"""Device-side observation / reward normalisation and episode statistics (rex_norm_*, NormalizedVecRandomEnv) against the fp64
oracle of tests/vecnorm_oracle.py.  At every step the oracle is fed the RAW device outputs of that step, so the physics plays no
part.  Tolerances (test_vecnorm_host.py states and shares them): running mean / var within 1e-9 relative (fp64 sums of
n <= 2^20 terms err by at most n 2^-53 ~ 1.2e-10), normalised fp32 outputs within 1 ulp of the oracle's value rounded to fp32
and exactly +-clip at a clip bound, episode lengths exact, fp64 per-lane sums and aggregates within 1e-12 relative."""
import ctypes

import numpy as np
import pytest

from test_vecnorm_host import assert_f32_within_one_ulp, assert_stats_close
from vecnorm_oracle import VecNormOracle

pytestmark = pytest.mark.gpu

STEPS = 30


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _make(env_id, B, seed=5, dr=False, **kw):
    import random_envs_amd as rex
    env = rex.make(env_id, batch=B, seed=seed, **kw)
    if dr:
        nom = np.array(env.original_task)
        env.set_dr_distribution("uniform", np.stack([0.9 * nom, 1.1 * nom], 1).ravel().tolist())
        env.set_dr_training(True)
    return env


def _action(torch, env, gen):
    if env.dims.discrete_action:
        return torch.randint(0, 2, (env.batch,), generator=gen)
    amp = 0.4 if env.kind == "humanoid" else 1.0
    return (torch.rand(env.batch, env.dims.act_dim, generator=gen) * 2 - 1) * amp


def _np(t):
    return t.detach().cpu().numpy()


def _rel_close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), "%s: %.3g" % (what, np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _parity_run(torch, env_id, B, dr, steps=STEPS):
    import random_envs_amd as rex
    env = _make(env_id, B, dr=dr)
    w = rex.NormalizedVecRandomEnv(env)
    D = env.dims.obs_dim
    o = VecNormOracle(D, B)
    gen = torch.Generator().manual_seed(B)
    worst = dict(mean=0.0, var=0.0, ulp=0)
    nobs = w.reset()
    ref = o.reset(_np(env._obs))
    worst["ulp"] = max(worst["ulp"], assert_f32_within_one_ulp(_np(nobs).T, ref, 10.0, "reset obs"))
    assert_stats_close(w.stats(), o.stats(), "reset")
    finished = 0
    for k in range(steps):
        nobs, nrew, done, info = w.step(_action(torch, env, gen))
        what = "%s B=%d step %d" % (env_id, B, k)
        out = o.step(_np(env._obs), _np(env._reward), _np(env._done), _np(env._term_obs))
        d = out["done"]
        assert np.array_equal(_np(done), d)
        em, ev = assert_stats_close(w.stats(), o.stats(), what)
        worst["mean"], worst["var"] = max(worst["mean"], em), max(worst["var"], ev)
        u = max(assert_f32_within_one_ulp(_np(nobs).T, out["obs"], 10.0, what + " obs"),
                assert_f32_within_one_ulp(_np(nrew), out["reward"], 10.0, what + " reward"),
                assert_f32_within_one_ulp(_np(info["terminal_observation"]).T[:, d], out["term_obs"][:, d], 10.0, what + " terminal obs"))
        worst["ulp"] = max(worst["ulp"], u)
        ls = w.lane_state()
        assert np.array_equal(_np(ls["ep_len"]), o.ep_len), what
        assert np.array_equal(_np(info["episode_length"])[d], out["ep_len"][d]), what
        _rel_close(_np(ls["ep_return"]), o.ep_return, what + " ep_return")
        _rel_close(_np(info["episode_return"])[d], out["ep_return"][d], what + " episode_return")
        _rel_close(_np(ls["ret"]), o.ret, what + " ret")
        finished += int(d.sum())
    s = w.episode_summary(clear=True)
    assert s["episodes"] == o.episodes == finished and s["length_sum"] == o.sum_length and s["nonfinite"] == 0 == o.nonfinite
    _rel_close(s["return_sum"], o.sum_return, "sum of returns")
    assert w.episode_summary()["episodes"] == 0                    # cleared
    print("vecnorm parity %s B=%d: episodes %d, max rel err mean %.3g var %.3g, max ulp %d" % (env_id, B, finished, worst["mean"], worst["var"], worst["ulp"]))
    env.close()
    return finished


@pytest.mark.parametrize("B", [1, 63, 4097, 32768])
@pytest.mark.parametrize("env_id,dr", [("RandomCartPole-v0", False), ("RandomHopper-v0", False), ("RandomWalker2d-v0", True)])
def test_parity_with_the_oracle(torch_mod, env_id, dr, B):
    finished = _parity_run(torch_mod, env_id, B, dr)
    if B >= 4097:
        assert finished > 0, "the run must contain auto-resets"


@pytest.mark.parametrize("B", [63, 4097])
def test_parity_with_the_oracle_humanoid(torch_mod, B):
    """376 rows; constant rows (body masses) included.  Two sizes to bound the test's time."""
    _parity_run(torch_mod, "RandomHumanoid-v0", B, False)


def _run(torch, wrapped, steps, B=4097, env_id="RandomHopper-v0", seed=9):
    import random_envs_amd as rex
    env = _make(env_id, B, seed=seed, dr=True)
    e = rex.NormalizedVecRandomEnv(env) if wrapped else env
    gen = torch.Generator().manual_seed(1)
    e.reset()
    outs = []
    for _ in range(steps):
        ob, r, d, _ = e.step(_action(torch, env, gen))
        outs.append((ob.clone(), r.clone(), d.clone(), env._obs.clone(), env._reward.clone(), env._done.clone()))
    return e, env, outs


def test_raw_outputs_untouched(torch_mod):
    torch = torch_mod
    w, envw, a = _run(torch, True, 25)
    p, envp, b = _run(torch, False, 25)
    assert sum(int(x[5].sum()) for x in a) > 0
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x[3], y[3]) and torch.equal(x[4], y[4]) and torch.equal(x[5], y[5]), "raw buffers differ at step %d" % k
        assert torch.equal(y[0], y[3].t()) and torch.equal(w.get_original_obs(), envw._obs.t())
        assert not torch.equal(x[0], x[3].t())                     # ... and the wrapper's outputs are normalised
    assert torch.equal(w.get_original_reward(), envw._reward)
    envw.close(); envp.close()


def test_two_runs_agree_bit_for_bit(torch_mod):
    torch = torch_mod
    w1, e1, a = _run(torch, True, 20, B=32768)
    w2, e2, b = _run(torch, True, 20, B=32768)
    for x, y in zip(a, b):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    s1, s2 = w1.stats(), w2.stats()
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
    assert w1.episode_summary() == w2.episode_summary()
    e1.close(); e2.close()


def test_resume_is_bit_exact(torch_mod, tmp_path):
    import random_envs_amd as rex
    torch = torch_mod
    B = 4097
    gen = torch.Generator().manual_seed(2)
    env = _make("RandomHopper-v0", B, seed=21, dr=True)
    acts = [_action(torch, env, gen) for _ in range(40)]
    w = rex.NormalizedVecRandomEnv(env)
    w.reset()
    for t in range(20):
        w.step(acts[t])
    snap = env.get_full_state()
    path = w.save(str(tmp_path / "norm"))
    assert path.endswith(".npz")
    ref = []
    for t in range(20, 40):
        ob, r, d, info = w.step(acts[t])
        ref.append((ob.clone(), r.clone(), d.clone(), info["episode_return"].clone(), info["episode_length"].clone()))
    assert sum(int(x[2].sum()) for x in ref) > 0
    env2 = _make("RandomHopper-v0", B, seed=21, dr=True)
    w2 = rex.NormalizedVecRandomEnv(env2)
    w2.reset()
    for t in range(3):                                             # a different history, then the snapshot
        w2.step(acts[39 - t])
    env2.set_full_state(snap)
    w2.load(path)
    for t in range(20, 40):
        ob, r, d, info = w2.step(acts[t])
        x = ref[t - 20]
        assert torch.equal(d, x[2]) and torch.equal(ob, x[0]) and torch.equal(r, x[1]), "step %d after resume" % t
        assert torch.equal(info["episode_return"][d], x[3][d]) and torch.equal(info["episode_length"][d], x[4][d])
    s1, s2 = w.stats(), w2.stats()
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
    env.close(); env2.close()


def test_frozen_statistics(torch_mod):
    torch = torch_mod
    w, env, _ = _run(torch, True, 10, B=4097)
    w.set_training(False)
    assert w.training is False
    before = w.stats()
    o = VecNormOracle(env.dims.obs_dim, env.batch, training=False)
    o.count, o.mean, o.var = before["count"].copy(), before["mean"].copy(), before["var"].copy()
    o.ret = _np(w.lane_state()["ret"]).copy()
    gen = torch.Generator().manual_seed(4)
    for k in range(8):
        nobs, nrew, done, info = w.step(_action(torch, env, gen))
        out = o.step(_np(env._obs), _np(env._reward), _np(env._done), _np(env._term_obs))
        assert_f32_within_one_ulp(_np(nobs).T, out["obs"], 10.0, "frozen obs")
        assert_f32_within_one_ulp(_np(nrew), out["reward"], 10.0, "frozen reward")
        _rel_close(_np(w.lane_state()["ret"]), o.ret, "frozen ret")
    after = w.stats()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    w.training = True
    w.step(_action(torch, env, gen))
    assert w.stats()["count"][0] == before["count"][0] + env.batch
    env.close()


def _raw_call(torch, env, L, obs_in, obs_out, term_in, term_out, rew_out, er, el):
    from random_envs_amd import _native
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _native.check(L.rex_norm_step(env._h, p(obs_in), p(env._reward), p(env._done), p(term_in), p(obs_out), p(rew_out), p(term_out), p(er), p(el),
                                  env._stream()))


@pytest.mark.parametrize("B", [4097, 8192])
def test_in_place_gives_the_same_bits(torch_mod, B):
    """obs_out == obs_in (and the same for reward and terminal observations): the bits of the out-of-place call, for a ragged batch
    (element loads) and an aligned one (16-byte loads)"""
    from random_envs_amd import _native
    torch = torch_mod
    L = _native.lib()
    envs = [_make("RandomWalker2d-v0", B, seed=13, dr=True) for _ in range(2)]
    for e in envs:
        _native.check(L.rex_norm_enable(e._h, None))
        e.reset()
    f = dict(device=envs[0].device)
    D = envs[0].dims.obs_dim
    outs = [torch.zeros(D, B, **f), torch.zeros(D, B, **f), torch.zeros(B, **f)]
    er = torch.zeros(B, dtype=torch.float64, **f); el = torch.zeros(B, dtype=torch.int32, **f)
    gen = torch.Generator().manual_seed(6)
    n_done = 0
    for k in range(25):
        a = _action(torch, envs[0], gen)
        for e in envs:
            e.step(a)
        a_, b_ = envs
        term_before = b_._term_obs.clone()
        _raw_call(torch, a_, L, a_._obs, outs[0], a_._term_obs, outs[1], outs[2], er, el)
        _raw_call(torch, b_, L, b_._obs, b_._obs, b_._term_obs, b_._term_obs, b_._reward, er, el)
        d = a_._done.bool()
        n_done += int(d.sum())
        assert torch.equal(outs[0], b_._obs) and torch.equal(outs[2], b_._reward), "step %d" % k
        assert torch.equal(outs[1][:, d], b_._term_obs[:, d]) and torch.equal(term_before[:, ~d], b_._term_obs[:, ~d])
    assert n_done > 0
    for e in envs:
        e.close()


def test_calls_before_enable_return_state_error(torch_mod):
    from random_envs_amd import _native
    L = _native.lib()
    env = _make("RandomHopper-v0", 64)
    env.reset()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    buf = (ctypes.c_double * (3 * (env.dims.obs_dim + 1)))()
    four = (ctypes.c_double * 4)()
    S = -3                                                         # REX_ERR_STATE
    assert L.rex_norm_set_training(env._h, 1) == S
    assert L.rex_norm_reset(env._h, None, p(env._obs), p(env._obs), None) == S
    assert L.rex_norm_step(env._h, p(env._obs), p(env._reward), p(env._done), None, p(env._obs), None, None, None, None, None) == S
    assert L.rex_norm_get_stats(env._h, buf) == S and L.rex_norm_set_stats(env._h, buf) == S
    assert L.rex_norm_get_lane_state(env._h, None, None, None, None) == S and L.rex_norm_set_lane_state(env._h, None, None, None, None) == S
    assert L.rex_norm_read_episodes(env._h, four, 0) == S and b"rex_norm_enable" in L.rex_last_error()
    assert L.rex_norm_enable(env._h, None) == 0
    assert L.rex_norm_step(env._h, p(env._obs), None, None, None, p(env._obs), None, None, None, None, None) == -1      # REX_ERR_ARG
    assert L.rex_norm_step(env._h, p(env._obs), p(env._reward), p(env._done), None, None, None, None, None, None, None) == -1
    assert L.rex_norm_get_stats(env._h, buf) == 0 and buf[0] == 1e-4 and buf[2 * (env.dims.obs_dim + 1)] == 1.0
    buf[0] = -1.0
    assert L.rex_norm_set_stats(env._h, buf) == -1
    env.close()


def test_nonfinite_input_does_not_poison_the_statistics(torch_mod):
    """NaN / inf injected into an INPUT buffer of the normaliser (never into the simulator)"""
    import random_envs_amd as rex
    torch = torch_mod
    B = 4097
    env = _make("RandomHopper-v0", B)
    w = rex.NormalizedVecRandomEnv(env)
    o = VecNormOracle(env.dims.obs_dim, B)
    w.reset(); o.reset(_np(env._obs))
    gen = torch.Generator().manual_seed(8)
    for k in range(3):
        env.step(_action(torch, env, gen))
        if k == 1:
            env._obs[2, 17] = float("nan"); env._obs[4, 0] = float("inf"); env._obs[4, 4096] = float("nan")
        w._norm_step(True)
        o.step(_np(env._obs), _np(env._reward), _np(env._done), _np(env._term_obs))
        if k == 1:
            w.reset(); o.reset(_np(env._obs))
        assert_stats_close(w.stats(), o.stats(), "step %d" % k)
    s = w.stats()
    assert np.isfinite(s["mean"]).all() and np.isfinite(s["var"]).all()
    assert abs(s["count"][0] - s["count"][2] - 1) < 1e-6 and abs(s["count"][0] - s["count"][4] - 2) < 1e-6
    assert w.episode_summary()["nonfinite"] == 3
    env.close()


def test_masked_reset_counts_the_masked_lanes(torch_mod):
    import random_envs_amd as rex
    torch = torch_mod
    B = 4097
    env = _make("RandomHopper-v0", B, autoreset=False)
    w = rex.NormalizedVecRandomEnv(env)
    o = VecNormOracle(env.dims.obs_dim, B)
    w.reset(); o.reset(_np(env._obs))
    gen = torch.Generator().manual_seed(10)
    for _ in range(5):
        w.step(_action(torch, env, gen))
        o.step(_np(env._obs), _np(env._reward), _np(env._done), _np(env._term_obs))
    mask = torch.rand(B, generator=gen) < 0.25
    before = w._nobs.clone()
    nobs = w.reset(mask)
    ref = o.reset(_np(env._obs), _np(mask))
    m = _np(mask)
    assert_stats_close(w.stats(), o.stats(), "masked reset")
    assert abs(w.stats()["count"][0] - (1e-4 + B * 6 + int(m.sum()))) < 1e-6
    assert_f32_within_one_ulp(_np(nobs).T[:, m], ref[:, m], 10.0, "masked reset obs")
    md = mask.to(env.device)
    assert torch.equal(nobs[~md], before.t()[~md])
    ls = w.lane_state()
    assert (ls["ret"][md] == 0).all() and (ls["ep_len"][md] == 0).all()
    assert np.array_equal(_np(ls["ep_len"]), o.ep_len)
    env.close()


def test_switches_and_step_soa(torch_mod):
    import random_envs_amd as rex
    torch = torch_mod
    B = 1024
    env = _make("RandomHopper-v0", B)
    w = rex.NormalizedVecRandomEnv(env, norm_obs=False, gamma=0.9, clip_reward=0.5)
    o = VecNormOracle(env.dims.obs_dim, B, norm_obs=False, gamma=0.9, clip_reward=0.5)
    ob = w.reset(); o.reset(_np(env._obs))
    assert ob.data_ptr() == env._obs.data_ptr()
    gen = torch.Generator().manual_seed(12)
    for _ in range(6):
        a = _action(torch, env, gen).t().contiguous().to(env.device)
        ob, r, d = w.step_soa(a)
        out = o.step(_np(env._obs), _np(env._reward), _np(env._done))
        assert ob.data_ptr() == env._obs.data_ptr() and r.data_ptr() != env._reward.data_ptr()
        assert_f32_within_one_ulp(_np(r), out["reward"], 0.5, "reward")
    assert (np.abs(_np(r)) == 0.5).any()                           # the clip is reached, exactly
    assert_stats_close(w.stats(), o.stats(), "norm_obs off")
    assert w.batch == B and w.kind == "hopper"                     # everything else is delegated
    env.close()


def test_load_stats_and_merge_across_two_shards(torch_mod):
    """index-sharded: the statistics of two shards, merged in order, equal the statistics of ONE stream over the shards' raw outputs"""
    import random_envs_amd as rex
    torch = torch_mod
    B = 2048
    halves = [rex.NormalizedVecRandomEnv(_make("RandomHopper-v0", B, seed=3, env_offset=k * B)) for k in range(2)]
    D = halves[0].dims.obs_dim
    whole = VecNormOracle(D, 2 * B)
    cat = lambda name: np.concatenate([_np(getattr(h.env, name)) for h in halves], -1)
    for h in halves:
        h.reset()
    whole.reset(cat("_obs"))
    gen = torch.Generator().manual_seed(14)
    for _ in range(10):
        a = _action(torch, halves[0].env, gen)
        for h in halves:
            h.step(a)
        whole.step(cat("_obs"), cat("_reward"), cat("_done"))
    merged = rex.merge_stats([h.stats() for h in halves])
    ref = whole.stats()
    assert np.allclose(merged["count"], ref["count"], rtol=1e-12, atol=0)
    merged["count"] = ref["count"]
    assert_stats_close(merged, ref, "merged shards")
    merged = rex.merge_stats([h.stats() for h in halves])
    halves[0].load_stats(merged)
    got = halves[0].stats()
    assert all(np.array_equal(got[k], merged[k]) for k in got)
    assert halves[0].sync_stats() is not None                      # no process group: the identity
    for h in halves:
        h.env.close()


def test_adapter_emits_episode_infos_over_the_wrapper_only(torch_mod):
    import random_envs_amd as rex
    from random_envs_amd.sb3_adapter import SB3VecEnvAdapter
    torch = torch_mod
    B = 256
    gen = torch.Generator().manual_seed(16)
    env = _make("RandomCartPole-v0", B, seed=2)
    w = rex.NormalizedVecRandomEnv(env)
    ad = SB3VecEnvAdapter(w)
    o = VecNormOracle(env.dims.obs_dim, B)
    ad.reset(); o.reset(_np(env._obs))
    plain = SB3VecEnvAdapter(_make("RandomCartPole-v0", B, seed=2))
    plain.reset()
    seen = 0
    for _ in range(40):
        a = _np(_action(torch, env, gen))
        obs, rew, dones, infos = ad.step(a)
        out = o.step(_np(env._obs), _np(env._reward), _np(env._done), _np(env._term_obs))
        _, _, pd, pinfos = plain.step(a)
        assert np.array_equal(dones, out["done"]) and np.array_equal(pd, dones)
        assert all("episode" not in i for i in pinfos)
        for i in range(B):
            if dones[i]:
                ep = infos[i]["episode"]
                assert ep["l"] == out["ep_len"][i] and abs(ep["r"] - out["ep_return"][i]) <= 1e-12 * abs(out["ep_return"][i])
                assert "terminal_observation" in infos[i] and set(pinfos[i]) == {"terminal_observation", "TimeLimit.truncated"}
                seen += 1
            else:
                assert infos[i] == {}
    assert seen > 0
    ad.close(); plain.close()
