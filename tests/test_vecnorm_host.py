"""Device-side normalisation, CPU half: the oracle restatement holds to numpy, ``merge_stats`` to the unsharded stream, and the
kernels' own arithmetic (the __host__ __device__ functions of csrc/vecnorm.hpp, driven in grid / chunk / reduction order by
tests/host_harness/vecnorm_host.cpp) to the oracle under the tolerances of tests/test_gpu_vecnorm.py."""
import ctypes
import os

import numpy as np
import pytest

from host_harness.build import build_so
from vecnorm_oracle import VecNormOracle, f32_ulp_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "random-envs_amd", "csrc", "vecnorm.hpp")


# ------------------------------------------------------------------------------------------------- tolerances (shared with the GPU tests)
def assert_stats_close(got, ref, what=""):
    """|dmean| <= 1e-9 (|mean| + sqrt(var)), |dvar| <= 1e-9 var, counts equal: both sides sum in fp64 with shifted or merged
    moments, whose worst-case error for n <= 2^20 terms is n 2^-53 ~ 1.2e-10 relative."""
    dm = np.abs(got["mean"] - ref["mean"]); dv = np.abs(got["var"] - ref["var"])
    em = dm / (np.abs(ref["mean"]) + np.sqrt(ref["var"])); ev = dv / ref["var"]
    assert np.array_equal(got["count"], ref["count"]), what
    assert em.max() <= 1e-9 and ev.max() <= 1e-9, "%s: mean err %.3g, var err %.3g (rows %d / %d)" % (what, em.max(), ev.max(), em.argmax(), ev.argmax())
    return float(em.max()), float(ev.max())


def assert_f32_within_one_ulp(got, ref64, clip, what=""):
    """normalised fp32 outputs against the oracle's fp64 value rounded to fp32; at a clip bound exactly +-clip"""
    ref = np.asarray(ref64, dtype=np.float64).astype(np.float32)
    got = np.asarray(got, dtype=np.float32)
    if got.size == 0:
        return 0
    d = f32_ulp_distance(got, ref)
    assert d.max() <= 1, "%s: %d ulps" % (what, d.max())
    at = np.abs(np.asarray(ref64)) >= clip
    assert np.array_equal(got[at], ref[at]), what
    return int(d.max())


# ------------------------------------------------------------------------------------------------- oracle self-checks
def _batches(rng, k, D, B):
    scale = 10.0 ** rng.uniform(-3, 3, size=(D, 1)); off = rng.normal(size=(D, 1)) * 100
    return [rng.normal(size=(D, B)) * scale + off for _ in range(k)]


def _with_prior(x):
    """np.mean / np.var of the rows of x with RunningMeanStd's prior (1e-4 pseudo-samples of mean 0, var 1) folded in"""
    n = x.shape[1]; c = 1e-4; tot = c + n
    bm, bv = x.mean(1), x.var(1)
    mean = bm * n / tot
    m2 = c * 1.0 + bv * n + bm * bm * c * n / tot
    return tot, mean, m2 / tot


def test_oracle_batches_equal_the_concatenation():
    rng = np.random.default_rng(0)
    D, B = 5, 257
    bs = _batches(rng, 7, D, B)
    o = VecNormOracle(D, B, norm_reward=False)
    for b in bs:
        o.step(b, np.zeros(B), np.zeros(B, bool))
    tot, mean, var = _with_prior(np.concatenate(bs, 1))
    assert np.allclose(o.count[:D], tot, rtol=1e-15)
    assert np.allclose(o.mean[:D], mean, rtol=1e-11, atol=0) and np.allclose(o.var[:D], var, rtol=1e-11)


def test_merge_stats_of_shards_equals_the_unsharded_stream():
    from random_envs_amd.normalize import merge_stats
    rng = np.random.default_rng(1)
    D, B, shards = 4, 96, 3
    bs = _batches(rng, 6, D, B * shards)
    rew = [rng.normal(size=B * shards) for _ in bs]
    whole = VecNormOracle(D, B * shards)
    parts = [VecNormOracle(D, B) for _ in range(shards)]
    dn = np.zeros(B * shards, bool)
    for b, r in zip(bs, rew):
        whole.step(b, r, dn)
        for k, p in enumerate(parts):
            p.step(b[:, k * B:(k + 1) * B], r[k * B:(k + 1) * B], dn[:B])
    m = merge_stats([p.stats() for p in parts])
    assert_stats_close(m, whole.stats(), "merged shards")
    # a second period, merged against what the ranks shared at the first synchronisation
    base = m
    for p in parts:
        p.count, p.mean, p.var = base["count"].copy(), base["mean"].copy(), base["var"].copy()
    bs2 = _batches(rng, 4, D, B * shards)
    for b in bs2:
        r = rng.normal(size=B * shards)
        whole.step(b, r, dn)
        for k, p in enumerate(parts):
            p.step(b[:, k * B:(k + 1) * B], r[k * B:(k + 1) * B], dn[:B])
    m2 = merge_stats([p.stats() for p in parts], base=base)
    got = dict(m2); ref = whole.stats()
    assert np.allclose(got["count"], ref["count"], rtol=1e-12)
    got["count"] = ref["count"]
    assert_stats_close(got, ref, "second period")
    with pytest.raises(ValueError):
        merge_stats([])


def test_oracle_frozen_stats_stay_frozen():
    rng = np.random.default_rng(2)
    D, B = 3, 64
    o = VecNormOracle(D, B)
    o.step(rng.normal(size=(D, B)), rng.normal(size=B), np.zeros(B, bool))
    before = o.stats(); ret = o.ret.copy()
    o.training = False
    x = rng.normal(size=(D, B)) * 5 + 3
    out = o.step(x, rng.normal(size=B), np.zeros(B, bool))
    after = o.stats()
    assert all(np.array_equal(before[k], after[k]) for k in before) and np.array_equal(ret, o.ret)
    assert np.array_equal(out["obs"], np.clip((x - before["mean"][:D, None]) / np.sqrt(before["var"][:D, None] + 1e-8), -10, 10))


def test_oracle_masked_reset_counts_only_the_masked_lanes():
    rng = np.random.default_rng(3)
    D, B = 3, 100
    o = VecNormOracle(D, B)
    mask = rng.random(B) < 0.3
    x = rng.normal(size=(D, B))
    o.ret[:] = 5.0
    o.reset(x, mask)
    assert np.allclose(o.count[:D], 1e-4 + mask.sum()) and o.count[D] == 1e-4
    tot, mean, var = _with_prior(x[:, mask])
    assert np.allclose(o.mean[:D], mean, rtol=1e-12) and np.allclose(o.var[:D], var, rtol=1e-12)
    assert np.all(o.ret[mask] == 0) and np.all(o.ret[~mask] == 5.0)
    o2 = VecNormOracle(D, B); o2.reset(x)
    assert np.allclose(o2.count[:D], 1e-4 + B)


def test_oracle_nan_element_leaves_the_statistic_as_without_it():
    rng = np.random.default_rng(4)
    D, B = 3, 50
    x = rng.normal(size=(D, B)); r = rng.normal(size=B)
    bad = x.copy(); bad[1, 7] = np.nan; bad[2, 9] = np.inf
    a = VecNormOracle(D, B); a.step(bad, r, np.zeros(B, bool))
    assert np.isfinite(a.mean).all() and np.isfinite(a.var).all() and a.nonfinite == 2
    b = VecNormOracle(D, B)
    for row in range(D):
        keep = np.isfinite(bad[row])
        b._update_row(row, x[row, keep])
    assert np.array_equal(a.mean[:D], b.mean[:D]) and np.array_equal(a.var[:D], b.var[:D]) and np.array_equal(a.count[:D], b.count[:D])
    assert a.count[0] == 1e-4 + B and a.count[1] == 1e-4 + B - 1


# ------------------------------------------------------------------------------------------------- the kernels' math on the CPU
_lib = None


def harness():
    """tests/host_harness/vecnorm_host.cpp built with g++ (rebuilt when it or a header is newer)"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("vecnorm_host", "vecnorm_host.cpp", ["-ffp-contract=off"]))
        _lib.vn_host_chunks.argtypes = [ctypes.c_longlong, ctypes.c_int]
        _lib.vn_host_walk.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]
        _lib.vn_host_walk.restype = ctypes.c_longlong
        vp = ctypes.c_void_p
        _lib.vn_host_call.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int] + [vp] * 6 + [ctypes.c_int] * 4 + [vp] * 10
    return _lib


class HostNorm:
    """The harness behind the oracle's interface."""

    def __init__(self, D, B, gamma=0.99, epsilon=1e-8, clip_obs=10.0, clip_reward=10.0, norm_obs=True, norm_reward=True, training=True):
        self.D, self.B = D, B
        self.cfg = np.array([gamma, epsilon, clip_obs, clip_reward], dtype=np.float64)
        self.norm_obs, self.norm_reward, self.training = norm_obs, norm_reward, training
        R = D + 1
        self.st = np.concatenate([np.full(R, 1e-4), np.zeros(R), np.ones(R)])
        self.ret = np.zeros(B); self.ep_return = np.zeros(B); self.ep_len = np.zeros(B, dtype=np.int32)
        self.agg = np.zeros(4)
        self.ep_return_out = np.zeros(B); self.ep_len_out = np.zeros(B, dtype=np.int32)

    def stats(self):
        R = self.D + 1
        return dict(count=self.st[:R].copy(), mean=self.st[R:2 * R].copy(), var=self.st[2 * R:].copy())

    def _call(self, mode, obs, reward, done, term, mask, obs_out=None):
        p = lambda a: None if a is None else a.ctypes.data
        obs_out = np.zeros_like(obs) if obs_out is None else obs_out
        rew_out = np.zeros(self.B, dtype=np.float32); term_out = None if term is None else np.zeros_like(term)
        rc = harness().vn_host_call(mode, self.B, self.D, p(obs), p(reward), p(done), p(term), p(mask), p(self.cfg), int(self.norm_obs),
                                    int(self.norm_reward), int(self.training), int(self.B % 4 == 0), p(self.st), p(self.ret), p(self.ep_return),
                                    p(self.ep_len), p(obs_out), p(rew_out), p(term_out), p(self.ep_return_out), p(self.ep_len_out), p(self.agg))
        assert rc == 0
        return obs_out, rew_out, term_out

    def step(self, obs, reward, done, term=None, obs_out=None):
        return self._call(0, obs, reward, done, term, None, obs_out)

    def reset(self, obs, mask=None):
        return self._call(1, obs, None, None, None, mask)[0]


def _rollout_data(rng, D, B, steps):
    """observations with rows of very different scale, one constant row and one nearly constant row; rewards; sparse dones"""
    scale = 10.0 ** rng.uniform(-2, 3, size=(D, 1)); off = rng.normal(size=(D, 1)) * 30
    for _ in range(steps):
        obs = (rng.normal(size=(D, B)) * scale + off).astype(np.float32)
        obs[0] = np.float32(8.9)                                   # constant over the batch (a body mass)
        obs[1] = np.float32(1.25) + (rng.random(B) < 0.01) * np.float32(1e-3)
        obs[2] *= (rng.random(B) < 0.05) * 40                      # mostly zero, rare large (a contact force)
        term = (rng.normal(size=(D, B)) * scale + off).astype(np.float32)
        rew = (rng.normal(size=B) + 1).astype(np.float32)
        done = (rng.random(B) < 0.08).astype(np.uint8)
        yield obs, rew, done, term


def _check_step(h, o, obs, rew, done, term, what):
    out = o.step(obs, rew, done, term)
    no, nr, nt = h.step(obs, rew, done, term)
    assert_stats_close(h.stats(), o.stats(), what)
    assert_f32_within_one_ulp(no, out["obs"], o.clip_obs, what + " obs")
    assert_f32_within_one_ulp(nr, out["reward"], o.clip_reward, what + " reward")
    d = done.astype(bool)
    assert_f32_within_one_ulp(nt[:, d], out["term_obs"][:, d], o.clip_obs, what + " terminal obs")
    assert np.all(nt[:, ~d] == 0)                                  # lanes that did not finish are left as they were
    assert np.array_equal(h.ep_len, o.ep_len) and np.array_equal(h.ep_len_out[d], out["ep_len"][d])
    assert np.allclose(h.ep_return, o.ep_return, rtol=1e-12, atol=0) and np.allclose(h.ep_return_out[d], out["ep_return"][d], rtol=1e-12, atol=0)
    assert np.allclose(h.ret, o.ret, rtol=1e-12, atol=0)
    assert h.agg[0] == o.episodes and h.agg[2] == o.sum_length and np.isclose(h.agg[1], o.sum_return, rtol=1e-12, atol=0)


@pytest.mark.parametrize("B", [1, 63, 64, 4097])
def test_kernel_math_matches_the_oracle(B):
    D = 6
    rng = np.random.default_rng(B)
    h, o = HostNorm(D, B), VecNormOracle(D, B)
    first = next(_rollout_data(rng, D, B, 1))[0]
    assert_f32_within_one_ulp(h.reset(first), o.reset(first), 10.0, "reset")
    assert_stats_close(h.stats(), o.stats(), "reset")
    for k, (obs, rew, done, term) in enumerate(_rollout_data(rng, D, B, 12)):
        _check_step(h, o, obs, rew, done, term, "B=%d step %d" % (B, k))
    # frozen: bitwise constant statistics, outputs follow them
    h.training = o.training = False
    before = h.st.copy()
    for k, (obs, rew, done, term) in enumerate(_rollout_data(rng, D, B, 3)):
        _check_step(h, o, obs, rew, done, term, "B=%d frozen step %d" % (B, k))
    assert np.array_equal(before, h.st)


def test_kernel_math_many_chunks_and_grid_stride():
    """past the chunk cap every block strides over several tiles; the merged partials still hold the tolerance"""
    D, B = 3, 70_001
    assert harness().vn_host_chunks(B, D + 1) == 64 and harness().vn_host_chunks(2 ** 20, 377) == 10 and harness().vn_host_chunks(1, 12) == 1
    rng = np.random.default_rng(5)
    h, o = HostNorm(D, B), VecNormOracle(D, B)
    for k, (obs, rew, done, term) in enumerate(_rollout_data(rng, D, B, 3)):
        _check_step(h, o, obs, rew, done, term, "step %d" % k)


@pytest.mark.parametrize("rows", [1, 12, 377])
@pytest.mark.parametrize("N", [1, 3, 4, 1023, 1024, 1025, 5 * 1024 + 2])
def test_chunk_walk_hands_out_every_group_once(N, rows):
    """postpass.hpp's for_thread_groups over all (chunk, t) of the launch's own chunking: the group starts are exactly
    {0, 4, 8, .. < N}, each handed out once"""
    counts = np.zeros((N + 3) // 4, dtype=np.int32)
    assert harness().vn_host_walk(N, rows, counts.ctypes.data) == 0
    assert np.array_equal(counts, np.ones_like(counts))


def test_kernel_math_masked_reset_and_nan():
    D, B = 4, 4097
    rng = np.random.default_rng(6)
    h, o = HostNorm(D, B), VecNormOracle(D, B)
    data = list(_rollout_data(rng, D, B, 4))
    for obs, rew, done, term in data[:2]:
        _check_step(h, o, obs, rew, done, term, "warm")
    mask = (rng.random(B) < 0.2).astype(np.uint8)
    obs = data[2][0]
    got = h.reset(obs, mask); ref = o.reset(obs, mask)
    m = mask.astype(bool)
    assert_stats_close(h.stats(), o.stats(), "masked reset")
    assert_f32_within_one_ulp(got[:, m], ref[:, m], 10.0, "masked reset obs")
    assert np.all(got[:, ~m] == 0) and np.all(h.ret[m] == 0) and np.allclose(h.ret, o.ret, rtol=1e-12, atol=0) and np.array_equal(h.ep_len, o.ep_len)
    # a NaN and an inf in the normaliser's INPUT: the row's statistic stays finite and equals the one without them
    obs, rew, done, term = data[3]
    obs = obs.copy(); obs[1, 5] = np.nan; obs[3, 4000] = np.inf; obs[3, 0] = np.nan     # [3, 0] is the row's shift element
    _check_step(h, o, obs, rew, done, term, "non-finite")
    assert np.isfinite(h.st).all() and h.agg[3] == 3 == o.nonfinite
    assert abs(h.stats()["count"][0] - h.stats()["count"][1] - 1) < 1e-6


def test_kernel_math_in_place():
    D, B = 5, 4100
    rng = np.random.default_rng(7)
    a, b = HostNorm(D, B), HostNorm(D, B)
    for obs, rew, done, term in _rollout_data(rng, D, B, 3):
        out = a.step(obs, rew, done, term)[0]
        buf = obs.copy()
        b.step(buf, rew, done, term, obs_out=buf)
        assert np.array_equal(out.view(np.int32), buf.view(np.int32)) and np.array_equal(a.st, b.st)


def test_switches_leave_their_side_alone():
    D, B = 3, 130
    rng = np.random.default_rng(8)
    h, o = HostNorm(D, B, norm_obs=False), VecNormOracle(D, B, norm_obs=False)
    g, p = HostNorm(D, B, norm_reward=False), VecNormOracle(D, B, norm_reward=False)
    for obs, rew, done, term in _rollout_data(rng, D, B, 3):
        out = o.step(obs, rew, done, term); no, nr, _ = h.step(obs, rew, done, term)
        assert np.all(no == 0) and np.array_equal(h.stats()["count"][:D], np.full(D, 1e-4))
        assert_f32_within_one_ulp(nr, out["reward"], 10.0, "reward")
        out = p.step(obs, rew, done, term); no, nr, _ = g.step(obs, rew, done, term)
        assert np.all(nr == 0) and np.all(g.ret == 0) and g.stats()["count"][D] == 1e-4
        assert_f32_within_one_ulp(no, out["obs"], 10.0, "obs")
        assert np.array_equal(g.ep_len, p.ep_len)


# ------------------------------------------------------------------------------------------------- the surface exists
def test_package_exports_the_wrapper_and_the_abi_declares_the_calls():
    import random_envs_amd as rex
    from random_envs_amd import _native
    assert hasattr(rex, "NormalizedVecRandomEnv") and callable(rex.merge_stats)
    want = {"rex_norm_enable", "rex_norm_set_training", "rex_norm_reset", "rex_norm_step", "rex_norm_get_stats", "rex_norm_set_stats",
            "rex_norm_get_lane_state", "rex_norm_set_lane_state", "rex_norm_read_episodes"}
    assert want <= set(_native.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "rex.h")).read()
    assert all(w + "(" in hdr for w in want)
    src = open(HEADER).read() + open(os.path.join(os.path.dirname(HEADER), "postpass.hpp")).read()   # the chunking and block_sum moved there
    assert "getenv" not in src


def test_sb3_cross_check_when_installed():
    """the restatement against the real VecNormalize on random data; skips where stable_baselines3 is not installed"""
    sb3 = pytest.importorskip("stable_baselines3")
    from stable_baselines3.common.running_mean_std import RunningMeanStd
    del sb3
    rng = np.random.default_rng(9)
    D, B = 4, 33
    o = VecNormOracle(D, B)
    obs_rms, ret_rms = RunningMeanStd(shape=(D,)), RunningMeanStd(shape=())
    ret = np.zeros(B)
    for _ in range(5):
        x = rng.normal(size=(D, B)) * 3 + 1; r = rng.normal(size=B); d = rng.random(B) < 0.1
        out = o.step(x, r, d)
        obs_rms.update(x.T); ret = ret * 0.99 + r; ret_rms.update(ret)
        assert np.allclose(out["obs"].T, np.clip((x.T - obs_rms.mean) / np.sqrt(obs_rms.var + 1e-8), -10, 10), rtol=1e-12)
        assert np.allclose(out["reward"], np.clip(r / np.sqrt(ret_rms.var + 1e-8), -10, 10), rtol=1e-12)
        ret[d] = 0
    assert np.allclose(o.mean[:D], obs_rms.mean) and np.allclose(o.var[:D], obs_rms.var) and np.isclose(o.var[D], ret_rms.var)
