"""Device-side rollout buffer, CPU half: the kernels' own arithmetic and addressing (the __host__ __device__ functions of
csrc/rollout.hpp, driven in grid order by tests/host_harness/rollout_host.cpp) against the numpy fp64 oracle of
tests/rollout_oracle.py.  GAE, the stored rows, the bootstrapped reward and the gather are held to IDENTICAL BITS; the moments to
the bound of tests/test_vecnorm_host.py (n <= 2^22 fp64 terms err by n 2^-53 ~ 5e-10 < 1e-9), normalised advantages to 1 fp32 ulp."""
import ctypes

import numpy as np
import pytest

import rollout_oracle as oracle
from host_harness.build import build_so

FIELDS = ("obs", "action", "reward", "value", "log_prob", "advantage", "returns", "done")

_lib = None


def harness():
    """tests/host_harness/rollout_host.cpp built with g++ (rebuilt when it or a header is newer); no fused multiply-add"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("rollout_host", "rollout_host.cpp", ["-ffp-contract=off"]))
        vp, ll, i32, f64 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double
        _lib.ro_host_parts.argtypes = [ll]
        _lib.ro_host_tile.argtypes = [vp, i32, i32, vp, i32, i32]
        _lib.ro_host_tile.restype = None
        _lib.ro_host_add.argtypes = [vp, ll, ll, i32, i32, ll, vp, f64, i32]
        _lib.ro_host_gae.argtypes = [vp, ll, ll, vp, f64, f64]
        _lib.ro_host_adv_stats.argtypes = [vp, ll, i32, i32, vp]
        _lib.ro_host_gather.argtypes = [vp, ll, ll, i32, i32, vp, ll, vp, vp]
    return _lib


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def empty_buffers(T, B, D, A, act_dtype=np.float32):
    return dict(obs=np.zeros((T, D, B), np.float32), action=np.zeros((T, A, B), act_dtype), reward=np.zeros((T, B), np.float32),
                value=np.zeros((T, B), np.float32), log_prob=np.zeros((T, B), np.float32), advantage=np.zeros((T, B), np.float32),
                returns=np.zeros((T, B), np.float32), done=np.zeros((T, B), np.uint8))


def random_step(rng, B, D, A, discrete=False, p_done=0.1, p_trunc=0.2):
    """one step's inputs with awkward float32 bit patterns in them (denormals, -0, huge values)"""
    obs = (rng.normal(size=(D, B)) * 10.0 ** rng.uniform(-3, 3, size=(D, 1))).astype(np.float32)
    obs.ravel()[::7] = np.float32(-0.0)
    if B > 2:
        obs[0, 1] = np.float32(1e-42); obs[-1, -1] = np.float32(3e38)
    act = rng.integers(0, 2, size=(A, B)).astype(np.int32) if discrete else rng.uniform(-1, 1, size=(A, B)).astype(np.float32)
    return dict(obs=obs, action=act, reward=rng.normal(size=B).astype(np.float32), done=(rng.random(B) < p_done).astype(np.uint8),
                value=(rng.normal(size=B) * 3).astype(np.float32), log_prob=(-rng.random(B) * 5).astype(np.float32),
                truncated=(rng.random(B) < p_trunc).astype(np.uint8), terminal_value=(rng.normal(size=B) * 3).astype(np.float32))


def random_rollout(rng, T, B, density, scale=1.0):
    reward = (rng.normal(size=(T, B)) * scale).astype(np.float32)
    value = (rng.normal(size=(T, B)) * 3 * scale).astype(np.float32)
    done = (rng.random((T, B)) < density).astype(np.uint8)
    last = (rng.normal(size=B) * 3 * scale + 1.0).astype(np.float32)
    return reward, value, done, last


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def assert_same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, "%s: %s %s against %s %s" % (what, got.shape, got.dtype, ref.shape, ref.dtype)
    bad = bits(got) != bits(ref)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def assert_moments_close(got, ref, what=""):
    """counts equal, |dmean| <= 1e-9 (|mean| + sigma), |dM2| <= 1e-9 M2 (the bound of tests/test_vecnorm_host.py)"""
    assert got["n"] == ref["n"] and got["nonfinite"] == ref["nonfinite"], "%s: %s against %s" % (what, got, ref)
    if ref["n"] == 0:
        return
    sigma = np.sqrt(ref["m2"] / ref["n"])
    assert abs(got["mean"] - ref["mean"]) <= 1e-9 * (abs(ref["mean"]) + sigma), "%s: mean %r against %r" % (what, got["mean"], ref["mean"])
    assert abs(got["m2"] - ref["m2"]) <= 1e-9 * ref["m2"], "%s: M2 %r against %r" % (what, got["m2"], ref["m2"])


def assert_normalised_within_one_ulp(got, ref64, what=""):
    d = oracle.f32_ulp_distance(got, np.asarray(ref64, dtype=np.float64).astype(np.float32))
    assert d.max() <= 1, "%s: %d ulps" % (what, d.max())


# ------------------------------------------------------------------------------------------------- the harness behind plain functions
def host_add(bufs, slot, step, gamma, with_trunc=True, vec_ok=None):
    T, D, B = bufs["obs"].shape
    A = bufs["action"].shape[1]
    src = [step[k] for k in ("obs", "action", "reward", "done", "value", "log_prob")] + ([step["truncated"], step["terminal_value"]] if with_trunc else [None, None])
    vec = (B % 4 == 0) if vec_ok is None else vec_ok
    return harness().ro_host_add(_ptrs([bufs[k] for k in FIELDS]), T, B, D, A, slot, _ptrs(src), gamma, int(vec))


def host_gae(reward, value, done, last_value, gamma, lam):
    T, B = reward.shape
    bufs = dict(reward=np.ascontiguousarray(reward), value=np.ascontiguousarray(value), done=np.ascontiguousarray(done),
                advantage=np.zeros((T, B), np.float32), returns=np.zeros((T, B), np.float32))
    rc = harness().ro_host_gae(_ptrs([bufs.get(k) for k in FIELDS]), T, B, np.ascontiguousarray(last_value).ctypes.data, gamma, lam)
    assert rc == 0
    return bufs["advantage"], bufs["returns"]


def host_adv_stats(adv, normalise=False, vec_ok=True):
    """(statistics, the flat buffer after the call)"""
    x = np.ascontiguousarray(adv, dtype=np.float32).ravel().copy()
    out = np.zeros(4)
    assert harness().ro_host_adv_stats(x.ctypes.data, x.size, int(normalise), int(vec_ok), out.ctypes.data) == 0
    return dict(n=int(out[0]), mean=out[1], m2=out[2], nonfinite=int(out[3])), x


def host_gather(bufs, index, skip=()):
    T, D, B = bufs["obs"].shape
    A = bufs["action"].shape[1]
    idx = np.ascontiguousarray(index, dtype=np.int64)
    n = idx.size
    out = dict(obs=np.full((n, D), 7, np.float32), action=np.full((n, A), 7, bufs["action"].dtype), advantage=np.full(n, 7, np.float32),
               returns=np.full(n, 7, np.float32), value=np.full(n, 7, np.float32), log_prob=np.full(n, 7, np.float32))
    bad = ctypes.c_longlong(0)
    outs = [None if k in skip else out[k] for k in ("obs", "action", "advantage", "returns", "value", "log_prob")]
    assert harness().ro_host_gather(_ptrs([bufs[k] for k in FIELDS]), T, B, D, A, idx.ctypes.data, n, _ptrs(outs), ctypes.byref(bad)) == 0
    return out, bad.value


def filled_buffers(rng, T, B, D, A, discrete=False):
    b = empty_buffers(T, B, D, A, np.int32 if discrete else np.float32)
    for k in FIELDS:
        if k == "done":
            b[k][:] = rng.random((T, B)) < 0.3
        elif k == "action" and discrete:
            b[k][:] = rng.integers(0, 2, size=b[k].shape)
        else:
            b[k][:] = rng.normal(size=b[k].shape) * 100
    return b


# ------------------------------------------------------------------------------------------------- GAE
SHAPES = [(T, B) for T in (1, 2, 7, 33) for B in (1, 63, 64, 257)]


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0)])
@pytest.mark.parametrize("density", [0.0, 0.1, 1.0])
def test_gae_bits_equal_the_oracle(density, gamma, lam):
    rng = np.random.default_rng(int(density * 10) + 7)
    for T, B in SHAPES:
        reward, value, done, last = random_rollout(rng, T, B, density)
        adv, ret = host_gae(reward, value, done, last, gamma, lam)
        ref_adv, ref_ret = oracle.gae(reward, value, done, last, gamma, lam)
        assert_same_bits(adv, ref_adv, "advantage T=%d B=%d" % (T, B))
        assert_same_bits(ret, ref_ret, "returns T=%d B=%d" % (T, B))


@pytest.mark.parametrize("T", [1, 7, 33])
def test_gae_final_done_cuts_the_bootstrap(T):
    """done[T-1] set and last_value far from 0: the last step's delta must not see last_value"""
    rng = np.random.default_rng(T)
    reward, value, done, _ = random_rollout(rng, T, 63, 0.0)
    done[T - 1] = 1
    last = np.full(63, 1000.0, np.float32)
    adv, ret = host_gae(reward, value, done, last, 0.99, 0.95)
    ref_adv, ref_ret = oracle.gae(reward, value, done, last, 0.99, 0.95)
    assert_same_bits(adv, ref_adv); assert_same_bits(ret, ref_ret)
    assert_same_bits(adv[T - 1], (reward[T - 1].astype(np.float64) - value[T - 1].astype(np.float64)).astype(np.float32))
    open_adv, _ = host_gae(reward, value, np.zeros_like(done), last, 0.99, 0.95)
    assert np.all(np.abs(open_adv[T - 1] - adv[T - 1]) > 900)


def test_gae_with_wide_range_values():
    """sums that cancel and operands of very different magnitude: where a fused multiply-add would change the bits"""
    rng = np.random.default_rng(3)
    T, B = 33, 257
    reward, value, done, last = random_rollout(rng, T, B, 0.1)
    reward *= (10.0 ** rng.uniform(-6, 6, size=(T, B))).astype(np.float32)
    value[::2] = (reward[::2] * np.float32(1.0000001)).astype(np.float32)
    adv, ret = host_gae(reward, value, done, last, 0.99, 0.95)
    ref_adv, ref_ret = oracle.gae(reward, value, done, last, 0.99, 0.95)
    assert_same_bits(adv, ref_adv); assert_same_bits(ret, ref_ret)


# ------------------------------------------------------------------------------------------------- add
@pytest.mark.parametrize("B", [1, 63, 64, 257, 4100])
@pytest.mark.parametrize("discrete", [False, True])
def test_add_stores_the_rows_bit_for_bit(B, discrete):
    rng = np.random.default_rng(B)
    T, D, A, gamma = 3, (4 if discrete else 11), (1 if discrete else 3), 0.99
    bufs = empty_buffers(T, B, D, A, np.int32 if discrete else np.float32)
    steps = [random_step(rng, B, D, A, discrete) for _ in range(T)]
    for t in (2, 0, 1):                                # any order: the slot is an argument
        assert host_add(bufs, t, steps[t], gamma, with_trunc=(t != 1)) == 0
    for t, s in enumerate(steps):
        for k in ("obs", "action", "value", "log_prob", "done"):
            assert_same_bits(bufs[k][t], s[k], "%s slot %d" % (k, t))
        m = s["truncated"].astype(bool)
        if t == 1:                                     # no truncated / terminal_value given: a plain copy
            assert_same_bits(bufs["reward"][t], s["reward"])
            continue
        boot = (np.float64(1) * s["reward"].astype(np.float64) + gamma * s["terminal_value"].astype(np.float64)).astype(np.float32)
        assert_same_bits(bufs["reward"][t][m], boot[m], "bootstrapped reward")
        assert_same_bits(bufs["reward"][t][~m], s["reward"][~m], "other lanes")
        assert_same_bits(bufs["reward"][t], oracle.bootstrap_reward(s["reward"], s["truncated"], s["terminal_value"], gamma))
    assert not bufs["advantage"].any() and not bufs["returns"].any()
    assert host_add(bufs, T, steps[0], gamma) != 0 and host_add(bufs, -1, steps[0], gamma) != 0


def test_add_bits_do_not_depend_on_the_access_width():
    rng = np.random.default_rng(0)
    T, B, D, A = 2, 2052, 5, 2
    step = random_step(rng, B, D, A)
    wide, narrow = empty_buffers(T, B, D, A), empty_buffers(T, B, D, A)
    host_add(wide, 1, step, 0.99, vec_ok=True); host_add(narrow, 1, step, 0.99, vec_ok=False)
    for k in FIELDS:
        assert_same_bits(wide[k], narrow[k], k)


# ------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("T,B", [(1, 1), (1, 2), (7, 63), (33, 257), (128, 8192 + 5)])
def test_moments_and_normalisation(T, B):
    rng = np.random.default_rng(T * B)
    adv = (rng.normal(size=(T, B)) * 3 + 50).astype(np.float32)     # a mean far from 0 against the spread
    ref = oracle.adv_stats(adv)
    for vec in (True, False):
        got, after = host_adv_stats(adv, normalise=False, vec_ok=vec)
        assert_moments_close(got, ref, "T=%d B=%d" % (T, B))
        assert_same_bits(after.reshape(T, B), adv, "untouched without normalise")
        got_n, after = host_adv_stats(adv, normalise=True, vec_ok=vec)
        assert got_n == got
        assert_normalised_within_one_ulp(after, oracle.normalised(adv, ref).ravel(), "T=%d B=%d" % (T, B))
    if T * B > 1:
        assert abs(after.astype(np.float64).mean()) < 1e-3 and abs(after.astype(np.float64).std(ddof=1) - 1) < 1e-3


def test_moments_block_count_depends_on_the_size_only():
    L = harness()
    assert [L.ro_host_parts(n) for n in (1, 1024, 1025, 1024 * 1024, 1024 * 1024 + 1, 1 << 22)] == [1, 1, 2, 1024, 1024, 1024]


def test_moments_leave_out_and_count_non_finite_elements():
    rng = np.random.default_rng(5)
    adv = rng.normal(size=(9, 300)).astype(np.float32)
    adv[0, 0] = np.nan; adv[3, 17] = np.inf; adv[8, 299] = -np.inf; adv[4, 4] = np.nan
    ref = oracle.adv_stats(adv)
    assert ref["nonfinite"] == 4 and ref["n"] == adv.size - 4
    got, _ = host_adv_stats(adv)
    assert_moments_close(got, ref, "non-finite planted")
    _, after = host_adv_stats(adv, normalise=True)
    ok = np.isfinite(adv).ravel()
    assert_normalised_within_one_ulp(after[ok], oracle.normalised(adv, ref).ravel()[ok])


# ------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("nr", [1, 63, 64])
@pytest.mark.parametrize("n", [1, 63, 64])
def test_lds_tile_round_trip_is_the_transpose(n, nr):
    """postpass.hpp's tile_stage / tile_write on one block: a source whose word encodes (item, row) comes out transposed in rows
    [r0, r0 + nr) of the first n items of an exactly sized destination; every other word keeps its sentinel"""
    dim, r0, sentinel = nr + 5, 3, 0xDEADBEEF
    item, row = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(nr, dtype=np.uint32))      # [nr][n]
    src = np.ascontiguousarray((item << 16) | row)
    dst = np.full((n, dim), sentinel, dtype=np.uint32)
    harness().ro_host_tile(src.ctypes.data, n, nr, dst.ctypes.data, dim, r0)
    assert np.array_equal(dst[:, r0:r0 + nr], src.T)
    assert np.all(dst[:, :r0] == sentinel) and np.all(dst[:, r0 + nr:] == sentinel)


@pytest.mark.parametrize("T,B,D,A,discrete", [(7, 63, 11, 3, False), (3, 63, 376, 17, False), (5, 130, 4, 1, True), (1, 1, 1, 1, False), (2, 64, 65, 64, False)])
def test_gather_equals_fancy_indexing(T, B, D, A, discrete):
    rng = np.random.default_rng(D)
    bufs = filled_buffers(rng, T, B, D, A, discrete)
    N = T * B
    for n in (1, 63, 64, 65, 200):
        idx = rng.integers(0, N, size=n)
        idx[n // 2:] = idx[:n - n // 2]              # duplicates
        out, bad = host_gather(bufs, idx)
        ref = oracle.gather(bufs, idx)
        assert bad == 0
        for k, v in ref.items():
            assert_same_bits(out[k], np.ascontiguousarray(v), "%s n=%d" % (k, n))
    out, _ = host_gather(bufs, np.arange(N), skip=("obs", "value"))
    assert np.all(out["obs"] == 7) and np.all(out["value"] == 7)          # skipped outputs are not written
    assert_same_bits(out["returns"], bufs["returns"].ravel())


def test_gather_guards_out_of_range_indices():
    rng = np.random.default_rng(1)
    T, B, D, A = 3, 70, 11, 3
    bufs = filled_buffers(rng, T, B, D, A)
    N = T * B
    idx = rng.integers(0, N, size=150)
    wrong = {0: -1, 5: N, 64: N + 12345, 100: -(1 << 62), 149: (1 << 62)}
    for k, v in wrong.items():
        idx[k] = v
    out, bad = host_gather(bufs, idx)
    assert bad == len(wrong)
    good = np.array([k not in wrong for k in range(idx.size)])
    ref = oracle.gather(bufs, idx[good])
    for k, v in ref.items():
        assert_same_bits(out[k][good], np.ascontiguousarray(v), k)
        assert not bits(out[k][~good]).any(), k      # zero rows
