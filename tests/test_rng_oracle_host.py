"""tests/rng_oracle.py against rocRAND's own engine on the host, the region budget of the stream map, and the oracle's sample_task rules.

rocRAND's device engine is ``__host__ __device__``: tests/host_harness/rocrand_host.cpp wraps rocrand_init / rocrand / rocrand_uniform /
rocrand_normal and includes nothing of csrc/.  Raw words and uniforms are integer / exact fp32 arithmetic and must be BIT-EQUAL.

Normals: the host engine evaluates ``s = sqrtf(-2 logf(u))``, ``sinf(v) * s``, ``cosf(v) * s`` in fp32, the oracle the same u and v in fp64.
With eps = 2^-24 (half an fp32 ulp, relative): logf is within 1 ulp (2 eps relative), the product with -2 is exact, the square root halves the
relative error and sqrtf adds its own rounding: |ds| <= 2 eps s.  sinf / cosf are within 1 ulp of a value below 1, an absolute 2 eps; the
final product rounds once more, eps relative.  |d(s sin v)| <= s (2 eps + 2 eps + eps) = 5 eps s, about 2.5 fp32 ulps of s, and
s <= sqrt(-2 ln 2^-32) = 6.66.  The tests allow 6 eps s (three ulps), per draw, with the draw's own s.
"""
import ctypes
import math
import os

import numpy as np
import pytest

import rng_oracle as R
from random_envs_amd.specs import SPECS, UNMODELED_SPECS
from replay_buffer_oracle import PHILOX_KAT, philox4x32_10

EPS = 2.0 ** -24


def _rocm_include():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "rocrand", "rocrand_kernel.h")):
            return os.path.join(root, "include")
    return None


@pytest.fixture(scope="module")
def rr():
    inc = _rocm_include()
    if inc is None:
        pytest.skip("rocRAND headers (rocrand/rocrand_kernel.h) not found under ROCM_PATH or /opt/rocm")
    from host_harness.build import build_so
    L = ctypes.CDLL(build_so("rocrand_host", "rocrand_host.cpp", extra_flags=("-w", "-D__HIP_PLATFORM_AMD__", "-I" + inc)))
    u64 = ctypes.c_uint64
    L.rr_draws.argtypes = [u64, u64, u64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)]
    L.rr_uniform_of.argtypes = [ctypes.c_uint32]; L.rr_uniform_of.restype = ctypes.c_float
    return L


def _engine(L, seed, subseq, offset, ops):
    ops = np.ascontiguousarray(ops, dtype=np.int32); n = len(ops)
    words = np.zeros(n, dtype=np.uint32); vals = np.zeros(n, dtype=np.float32)
    rc = L.rr_draws(seed, subseq, offset, n, ops.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                    vals.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    assert rc == 0
    return words, vals


SEEDS = [11, (1 << 33) + 11, 0xFEDCBA9876543210]
SUBSEQS = [0, 5, 199, (1 << 32) + 7, (1 << 40) + 123456789]
EPISODES = [1, 3, 4, 5, 1 << 20]          # the high word of the block counter is non-zero from episode 4 (4 * 2^32 / 4 = 2^32)
REGIONS = [0, 256, 512, 512 + 64 * 1, 512 + 64 * 7, 512 + 64 * 499]
OFFSETS = [ep * R.EP_STRIDE + r for ep in EPISODES for r in REGIONS]


def test_philox_known_answers():
    for ctr, key, out in PHILOX_KAT:
        assert philox4x32_10(ctr, key) == out


@pytest.mark.parametrize("seed", SEEDS)
def test_words_and_uniforms_bit_equal(rr, seed):
    """37 draws cross nine blocks; every combination of subsequence and offset of the stream map"""
    n = 37
    for subseq in SUBSEQS:
        for off in OFFSETS:
            words, _ = _engine(rr, seed, subseq, off, [0] * n)
            mine = [R.word(seed, subseq, off + j) for j in range(n)]
            assert [int(w) for w in words] == mine, (seed, subseq, off)
            _, us = _engine(rr, seed, subseq, off, [1] * n)
            st = R.Stream(seed, subseq, off)
            ou = np.array([st.uniform() for _ in range(n)], dtype=np.float32)
            assert ou.dtype == np.float32 and np.array_equal(ou.view(np.uint32), us.view(np.uint32)), (seed, subseq, off)
            assert st.words_used == n


def test_offsets_that_are_no_multiple_of_four(rr):
    """the issue's hand check -- rocrand_init(11, 5, (3 << 32) + 256) -- and offsets inside a block"""
    for off in [(3 << 32) + 256, (3 << 32) + 257, (3 << 32) + 258, (3 << 32) + 259, 1, 2, 3, (1 << 34) - 1]:
        words, _ = _engine(rr, 11, 5, off, [0] * 9)
        assert [int(w) for w in words] == [R.word(11, 5, off + j) for j in range(9)], off


def test_uniform_conversion_edges(rr):
    for w in [0, 1, 2, 127, 128, 129, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 31) - 1, 1 << 31, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFF81, 0xFFFFFFFF]:
        a, b = np.float32(rr.rr_uniform_of(w)), R.uniform(w)
        assert a.view(np.uint32) == b.view(np.uint32), hex(w)
    assert R.uniform(0) > 0 and R.uniform(0xFFFFFFFF) == np.float32(1.0)


def _check_normals(rr, seed, subseq, off, ops):
    words, vals = _engine(rr, seed, subseq, off, ops)
    st = R.Stream(seed, subseq, off)
    worst = 0.0
    for j, op in enumerate(ops):
        if op == 0:
            assert int(words[j]) == st.next_word(), (seed, subseq, off, j)
        elif op == 1:
            assert np.float32(vals[j]).view(np.uint32) == st.uniform().view(np.uint32), (seed, subseq, off, j)
        else:
            z = st.normal()
            err, tol = abs(float(vals[j]) - z), 6 * EPS * st.last_scale
            worst = max(worst, err / max(st.last_scale, 1e-30) / EPS)
            assert err <= tol, (seed, subseq, off, j, float(vals[j]), z, err, tol)
    return st.words_used, worst


@pytest.mark.parametrize("seed", SEEDS)
def test_normals_within_three_ulps_of_s(rr, seed):
    worst = 0.0
    for subseq in SUBSEQS:
        for off in OFFSETS:
            used, w = _check_normals(rr, seed, subseq, off, [2] * 45)        # 45: the humanoid's noisy rows, an odd count
            assert used == 46
            worst = max(worst, w)
    print("largest |host engine - oracle| of a normal: %.2f eps s (allowed 6)" % worst)


@pytest.mark.parametrize("seed", SEEDS)
def test_interleaved_uniform_and_normal_keep_the_saved_half(rr, seed):
    """the half-cheetah pattern -- qpos[2p] uniform, qvel[2p] normal (.x of a new pair), qpos[2p+1] uniform, qvel[2p+1] normal (the saved .y)
    -- takes words (u, pair, pair, u); then a raw word between the two halves of a pair"""
    for subseq in SUBSEQS:
        for off in OFFSETS[::5]:
            used, _ = _check_normals(rr, seed, subseq, off, [1, 2] * 9)
            assert used == 4 * 4 + 3                                          # nine dofs: four full groups of four words, then u, pair, pair
            _check_normals(rr, seed, subseq, off, [2, 0, 1, 2, 2, 1, 0, 2, 2, 2, 1])


def test_init_state_takes_the_documented_words():
    """word 2k -> qpos[k], word 2k+1 -> qvel[k] (hopper, walker2d); (qpos[2p], pair, pair, qpos[2p+1]) (half-cheetah); q then v (humanoid);
    x, x_dot, theta, theta_dot (cartpole) -- against the words picked by index"""
    seed, subseq, ep = (1 << 33) + 11, (1 << 32) + 7, 5
    base = ep * R.EP_STRIDE
    U = lambda j: float(R.uniform(R.word(seed, subseq, base + j)))
    q, v, n = R.init_state("hopper", seed, subseq, ep)
    c = float(np.float32(0.005))
    assert n == 12 and q[1] == 1.25 + c * (2 * (1 - U(2)) - 1) and v[4] == c * (2 * (1 - U(9)) - 1) and q[5] == c * (2 * (1 - U(10)) - 1)
    q, v, n = R.init_state("walker2d", seed, subseq, ep)
    assert n == 18 and q[8] == c * (2 * (1 - U(16)) - 1) and v[8] == c * (2 * (1 - U(17)) - 1)
    q, v, n = R.init_state("halfcheetah", seed, subseq, ep)
    c = float(np.float32(0.1))
    x, y = R.normal2(R.word(seed, subseq, base + 5), R.word(seed, subseq, base + 6))
    assert n == 19 and q[2] == c * (2 * (1 - U(4)) - 1) and q[3] == c * (2 * (1 - U(7)) - 1) and v[2] == c * x and v[3] == c * y
    assert q[8] == c * (2 * (1 - U(16)) - 1) and v[8] == c * R.normal2(R.word(seed, subseq, base + 17), R.word(seed, subseq, base + 18))[0]
    q, v, n = R.init_state("humanoid", seed, subseq, ep)
    c = float(np.float32(0.01))
    assert n == 47 and q[2] == 1.4 + c * (2 * (1 - U(2)) - 1) and q[3] == 1.0 + c * (2 * (1 - U(3)) - 1) and v[0] == c * (2 * (1 - U(24)) - 1) and v[22] == c * (2 * (1 - U(46)) - 1)
    q, v, n = R.init_state("cartpole", seed, subseq, ep)
    d = [float(-np.float32(0.05)) + float(np.float32(0.1)) * (1 - U(j)) for j in range(4)]
    assert n == 4 and list(q) == [d[0], d[2]] and list(v) == [d[1], d[3]]
    assert np.abs(q).max() <= 0.05 + 1e-9 and np.abs(v).max() <= 0.05 + 1e-9


OBS_DIMS = {"cartpole": 4, "hopper": 11, "halfcheetah": 17, "walker2d": 17, "humanoid": 376}
NOISY_ROWS = {"cartpole": 0, "hopper": 11, "halfcheetah": 17, "walker2d": 17, "humanoid": 45}   # rows of the observation that take noise


def test_region_budget():
    """A longer state, observation or task vector must fail HERE, not run one region of a stream into the next."""
    assert R.INIT_BASE + R.INIT_WORDS <= R.XI_BASE and R.XI_BASE + R.XI_WORDS <= R.STEP_BASE and R.STEP_BASE % 4 == 0 and R.STEP_STRIDE % 4 == 0
    for kind in SPECS:
        assert R.init_words(kind) <= R.INIT_WORDS, kind
        assert R.obs_noise_words(NOISY_ROWS[kind]) <= R.STEP_WORDS, kind
    st = R.Stream(1, 2, R.STEP_BASE)
    for _ in range(45):
        st.normal()
    assert st.words_used == R.obs_noise_words(45) == 46
    for table in (SPECS, UNMODELED_SPECS):
        for kind, spec in table.items():
            dim = len(spec.names)
            assert dim <= 32                                                  # MAX_XI rows of the distribution block
            for dr_type in ("uniform", "truncnorm", "gaussian", "fullgaussian"):
                worst = R.xi_words_worst(dr_type, dim)
                assert worst <= R.XI_WORDS and worst <= R.SAMPLE_WORDS, (kind, dr_type, worst)
    assert R.xi_words_worst("truncnorm", 30) == 90 and R.xi_words_worst("gaussian", 30) == 90 and R.xi_words_worst("gaussian", 13) == 40
    assert R.xi_words_worst("fullgaussian", 13) == 14 and R.xi_words_worst("fullgaussian", 30) == 30
    # the oracle's own count reaches the stated worst case: every draw of every dim below its floor
    for dr_type, dim in (("truncnorm", 30), ("gaussian", 30), ("gaussian", 13)):
        dr = R.dr_params(dr_type, np.stack([np.full(dim, -50.0), np.ones(dim)], 1).ravel(), lower_bounds=np.full(dim, 0.1))
        out = R.sample_task(dr, 3, 4, 256)
        assert out["words_used"] == R.xi_words_worst(dr_type, dim) and out["clamped"].all() and (out["redraws"] == 2).all()
    dim = 13
    A = np.random.RandomState(0).randn(dim, dim) * 0.1
    dr = R.dr_params("fullgaussian", {"mean": np.full(dim, 2.0), "cov": A @ A.T + 0.05 * np.eye(dim)}, search_bounds=(np.zeros(dim), np.ones(dim)))
    assert R.sample_task(dr, 3, 4, 256)["words_used"] == R.xi_words_worst("fullgaussian", dim)


def test_sample_task_far_bounds_take_no_redraw():
    dim = 13
    spec = SPECS["walker2d"]; mean = np.array(spec.nominal_task); std = 0.1 * mean
    for dr_type in ("truncnorm", "gaussian"):
        dr = R.dr_params(dr_type, np.stack([mean + 10.0, std], 1).ravel(), lower_bounds=spec.lower_bounds)
        for subseq in range(64):
            out = R.sample_task(dr, 7, subseq, R.EP_STRIDE + 256)
            assert not out["redraws"].any() and not out["clamped"].any()
            assert out["words_used"] == (dim if dr_type == "truncnorm" else dim + 1)
            z = (out["xi"] - dr["a"]) / dr["b"]
            assert np.abs(z).max() <= (2.0 if dr_type == "truncnorm" else 6.7)
    dr = R.dr_params("uniform", np.stack([0.9 * mean, 1.1 * mean], 1).ravel())
    out = R.sample_task(dr, 7, 3, R.EP_STRIDE + 256)
    assert out["words_used"] == dim and (out["xi"] >= dr["a"]).all() and (out["xi"] <= dr["b"]).all()
    u3 = float(R.uniform(R.word(7, 3, R.EP_STRIDE + 256 + 3)))
    assert out["xi"][3] == dr["a"][3] + (dr["b"][3] - dr["a"][3]) * (1 - u3)


@pytest.mark.parametrize("dr_type", ["truncnorm", "gaussian"])
def test_sample_task_branch_shares(dr_type):
    """mean = floor + 0.5 sigma: a draw falls below the floor with p = (Phi(-0.5) - Phi(-2)) / (Phi(2) - Phi(-2)) = 0.2994 (truncnorm) or
    Phi(-0.5) = 0.3085 (gaussian).  P(exactly k redraws) = p^k (1 - p) for k < 2, P(two redraws) = p^2, P(clamped) = p^3; each count over
    N = 4096 subsequences within 4 sigma of its binomial.

    tests/test_dr_host.py and tests/test_gpu_reset_dr.py use 0.2858 for the truncnorm share: that is Phi(-0.5) - Phi(-2) WITHOUT the division by
    the mass of [-2, 2] (0.9545), 1.4 points low; their windows of 0.01 on p^3 (0.0233 against 0.0268) do not see it.  The truncnorm counts are
    held to that figure's shares as well, so this oracle and oracle/dr_sampler.py stay tied to one number, but the exact share is the one that
    decides."""
    N = 4096
    nd = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))
    p = (nd(-0.5) - nd(-2)) / (nd(2) - nd(-2)) if dr_type == "truncnorm" else nd(-0.5)
    assert abs(nd(-0.5) - nd(-2) - 0.2858) < 5e-5 and abs((nd(-0.5) - nd(-2)) / (nd(2) - nd(-2)) - 0.29941) < 5e-6
    dr = R.dr_params(dr_type, [0.15, 0.1], lower_bounds=[0.1])
    red = np.zeros(N, dtype=np.int64); cl = np.zeros(N, dtype=bool); xs = np.zeros(N)
    for i in range(N):
        out = R.sample_task(dr, (1 << 33) + 11, (1 << 32) + i, 2 * R.EP_STRIDE + 256)
        red[i], cl[i], xs[i] = out["redraws"][0], out["clamped"][0], out["xi"][0]
    assert xs.min() >= float(np.float32(0.1)) and (xs[cl] == float(np.float32(0.1))).all() and not (cl & (red < 2)).any()
    if dr_type == "truncnorm":
        assert xs.max() <= float(np.float32(0.15)) + 2 * float(np.float32(0.1))
    counts = {"0 redraws": (red == 0).sum(), "1 redraw": (red == 1).sum(), "2 redraws": (red == 2).sum(), "clamped": cl.sum()}
    for q in [p] + ([0.2858] if dr_type == "truncnorm" else []):
        shares = {"0 redraws": 1 - q, "1 redraw": q * (1 - q), "2 redraws": q * q, "clamped": q ** 3}
        for name, share in shares.items():
            sigma = math.sqrt(N * share * (1 - share))
            print("%s p=%.4f %s: %d of %d, expected %.1f +- %.1f" % (dr_type, q, name, counts[name], N, N * share, sigma))
            assert abs(counts[name] - N * share) <= 4 * sigma, (dr_type, q, name, int(counts[name]), N * share, sigma)


def test_fullgaussian_is_mean_plus_lower_factor_times_z():
    d = 8
    A = np.random.RandomState(0).randn(d, d) * 0.1; cov = A @ A.T + 0.05 * np.eye(d)
    mean = np.full(d, 2.0); mean[:2] = 0.2; mean[2:4] = 3.8
    lo, hi = np.full(d, 0.5), np.full(d, 10.0)
    dr = R.dr_params("fullgaussian", {"mean": mean, "cov": cov}, search_bounds=(lo, hi))
    assert np.allclose(dr["chol"] @ dr["chol"].T, cov, atol=1e-6) and np.array_equal(dr["chol"], np.tril(dr["chol"]))
    seen_low = seen_high = 0
    for subseq in range(200):
        out = R.sample_task(dr, 5, subseq, R.EP_STRIDE + 256)
        st = R.Stream(5, subseq, R.EP_STRIDE + 256)
        z = np.array([st.normal() for _ in range(d)])
        x = np.clip(dr["a"] + dr["chol"] @ z, 0, 4)
        assert np.allclose(out["xi"], x * (hi - lo) / 4 + lo, rtol=1e-12, atol=1e-12) and out["words_used"] == 8
        seen_low += int((x == 0).sum()); seen_high += int((x == 4).sum())
    assert seen_low >= 3 and seen_high >= 3                                   # both clips act at these means


def test_gpu_cases_populate_every_branch_under_the_widest_exclusion():
    """The seed, offsets and parameters of tests/test_gpu_rng_streams.py, from the oracle alone: with the exclusion radius at its cap (1 % of
    sigma; the measured tolerances are far inside) at most 1 % of a case's lane-dimensions sit next to a threshold, every redraw branch keeps
    at least 3 compared lane-dimensions, and both fullgaussian clips act."""
    import test_gpu_rng_streams as G
    from random_envs_amd import registry
    cases = [(eid, mode, "reset") for eid in G.XI_IDS for mode in ("truncnorm", "gaussian", "fullgaussian")]
    cases += [("RandomHopper-v0", "gaussian", "sample"), ("RandomWalker2dUnmodeled-v0", "truncnorm", "sample"), ("RandomHumanoid-v0", "fullgaussian", "sample")]
    for eid, mode, what in cases:
        dr_type, _, dr = G.dr_case(registry.spec(eid), mode)
        for off in G.ENV_OFFSETS:
            for k in range(3 if what == "sample" else 1):
                if what == "sample":
                    outs = [R.sample_task_draw(dr, G.SEED, off + i, k) for i in range(G.B)]
                else:
                    outs = [R.reset_xi(dr, G.SEED, off + i, 1) for i in range(G.B)]
                assert max(o["words_used"] for o in outs) <= R.xi_words_worst(dr_type, dr["dim"])
                if dr_type == "fullgaussian":
                    clip = np.array([o["clamped"] for o in outs]); ref = np.array([o["xi"] for o in outs]); mid = 0.5 * (dr["lo"] + dr["hi"])[None]
                    assert (clip & (ref < mid)).sum() >= 3 and (clip & (ref > mid)).sum() >= 3, (eid, mode, off, k)
                else:
                    keep, census = G.branch_census(outs, G.CAP[dr_type])
                    assert (~keep).sum() <= 0.01 * keep.size and min(census.values()) >= 3, (eid, mode, off, k, int((~keep).sum()), census)
