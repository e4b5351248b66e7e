"""Sequence windows from the replay buffer, CPU half: the kernel's own arithmetic and addressing (the __host__ __device__ functions of
csrc/seq_replay.hpp, driven in grid order by tests/host_harness/seq_host.cpp -- a block row per sample, the ballot as an array, every
thread's walk through the sample's output) against the numpy oracle of tests/seq_replay_oracle.py.  Every field is held to IDENTICAL BITS
(copies and exact integer arithmetic on both sides) except normalised values, which are held within 1 fp32 ulp by
assert_f32_within_one_ulp, the criterion of tests/test_replay_buffer_host.py.  The harness hands the launch outputs full of NaN / -7, so
padding the launch does not write itself shows."""
import os
import subprocess

import numpy as np
import pytest

import replay_buffer_oracle as rb_oracle
import seq_replay_oracle as oracle
from host_harness import rbuf as rb_host
from host_harness import seq as host
from test_nstep_replay_host import ENDINGS, heads_of, some_ids, window_buffers, window_ids
from test_replay_buffer_host import DIMS, SHAPES, random_norm
from test_rollout_host import assert_same_bits
from test_vecnorm_host import assert_f32_within_one_ulp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "host_harness")
SEQ_LENS = (1, 3, 5)
SEQ = ("obs", "action", "reward", "done", "mask", "length")
# the second case that must show every ending: windows of the full 64 steps (T, B, probability of a done, lengths, heads, seed of the data)
LONGEST = dict(T=70, B=5, p_done=0.005, n_steps=(64,), heads=(0, 35, 69), seed=0)


def assert_every_ending(case, head, L, info, bufs):
    """the conditions on the ORACLE's output under which no ending goes untested"""
    counts = [int((info["ending"] == e).sum()) for e in (oracle.END_EPISODE, oracle.END_HEAD, oracle.END_FULL)]
    full_wraps = int((info["wrapped"] & (info["ending"] == oracle.END_FULL)).sum())
    print("T=%d head=%d L=%d: endings (episode, head, full) %s, %d full-length windows wrap" % (case["T"], head, L, counts, full_wraps))
    if case is ENDINGS:
        assert (bufs["timeout"] != 0).any() and ((bufs["done"] != 0) & (bufs["timeout"] == 0)).any()
        assert min(counts) >= 57, counts
        if head == 4:
            assert full_wraps >= 1, full_wraps
    else:
        assert counts[0] >= 40 and counts[1] >= 150 and counts[2] >= 12, counts
        assert int((info["m"] == 64).sum()) >= 12
        if head == 35:
            assert full_wraps >= 12, full_wraps


def assert_outputs(got, ref, what, keys=None):
    for k in (keys or got):
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert_same_bits(got[k], np.ascontiguousarray(ref[k]).astype(got[k].dtype, copy=False), "%s %s" % (what, k))


def assert_first_step_is_the_plain_gather(got, plain, what):
    """with L = 1: obs[:, 0], obs[:, 1], action[:, 0], reward[:, 0], done[:, 0] are the five outputs of the plain launch"""
    pairs = (("obs", got["obs"][:, 0]), ("next_obs", got["obs"][:, 1]), ("action", got["action"][:, 0]), ("reward", got["reward"][:, 0]),
             ("done", got["done"][:, 0]))
    for k, v in pairs:
        assert_same_bits(np.ascontiguousarray(v), plain[k], "%s: L == 1 against the plain gather, %s" % (what, k))


# ------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("D,A", DIMS)
@pytest.mark.parametrize("T,B", SHAPES)
def test_gather_seq_equals_the_oracle(T, B, D, A):
    rng = np.random.default_rng(T * 7 + B + D)
    bufs = window_buffers(rng, T, B, D, A, 0.15, np.int32 if A == 1 else np.float32)
    idx = some_ids(rng, T * B, cap=200 if D > 100 else 600)
    for L in SEQ_LENS:
        for head in heads_of(T):
            ref, info = oracle.gather_seq(bufs, idx, head, L)
            assert info["bad"] == 0 and info["m"].min() >= 1 and info["m"].max() <= min(L, T)
            for scalar in (False, True):
                rc, got, bad = host.sample(bufs, len(idx), head, L, index=idx, force_scalar=scalar)
                assert rc == 0 and bad == 0 and "index" not in got
                assert_outputs(got, ref, "T=%d B=%d D=%d L=%d head=%d scalar=%d" % (T, B, D, L, head, scalar))
            if L == 1:                               # the plain launch, bit for bit, whatever the head
                rc, plain, _ = rb_host.sample(bufs, len(idx), index=idx)
                assert_first_step_is_the_plain_gather(got, plain, "head=%d" % head)
                assert (got["length"] == 1).all() and (got["mask"] == 1).all()


@pytest.mark.parametrize("case", [ENDINGS, LONGEST], ids=["endings", "longest"])
def test_every_ending_of_a_window(case):
    T, B, D, A = case["T"], case["B"], 11, 3
    bufs = window_buffers(np.random.default_rng(case["seed"]), T, B, D, A, case["p_done"])
    idx = window_ids(T, B)
    for L in case["n_steps"]:
        for head in case["heads"]:
            ref, info = oracle.gather_seq(bufs, idx, head, L)
            assert_every_ending(case, head, L, info, bufs)
            rc, got, bad = host.sample(bufs, len(idx), head, L, index=idx)
            assert rc == 0 and bad == 0
            assert_outputs(got, ref, "T=%d L=%d head=%d" % (T, L, head))
            assert np.array_equal(got["length"], info["m"].astype(np.int32))
            assert np.array_equal(got["mask"].sum(1), info["m"])


def test_a_ring_shorter_than_the_window():
    """T < L: every window ends by episode or head, with m <= T"""
    T, B, D, A, L = 3, 63, 11, 3, 5
    bufs = window_buffers(np.random.default_rng(8), T, B, D, A, 0.15)
    idx = np.arange(T * B, dtype=np.int64)
    for head in heads_of(T):
        ref, info = oracle.gather_seq(bufs, idx, head, L)
        assert info["m"].max() == T and not (info["ending"] == oracle.END_FULL).any()
        assert (info["ending"] == oracle.END_EPISODE).sum() > 20 and (info["ending"] == oracle.END_HEAD).sum() > 20
        assert info["wrapped"].sum() > 20 or head == T - 1
        for scalar in (False, True):
            rc, got, bad = host.sample(bufs, len(idx), head, L, index=idx, force_scalar=scalar)
            assert rc == 0 and bad == 0
            assert_outputs(got, ref, "T < L, head=%d" % head)
            assert not got["obs"][:, T + 1:].any() and not got["mask"][:, T:].any()


# ------------------------------------------------------------------------------------------------- sample
@pytest.mark.parametrize("T,B,D,A", [(3, 63, 11, 3), (5, 64, 4, 1), (3, 63, 376, 17), (4, 4097, 11, 3)])
def test_sample_seq_draws_the_ids_of_sample(T, B, D, A):
    rng = np.random.default_rng(B + D)
    bufs = window_buffers(rng, T, B, D, A, 0.15)
    for size, head, n, seed, draw in ((T, T // 2, 257, 3, 0), (T, T - 1, 64, 3, 1), (1, 0, 9, 2 ** 40 + 1, 2 ** 32)):
        n = min(n, 64) if D > 100 else n
        ref, _ = oracle.sample_seq(bufs, size, head, n, seed, draw, 3)
        assert np.array_equal(ref["index"], rb_oracle.sample_ids(seed, draw, size, B, n))
        rc, got, bad = host.sample(bufs, n, head, 3, size=size, seed=seed, draw=draw)
        assert rc == 0 and bad == 0
        assert np.array_equal(got["index"], ref["index"]) and got["index"].max() < size * B
        assert_outputs(got, ref, "size=%d n=%d" % (size, n))
        rc, plain, _ = rb_host.sample(bufs, n, size=size, seed=seed, draw=draw)
        assert np.array_equal(got["index"], plain["index"])          # the ids of the plain sample launch


def test_no_window_reads_past_the_head_of_a_ring_that_is_not_full():
    T, B, D, A, size = 9, 63, 11, 3, 4
    bufs = window_buffers(np.random.default_rng(9), T, B, D, A, 0.05)
    for k in ("obs", "next_obs", "reward"):          # whatever a window took from the empty slots would show
        bufs[k][size:] = np.nan
    bufs["action"][size:] = np.nan
    bufs["done"][size:] = 255
    bufs["timeout"][size:] = 255
    for L in (3, 5, 64):
        ref, info = oracle.sample_seq(bufs, size, size - 1, 500, 1, 0, L)
        rc, got, bad = host.sample(bufs, 500, size - 1, L, size=size, seed=1, draw=0)
        assert rc == 0 and bad == 0
        assert_outputs(got, ref, "size < T, L=%d" % L)
        assert info["steps"].max() < size * B and (info["ending"] == oracle.END_HEAD).sum() > 50
        for k in SEQ:
            assert np.isfinite(got[k]).all(), k
        assert (got["done"] == ref["done"]).all() and got["length"].max() <= size


def test_out_of_range_ids_give_zeros_and_are_counted():
    T, B, D, A = 3, 63, 11, 3
    rng = np.random.default_rng(1)
    bufs = window_buffers(rng, T, B, D, A, 0.15)
    idx = np.array([5, -1, T * B, 2 ** 62, T * B - 1, -2 ** 63, 17, 0, 188], np.int64)
    for norm in (None, random_norm(rng, D)):
        ref, info = oracle.gather_seq(bufs, idx, 1, 3, norm)
        rc, got, bad = host.sample(bufs, len(idx), 1, 3, index=idx, norm=norm)
        assert rc == 0 and bad == info["bad"] == 4
        for k in SEQ:
            assert not got[k][[1, 2, 3, 5]].any(), k
            assert not np.isnan(got[k]).any(), k     # the padding too is written
        assert (got["length"][[0, 4, 6, 7, 8]] >= 1).all()
        if norm is None:
            assert_outputs(got, ref, "out of range")


def test_optional_outputs_are_skipped():
    T, B, D, A = 3, 63, 11, 3
    rng = np.random.default_rng(2)
    bufs = window_buffers(rng, T, B, D, A, 0.15)
    idx = rng.integers(0, T * B, size=20)
    ref, _ = oracle.gather_seq(bufs, idx, 2, 3)
    for want in (("obs",), ("action", "done"), ("action", "reward"), ("reward",), ("mask",), ("length", "obs"), ()):
        rc, got, _ = host.sample(bufs, len(idx), 2, 3, index=idx, want=want)
        assert rc == 0 and set(got) == set(want)
        assert_outputs(got, ref, str(want))


def test_refused_arguments():
    T, B, D, A = 4, 64, 11, 3
    bufs = window_buffers(np.random.default_rng(3), T, B, D, A, 0.1)
    idx = np.arange(8, dtype=np.int64)
    ok = lambda **kw: host.sample(bufs, 8, **{**dict(head=1, seq_len=3, index=idx), **kw})[0]
    assert ok() == 0 and ok(seq_len=1) == 0 and ok(seq_len=64) == 0 and ok(head=0) == 0 and ok(head=T - 1) == 0
    assert ok(seq_len=0) == -1 and ok(seq_len=65) == -1 and ok(seq_len=-1) == -1
    assert ok(head=-1) == -1 and ok(head=T) == -1
    drawn = lambda size, head: host.sample(bufs, 8, head, 3, size=size)[0]
    assert drawn(T, 0) == 0 and drawn(T, T - 1) == 0 and drawn(2, 1) == 0 and drawn(1, 0) == 0
    assert drawn(0, 0) == -1 and drawn(T + 1, 0) == -1 and drawn(2, 0) == -1 and drawn(2, 2) == -1


# ------------------------------------------------------------------------------------------------- normalised
@pytest.mark.parametrize("norm_obs,norm_reward", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("T,B,D,A", [(3, 63, 11, 3), (5, 64, 4, 1), (3, 63, 376, 17), (2, 5, 600, 2)])
def test_normalised_outputs_within_one_ulp(T, B, D, A, norm_obs, norm_reward):
    """(2, 5, 600, 2): three passes of the statistics, the last one ragged"""
    rng = np.random.default_rng(D + norm_obs * 2 + norm_reward)
    bufs = window_buffers(rng, T, B, D, A, 0.15)
    norm = random_norm(rng, D, norm_obs, norm_reward)
    idx = rng.permutation(T * B)[:100]
    for L in (1, 3):
        ref, info = oracle.gather_seq(bufs, idx, T // 2, L, norm)
        raw, _ = oracle.gather_seq(bufs, idx, T // 2, L)
        results = []
        for scalar in (False, True):
            rc, got, bad = host.sample(bufs, len(idx), T // 2, L, index=idx, norm=norm, force_scalar=scalar)
            assert rc == 0 and bad == 0
            for k, clip, on in (("obs", norm["clip_obs"], norm_obs), ("reward", norm["clip_reward"], norm_reward)):
                if on:
                    assert_f32_within_one_ulp(got[k], ref[k], clip, k)
                else:
                    assert_same_bits(got[k], ref[k], k + " stays raw")
            written = np.arange(L + 1)[None, :] <= info["m"][:, None]
            assert not got["obs"][~written].any() and not got["reward"][got["mask"] == 0].any()      # the padding stays zero
            assert_outputs(got, raw, "never normalised", keys=("action", "done", "mask", "length"))
            results.append(got)
        assert_outputs(results[1], results[0], "16-byte and 4-byte paths")
        # ---- a normalised row of a window is the normalised row the plain gather returns for that step's id, bit for bit
        got = results[0]
        for k in range(L):
            on = info["m"] > k
            rc, plain, _ = rb_host.sample(bufs, int(on.sum()), index=info["steps"][on, k], norm=norm)
            assert_same_bits(np.ascontiguousarray(got["obs"][on, k]), plain["obs"], "row %d against the plain normalised gather" % k)
            assert_same_bits(np.ascontiguousarray(got["reward"][on, k]), plain["reward"], "reward %d" % k)
            last = info["m"] == k + 1
            assert_same_bits(np.ascontiguousarray(got["obs"][last, k + 1]), plain["next_obs"][last[on]], "the row to bootstrap from")


# ------------------------------------------------------------------------------------------------- sanitizers, surface
def test_host_functions_stay_inside_exactly_sized_buffers_under_sanitizers(tmp_path):
    """tests/host_harness/seq_sanitize_main.cpp: a program of its own (the sanitizer runtimes are linked into it; nothing is preloaded)"""
    exe = str(tmp_path / "seq_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(HARNESS, "seq_sanitize_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "T=4 B=4097 D=376 A=17" in run.stdout and "bad=3" in run.stdout


def test_package_and_abi_declare_the_seq_calls():
    import random_envs_amd as rex
    from random_envs_amd import _native
    for name in ("rex_rbuf_gather_seq", "rex_rbuf_sample_seq", "rex_per_sample_seq"):
        assert name in _native.SYMBOLS
    header = open(os.path.join(ROOT, "include", "rex.h")).read()
    for name in ("rex_rbuf_gather_seq(", "rex_rbuf_sample_seq(", "rex_per_sample_seq("):
        assert name in header
    for cls, names in ((rex.ReplayBuffer, ("sample_seq", "gather_seq")), (rex.PrioritizedReplayBuffer, ("sample_seq",))):
        for name in names:
            assert callable(getattr(cls, name))
