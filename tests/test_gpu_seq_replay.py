"""Sequence windows from the replay buffer on the device (rex_rbuf_gather_seq, rex_rbuf_sample_seq, rex_per_sample_seq through
ReplayBuffer / PrioritizedReplayBuffer) against the numpy oracle of tests/seq_replay_oracle.py, under the criteria
test_seq_replay_host.py states and shares: every field to IDENTICAL BITS, normalised values within 1 fp32 ulp.  The stored tensors are
written directly (the add launch has its own tests), ``pos`` / ``full`` place the head.  The Python layer allocates with ``torch.empty``, so
the padding compared here is what the launch wrote.  The end-to-end run feeds the oracle the RAW device outputs of every step, so the
physics plays no part."""
import ctypes
import itertools

import numpy as np
import pytest

import replay_buffer_oracle as rb_oracle
import seq_replay_oracle as oracle
from test_gpu_replay_buffer import SEED, _dev, _make, _np
from test_nstep_replay_host import ENDINGS, heads_of, some_ids, window_buffers, window_ids
from test_replay_buffer_host import FIELDS, SHAPES, random_norm
from test_rollout_host import assert_same_bits
from test_seq_replay_host import LONGEST, SEQ, SEQ_LENS, assert_every_ending
from test_vecnorm_host import assert_f32_within_one_ulp

pytestmark = pytest.mark.gpu

PLAIN = ("obs", "next_obs", "action", "reward", "done")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _p(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def _load(torch, buf, bufs, head, size=None):
    """the numpy buffers into the ReplayBuffer's tensors; a full ring whose newest slot is ``head``, or ``size`` slots filled from slot 0"""
    for k in FIELDS:
        getattr(buf, k).copy_(torch.as_tensor(bufs[k]))
    if size is None:
        buf.pos, buf.full = (head + 1) % buf.n_slots, True
    else:
        assert head == size - 1 and size < buf.n_slots
        buf.pos, buf.full = size, False
    assert buf._head() == head


def _assert_outputs(got, ref, what, keys=SEQ):
    for k in keys:
        g = _np(got[k])
        assert g.shape == ref[k].shape, (what, k, g.shape, ref[k].shape)
        assert_same_bits(g, np.ascontiguousarray(ref[k]).astype(g.dtype, copy=False), "%s %s" % (what, k))


def _buffer(torch, env_id, T, B, p_done, seed, buf_seed=11, cls="ReplayBuffer", wrap=None):
    import random_envs_amd as rex
    env = _make(env_id, B)
    top = wrap(rex, env) if wrap else env
    D, A = env.dims.obs_dim, env.dims.act_dim
    buf = getattr(rex, cls)(top, T, seed=buf_seed)
    bufs = window_buffers(np.random.default_rng(seed), T, B, D, A, p_done, np.int32 if env.dims.discrete_action else np.float32)
    return env, buf, bufs


def _first_step(out):
    """what the five outputs of the plain launch are called in a window of one step"""
    return dict(obs=out["obs"][:, 0], next_obs=out["obs"][:, 1], action=out["action"][:, 0], reward=out["reward"][:, 0], done=out["done"][:, 0])


def _same_bits(torch, a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------- ragged tiles, unaligned and wide rows
CASES = [("RandomHopper-v0", T, B) for T, B in SHAPES] + [("RandomCartPole-v0", T, B) for T, B in SHAPES] + [("RandomHumanoid-v0", 3, 63)]


@pytest.mark.parametrize("env_id,T,B", CASES)
def test_gather_and_sample_seq_equal_the_oracle(torch_mod, env_id, T, B):
    torch = torch_mod
    env, buf, bufs = _buffer(torch, env_id, T, B, 0.15, T * 100 + B)
    with pytest.raises(RuntimeError):
        buf.sample_seq(4, 3)                         # empty, as sample
    rng = np.random.default_rng(B)
    idx = some_ids(rng, T * B)
    d_idx = _dev(torch, env, idx)
    for head in heads_of(T):
        _load(torch, buf, bufs, head)
        for L in SEQ_LENS:
            ref, info = oracle.gather_seq(bufs, idx, head, L)
            out = buf.gather_seq(d_idx, L)
            _assert_outputs(out, ref, "%s T=%d B=%d L=%d head=%d" % (env_id, T, B, L, head))
            assert out["index"] is d_idx and out["length"].dtype == torch.int32 and out["action"].dtype == buf.action.dtype
            assert tuple(out["obs"].shape) == (len(idx), L + 1, buf.obs_dim) and tuple(out["action"].shape) == (len(idx), L, buf.act_dim)
            if L == 1:                               # the plain launch, bit for bit, whatever the head
                plain, first = buf.gather(d_idx), _first_step(out)
                for k in PLAIN:
                    assert _same_bits(torch, first[k], plain[k]), k
                assert (_np(out["length"]) == 1).all() and (_np(out["mask"]) == 1).all()
        # ---- sample_seq: the ids sample would draw at this draw number, and the draw after it is sample's next
        draw = buf.draws
        out = buf.sample_seq(300, 3)
        ref, _ = oracle.sample_seq(bufs, T, head, 300, 11, draw, 3)
        assert np.array_equal(_np(out["index"]), rb_oracle.sample_ids(11, draw, T, B, 300)) and buf.draws == draw + 1
        _assert_outputs(out, ref, "sample_seq head=%d" % head)
        nxt = buf.sample(300)
        assert np.array_equal(_np(nxt["index"]), rb_oracle.sample_ids(11, draw + 1, T, B, 300)) and buf.draws == draw + 2
    assert buf.bad_indices() == 0
    env.close()


# ------------------------------------------------------------------------------------------------- every ending, the longest window
@pytest.mark.parametrize("case", [ENDINGS, LONGEST], ids=["endings", "longest"])
def test_every_ending_of_a_window(torch_mod, case):
    torch = torch_mod
    T, B = case["T"], case["B"]
    env, buf, bufs = _buffer(torch, "RandomHopper-v0", T, B, case["p_done"], case["seed"])
    idx = window_ids(T, B)
    d_idx = _dev(torch, env, idx)
    for L in case["n_steps"]:
        for head in case["heads"]:
            ref, info = oracle.gather_seq(bufs, idx, head, L)
            assert_every_ending(case, head, L, info, bufs)
            _load(torch, buf, bufs, head)
            out = buf.gather_seq(d_idx, L)
            _assert_outputs(out, ref, "T=%d L=%d head=%d" % (T, L, head))
            assert np.array_equal(_np(out["length"]), info["m"].astype(np.int32))
    env.close()


def test_a_ring_shorter_than_the_window(torch_mod):
    torch = torch_mod
    T, B, L = 3, 63, 5
    env, buf, bufs = _buffer(torch, "RandomHopper-v0", T, B, 0.15, 8)
    idx = np.arange(T * B, dtype=np.int64)
    for head in heads_of(T):
        ref, info = oracle.gather_seq(bufs, idx, head, L)
        assert info["m"].max() == T and not (info["ending"] == oracle.END_FULL).any()
        _load(torch, buf, bufs, head)
        _assert_outputs(buf.gather_seq(_dev(torch, env, idx), L), ref, "T < L, head=%d" % head)
    env.close()


def test_no_window_reads_past_the_head_of_a_ring_that_is_not_full(torch_mod):
    torch = torch_mod
    T, B, size = 9, 63, 4
    env, buf, bufs = _buffer(torch, "RandomHopper-v0", T, B, 0.05, 9, buf_seed=1)
    for k in ("obs", "next_obs", "action", "reward"):    # whatever a window took from the empty slots would show
        bufs[k][size:] = np.nan
    bufs["done"][size:] = 255
    bufs["timeout"][size:] = 255
    _load(torch, buf, bufs, size - 1, size=size)
    for L in (3, 5, 64):
        draw = buf.draws
        ref, info = oracle.sample_seq(bufs, size, size - 1, 500, 1, draw, L)
        out = buf.sample_seq(500, L)
        assert np.array_equal(_np(out["index"]), ref["index"]) and int(out["index"].max()) < size * B
        _assert_outputs(out, ref, "size < T, L=%d" % L)
        assert info["steps"].max() < size * B and (info["ending"] == oracle.END_HEAD).sum() > 50
        for k in SEQ:
            assert np.isfinite(_np(out[k])).all(), k
    env.close()


def test_out_of_range_ids_give_zeros_and_are_counted(torch_mod):
    torch = torch_mod
    T, B = 3, 63
    env, buf, bufs = _buffer(torch, "RandomHopper-v0", T, B, 0.15, 1)
    _load(torch, buf, bufs, 1)
    rng = np.random.default_rng(2)
    idx = np.concatenate([rng.integers(0, T * B, size=30), [-1, T * B], rng.integers(0, T * B, size=30)]).astype(np.int64)
    ref, info = oracle.gather_seq(bufs, idx, 1, 3)
    out = buf.gather_seq(_dev(torch, env, idx), 3)
    _assert_outputs(out, ref, "ids out of range")
    for k in SEQ:
        assert not _np(out[k])[30:32].any(), k
    assert info["bad"] == 2 and buf.bad_indices() == 2 and buf.bad_indices() == 0
    env.close()


# ------------------------------------------------------------------------------------------------- the C-ABI: errors, optional outputs
def test_abi_error_paths_and_optional_outputs(torch_mod):
    torch = torch_mod
    from random_envs_amd import _native
    T, B, n, L0 = 4, 64, 8, 3
    env = _make("RandomHopper-v0", B)
    L, h, s = env._L, env._h, env._stream
    bufs = window_buffers(np.random.default_rng(3), T, B, 11, 3, 0.1)
    t = {k: _dev(torch, env, bufs[k]) for k in FIELDS}
    desc = _native.RexRbufBuffers(*[t[k].data_ptr() for k in FIELDS], T)
    pr, mx = torch.zeros(T * B, device=env.device), torch.ones(1, device=env.device)
    tree = torch.zeros(int(L.rex_per_tree_len(T * B)), dtype=torch.float64, device=env.device)
    per = _native.RexPerBuffers(pr.data_ptr(), tree.data_ptr(), mx.data_ptr(), T)
    f32 = dict(dtype=torch.float32, device=env.device)
    # room for the longest window, so that every accepted seq_len writes inside these
    o = dict(obs=torch.zeros(n, 65, 11, **f32), action=torch.zeros(n, 64, 3, **f32), reward=torch.zeros(n, 64, **f32), done=torch.zeros(n, 64, **f32),
             mask=torch.zeros(n, 64, **f32), length=torch.zeros(n, dtype=torch.int32, device=env.device))
    idx = _dev(torch, env, np.arange(n, dtype=np.int64) * 9)
    o_idx, o_prob = torch.zeros(n, dtype=torch.int64, device=env.device), torch.zeros(n, **f32)
    outs = lambda want: [_p(o[k]) if k in want else None for k in SEQ]

    def gather(head=1, seq_len=L0, normalise=0, want=SEQ, count=n):
        return L.rex_rbuf_gather_seq(h, ctypes.byref(desc), _p(idx), count, head, seq_len, normalise, *outs(want), s())

    def sample(size=T, head=1, seq_len=L0, normalise=0, count=n):
        return L.rex_rbuf_sample_seq(h, ctypes.byref(desc), size, head, count, 1, 0, seq_len, normalise, *outs(SEQ), _p(o_idx), s())

    def per_sample(head=1, seq_len=L0, normalise=0, count=n):
        return L.rex_per_sample_seq(h, ctypes.byref(desc), ctypes.byref(per), count, head, 1, 0, seq_len, normalise, *outs(SEQ), _p(o_idx), _p(o_prob), s())

    for c in (gather, sample, per_sample):
        assert c() == -3 and c(seq_len=0) == -3      # REX_ERR_STATE before rex_rbuf_enable, and before any argument is looked at
    assert "_enable" in L.rex_last_error().decode()
    assert L.rex_rbuf_enable(h) == 0
    assert gather() == 0 and sample() == 0 and per_sample() == -3 and "rex_per_enable" in L.rex_last_error().decode()
    assert L.rex_per_enable(h) == 0 and L.rex_per_init(h, ctypes.byref(per), s()) == 0 and per_sample() == 0
    for c in (gather, sample, per_sample):           # REX_ERR_ARG
        assert c(seq_len=0) == -1 and c(seq_len=65) == -1 and c(seq_len=-1) == -1 and c(seq_len=1) == 0 and c(seq_len=64) == 0
        assert c(head=-1) == -1 and c(head=T) == -1 and c(head=0) == 0 and c(head=T - 1) == 0
        assert c(count=-1) == -1 and c(count=0) == 0
        assert c(normalise=1) == -3 and "rex_norm_enable" in L.rex_last_error().decode()
    assert sample(size=0) == -1 and sample(size=T + 1) == -1 and sample(size=2, head=0) == -1 and sample(size=2, head=2) == -1
    assert sample(size=2, head=1) == 0 and sample(size=1, head=0) == 0 and sample(size=T, head=0) == 0
    assert L.rex_rbuf_gather_seq(h, None, _p(idx), n, 1, L0, 0, *outs(SEQ), s()) == -1      # a NULL struct pointer
    assert L.rex_rbuf_gather_seq(h, ctypes.byref(desc), None, n, 1, L0, 0, *outs(SEQ), s()) == -1
    assert L.rex_norm_enable(h, None) == 0
    assert gather(normalise=1) == 0 and sample(normalise=1) == 0 and per_sample(normalise=1) == 0
    # ---- optional outputs left out, EVERY subset: the others are written, the skipped ones keep their content
    ref, _ = oracle.gather_seq(bufs, _np(idx), 1, L0)
    shape = dict(obs=(n, L0 + 1, 11), action=(n, L0, 3), reward=(n, L0), done=(n, L0), mask=(n, L0), length=(n,))
    o = {k: torch.zeros(*shape[k], dtype=o[k].dtype, device=env.device) for k in SEQ}
    for r in range(len(SEQ) + 1):
        for want in itertools.combinations(SEQ, r):
            for k in SEQ:
                o[k].fill_(-7)
            assert gather(want=want) == 0
            for k in SEQ:
                if k in want:
                    _assert_outputs(o, ref, str(want), keys=(k,))
                else:
                    assert (_np(o[k]) == -7).all(), (want, k)
    torch.cuda.synchronize()
    env.close()


# ------------------------------------------------------------------------------------------------- normalised
def _normalised(norm):
    def wrap(rex, env):
        w = rex.NormalizedVecRandomEnv(env, norm_obs=norm["norm_obs"], norm_reward=norm["norm_reward"])
        w.reset()
        w.set_training(False)
        R = len(norm["mean"])
        w.load_stats(dict(count=np.full(R, 100.0), mean=norm["mean"], var=norm["var"]))
        assert (w.epsilon, w.clip_obs, w.clip_reward) == (norm["epsilon"], norm["clip_obs"], norm["clip_reward"])
        return w
    return wrap


@pytest.mark.parametrize("norm_obs,norm_reward", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("env_id", ["RandomHopper-v0", "RandomHumanoid-v0"])
def test_normalised_outputs_within_one_ulp(torch_mod, env_id, norm_obs, norm_reward):
    torch = torch_mod
    T, B = 3, 63
    D = 11 if "Hopper" in env_id else 376
    norm = random_norm(np.random.default_rng(D + norm_obs * 2 + norm_reward), D, norm_obs, norm_reward)
    env, buf, bufs = _buffer(torch, env_id, T, B, 0.15, 4, wrap=_normalised(norm))
    assert env.dims.obs_dim == D
    _load(torch, buf, bufs, 1)
    idx = np.random.default_rng(1).permutation(T * B).astype(np.int64)
    d_idx = _dev(torch, env, idx)
    for L in (1, 3):
        ref, info = oracle.gather_seq(bufs, idx, 1, L, norm)
        raw, _ = oracle.gather_seq(bufs, idx, 1, L)
        out = buf.gather_seq(d_idx, L)               # normalize=None: yes, the env is a NormalizedVecRandomEnv
        for k, clip, on in (("obs", norm["clip_obs"], norm_obs), ("reward", norm["clip_reward"], norm_reward)):
            if on:
                assert_f32_within_one_ulp(_np(out[k]), ref[k], clip, k)
            else:
                _assert_outputs(out, raw, "stays raw", keys=(k,))
        written = np.arange(L + 1)[None, :] <= info["m"][:, None]
        assert not _np(out["obs"])[~written].any() and not _np(out["reward"])[_np(out["mask"]) == 0].any()      # the padding stays zero
        _assert_outputs(out, raw, "never normalised", keys=("action", "done", "mask", "length"))
        _assert_outputs(buf.gather_seq(d_idx, L, normalize=False), raw, "normalize=False")
        # ---- valid rows k of obs are the rows buf.gather returns for the ids s_k, bit for bit; row m is its next_obs row
        for k in range(L):
            on = info["m"] > k
            plain = buf.gather(_dev(torch, env, info["steps"][on, k]))
            sel = torch.as_tensor(on, device=env.device)
            assert _same_bits(torch, out["obs"][sel, k], plain["obs"]), k
            assert _same_bits(torch, out["reward"][sel, k], plain["reward"]), k
            last = torch.as_tensor(info["m"] == k + 1, device=env.device)
            assert _same_bits(torch, out["obs"][last, k + 1], plain["next_obs"][last[sel]]), k
    s = buf.sample_seq(200, 3)                       # the sample path normalises the same way
    g = buf.gather_seq(s["index"], 3)
    for k in SEQ:
        assert _same_bits(torch, s[k], g[k]), k
    env.close()


# ------------------------------------------------------------------------------------------------- prioritised
def test_prioritised_sample_seq_is_the_draw_of_sample_and_the_seq_gather(torch_mod):
    torch = torch_mod
    T, B = 9, 63
    env, buf, bufs = _buffer(torch, "RandomHopper-v0", T, B, 0.15, 6, buf_seed=21, cls="PrioritizedReplayBuffer")
    with pytest.raises(RuntimeError):
        buf.sample_seq(4, 3)
    _load(torch, buf, bufs, 4)
    rng = np.random.default_rng(5)
    every = torch.arange(T * B, device=env.device)
    buf.update_priorities(every, _dev(torch, env, (rng.normal(size=T * B) * 3).astype(np.float32)))
    for n in (1, 9, 300):
        draw = buf.draws
        out = buf.sample_seq(n, 5, beta=0.5)
        assert buf.draws == draw + 1
        buf.draws = draw
        same = buf.sample(n, beta=0.5)               # the same draw number: the same ids, probabilities and weights
        assert torch.equal(out["index"], same["index"]) and int(out["index"].min()) >= 0
        for k in ("prob", "weight"):
            assert _same_bits(torch, out[k], same[k]), k
        g = buf.gather_seq(out["index"], 5)
        for k in SEQ:
            assert _same_bits(torch, out[k], g[k]), k
        ref, _ = oracle.gather_seq(bufs, _np(out["index"]), 4, 5)
        _assert_outputs(out, ref, "prioritised n=%d" % n)
    assert buf.bad_indices() == 0
    # ---- nothing to draw: ids of -1 meet the guard
    L, h = env._L, env._h
    zeros = torch.zeros(T * B, device=env.device)
    assert L.rex_per_update(h, ctypes.byref(buf._per), _p(every), _p(zeros), T * B, env._stream()) == 0
    out = buf.sample_seq(5, 5)
    assert (_np(out["index"]) == -1).all() and not _np(out["prob"]).any() and not _np(out["weight"]).any()
    for k in SEQ:
        assert not _np(out[k]).any(), k
    assert buf.bad_indices() == 5
    env.close()


# ------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_hopper_collect_wrap_and_gather_seq(torch_mod):
    """the seed, the actions and the time-limit lanes of test_gpu_nstep_replay.py's end-to-end run: 9 steps into a ring of 6, so it wraps
    and the head is slot 2"""
    torch = torch_mod
    import random_envs_amd as rex
    steps, B, T = 9, 4097, 6
    env = _make("RandomHopper-v0", B, dr=True, autoreset=True)
    env.reset()
    st = env.get_full_state()
    st["t"][::3] = 494                                # every third lane meets the time limit (500) at step 5: slot 5, which the wrap leaves
    env.set_full_state(st)
    buf = rex.ReplayBuffer(env, T)
    D, A = env.dims.obs_dim, env.dims.act_dim
    gen = torch.Generator().manual_seed(SEED)
    ref = rb_oracle.empty_buffers(T, B, D, A)
    for t in range(steps):
        prev_obs = env._obs.clone()
        a_soa = (torch.rand(B, 3, generator=gen) * 2 - 1).t().contiguous().to(env.device)
        obs, reward, done, trunc, term = env.step_soa_full(a_soa)
        buf.add(prev_obs, a_soa, reward, done, obs, term, trunc)
        rb_oracle.add(ref, t % T, _np(prev_obs), _np(a_soa), _np(reward), _np(done), _np(obs), _np(term), _np(trunc))
    assert buf.full and buf.pos == 3 and buf._head() == 2
    for k in FIELDS:
        assert_same_bits(_np(getattr(buf, k)), ref[k], k + " stored")
    idx = np.arange(T * B, dtype=np.int64)
    wanted, info = oracle.gather_seq(ref, idx, 2, 3)
    counts = [int((info["ending"] == e).sum()) for e in (oracle.END_EPISODE, oracle.END_HEAD, oracle.END_FULL)]
    print("end to end: endings (episode, head, full) %s, %d wraps, %d timeouts stored" % (counts, info["wrapped"].sum(), (ref["timeout"] != 0).sum()))
    assert min(counts) > 0 and info["wrapped"].any() and (ref["timeout"] != 0).any() and ((ref["done"] != 0) & (ref["timeout"] == 0)).any()   # not vacuous
    out = buf.gather_seq(_dev(torch, env, idx), 3, normalize=False)
    _assert_outputs(out, wanted, "all ids, L = 3")
    env.close()
