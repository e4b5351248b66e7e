"""N-step returns from the replay buffer on the device (rex_rbuf_gather_nstep, rex_rbuf_sample_nstep, rex_per_sample_nstep through
ReplayBuffer / PrioritizedReplayBuffer) against the numpy float64 oracle of tests/nstep_replay_oracle.py, under the criteria
test_nstep_replay_host.py states and shares: every field to IDENTICAL BITS, normalised values within 1 fp32 ulp.  The stored tensors are
written directly (the add launch has its own tests), ``pos`` / ``full`` place the head.  The end-to-end run feeds the oracle the RAW device
outputs of every step, so the physics plays no part."""
import ctypes

import numpy as np
import pytest

import nstep_replay_oracle as oracle
import replay_buffer_oracle as rb_oracle
from test_gpu_replay_buffer import SEED, _dev, _make, _np
from test_nstep_replay_host import (ENDINGS, LONGEST, N_STEPS, PLAIN, assert_every_ending, heads_of, some_ids, window_buffers, window_ids)
from test_replay_buffer_host import FIELDS, SHAPES, random_norm
from test_rollout_host import assert_same_bits
from test_vecnorm_host import assert_f32_within_one_ulp

pytestmark = pytest.mark.gpu

NSTEP = PLAIN + ("discount", "steps")


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


def _assert_outputs(got, ref, what, keys=NSTEP):
    for k in keys:
        g = _np(got[k])
        assert_same_bits(g, np.ascontiguousarray(ref[k]).astype(g.dtype, copy=False), "%s %s" % (what, k))


def _buffer(torch, env_id, T, B, p_done, seed, buf_seed=11, cls="ReplayBuffer", wrap=None):
    import random_envs_amd as rex
    env = _make(env_id, B)
    top = wrap(rex, env) if wrap else env
    D, A = env.dims.obs_dim, env.dims.act_dim
    buf = getattr(rex, cls)(top, T, seed=buf_seed)
    bufs = window_buffers(np.random.default_rng(seed), T, B, D, A, p_done, np.int32 if env.dims.discrete_action else np.float32)
    return env, buf, bufs


# ------------------------------------------------------------------------------------------------- ragged tiles, unaligned and wide rows
CASES = [("RandomHopper-v0", T, B) for T, B in SHAPES] + [("RandomCartPole-v0", T, B) for T, B in SHAPES] + [("RandomHumanoid-v0", 3, 63)]


@pytest.mark.parametrize("env_id,T,B", CASES)
def test_gather_and_sample_nstep_equal_the_oracle(torch_mod, env_id, T, B):
    torch = torch_mod
    env, buf, bufs = _buffer(torch, env_id, T, B, 0.15, T * 100 + B)
    with pytest.raises(RuntimeError):
        buf.sample_nstep(4, 3, 0.99)                 # empty, as sample
    rng = np.random.default_rng(B)
    idx = some_ids(rng, T * B)
    d_idx = _dev(torch, env, idx)
    for head in heads_of(T):
        _load(torch, buf, bufs, head)
        for n_step in N_STEPS:
            ref, info = oracle.gather_nstep(bufs, idx, head, n_step, 0.97)
            out = buf.gather_nstep(d_idx, n_step, 0.97)
            _assert_outputs(out, ref, "%s T=%d B=%d n_step=%d head=%d" % (env_id, T, B, n_step, head))
            assert out["index"] is d_idx and out["steps"].dtype == torch.int32 and out["discount"].dtype == torch.float32
            if n_step == 1:                          # the plain launch, bit for bit, whatever the head
                plain = buf.gather(d_idx)
                for k in PLAIN:
                    assert torch.equal(out[k].view(torch.int32), plain[k].view(torch.int32)), k
                assert (_np(out["steps"]) == 1).all() and (_np(out["discount"]) == np.float32(0.97)).all()
        # ---- sample_nstep: the ids sample would draw at this draw number, and the draw after it is sample's next
        draw = buf.draws
        out = buf.sample_nstep(300, 3, 0.97)
        ref, _ = oracle.sample_nstep(bufs, T, head, 300, 11, draw, 3, 0.97)
        assert np.array_equal(_np(out["index"]), rb_oracle.sample_ids(11, draw, T, B, 300)) and buf.draws == draw + 1
        _assert_outputs(out, ref, "sample_nstep head=%d" % head)
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
    for n_step in case["n_steps"]:
        for head in case["heads"]:
            ref, info = oracle.gather_nstep(bufs, idx, head, n_step, 0.99)
            assert_every_ending(case, head, n_step, info)
            _load(torch, buf, bufs, head)
            out = buf.gather_nstep(d_idx, n_step, 0.99)
            _assert_outputs(out, ref, "T=%d n_step=%d head=%d" % (T, n_step, head))
            assert np.array_equal(_np(out["steps"]), info["m"].astype(np.int32))
    env.close()


@pytest.mark.parametrize("gamma", [0.0, 1.0])
def test_gamma_zero_and_one(torch_mod, gamma):
    torch = torch_mod
    T, B = 9, 63
    env, buf, bufs = _buffer(torch, "RandomHopper-v0", T, B, 0.1, 5)
    idx = np.arange(T * B, dtype=np.int64)
    _load(torch, buf, bufs, 4)
    ref, info = oracle.gather_nstep(bufs, idx, 4, 5, gamma)
    out = buf.gather_nstep(_dev(torch, env, idx), 5, gamma)
    assert info["m"].max() == 5
    _assert_outputs(out, ref, "gamma=%g" % gamma)
    assert (_np(out["discount"]) == np.float32(gamma)).all()
    env.close()


def test_no_window_reads_past_the_head_of_a_ring_that_is_not_full(torch_mod):
    torch = torch_mod
    T, B, size = 9, 63, 4
    env, buf, bufs = _buffer(torch, "RandomHopper-v0", T, B, 0.05, 9, buf_seed=1)
    bufs["reward"][size:] = np.nan                   # whatever a window took from the empty slots would show
    bufs["done"][size:] = 255
    bufs["next_obs"][size:] = np.nan
    _load(torch, buf, bufs, size - 1, size=size)
    for n_step in (3, 5, 32):
        draw = buf.draws
        ref, info = oracle.sample_nstep(bufs, size, size - 1, 500, 1, draw, n_step, 0.9)
        out = buf.sample_nstep(500, n_step, 0.9)
        assert np.array_equal(_np(out["index"]), ref["index"]) and int(out["index"].max()) < size * B
        _assert_outputs(out, ref, "size < T, n_step=%d" % n_step)
        assert info["last"].max() < size * B and (info["ending"] == oracle.END_HEAD).sum() > 50
        assert np.isfinite(_np(out["reward"])).all() and np.isfinite(_np(out["next_obs"])).all()
    env.close()


def test_out_of_range_ids_give_zeros_and_are_counted(torch_mod):
    torch = torch_mod
    T, B = 3, 63
    env, buf, bufs = _buffer(torch, "RandomHopper-v0", T, B, 0.15, 1)
    _load(torch, buf, bufs, 1)
    rng = np.random.default_rng(2)
    idx = np.concatenate([rng.integers(0, T * B, size=30), [-1, T * B], rng.integers(0, T * B, size=30)]).astype(np.int64)
    ref, info = oracle.gather_nstep(bufs, idx, 1, 3, 0.9)
    out = buf.gather_nstep(_dev(torch, env, idx), 3, 0.9)
    _assert_outputs(out, ref, "ids out of range")
    for k in NSTEP:
        assert not _np(out[k])[30:32].any(), k
    assert info["bad"] == 2 and buf.bad_indices() == 2 and buf.bad_indices() == 0
    env.close()


# ------------------------------------------------------------------------------------------------- the C-ABI: errors, optional outputs
def test_abi_error_paths_and_optional_outputs(torch_mod):
    torch = torch_mod
    import random_envs_amd as rex
    from random_envs_amd import _native
    T, B, n = 4, 64, 8
    env = _make("RandomHopper-v0", B)
    L, h, s = env._L, env._h, env._stream
    bufs = window_buffers(np.random.default_rng(3), T, B, 11, 3, 0.1)
    t = {k: _dev(torch, env, bufs[k]) for k in FIELDS}
    desc = _native.RexRbufBuffers(*[t[k].data_ptr() for k in FIELDS], T)
    pr, mx = torch.zeros(T * B, device=env.device), torch.ones(1, device=env.device)
    tree = torch.zeros(int(L.rex_per_tree_len(T * B)), dtype=torch.float64, device=env.device)
    per = _native.RexPerBuffers(pr.data_ptr(), tree.data_ptr(), mx.data_ptr(), T)
    f32 = dict(dtype=torch.float32, device=env.device)
    o = dict(obs=torch.zeros(n, 11, **f32), next_obs=torch.zeros(n, 11, **f32), action=torch.zeros(n, 3, **f32), reward=torch.zeros(n, **f32),
             done=torch.zeros(n, **f32), discount=torch.zeros(n, **f32), steps=torch.zeros(n, dtype=torch.int32, device=env.device))
    idx = _dev(torch, env, np.arange(n, dtype=np.int64) * 9)
    o_idx, o_prob = torch.zeros(n, dtype=torch.int64, device=env.device), torch.zeros(n, **f32)
    outs = lambda want: [_p(o[k]) if k in want else None for k in NSTEP]

    def gather(head=1, n_step=3, gamma=0.9, normalise=0, want=NSTEP, count=n):
        return L.rex_rbuf_gather_nstep(h, ctypes.byref(desc), _p(idx), count, head, n_step, gamma, normalise, *outs(want), s())

    def sample(size=T, head=1, n_step=3, gamma=0.9, normalise=0, count=n):
        return L.rex_rbuf_sample_nstep(h, ctypes.byref(desc), size, head, count, 1, 0, n_step, gamma, normalise, *outs(NSTEP), _p(o_idx), s())

    def per_sample(head=1, n_step=3, gamma=0.9, normalise=0, count=n):
        return L.rex_per_sample_nstep(h, ctypes.byref(desc), ctypes.byref(per), count, head, 1, 0, n_step, gamma, normalise, *outs(NSTEP), _p(o_idx), _p(o_prob), s())

    for c in (gather, sample, per_sample):
        assert c() == -3                              # REX_ERR_STATE before rex_rbuf_enable
    assert "_enable" in L.rex_last_error().decode()
    assert L.rex_rbuf_enable(h) == 0
    assert gather() == 0 and sample() == 0 and per_sample() == -3 and "rex_per_enable" in L.rex_last_error().decode()
    assert L.rex_per_enable(h) == 0 and L.rex_per_init(h, ctypes.byref(per), s()) == 0 and per_sample() == 0
    for c in (gather, sample, per_sample):           # REX_ERR_ARG
        assert c(n_step=0) == -1 and c(n_step=33) == -1 and c(n_step=-1) == -1 and c(n_step=1) == 0 and c(n_step=32) == 0
        assert c(gamma=-1e-9) == -1 and c(gamma=1.0 + 1e-9) == -1 and c(gamma=float("nan")) == -1 and c(gamma=float("inf")) == -1
        assert c(gamma=0.0) == 0 and c(gamma=1.0) == 0
        assert c(head=-1) == -1 and c(head=T) == -1 and c(head=0) == 0 and c(head=T - 1) == 0
        assert c(count=-1) == -1 and c(count=0) == 0
        assert c(normalise=1) == -3 and "rex_norm_enable" in L.rex_last_error().decode()
    assert sample(size=0) == -1 and sample(size=T + 1) == -1 and sample(size=2, head=0) == -1 and sample(size=2, head=2) == -1
    assert sample(size=2, head=1) == 0 and sample(size=1, head=0) == 0 and sample(size=T, head=0) == 0
    assert L.rex_rbuf_gather_nstep(h, None, _p(idx), n, 1, 3, 0.9, 0, *outs(NSTEP), s()) == -1      # a NULL struct pointer
    assert L.rex_rbuf_gather_nstep(h, ctypes.byref(desc), None, n, 1, 3, 0.9, 0, *outs(NSTEP), s()) == -1
    assert L.rex_norm_enable(h, None) == 0
    assert gather(normalise=1) == 0 and sample(normalise=1) == 0 and per_sample(normalise=1) == 0
    # ---- optional outputs left out: the others are written, the skipped ones keep their content
    ref, _ = oracle.gather_nstep(bufs, _np(idx), 1, 3, 0.9)
    for want in (("obs",), ("next_obs", "done"), ("action", "reward"), ("discount",), ("steps", "next_obs"), ()):
        for k in NSTEP:
            o[k].fill_(-7)
        assert gather(want=want) == 0
        for k in NSTEP:
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
    for n_step in (1, 3):
        ref, _ = oracle.gather_nstep(bufs, idx, 1, n_step, 0.95, norm)
        raw, _ = oracle.gather_nstep(bufs, idx, 1, n_step, 0.95)
        out = buf.gather_nstep(d_idx, n_step, 0.95)  # normalize=None: yes, the env is a NormalizedVecRandomEnv
        for k, clip, on in (("obs", norm["clip_obs"], norm_obs), ("next_obs", norm["clip_obs"], norm_obs), ("reward", norm["clip_reward"], norm_reward)):
            if on:
                assert_f32_within_one_ulp(_np(out[k]), ref[k], clip, k)
            else:
                _assert_outputs(out, raw, "stays raw", keys=(k,))
        _assert_outputs(out, raw, "never normalised", keys=("action", "done", "discount", "steps"))
        _assert_outputs(buf.gather_nstep(d_idx, n_step, 0.95, normalize=False), raw, "normalize=False")
        if n_step == 1:                              # the plain normalised gather, bit for bit
            plain = buf.gather(d_idx)
            for k in PLAIN:
                assert torch.equal(out[k].view(torch.int32), plain[k].view(torch.int32)), k
    s = buf.sample_nstep(200, 3, 0.95)               # the sample path normalises the same way
    g = buf.gather_nstep(s["index"], 3, 0.95)
    for k in NSTEP:
        assert torch.equal(s[k].view(torch.int32), g[k].view(torch.int32)), k
    env.close()


# ------------------------------------------------------------------------------------------------- prioritised
def test_prioritised_sample_nstep_is_the_draw_of_sample_and_the_nstep_gather(torch_mod):
    torch = torch_mod
    T, B = 9, 63
    env, buf, bufs = _buffer(torch, "RandomHopper-v0", T, B, 0.15, 6, buf_seed=21, cls="PrioritizedReplayBuffer")
    with pytest.raises(RuntimeError):
        buf.sample_nstep(4, 3, 0.99)
    _load(torch, buf, bufs, 4)
    rng = np.random.default_rng(5)
    every = torch.arange(T * B, device=env.device)
    buf.update_priorities(every, _dev(torch, env, (rng.normal(size=T * B) * 3).astype(np.float32)))
    for n in (1, 9, 300):
        draw = buf.draws
        out = buf.sample_nstep(n, 5, 0.99, beta=0.5)
        assert buf.draws == draw + 1
        buf.draws = draw
        same = buf.sample(n, beta=0.5)               # the same draw number: the same ids, probabilities and weights
        assert torch.equal(out["index"], same["index"]) and int(out["index"].min()) >= 0
        for k in ("prob", "weight"):
            assert torch.equal(out[k].view(torch.int32), same[k].view(torch.int32)), k
        g = buf.gather_nstep(out["index"], 5, 0.99)
        for k in NSTEP:
            assert torch.equal(out[k].view(torch.int32), g[k].view(torch.int32)), k
        ref, _ = oracle.gather_nstep(bufs, _np(out["index"]), 4, 5, 0.99)
        _assert_outputs(out, ref, "prioritised n=%d" % n)
    assert buf.bad_indices() == 0
    # ---- nothing to draw: ids of -1 meet the guard
    L, h = env._L, env._h
    zeros = torch.zeros(T * B, device=env.device)
    assert L.rex_per_update(h, ctypes.byref(buf._per), _p(every), _p(zeros), T * B, env._stream()) == 0
    out = buf.sample_nstep(5, 5, 0.99)
    assert (_np(out["index"]) == -1).all() and not _np(out["prob"]).any() and not _np(out["weight"]).any()
    for k in NSTEP:
        assert not _np(out[k]).any(), k
    assert buf.bad_indices() == 5
    env.close()


# ------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_hopper_collect_wrap_and_gather_nstep(torch_mod):
    """the seed and the actions of test_gpu_replay_buffer.py's end-to-end run, its time-limit lanes three steps later (the ring keeps steps
    3 .. 8 only): 9 steps into a ring of 6, so it wraps and the head is slot 2"""
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
    wanted, info = oracle.gather_nstep(ref, idx, 2, 3, 0.99)
    counts = [int((info["ending"] == e).sum()) for e in (oracle.END_EPISODE, oracle.END_HEAD, oracle.END_FULL)]
    print("end to end: endings (episode, head, n_step) %s, %d wraps, %d timeouts stored" % (counts, info["wrapped"].sum(), (ref["timeout"] != 0).sum()))
    assert min(counts) > 0 and info["wrapped"].any() and (ref["timeout"] != 0).any() and ((ref["done"] != 0) & (ref["timeout"] == 0)).any()   # not vacuous
    out = buf.gather_nstep(_dev(torch, env, idx), 3, 0.99, normalize=False)
    _assert_outputs(out, wanted, "all ids, n_step = 3")
    env.close()
