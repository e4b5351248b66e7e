"""The acting-time history stack on the device (rex_hist_* through HistoryStack) against the shift-based numpy oracle of tests/hist_oracle.py:
every word to IDENTICAL BITS.  The synthetic cases hand the launches arbitrary bit patterns; the end-to-end runs feed the oracle the RAW device
outputs of every step, so the physics plays no part."""
import ctypes

import numpy as np
import pytest

from hist_oracle import HistOracle, bits
from test_gpu_replay_buffer import _dev, _make, _np
from test_history_host import _words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _assert_state(hist, ora, term, what, lanes=None):
    """length, the strided view, its flattening, the mirror and terminal_window against the oracle (the rows of ``lanes`` only when given)"""
    sel = slice(None) if lanes is None else lanes
    assert np.array_equal(_np(hist.length), ora.length), what
    win = hist.window()
    K, W = hist.k, hist.width
    assert tuple(win.shape) == (hist.batch, K, W) and win.stride() == (2 * K * W, W, 1) and win.data_ptr() != hist.frames.data_ptr()
    assert _same(_np(win[sel]), ora.win[sel]), what
    assert _same(_np(hist.terminal_window[sel]), term[sel]), what + ": terminal_window"
    if lanes is None:
        fr = _np(hist.frames)
        assert _same(fr[:, :K], fr[:, K:]), what + ": rows r and r + K differ"
        flat = hist.flat()
        assert tuple(flat.shape) == (hist.batch, K * W) and flat.stride() == (2 * K * W, 1) and flat.data_ptr() == win.data_ptr()
        assert _same(_np(flat), ora.win.reshape(hist.batch, K * W)), what + ": flat"


# ------------------------------------------------------------------------------------------------- synthetic tensors through push_buffers
SYNTH = [("RandomHopper-v0", B, K) for B in (1, 65, 130) for K in (1, 3, 64)] + [("RandomCartPole-v0", 65, 3), ("RandomHumanoid-v0", 130, 3),
                                                                                ("RandomHumanoid-v0", 65, 64)]


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("env_id,B,K", SYNTH)
def test_push_buffers_reset_and_materialize_equal_the_oracle(torch_mod, env_id, B, K, rows):
    """3K + 2 pushes of arbitrary bit patterns (the ring wraps twice; slot 0 and slot K - 1 both meet a done) under seeded p = 0.3 dones, with and
    without action, a full reset before the first push and a masked one in mid-run; frame widths 14, 5, 11 and 393 (seven row groups)"""
    import random_envs_amd as rex
    torch = torch_mod
    env = _make(env_id, B, row_major=rows)
    D, A, disc = env.dims.obs_dim, env.dims.act_dim, bool(env.dims.discrete_action)
    P = 3 * K + 2
    own_obs = env._obs_rows if rows else env._obs
    lay = (lambda x: x) if rows else (lambda x: np.swapaxes(x, -1, -2))     # batch-major -> what the launch is handed
    for with_action in (True, False):
        rng = np.random.default_rng(1000 * K + B + int(with_action))
        obs, tobs, robs = _words(rng, P, B, D), _words(rng, P, B, D), _words(rng, 2, B, D)
        act = rng.integers(0, 2, size=(P, B, 1)).astype(np.int32) if disc else _words(rng, P, B, A)
        done = (rng.random((P, B)) < 0.3).astype(np.uint8)
        done[[K - 1, 2 * K - 2], 0] = 1                                     # (a full reset takes slot 0: push p goes to slot (p + 1) % K)
        mask = (rng.random(B) < 0.5).astype(np.uint8)
        d_obs, d_tobs, d_robs = (_dev(torch, env, lay(x)) for x in (obs, tobs, robs))
        d_done = _dev(torch, env, done)
        d_act = _dev(torch, env, act[:, :, 0] if disc and rows else lay(act))
        hist = rex.HistoryStack(env, K, with_action=with_action)
        ora = HistOracle(B, K, D, A, with_action)
        term = np.zeros((B, K, ora.W), np.float32)
        assert not bits(_np(hist.frames)).any() and not _np(hist.length).any()           # rex_hist_init wrote every word
        own_obs.copy_(d_robs[0]); hist.reset(); ora.reset(None, robs[0])
        _assert_state(hist, ora, term, "full reset")
        met = set()
        for p in range(P):
            with_term = p % 5 != 4
            if done[p].any():
                met.add(hist.count % K)
            hist.push_buffers(d_obs[p], d_act[p] if with_action else None, d_done[p] if p % 7 else d_done[p].bool(), d_tobs[p] if with_term else None,
                              rows=rows)
            ora.push(obs[p], act[p], done[p], tobs[p] if with_term else None, term if with_term else None)
            if K <= 3 or p % 16 == 0 or p == P - 1:
                _assert_state(hist, ora, term, "push %d" % p)
            if p == K + 1:
                own_obs.copy_(d_robs[1]); hist.reset(mask); ora.reset(mask, robs[1])
                _assert_state(hist, ora, term, "masked reset")
        assert {0, K - 1} <= met
        out = hist.materialize()
        assert out.is_contiguous() and _same(_np(out), ora.win)
        mine = torch.full((B, K, ora.W), float("nan"), device=env.device)
        assert hist.materialize(mine) is mine and _same(_np(mine), ora.win)
        assert np.array_equal(_np(hist.mask()), ora.mask())
    env.close()


def test_a_null_done_pushes_every_lane(torch_mod):
    import random_envs_amd as rex
    torch = torch_mod
    env = _make("RandomHopper-v0", 65)
    hist, ora = rex.HistoryStack(env, 3), HistOracle(65, 3, 11, 3)
    rng = np.random.default_rng(3)
    term = np.zeros((65, 3, 14), np.float32)
    for p in range(5):
        obs, act = _words(rng, 65, 11), _words(rng, 65, 3)
        hist.push_buffers(_dev(torch, env, obs.T), _dev(torch, env, act.T), None)
        ora.push(obs, act)
        _assert_state(hist, ora, term, "push %d" % p)
    with pytest.raises(ValueError):
        hist.push_buffers(_dev(torch, env, obs), _dev(torch, env, act.T), None)      # a [B, D] tensor without rows=True
    env.close()


# ------------------------------------------------------------------------------------------------- end to end
def _drive(torch, env, top, hist, ora, term, steps, rows, seed, soa_full=False):
    """``steps`` steps under uniform random actions; the oracle takes the raw device buffers the step wrote.  Returns (any done, any full)."""
    base = env
    B, A = base.batch, base.dims.act_dim
    g = torch.Generator(device="cpu").manual_seed(seed)
    lo, hi = float(base.dims.act_low), float(base.dims.act_high)
    saw_done = saw_full = False
    for s in range(steps):
        if base.dims.discrete_action:
            a = torch.randint(0, 2, (B,), generator=g, dtype=torch.int32).to(base.device)
            a_np = _np(a).reshape(B, 1)
        else:
            a = (torch.rand(B, A, generator=g) * (hi - lo) + lo).to(base.device)
            a_np = _np(a)
        if soa_full:                               # the zero-copy path: the caller's SoA action, read by pointer in both calls
            a_soa = a.t().contiguous()
            top.step_soa_full(a_soa)
            hist.push(a_soa)
        else:
            top.step(a)
            hist.push(a if rows or s % 2 else None)   # row-major: the tensor step() read by pointer; else the env's own action buffer, which step() filled
        if rows:
            obs, tobs, done = _np(base._obs_rows), _np(base._term_rows), _np(base._done_b)
        elif top is not base and top.norm_obs:
            obs, tobs, done = _np(top._nobs).T, _np(top._nterm).T, _np(base._done)
        else:
            obs, tobs, done = _np(base._obs).T, _np(base._term_obs).T, _np(base._done)
        ora.push(obs, a_np, done, tobs, term)
        _assert_state(hist, ora, term, "step %d" % s)
        saw_done |= bool(done.any())
        saw_full |= bool((ora.length == ora.K).any())
    return saw_done, saw_full


@pytest.mark.parametrize("rows", [False, True])
def test_hopper_end_to_end_in_both_layouts(torch_mod, rows):
    import random_envs_amd as rex
    torch = torch_mod
    B, K = 130, 8
    env = _make("RandomHopper-v0", B, dr=True, row_major=rows)
    hist, ora = rex.HistoryStack(env, K), HistOracle(B, K, 11, 3)
    term = np.zeros((B, K, 14), np.float32)
    first = env.reset()
    hist.reset(); ora.reset(None, _np(first))
    _assert_state(hist, ora, term, "reset")
    d1, f1 = _drive(torch, env, env, hist, ora, term, 40, rows, seed=0)
    # a resume is exact: a second stack loaded from state() follows the first bit for bit
    twin = rex.HistoryStack(env, K)
    twin.load_state(hist.state())
    assert twin.count == hist.count
    d2, f2 = _drive(torch, env, env, hist, ora, term, 24, rows, seed=1, soa_full=not rows)
    assert d1 or d2, "no lane finished an episode in 64 steps"
    assert f1 or f2, "no lane reached length == K in 64 steps"
    env_state = hist.state()
    assert not torch.equal(twin.frames, env_state["frames"])               # the twin stayed where it was loaded ...
    twin.load_state(env_state)
    assert torch.equal(twin.window().contiguous().view(torch.int32), hist.window().contiguous().view(torch.int32)) and twin.count == hist.count
    # a masked env.reset in mid-run
    mask = torch.arange(B, device=env.device) % 3 == 0
    obs = env.reset(mask)
    hist.reset(mask)
    ora.reset(_np(mask), _np(obs))
    _assert_state(hist, ora, term, "masked reset")
    _drive(torch, env, env, hist, ora, term, 3, rows, seed=2)
    env.close()


def test_over_a_normalizing_wrapper_the_normalised_buffers_are_stored(torch_mod):
    import random_envs_amd as rex
    torch = torch_mod
    B, K = 65, 4
    env = _make("RandomHopper-v0", B, dr=True)
    nenv = rex.NormalizedVecRandomEnv(env)
    hist, ora = rex.HistoryStack(nenv, K), HistOracle(B, K, 11, 3)
    term = np.zeros((B, K, 14), np.float32)
    first = nenv.reset()
    hist.reset(); ora.reset(None, _np(first))
    assert _same(_np(hist.window()[:, -1, :11]), _np(nenv._nobs).T) and not _same(_np(nenv._nobs), _np(env._obs))
    saw_done, saw_full = _drive(torch, env, nenv, hist, ora, term, 40, False, seed=4)
    assert saw_done and saw_full
    env.close()


def test_cartpole_actions_are_stored_as_floats(torch_mod):
    import random_envs_amd as rex
    torch = torch_mod
    B, K = 65, 3
    for rows in (False, True):
        env = _make("RandomCartPole-v0", B, row_major=rows)
        hist, ora = rex.HistoryStack(env, K), HistOracle(B, K, 4, 1)
        term = np.zeros((B, K, 5), np.float32)
        first = env.reset()
        hist.reset(); ora.reset(None, _np(first))
        saw_done, saw_full = _drive(torch, env, env, hist, ora, term, 40, rows, seed=6)
        assert saw_done and saw_full
        col = _np(hist.window())[:, :, 4]
        assert set(np.unique(col).tolist()) == {0.0, 1.0} and hist.frames.dtype == torch.float32
        env.close()


# ------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_by_code_and_message_and_nothing_is_launched(torch_mod):
    from random_envs_amd import _native
    import random_envs_amd as rex
    torch = torch_mod
    B, K = 65, 3
    env = _make("RandomHopper-v0", B)
    hist = rex.HistoryStack(env, K)
    L, h, st = env._L, env._h, env._stream()
    hist.frames.fill_(7.0); hist.length.fill_(7); hist.terminal_window.fill_(7.0)
    out = torch.full((B, K, 14), 7.0, device=env.device)
    obs, act, tobs = (torch.zeros(n, B, device=env.device) for n in (11, 3, 11))
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())

    def desc(frames=hist.frames, length=hist.length, k=K, with_action=1):
        return ctypes.byref(_native.RexHistBuffers(None if frames is None else frames.data_ptr(), None if length is None else length.data_ptr(), k,
                                                   with_action))

    push = lambda d, slot=0, o=obs, a=act, t=None, w=None: L.rex_hist_push(h, d, slot, p(o), p(a), None, p(t), p(w), 0, st)
    cases = [
        ("rex_hist_init", lambda: L.rex_hist_init(h, None, st)),
        ("rex_hist_init", lambda: L.rex_hist_init(h, desc(frames=None), st)),
        ("rex_hist_init", lambda: L.rex_hist_init(h, desc(length=None), st)),
        ("rex_hist_init", lambda: L.rex_hist_init(h, desc(k=0), st)),
        ("rex_hist_init", lambda: L.rex_hist_init(h, desc(k=65), st)),
        ("rex_hist_push", lambda: push(None)),
        ("rex_hist_push", lambda: push(desc(frames=None))),
        ("rex_hist_push", lambda: push(desc(length=None))),
        ("rex_hist_push", lambda: push(desc(k=0))),
        ("rex_hist_push", lambda: push(desc(k=65))),
        ("rex_hist_push", lambda: push(desc(), slot=-1)),
        ("rex_hist_push", lambda: push(desc(), slot=K)),
        ("rex_hist_push", lambda: push(desc(), o=None)),
        ("rex_hist_push", lambda: push(desc(), a=None)),
        ("rex_hist_push", lambda: push(desc(), w=hist.terminal_window)),
        ("rex_hist_reset", lambda: L.rex_hist_reset(h, desc(frames=None), 0, None, p(obs), 0, st)),
        ("rex_hist_reset", lambda: L.rex_hist_reset(h, desc(k=65), 0, None, p(obs), 0, st)),
        ("rex_hist_reset", lambda: L.rex_hist_reset(h, desc(), K, None, p(obs), 0, st)),
        ("rex_hist_reset", lambda: L.rex_hist_reset(h, desc(), 0, None, None, 0, st)),
        ("rex_hist_window", lambda: L.rex_hist_window(h, desc(length=None), 0, p(out), st)),
        ("rex_hist_window", lambda: L.rex_hist_window(h, desc(k=0), 0, p(out), st)),
        ("rex_hist_window", lambda: L.rex_hist_window(h, desc(), -1, p(out), st)),
        ("rex_hist_window", lambda: L.rex_hist_window(h, desc(), 0, None, st)),
        ("rex_hist_push", lambda: L.rex_hist_push(None, desc(), 0, p(obs), p(act), None, None, None, 0, st)),
    ]
    for fn, call in cases:
        assert call() == -1, fn                                                   # REX_ERR_ARG
        assert L.rex_last_error().decode().startswith(fn + ":"), L.rex_last_error()
    torch.cuda.synchronize()
    for x in (hist.frames, hist.terminal_window, out):
        assert bool((x == 7.0).all())
    assert bool((hist.length == 7).all())
    # the same calls with nothing wrong are accepted: without action a null action, term_out with terminal_obs
    assert push(desc(with_action=0), a=None) == 0
    assert push(desc(), t=tobs, w=hist.terminal_window) == 0
    with pytest.raises(ValueError):
        rex.HistoryStack(env, 0)
    with pytest.raises(ValueError):
        rex.HistoryStack(env, 65)
    env.close()


# ------------------------------------------------------------------------------------------------- the learner's side
def test_the_window_is_the_sequence_gather_shifted_by_one_action(torch_mod):
    """The same synthetic steps into a ReplayBuffer and a HistoryStack: on the lanes with no done inside the window, the obs part of window()
    is gather_seq(seq_len = K - 1)'s obs rows 0 .. K - 1 started K - 1 slots back, and frame k >= 1 carries action[k - 1]."""
    import random_envs_amd as rex
    torch = torch_mod
    B, K, T, P = 130, 8, 16, 12
    env = _make("RandomHopper-v0", B)
    D, A = 11, 3
    rng = np.random.default_rng(8)
    o = rng.standard_normal((P + 1, D, B)).astype(np.float32)                # o[t]: what the policy saw at step t; o[t + 1] what step t returned
    a = rng.standard_normal((P, A, B)).astype(np.float32)
    tobs = rng.standard_normal((P, D, B)).astype(np.float32)
    done = (rng.random((P, B)) < 0.02).astype(np.uint8)
    d_o, d_a, d_t, d_done = (_dev(torch, env, x) for x in (o, a, tobs, done))
    reward = torch.zeros(B, device=env.device)
    buf, hist = rex.ReplayBuffer(env, T), rex.HistoryStack(env, K)
    env._obs.copy_(d_o[0]); hist.reset()
    for t in range(P):
        buf.add(d_o[t], d_a[t], reward, d_done[t], d_o[t + 1], d_t[t])
        hist.push_buffers(d_o[t + 1], d_a[t], d_done[t], d_t[t])
    t0 = P - (K - 1)
    ids = (t0 * B + torch.arange(B, device=env.device)).to(torch.int64)
    seq = buf.gather_seq(ids, K - 1)
    win = hist.window()
    ok = ~(d_done[t0:P].bool().any(0))
    assert int(ok.sum()) * 2 >= B, "fewer than half the lanes hold no done in the window"
    assert bool((seq["length"][ok] == K - 1).all())
    same = lambda x, y: torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
    assert same(win[ok][:, :, :D], seq["obs"][ok])
    assert same(win[ok][:, 1:, D:], seq["action"][ok])
    assert bool((hist.length[ok] == K).all())
    env.close()
