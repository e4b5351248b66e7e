"""Row-major gym surface, CPU half: the humanoid transposer's tile walk and the action walk (the __host__ __device__ index functions of
csrc/rows.hpp, driven block by block and thread by thread by tests/host_harness/rows_host.cpp) against numpy: every output word is
written exactly once with the transposed value, or not at all where a keep mask or the done flags exclude its env; nothing is written
outside the buffers; and the padded tile is conflict-free in both phases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from host_harness.build import build_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "host_harness")
BATCHES = [1, 63, 64, 65, 67]
DIMS = [4, 11, 17, 376]
GUARD = 16
SENTINEL = np.float32(-7.25)

_lib = None


def harness():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("rows_host", "rows_host.cpp"))
        vp, ll, i32 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
        _lib.rows_host_transpose.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, ll, vp, vp]
        _lib.rows_host_transpose.restype = ll
        _lib.rows_host_action.argtypes = [vp, vp, i32, ll]
        _lib.rows_host_wave_words.argtypes = [i32, i32, i32, vp]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


def _guarded(n):
    """a float32 output of n words holding a sentinel, with GUARD more words behind it"""
    buf = np.full(n + GUARD, SENTINEL, np.float32)
    return buf, buf[:n]


def _transpose(B, D, keep=None, done=None, seed=0):
    rng = np.random.default_rng(seed + 1000 * B + D)
    soa = rng.standard_normal((D, B)).astype(np.float32)
    term = rng.standard_normal((D, B)).astype(np.float32)
    obuf, out = _guarded(B * D)
    tbuf, tout = _guarded(B * D)
    wo, wt = np.zeros(B * D, np.int32), np.zeros(B * D, np.int32)
    walked = harness().rows_host_transpose(_p(soa), _p(obuf), _p(keep), 1, _p(term) if done is not None else None, _p(tbuf) if done is not None else None,
                                           _p(done), D, B, _p(wo), _p(wt))
    assert (obuf[B * D:] == SENTINEL).all() and (tbuf[B * D:] == SENTINEL).all(), "a store past the end"
    return soa, term, out.reshape(B, D), tout.reshape(B, D), wo.reshape(B, D), wt.reshape(B, D), walked


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("B", BATCHES)
def test_every_row_word_is_written_once_with_the_transposed_value(B, D):
    soa, _, out, tout, wo, wt, walked = _transpose(B, D)
    assert (wo == 1).all() and np.array_equal(out.view(np.uint32), np.ascontiguousarray(soa.T).view(np.uint32))
    assert walked == 0 and not wt.any() and (tout == SENTINEL).all()


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("B", BATCHES)
def test_keep_mask_leaves_the_unmasked_rows_untouched(B, D):
    rng = np.random.default_rng(B * 7 + D)
    keep = (rng.random(B) < 0.5).astype(np.uint8)
    keep[0] = 1 if B == 1 else keep[0]
    soa, _, out, _, wo, _, _ = _transpose(B, D, keep=keep)
    m = keep != 0
    assert (wo[m] == 1).all() and not wo[~m].any()
    assert np.array_equal(out[m].view(np.uint32), np.ascontiguousarray(soa.T)[m].view(np.uint32)) and (out[~m] == SENTINEL).all()
    # a mask whose bytes lack bit 1 selects nothing (rex_reset's `mask[i] & 1`)
    _, _, out2, _, wo2, _, _ = _transpose(B, D, keep=(keep * 2).astype(np.uint8))
    assert not wo2.any() and (out2 == SENTINEL).all()


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("B", BATCHES)
def test_terminal_rows_are_copied_for_done_envs_only(B, D):
    rng = np.random.default_rng(B * 11 + D)
    for frac in (0.0, 0.3, 1.0):
        done = (rng.random(B) < frac).astype(np.uint8)
        soa, term, out, tout, wo, wt, walked = _transpose(B, D, done=done)
        d = done != 0
        assert (wo == 1).all() and np.array_equal(out, soa.T)               # the observation does not depend on done
        assert (wt[d] == 1).all() and not wt[~d].any()
        assert np.array_equal(tout[d].view(np.uint32), np.ascontiguousarray(term.T)[d].view(np.uint32)) and (tout[~d] == SENTINEL).all()
        tiles_with_done = sum(int(done[e0:e0 + 64].any()) for e0 in range(0, B, 64)) * -(-D // 64)
        assert walked == tiles_with_done                                      # tiles without a finished env skip the second walk


def test_keep_mask_and_terminal_copy_together():
    B, D = 67, 376
    rng = np.random.default_rng(5)
    keep, done = (rng.random(B) < 0.5).astype(np.uint8), (rng.random(B) < 0.3).astype(np.uint8)
    soa, term, out, tout, wo, wt, _ = _transpose(B, D, keep=keep, done=done)
    assert np.array_equal(wo, np.repeat(keep[:, None], D, 1)) and np.array_equal(wt, np.repeat(done[:, None], D, 1))
    assert np.array_equal(out[keep != 0], soa.T[keep != 0]) and np.array_equal(tout[done != 0], term.T[done != 0])


@pytest.mark.parametrize("NU", [1, 3, 6, 17])
@pytest.mark.parametrize("B", BATCHES)
def test_action_rows_become_the_soa_staging(B, NU):
    rng = np.random.default_rng(B + NU)
    a = rng.standard_normal((B, NU)).astype(np.float32)
    buf, out = _guarded(NU * B)
    assert harness().rows_host_action(_p(a), _p(buf), NU, B) == 0
    assert np.array_equal(out.reshape(NU, B).view(np.uint32), np.ascontiguousarray(a.T).view(np.uint32)) and (buf[NU * B:] == SENTINEL).all()


def test_the_padded_tile_has_no_bank_conflicts_in_either_phase():
    """64 lanes of a wave touch 64 different LDS banks (word % 64) in every load pass and in every store pass, inside the tile"""
    words = np.zeros(64, np.int32)
    for phase in (0, 1):
        for wave in range(4):
            for p in range(16):
                n = harness().rows_host_wave_words(phase, wave, p, _p(words))
                assert words.min() >= 0 and words.max() < n
                assert len(set(int(w) % 64 for w in words)) == 64, (phase, wave, p)


def test_tile_walk_stays_inside_exactly_sized_buffers_under_sanitizers(tmp_path):
    """tests/host_harness/rows_sanitize_main.cpp: a program of its own (the sanitizer runtimes are linked into it; nothing is preloaded)"""
    exe = str(tmp_path / "rows_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(HARNESS, "rows_sanitize_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "B=67 D=376 masked=1" in run.stdout and "bad=0" in run.stdout and "bad=1" not in run.stdout
