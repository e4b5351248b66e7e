"""Builds and binds the host instantiation of the replay buffer kernels' math, rbuf_host.cpp (TEST HARNESS ONLY): numpy arrays in, the
functions of csrc/replay_buffer.hpp driven block by block and thread by thread, numpy arrays out."""
import ctypes

import numpy as np

from .build import build_so

FIELDS = ("obs", "next_obs", "action", "reward", "done", "timeout")
_lib = None


def lib():
    """rbuf_host.cpp built with g++ (rebuilt when it or a header is newer); no fused multiply-add"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("rbuf_host", "rbuf_host.cpp", ["-ffp-contract=off"]))
        vp, ll, u64, i32, f64 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_double
        _lib.rb_host_philox.argtypes = [vp, vp, vp]
        _lib.rb_host_philox.restype = None
        _lib.rb_host_ids.argtypes = [u64, u64, ll, ll, vp, vp]
        _lib.rb_host_ids.restype = None
        _lib.rb_host_add.argtypes = [vp, ll, ll, i32, i32, ll, vp]
        _lib.rb_host_sample.argtypes = [vp, ll, ll, i32, i32, vp, ll, ll, u64, u64, vp, vp, i32, i32, f64, f64, f64, i32, vp]
    return _lib


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def philox(counter, key):
    c, k, out = np.array(counter, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    lib().rb_host_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return tuple(int(v) for v in out)


def ids(seed, draw, N, n):
    """(ids int64 [n], raw 64-bit words uint64 [n]) of one draw over N transitions"""
    out, bits = np.zeros(n, np.int64), np.zeros(n, np.uint64)
    lib().rb_host_ids(seed, draw, N, n, out.ctypes.data, bits.ctypes.data)
    return out, bits


def empty_buffers(T, B, D, A, act_dtype=np.float32):
    return dict(obs=np.zeros((T, B, D), np.float32), next_obs=np.zeros((T, B, D), np.float32), action=np.zeros((T, B, A), act_dtype),
                reward=np.zeros((T, B), np.float32), done=np.zeros((T, B), np.uint8), timeout=np.zeros((T, B), np.uint8))


def add(bufs, slot, step, with_term=True, with_trunc=True):
    """step: dict of the SoA inputs obs [D, B], action [A, B], reward, done [B], next_obs [D, B], terminal_obs [D, B], truncated [B]"""
    T, B, D = bufs["obs"].shape
    A = bufs["action"].shape[2]
    src = [step[k] for k in ("obs", "action", "reward", "done", "next_obs")] + [step["terminal_obs"] if with_term else None,
                                                                                 step["truncated"] if with_trunc else None]
    assert all(a is None or a.flags.c_contiguous for a in src)
    return lib().rb_host_add(_ptrs([bufs[k] for k in FIELDS]), T, B, D, A, slot, _ptrs(src))


def sample(bufs, n, index=None, size=None, seed=0, draw=0, norm=None, force_scalar=False, want=("obs", "next_obs", "action", "reward", "done", "index")):
    """The sample launch: ``index`` given -> rex_rbuf_gather, else ids drawn over ``size`` slots.  ``norm``: None, or a dict of stats
    (float64 [3 * (D + 1)]: counts, means, variances), norm_obs, norm_reward, epsilon, clip_obs, clip_reward.  Returns (rc, outputs, bad)."""
    T, B, D = bufs["obs"].shape
    A = bufs["action"].shape[2]
    out = dict(obs=np.full((n, D), np.nan, np.float32), next_obs=np.full((n, D), np.nan, np.float32), action=np.full((n, A), -7, bufs["action"].dtype),
               reward=np.full(n, np.nan, np.float32), done=np.full(n, np.nan, np.float32), index=np.full(n, -7, np.int64))
    outs = [out[k] if k in want and (k != "index" or index is None) else None for k in ("obs", "next_obs", "action", "reward", "done", "index")]
    bad = np.zeros(1, np.int64)
    idx = None if index is None else np.ascontiguousarray(index, np.int64)
    stats = None if norm is None else np.ascontiguousarray(norm["stats"], np.float64)
    nz = norm or dict(norm_obs=0, norm_reward=0, epsilon=0.0, clip_obs=0.0, clip_reward=0.0)
    rc = lib().rb_host_sample(_ptrs([bufs[k] for k in FIELDS]), T, B, D, A, None if idx is None else idx.ctypes.data, n, 0 if size is None else size,
                              seed, draw, _ptrs(outs), None if stats is None else stats.ctypes.data, int(nz["norm_obs"]), int(nz["norm_reward"]),
                              nz["epsilon"], nz["clip_obs"], nz["clip_reward"], int(force_scalar), bad.ctypes.data)
    return rc, {k: v for k, v, p in zip(out, out.values(), outs) if p is not None}, int(bad[0])
