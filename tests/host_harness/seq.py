"""Builds and binds the host instantiation of the sequence-window launch's math, seq_host.cpp (TEST HARNESS ONLY): numpy arrays in, the
functions of csrc/seq_replay.hpp driven block by block, wave by wave and lane by lane, numpy arrays out."""
import ctypes

import numpy as np

from .build import build_so
from .rbuf import FIELDS, _ptrs

OUTPUTS = ("obs", "action", "reward", "done", "mask", "length", "index")
_lib = None


def lib():
    """seq_host.cpp built with g++ (rebuilt when it or a header is newer); no fused multiply-add"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("seq_host", "seq_host.cpp", ["-ffp-contract=off"]))
        vp, ll, u64, i32, f64 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_double
        _lib.sq_host_sample.argtypes = [vp, ll, ll, i32, i32, vp, ll, ll, ll, u64, u64, i32, vp, vp, i32, i32, f64, f64, f64, i32, vp]
    return _lib


def sample(bufs, n, head, seq_len, index=None, size=None, seed=0, draw=0, norm=None, force_scalar=False, want=OUTPUTS):
    """The sequence launch: ``index`` given -> rex_rbuf_gather_seq, else ids drawn over ``size`` slots (rex_rbuf_sample_seq).  ``norm`` as in
    host_harness.rbuf.sample.  Returns (rc, outputs, bad); the outputs start out as NaN / -7, so a field the launch skips, or padding it does
    not write, shows."""
    T, B, D = bufs["obs"].shape
    A = bufs["action"].shape[2]
    L = max(int(seq_len), 0)
    out = dict(obs=np.full((n, L + 1, D), np.nan, np.float32), action=np.full((n, L, A), -7, bufs["action"].dtype),
               reward=np.full((n, L), np.nan, np.float32), done=np.full((n, L), np.nan, np.float32), mask=np.full((n, L), np.nan, np.float32),
               length=np.full(n, -7, np.int32), index=np.full(n, -7, np.int64))
    outs = [out[k] if k in want and (k != "index" or index is None) else None for k in OUTPUTS]
    bad = np.zeros(1, np.int64)
    idx = None if index is None else np.ascontiguousarray(index, np.int64)
    stats = None if norm is None else np.ascontiguousarray(norm["stats"], np.float64)
    nz = norm or dict(norm_obs=0, norm_reward=0, epsilon=0.0, clip_obs=0.0, clip_reward=0.0)
    rc = lib().sq_host_sample(_ptrs([bufs[k] for k in FIELDS]), T, B, D, A, None if idx is None else idx.ctypes.data, n, 0 if size is None else size,
                              head, seed, draw, seq_len, _ptrs(outs), None if stats is None else stats.ctypes.data, int(nz["norm_obs"]),
                              int(nz["norm_reward"]), nz["epsilon"], nz["clip_obs"], nz["clip_reward"], int(force_scalar), bad.ctypes.data)
    return rc, {k: out[k] for k, p in zip(OUTPUTS, outs) if p is not None}, int(bad[0])
