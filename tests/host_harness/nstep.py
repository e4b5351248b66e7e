"""Builds and binds the host instantiation of the n-step sample launch's math, nstep_host.cpp (TEST HARNESS ONLY): numpy arrays in, the
functions of csrc/nstep_replay.hpp driven block by block, wave by wave and lane by lane, numpy arrays out."""
import ctypes

import numpy as np

from .build import build_so
from .rbuf import FIELDS, _ptrs

OUTPUTS = ("obs", "next_obs", "action", "reward", "done", "index", "discount", "steps")
_lib = None


def lib():
    """nstep_host.cpp built with g++ (rebuilt when it or a header is newer); no fused multiply-add"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("nstep_host", "nstep_host.cpp", ["-ffp-contract=off"]))
        vp, ll, u64, i32, f64 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_double
        _lib.ns_host_step_slot.argtypes = [ll, ll, ll, i32, vp, vp]
        _lib.ns_host_step_slot.restype = None
        _lib.ns_host_sample.argtypes = [vp, ll, ll, i32, i32, vp, ll, ll, ll, u64, u64, i32, f64, vp, vp, i32, i32, f64, f64, f64, i32, vp]
    return _lib


def step_slot(T, B, s0, k):
    """(id, time slot) of step k of the window that starts at s0"""
    s, t = ctypes.c_longlong(), ctypes.c_longlong()
    lib().ns_host_step_slot(T, B, s0, k, ctypes.addressof(s), ctypes.addressof(t))
    return s.value, t.value


def sample(bufs, n, head, n_step, gamma, index=None, size=None, seed=0, draw=0, norm=None, force_scalar=False, want=OUTPUTS):
    """The n-step launch: ``index`` given -> rex_rbuf_gather_nstep, else ids drawn over ``size`` slots (rex_rbuf_sample_nstep).  ``norm`` as in
    host_harness.rbuf.sample.  Returns (rc, outputs, bad); the outputs start out as NaN / -7, so a field the launch skips shows."""
    T, B, D = bufs["obs"].shape
    A = bufs["action"].shape[2]
    out = dict(obs=np.full((n, D), np.nan, np.float32), next_obs=np.full((n, D), np.nan, np.float32), action=np.full((n, A), -7, bufs["action"].dtype),
               reward=np.full(n, np.nan, np.float32), done=np.full(n, np.nan, np.float32), index=np.full(n, -7, np.int64),
               discount=np.full(n, np.nan, np.float32), steps=np.full(n, -7, np.int32))
    outs = [out[k] if k in want and (k != "index" or index is None) else None for k in OUTPUTS]
    bad = np.zeros(1, np.int64)
    idx = None if index is None else np.ascontiguousarray(index, np.int64)
    stats = None if norm is None else np.ascontiguousarray(norm["stats"], np.float64)
    nz = norm or dict(norm_obs=0, norm_reward=0, epsilon=0.0, clip_obs=0.0, clip_reward=0.0)
    rc = lib().ns_host_sample(_ptrs([bufs[k] for k in FIELDS]), T, B, D, A, None if idx is None else idx.ctypes.data, n, 0 if size is None else size,
                              head, seed, draw, n_step, gamma, _ptrs(outs), None if stats is None else stats.ctypes.data, int(nz["norm_obs"]),
                              int(nz["norm_reward"]), nz["epsilon"], nz["clip_obs"], nz["clip_reward"], int(force_scalar), bad.ctypes.data)
    return rc, {k: out[k] for k, p in zip(OUTPUTS, outs) if p is not None}, int(bad[0])
