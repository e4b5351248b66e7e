"""Binds tests/host_harness/actor_host.cpp (TEST HARNESS ONLY): the host twin of rex_actor_act over numpy arrays, tanh32 and its sweep, and
the argument check."""
import ctypes

import numpy as np

from .build import build_so

_lib = None
MAX_HIDDEN = 3


def build_flags():
    return ["-ffp-contract=off"]


def lib():
    """actor_host.cpp built with g++ (rebuilt when it or a header is newer); no fused multiply-add beyond the fmaf calls written out"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("actor_host", "actor_host.cpp", build_flags()))
        vp, ll, i32 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
        _lib.actor_host_act.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ll, vp, vp, vp, vp, vp]
        _lib.actor_host_tanh.argtypes = [vp, vp, ll]
        _lib.actor_host_tanh_sweep.argtypes = [ctypes.c_uint, ctypes.c_uint, vp]
        _lib.actor_host_tanh_sweep.restype = ctypes.c_double
        _lib.actor_host_check.argtypes = [vp, vp, vp, i32, ll, i32, i32, ctypes.c_char_p, i32]
    return _lib


def _tower(layers):
    """(ints, pointer block, the arrays kept alive) of a list of (W, b) float32 arrays, hidden layers first, head last"""
    if layers is None:
        return None, None, None
    keep = [(np.ascontiguousarray(W, np.float32), np.ascontiguousarray(b, np.float32)) for W, b in layers]
    n_hidden = len(keep) - 1
    ints = np.array([n_hidden] + [keep[l][0].shape[0] if l < n_hidden else 0 for l in range(MAX_HIDDEN)], np.int32)
    ptrs = (ctypes.c_void_p * (2 * (MAX_HIDDEN + 1)))()
    for l, (W, b) in enumerate(keep):
        ptrs[l], ptrs[MAX_HIDDEN + 1 + l] = W.ctypes.data, b.ctypes.data
    return ints, ptrs, keep


def act(pi, vf, log_std, obs, act_dim, activation="tanh", rows=True, eps=None, std=None):
    """The twin's rex_actor_act: ``obs`` [B, in_dim] (rows) or [in_dim, B]; ``eps`` [B, act_dim] float32, or None for a deterministic call;
    ``std`` [act_dim] the fp32 std the device was handed (default: numpy's exp of log_std, rounded to fp32).
    Returns dict(action, logp, value, mean): action in the layout of obs, mean [B, act_dim]; the entries of an absent tower are None."""
    obs = np.ascontiguousarray(obs, np.float32)
    B, in_dim = (obs.shape if rows else obs.shape[::-1])
    A = int(act_dim)
    dims = np.array([in_dim, A, {"tanh": 0, "relu": 1}[activation], int(bool(rows)), int(eps is None)], np.int32)
    pi_i, pi_p, k1 = _tower(pi)
    vf_i, vf_p, k2 = _tower(vf)
    p = lambda a: None if a is None else a.ctypes.data
    ls = None if log_std is None else np.ascontiguousarray(log_std, np.float32)
    if ls is not None:
        std = np.exp(ls).astype(np.float32) if std is None else np.ascontiguousarray(std, np.float32)
    e = None if eps is None else np.ascontiguousarray(eps, np.float32)
    out = dict(action=np.zeros((B, A) if rows else (A, B), np.float32) if pi is not None else None, logp=np.zeros(B, np.float32) if pi is not None else None,
               value=np.zeros(B, np.float32) if vf is not None else None, mean=np.zeros((B, A), np.float32) if pi is not None else None)
    rc = lib().actor_host_act(p(dims), p(pi_i), pi_p, p(vf_i), vf_p, p(ls), p(std), p(obs), B, p(e),
                              p(out["action"]), p(out["logp"]), p(out["value"]), p(out["mean"]))
    assert rc == 0
    return out


def tanh(x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    lib().actor_host_tanh(x.ctypes.data, y.ctypes.data, x.size)
    return y


def tanh_sweep(lo, hi):
    """(worst error in ulp, the x it occurs at) over every fp32 in [lo, hi], 0 <= lo <= hi"""
    lo_bits, hi_bits = (int(np.float32(v).view(np.uint32)) for v in (lo, hi))
    where = ctypes.c_float()
    worst = lib().actor_host_tanh_sweep(lo_bits, hi_bits, ctypes.byref(where))
    return worst, where.value


def check(null_net=False, in_dim=11, activation=0, has_log_std=True, has_std=True, pi=(2, 64, 64, 0, -1), vf=(2, 64, 64, 0, -1), has_in=True, draw=0,
          has_action=True, has_value=True):
    """rex_actor_act's argument check: None, or the message.  A tower is (n_hidden, width0, width1, width2, null_layer) or None; null_layer
    -1: none, l: W[l] is null, 8 + l: b[l] is null."""
    net = np.array([int(null_net), in_dim, activation, int(has_log_std), int(has_std)], np.int32)
    t = lambda x: None if x is None else np.array(x, np.int32)
    pi_i, vf_i = t(pi), t(vf)
    why = ctypes.create_string_buffer(256)
    bad = lib().actor_host_check(net.ctypes.data, None if pi_i is None else pi_i.ctypes.data, None if vf_i is None else vf_i.ctypes.data, int(has_in), int(draw),
                                 int(has_action), int(has_value), why, 256)
    return why.value.decode() if bad else None
