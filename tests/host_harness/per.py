"""Builds and binds the host instantiation of the prioritised replay kernels' math, per_host.cpp (TEST HARNESS ONLY): numpy arrays in, the
functions of csrc/priority_replay.hpp driven launch by launch, block by block and thread by thread, numpy arrays out.  Every array the
functions write sits in front of guard words that :meth:`HostPer.guards_intact` checks."""
import ctypes

import numpy as np

from .build import build_so

_lib = None
GUARD = 8                                # guard items behind every buffer
_PATTERN = {np.dtype(np.float32): 0xDEADBEEF, np.dtype(np.float64): 0xDEADBEEFCAFEF00D, np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A}
_UINT = {4: np.uint32, 8: np.uint64}


def lib():
    """per_host.cpp built with g++ (rebuilt when it or a header is newer); no fused multiply-add"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("per_host", "per_host.cpp", ["-ffp-contract=off"]))
        vp, ll, u64, f64 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_double
        _lib.per_host_tree_len.argtypes = [ll]
        _lib.per_host_tree_len.restype = ll
        _lib.per_host_depth.argtypes = [ll]
        _lib.per_host_init.argtypes = [vp, ll, ll]
        _lib.per_host_add.argtypes = [vp, ll, ll, ll]
        _lib.per_host_update.argtypes = [vp, ll, ll, vp, vp, ll, vp]
        _lib.per_host_rebuild.argtypes = [vp, ll, ll]
        _lib.per_host_draw.argtypes = [vp, ll, ll, ll, u64, u64, vp, vp]
        _lib.per_host_x.argtypes = [u64, u64, u64, ll, f64]
        _lib.per_host_x.restype = f64
        _lib.per_host_descent.argtypes = [vp, ll, ll, vp, ll, vp, vp]
    return _lib


def tree_len(N):
    return int(lib().per_host_tree_len(N))


def depth(N):
    return int(lib().per_host_depth(N))


def sample_x(seed, draw, j, n, total):
    return float(lib().per_host_x(seed, draw, j, n, float(total)))


def guarded(n, dtype, fill):
    """(the whole allocation, the view of its first n items); the GUARD items behind the view hold a pattern"""
    whole = np.empty(n + GUARD, dtype)
    whole[:n] = fill
    whole[n:].view(_UINT[whole.itemsize])[:] = _PATTERN[np.dtype(dtype)]
    return whole, whole[:n]


def guard_ok(whole):
    return bool((whole[-GUARD:].view(_UINT[whole.itemsize]) == _PATTERN[whole.dtype]).all())


class HostPer:
    """priority / tree / max_priority of T slots over B envs as the kernels' functions leave them.  The arrays start as garbage
    (NaN): ``init`` is what defines them."""

    def __init__(self, T, B):
        self.T, self.B, self.N = T, B, T * B
        self._whole = {}
        self._whole["priority"], self.priority = guarded(self.N, np.float32, np.nan)
        self._whole["tree"], self.tree = guarded(tree_len(self.N), np.float64, np.nan)
        self._whole["max_priority"], self.max_priority = guarded(1, np.float32, np.nan)
        self.counters = np.zeros(2, np.int64)

    def _ptrs(self):
        return (ctypes.c_void_p * 3)(self.priority.ctypes.data, self.tree.ctypes.data, self.max_priority.ctypes.data)

    def init(self):
        return lib().per_host_init(self._ptrs(), self.T, self.B)

    def add(self, t):
        return lib().per_host_add(self._ptrs(), self.T, self.B, t)

    def update(self, index, value):
        idx, val = np.ascontiguousarray(index, np.int64), np.ascontiguousarray(value, np.float32)
        assert idx.shape == val.shape
        widx, gi = guarded(len(idx), np.int64, idx)
        wval, gv = guarded(len(val), np.float32, val)
        rc = lib().per_host_update(self._ptrs(), self.T, self.B, gi.ctypes.data, gv.ctypes.data, len(idx), self.counters.ctypes.data)
        assert guard_ok(widx) and guard_ok(wval) and np.array_equal(gi, idx)
        return rc

    def rebuild(self):
        return lib().per_host_rebuild(self._ptrs(), self.T, self.B)

    def draw(self, n, seed, draw):
        """(index int64 [n], prob float32 [n])"""
        widx, idx = guarded(n, np.int64, -7)
        wprob, prob = guarded(n, np.float32, np.nan)
        assert lib().per_host_draw(self._ptrs(), self.T, self.B, n, seed, draw, idx.ctypes.data, prob.ctypes.data) == 0
        assert guard_ok(widx) and guard_ok(wprob)
        return idx.copy(), prob.copy()

    def descent(self, x):
        x = np.ascontiguousarray(x, np.float64)
        idx, prob = np.full(len(x), -7, np.int64), np.full(len(x), np.nan, np.float32)
        assert lib().per_host_descent(self._ptrs(), self.T, self.B, x.ctypes.data, len(x), idx.ctypes.data, prob.ctypes.data) == 0
        return idx, prob

    def guards_intact(self):
        return all(guard_ok(w) for w in self._whole.values())
