"""Builds and binds the host instantiation of the history stack's launches, hist_host.cpp (TEST HARNESS ONLY): numpy arrays in, the
functions of csrc/hist.hpp driven block by block and thread by thread, numpy arrays out."""
import ctypes

import numpy as np

from .build import build_so

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("hist_host", "hist_host.cpp"))
        vp, ll, i32 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
        ring = [vp, vp, ll, i32, i32, i32]
        _lib.hs_host_init.argtypes = ring
        _lib.hs_host_push.argtypes = ring + [i32, vp, vp, i32, vp, vp, vp, i32]
        _lib.hs_host_reset.argtypes = ring + [i32, vp, vp, i32]
        _lib.hs_host_window.argtypes = ring + [i32, vp]
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def layout(a, rows):
    """a batch-major [B, dim] array in the layout a launch reads: itself (rows) or its SoA transpose [dim, B]"""
    if a is None:
        return None
    a = np.asarray(a)
    if a.ndim == 1:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a if rows else a.T)


class HostHist:
    """The four launches over numpy storage.  Inputs are batch-major; ``rows`` picks the layout the launch is handed.  ``frames`` starts out
    as NaN and ``length`` as -7, so anything init does not write shows."""

    def __init__(self, B, K, obs_dim, act_dim, with_action=True, int_action=False):
        self.B, self.K, self.D, self.A = B, K, obs_dim, act_dim if with_action else 0
        self.W = self.D + self.A
        self.int_action = int_action
        self.frames = np.full((B, 2 * K, self.W), np.nan, np.float32)
        self.length = np.full(B, -7, np.int32)
        self.term = np.full((B, K, self.W), np.nan, np.float32)
        self.pushes = 0
        assert lib().hs_host_init(*self._ring()) == 0

    def _ring(self):
        return [self.frames.ctypes.data, self.length.ctypes.data, self.B, self.K, self.D, self.A]

    def _slot(self):
        return (self.pushes - 1) % self.K if self.pushes else 0

    def push(self, obs, action, done=None, terminal_obs=None, rows=False):
        o, a, tm = layout(obs, rows), layout(action, rows) if self.A else None, layout(terminal_obs, rows)
        d = None if done is None else np.ascontiguousarray(done, np.uint8)
        self._keep = (o, a, tm, d)
        assert lib().hs_host_push(*self._ring(), self.pushes % self.K, _ptr(o), _ptr(a), int(self.int_action), _ptr(d), _ptr(tm),
                                  _ptr(self.term) if tm is not None else None, int(rows)) == 0
        self.pushes += 1

    def reset(self, mask, obs, rows=False):
        o = layout(obs, rows)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        assert lib().hs_host_reset(*self._ring(), self._slot(), _ptr(m), _ptr(o), int(rows)) == 0
        self.pushes = max(self.pushes, 1)           # before the first push the reset's frame takes slot 0: the next push goes to slot 1

    def window(self):
        out = np.full((self.B, self.K, self.W), np.nan, np.float32)
        assert lib().hs_host_window(*self._ring(), self._slot(), out.ctypes.data) == 0
        return out
