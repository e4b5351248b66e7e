"""Binds tests/host_harness/adr_host.cpp (TEST HARNESS ONLY): what rex_adr_enable sets up, in numpy arrays, and the three calls."""
import ctypes
import os

import numpy as np

from .build import build_so

_lib = None


def rocm_include():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "rocrand", "rocrand_kernel.h")):
            return os.path.join(root, "include")
    return None


def build_flags():
    return ["-ffp-contract=off", "-w", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include()]


def lib():
    """adr_host.cpp built with g++ (rebuilt when it or a header is newer); no fused multiply-add"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("adr_host", "adr_host.cpp", build_flags()))
        vp, ll, u64, i32 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_uint64, ctypes.c_int
        _lib.adr_host_blocks.argtypes = [ll]
        _lib.adr_host_record.argtypes = [vp, ll, ll, u64, ll, vp, vp, vp, i32]
        _lib.adr_host_assign.argtypes = [vp, ll, ll, u64, ll, vp, vp, vp]
        _lib.adr_host_update.argtypes = [vp, ll, ll, u64, ll, vp, vp, vp]
        _lib.adr_host_check.argtypes = [ll, vp, vp, vp, vp, vp, ctypes.c_char_p, i32]
    return _lib


def pack(d, act, row_map, p_b, delta, lim_lo, lim_hi, centre, t_lo, t_hi):
    f = lambda x: np.asarray(x, np.float32).reshape(d)
    ints = np.array([d, len(act)] + list(act) + list(row_map), np.int32)
    floats = np.concatenate([[np.float32(p_b)], f(delta), f(lim_lo), f(lim_hi), f(centre)]).astype(np.float32)
    return ints, floats, np.array([t_lo, t_hi], np.float64)


class HostBox:
    """The arguments of tests/adr_oracle.Box plus the row map and the handle's FULL xi block [full_rows, B]; every buffer exactly sized."""

    def __init__(self, B, d, act, p_b, m, t_lo, t_hi, delta, lim_lo, lim_hi, centre, init_lo, init_hi, seed, xi_full, row_map=None, env_offset=0):
        self.L = lib()
        self.B, self.d, self.J, self.m, self.seed, self.env_offset = B, d, 2 * len(act), int(m), int(seed), int(env_offset)
        self.map = list(range(d)) if row_map is None else list(row_map)
        self.ints, self.floats, self.doubles = pack(d, act, self.map, p_b, delta, lim_lo, lim_hi, centre, t_lo, t_hi)
        J, blocks = self.J, self.L.adr_host_blocks(B)
        self.lo, self.hi = np.array(init_lo, np.float32).reshape(d).copy(), np.array(init_hi, np.float32).reshape(d).copy()
        self.n, self.s, self.counters = np.zeros(J, np.int64), np.zeros(J, np.float64), np.zeros((3, J), np.int64)
        self.ret, self.len = np.zeros(B, np.float64), np.zeros(B, np.int32)
        self.bnd, self.ep = np.full(B, -1, np.int32), np.zeros(B, np.uint32)
        self.pcount, self.psum = np.zeros(blocks * J, np.int32), np.zeros(blocks * J, np.float64)
        self.mask = np.zeros(B, np.uint8)
        self.xi = np.ascontiguousarray(xi_full, np.float32).copy()

    def _call(self, fn, reward=None, done=None, *extra):
        arrs = [self.lo, self.hi, self.n, self.s, self.counters, self.ret, self.len, self.bnd, self.ep, self.pcount, self.psum, self.mask, self.xi, reward, done]
        ptrs = (ctypes.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])
        assert fn(ptrs, self.B, self.env_offset, self.seed, self.m, self.ints.ctypes.data, self.floats.ctypes.data, self.doubles.ctypes.data, *extra) == 0

    def record(self, reward, done, apply=True):
        self._call(self.L.adr_host_record, np.ascontiguousarray(reward, np.float32), np.ascontiguousarray(done, np.uint8), int(bool(apply)))

    def assign(self, mask=None):
        self._call(self.L.adr_host_assign, None, None if mask is None else np.ascontiguousarray(mask, np.uint8))

    def update(self):
        self._call(self.L.adr_host_update)

    @property
    def task(self):
        return self.xi[np.asarray(self.map)]

    def state(self):
        return dict(lo=self.lo.copy(), hi=self.hi.copy(), n=self.n.copy(), s=self.s.copy(), counters=self.counters.copy())

    def lane_state(self):
        return dict(ret=self.ret.copy(), len=self.len.copy(), bnd=self.bnd.copy(), ep=self.ep.copy())


def check(d, act, p_b, m, t_lo, t_hi, delta, lim_lo, lim_hi, centre, init_lo, init_hi):
    """rex_adr_enable's argument check: None, or the message"""
    ints, floats, doubles = pack(d, [a for a in act], list(range(d)), p_b, delta, lim_lo, lim_hi, centre, t_lo, t_hi)
    lo, hi = np.asarray(init_lo, np.float32).reshape(d).copy(), np.asarray(init_hi, np.float32).reshape(d).copy()
    why = ctypes.create_string_buffer(256)
    bad = lib().adr_host_check(int(m), ints.ctypes.data, floats.ctypes.data, doubles.ctypes.data, lo.ctypes.data, hi.ctypes.data, why, 256)
    return why.value.decode() if bad else None
