"""Episode ledger, CPU half: the kernels' own addressing, slot arithmetic and bookkeeping (the __host__ __device__ functions of
csrc/eplog.hpp, driven block by block in grid order by tests/host_harness/eplog_host.cpp) against the numpy restatement of the
contract in tests/eplog_oracle.py.  Every field, the per-lane state and the counters are held to IDENTICAL BITS: the ledger does one
fp64 addition per lane and step, in step order, and copies everything else."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import eplog_oracle as oracle
from eplog_oracle import assert_same_bits, assert_tables_equal
from host_harness.build import build_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "host_harness")
SIZES = [1, 63, 64, 257, 4097]
GUARD = 16                      # elements behind every buffer of the table
HOPPER_UNMODELED_MAP = [1, 2, 3]   # task row k = row 1 + k of the full hopper block (thigh, leg, foot masses; the torso mass is frozen)

_lib = None


def harness():
    """tests/host_harness/eplog_host.cpp built with g++ (rebuilt when it or a header is newer); no fused multiply-add"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("eplog_host", "eplog_host.cpp", ["-ffp-contract=off"]))
        vp, ll, i32 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
        _lib.el_host_blocks.argtypes = [ll]
        _lib.el_host_step.argtypes = [vp, ll, ll, i32, vp, ll]
        _lib.el_host_sync.argtypes = [vp, ll, i32, vp, i32]
        _lib.el_host_read.argtypes = [vp, ll, vp, i32]
    return _lib


class HostLedger:
    """what rex_eplog_enable sets up, in numpy arrays, with guard elements behind every buffer of the table"""

    def __init__(self, B, task_dim, capacity, xi_full, row_map=None, env_offset=0):
        self.L = harness()
        self.B, self.D, self.N, self.env_offset = B, task_dim, capacity, env_offset
        self.map = np.array(list(range(task_dim)) if row_map is None else row_map, np.int32)
        N = capacity
        self.buf = dict(task=np.zeros(task_dim * N + GUARD, np.float32), ep_return=np.zeros(N + GUARD, np.float64), ep_len=np.zeros(N + GUARD, np.int32),
                        flags=np.zeros(N + GUARD, np.uint8), env=np.zeros(N + GUARD, np.int64), step=np.zeros(N + GUARD, np.int64))
        self.guard = {k: (np.arange(GUARD) + 0x5A).astype(v.dtype) for k, v in self.buf.items()}
        for k, v in self.buf.items():
            v[-GUARD:] = self.guard[k]
        self.lane_return, self.lane_len = np.zeros(B, np.float64), np.zeros(B, np.int32)
        self.shadow = np.zeros((task_dim, B), np.float32)
        self.counts = np.zeros(self.L.el_host_blocks(B), np.int32)
        self.words = np.zeros(4, np.int64)
        self.sync(None, False, xi_full)                    # shadow = current task

    def _ptrs(self, xi, reward=None, done=None, truncated=None, mask=None):
        b = self.buf
        arrs = [b["task"], b["ep_return"], b["ep_len"], b["flags"], b["env"], b["step"], self.lane_return, self.lane_len, self.shadow, self.counts,
                self.words, xi, reward, done, truncated, mask]
        self._keep = arrs
        return (ctypes.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])

    def step(self, reward, done, truncated, xi_full):
        xi_full = np.ascontiguousarray(xi_full, np.float32)
        assert self.L.el_host_step(self._ptrs(xi_full, reward, done, truncated), self.B, self.env_offset, self.D, self.map.ctypes.data, self.N) == 0

    def sync(self, mask, restart, xi_full):
        xi_full = np.ascontiguousarray(xi_full, np.float32)
        assert self.L.el_host_sync(self._ptrs(xi_full, mask=mask), self.B, self.D, self.map.ctypes.data, int(restart)) == 0

    def read(self, clear=False):
        out = np.zeros(4, np.int64)
        self.L.el_host_read(self.words.ctypes.data, self.N, out.ctypes.data, int(clear))
        return tuple(int(v) for v in out)

    def table(self, full=False):
        n = self.N if full else min(self.read()[0], self.N)
        b = self.buf
        return dict(task=b["task"][:self.D * self.N].reshape(self.D, self.N)[:, :n].copy(), ep_return=b["ep_return"][:n].copy(), ep_len=b["ep_len"][:n].copy(),
                    flags=b["flags"][:n].copy(), env=b["env"][:n].copy(), step=b["step"][:n].copy())

    def assert_guards_untouched(self):
        for k, v in self.buf.items():
            assert_same_bits(v[-GUARD:], self.guard[k], "guard behind %s" % k)


def full_block(task, row_map, full_rows, fill=7.5):
    """the handle's full xi block holding `task` in the rows of the map (the other rows: a value no record may show)"""
    xi = np.full((full_rows, task.shape[1]), fill, np.float32)
    xi[np.asarray(row_map)] = task
    return xi


def assert_lanes_equal(host, ref, what):
    assert_same_bits(host.lane_return, ref.lane_return, what + " lane return")
    assert_same_bits(host.lane_len, ref.lane_len, what + " lane length")
    assert_same_bits(host.shadow, ref.shadow, what + " shadow task")


def run_both(B, task_dim, capacity, calls, row_map=None, full_rows=None, env_offset=0):
    row_map = list(range(task_dim)) if row_map is None else row_map
    full_rows = task_dim if full_rows is None else full_rows
    rng = np.random.default_rng(1000 + B)
    task0 = rng.uniform(0.5, 5.0, size=(task_dim, B)).astype(np.float32)
    host = HostLedger(B, task_dim, capacity, full_block(task0, row_map, full_rows), row_map, env_offset)
    ref = oracle.Ledger(B, task_dim, capacity, task0, env_offset)
    for c, s in enumerate(calls):
        host.step(s["reward"], s["done"], s["truncated"], full_block(s["task"], row_map, full_rows))
        ref.step(s["reward"], s["done"], s["truncated"], s["task"])
        assert host.read() == ref.read(), "counters after call %d" % c
    return host, ref


# ------------------------------------------------------------------------------------------------- the contract, every size
@pytest.mark.parametrize("B", SIZES)
def test_fields_equal_the_oracle_bit_for_bit(B):
    rng = np.random.default_rng(B)
    calls = oracle.synthetic_calls(rng, B, 4)
    assert not calls[4]["done"].any() and calls[7]["done"].all()
    host, ref = run_both(B, 4, 12 * B, calls, env_offset=1 << 33)     # a global index past 2^32 lands in the int64 field
    assert ref.read()[0] == sum(int((s["done"] != 0).sum()) for s in calls) and ref.read()[1] == 0 and ref.read()[2] == 12
    assert_tables_equal(host.table(full=True), ref.table(full=True), "B=%d" % B)
    assert_lanes_equal(host, ref, "B=%d" % B)
    host.assert_guards_untouched()
    t = ref.table()
    assert (np.diff(t["step"]) >= 0).all() and ((np.diff(t["env"]) > 0) | (np.diff(t["step"]) > 0)).all()    # call order, then env order
    if B > 2:
        assert np.isinf(t["ep_return"]).any()          # the +inf reward reached a record


def test_truncated_null_gives_zero_flags():
    B = 257
    calls = oracle.synthetic_calls(np.random.default_rng(3), B, 4)
    for s in calls:
        s["truncated"] = None
    host, ref = run_both(B, 4, 12 * B, calls)
    assert_tables_equal(host.table(), ref.table(), "no truncated buffer")
    assert not host.table()["flags"].any()


def test_overflow_keeps_the_earliest_records_and_counts_the_rest():
    B, N = 63, 100
    calls = oracle.synthetic_calls(np.random.default_rng(11), B, 4)
    host, ref = run_both(B, 4, N, calls)
    total = sum(int((s["done"] != 0).sum()) for s in calls)
    assert total > N and host.read() == (total, total - N, 12, N)
    assert_tables_equal(host.table(full=True), ref.table(full=True), "overflow")
    assert_lanes_equal(host, ref, "overflow")
    host.assert_guards_untouched()
    big, _ = run_both(B, 4, 12 * B, calls)                     # the kept records are the first N of the unbounded table
    for k, v in big.table().items():
        assert_same_bits(host.table()[k], v[..., :N], "first %d records, %s" % (N, k))


def test_reduced_row_map_of_the_unmodeled_hopper():
    B = 63
    calls = oracle.synthetic_calls(np.random.default_rng(5), B, 3)
    host, ref = run_both(B, 3, 12 * B, calls, row_map=HOPPER_UNMODELED_MAP, full_rows=4)
    assert_tables_equal(host.table(full=True), ref.table(full=True), "row map")
    assert_lanes_equal(host, ref, "row map")
    assert not (host.table()["task"] == np.float32(7.5)).any()     # the frozen row never shows


@pytest.mark.parametrize("restart", [False, True])
def test_sync_on_a_mask(restart):
    B = 257
    rng = np.random.default_rng(7)
    calls = oracle.synthetic_calls(rng, B, 4, calls=6)
    host, ref = run_both(B, 4, 12 * B, calls[:3])
    mask = (rng.random(B) < 0.4).astype(np.uint8)
    mask[mask != 0] = 3
    outside = rng.uniform(5.0, 9.0, size=(4, B)).astype(np.float32)     # a task set from outside
    host.sync(mask, restart, outside); ref.sync(mask, restart, outside)
    assert_lanes_equal(host, ref, "after sync")
    m = mask != 0
    assert (host.shadow[:, m] == outside[:, m]).all() and not (host.shadow[:, ~m] == outside[:, ~m]).any()
    assert ((host.lane_len[m] == 0).all() and (host.lane_return[m] == 0).all()) if restart else (host.lane_len[m] > 0).any()
    for s in calls[3:]:
        host.step(s["reward"], s["done"], s["truncated"], s["task"]); ref.step(s["reward"], s["done"], s["truncated"], s["task"])
    assert host.read() == ref.read()
    assert_tables_equal(host.table(full=True), ref.table(full=True), "after sync")
    host.sync(None, True, outside); ref.sync(None, True, outside)       # no mask: every lane
    assert_lanes_equal(host, ref, "after a full sync")
    assert not host.lane_len.any() and (host.shadow == outside).all()


def test_clear_restarts_the_slots_and_keeps_the_serial():
    B = 64
    calls = oracle.synthetic_calls(np.random.default_rng(9), B, 4)
    host, ref = run_both(B, 4, 12 * B, calls[:5])
    before = host.read(clear=True)
    assert before == ref.read(clear=True) and before[2] == 5
    assert host.read() == (0, 0, 5, 12 * B)
    for s in calls[5:]:
        host.step(s["reward"], s["done"], s["truncated"], s["task"]); ref.step(s["reward"], s["done"], s["truncated"], s["task"])
    assert host.read() == ref.read() and host.read()[2] == 12
    t = host.table()
    assert_tables_equal(t, ref.table(), "after clear")
    assert t["step"][0] == 5 and len(t["step"]) == host.read()[0]      # slot 0 again, serial 5 onwards (call 4 had no done lane)


def test_host_functions_stay_inside_exactly_sized_buffers_under_sanitizers(tmp_path):
    """tests/host_harness/eplog_sanitize_main.cpp: a program of its own (the sanitizer runtimes are linked into it; nothing is preloaded)"""
    exe = str(tmp_path / "eplog_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(HARNESS, "eplog_sanitize_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "B=4097 N=100 total=" in run.stdout and "dropped=0" in run.stdout


# ------------------------------------------------------------------------------------------------- merge_logs (pure numpy / torch)
def _drained(ledger):
    t = ledger.table()
    return dict(task=t["task"].T.copy(), episode_return=t["ep_return"], episode_length=t["ep_len"], truncated=(t["flags"] & 1).astype(bool), env=t["env"],
                step=t["step"], dropped=ledger.read()[1])


@pytest.mark.parametrize("split", [(64, 64), (1, 127)])
def test_merge_logs_of_shards_equals_the_unsharded_table(split):
    from random_envs_amd import merge_logs
    B, D = 128, 4
    rng = np.random.default_rng(21)
    calls = oracle.synthetic_calls(rng, B, D)
    task0 = rng.uniform(0.5, 5.0, size=(D, B)).astype(np.float32)
    whole = oracle.Ledger(B, D, 12 * B, task0)
    shards, lo = [], 0
    for n in split:
        shards.append((lo, lo + n, oracle.Ledger(n, D, 12 * B, task0[:, lo:lo + n], env_offset=lo))); lo += n
    for s in calls:
        whole.step(s["reward"], s["done"], s["truncated"], s["task"])
        for a, b, led in shards:
            led.step(s["reward"][a:b], s["done"][a:b], s["truncated"][a:b], s["task"][:, a:b])
    ref = _drained(whole)
    merged = merge_logs([_drained(led) for _, _, led in shards])
    assert merged["dropped"] == 0
    for k in ("task", "episode_return", "episode_length", "truncated", "env", "step"):
        assert_same_bits(merged[k], ref[k], "merged %s" % k)
    import torch
    as_t = lambda d: {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    merged_t = merge_logs([as_t(_drained(led)) for _, _, led in reversed(shards)])       # list order does not matter: (step, env) decides
    for k in ("task", "episode_return", "episode_length", "truncated", "env", "step"):
        assert isinstance(merged_t[k], torch.Tensor)
        assert_same_bits(merged_t[k].numpy(), ref[k], "merged tensors %s" % k)
