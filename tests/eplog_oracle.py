"""Numpy restatement of the episode ledger's contract (include/rex.h, rex_eplog_*), written from the contract and not from the
kernels: plain loops over lanes in env order, python ints for the counters, numpy fp64 for the returns.  The tests hold the host
harness and the GPU to it bit for bit."""
import numpy as np

FIELDS = ("task", "ep_return", "ep_len", "flags", "env", "step")


class Ledger:
    """A ledger of capacity N over B lanes with task_dim rows.  ``cur_task`` arguments are [task_dim, B] float32: the lanes' CURRENT
    task at the time of the call (what rex_get_task would return)."""

    def __init__(self, B, task_dim, capacity, cur_task, env_offset=0):
        self.B, self.D, self.N, self.env_offset = int(B), int(task_dim), int(capacity), int(env_offset)
        self.task = np.zeros((self.D, self.N), np.float32)
        self.ep_return = np.zeros(self.N, np.float64)
        self.ep_len = np.zeros(self.N, np.int32)
        self.flags = np.zeros(self.N, np.uint8)
        self.env = np.zeros(self.N, np.int64)
        self.step_ = np.zeros(self.N, np.int64)
        self.lane_return = np.zeros(self.B, np.float64)
        self.lane_len = np.zeros(self.B, np.int32)
        self.shadow = np.array(cur_task, dtype=np.float32).reshape(self.D, self.B).copy()
        self.total, self.serial = 0, 0

    def step(self, reward, done, truncated, cur_task):
        reward, done = np.asarray(reward, np.float32), np.asarray(done)
        cur_task = np.asarray(cur_task, np.float32).reshape(self.D, self.B)
        r = 0
        with np.errstate(all="ignore"):
            for i in range(self.B):
                self.lane_return[i] = self.lane_return[i] + np.float64(reward[i])
                self.lane_len[i] += 1
                if done[i] != 0:
                    slot = self.total + r
                    if slot < self.N:
                        self.task[:, slot] = self.shadow[:, i]
                        self.ep_return[slot] = self.lane_return[i]
                        self.ep_len[slot] = self.lane_len[i]
                        self.flags[slot] = 1 if (truncated is not None and truncated[i] != 0) else 0
                        self.env[slot] = self.env_offset + i
                        self.step_[slot] = self.serial
                    r += 1
                    self.lane_return[i] = 0.0
                    self.lane_len[i] = 0
                    self.shadow[:, i] = cur_task[:, i]
        self.total += r
        self.serial += 1

    def sync(self, mask, restart, cur_task):
        cur_task = np.asarray(cur_task, np.float32).reshape(self.D, self.B)
        for i in range(self.B):
            if mask is None or mask[i] != 0:
                self.shadow[:, i] = cur_task[:, i]
                if restart:
                    self.lane_return[i] = 0.0
                    self.lane_len[i] = 0

    def read(self, clear=False):
        out = (self.total, max(0, self.total - self.N), self.serial, self.N)
        if clear:
            self.total = 0
        return out

    def table(self, full=False):
        """the six fields: the first min(total, N) records (or all N slots with full=True)"""
        n = self.N if full else min(self.total, self.N)
        return dict(task=self.task[:, :n].copy(), ep_return=self.ep_return[:n].copy(), ep_len=self.ep_len[:n].copy(), flags=self.flags[:n].copy(),
                    env=self.env[:n].copy(), step=self.step_[:n].copy())


def synthetic_calls(rng, B, task_dim, calls=12, p_done=0.3, p_trunc=0.5):
    """`calls` steps of caller tensors: rewards with awkward float32 patterns, done with probability p_done -- one call with no
    done lane and one with every lane done among them -- truncated flags, and a fresh task per call."""
    out = []
    for c in range(calls):
        reward = (rng.normal(size=B) * 10.0 ** rng.uniform(-3, 3, size=B)).astype(np.float32)
        reward[::7] = np.float32(-0.0)
        if B > 2:
            reward[1] = np.float32(1e-42); reward[-1] = np.float32(3e38)
            if c == 2:
                reward[2] = np.float32(np.inf)     # stays +inf in the lane's return until its episode ends (no NaN is formed: the
                                                   # bits of a GENERATED NaN are the hardware's choice, not the contract's)
        done = (rng.random(B) < p_done).astype(np.uint8)
        if c == 4:
            done[:] = 0
        if c == 7:
            done[:] = 1
        done[done != 0] = rng.integers(1, 256, size=int((done != 0).sum())).astype(np.uint8)   # any non-zero byte is "done"
        trunc = (rng.random(B) < p_trunc).astype(np.uint8)
        task = rng.uniform(0.5, 5.0, size=(task_dim, B)).astype(np.float32)
        out.append(dict(reward=reward, done=done, truncated=trunc, task=task))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, "%s: %s %s against %s %s" % (what, got.shape, got.dtype, ref.shape, ref.dtype)
    bad = bits(got) != bits(ref)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def assert_tables_equal(got, ref, what="", skip=()):
    for k in FIELDS:
        if k not in skip:
            assert_same_bits(got[k], ref[k], "%s %s" % (what, k))
