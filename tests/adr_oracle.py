"""Numpy / Python-int restatement of the automatic-domain-randomisation contract (include/rex.h, rex_adr_*) -- TEST ORACLE ONLY.

Written from the contract and not from csrc/adr.hpp: plain loops over lanes in env order, Python ints for counts, Python floats (fp64) for
the tallies in the stated order, ``np.float32`` for the box and the draws, the Philox words and rocRAND's uniform from tests/rng_oracle.py.
The oracle counts its own events, so a test can require that a run contained what it is meant to exercise."""
import numpy as np

import rng_oracle

ADR_SEED_SALT = 0xD1B54A32D192ED03
M64 = (1 << 64) - 1
BLOCK = 256                    # lanes per block partial
F = np.float32

assert ADR_SEED_SALT != rng_oracle.SAMPLE_SEED_SALT


class Box:
    """``act``: the active task indices.  ``delta``, ``lim_lo``, ``lim_hi``, ``centre``, ``init_lo``, ``init_hi``: [d] float32 by task index.
    ``task``: the lanes' current task [d, B] float32 (rows in rex_get_task's order); assign writes into it."""

    def __init__(self, B, d, act, p_b, m, t_lo, t_hi, delta, lim_lo, lim_hi, centre, init_lo, init_hi, seed, task, env_offset=0):
        f = lambda x: np.array(x, dtype=F).reshape(d).copy()
        self.B, self.d, self.act, self.J = int(B), int(d), [int(a) for a in act], 2 * len(act)
        self.p_b, self.m, self.t_lo, self.t_hi = F(p_b), int(m), float(t_lo), float(t_hi)
        self.delta, self.lim_lo, self.lim_hi, self.centre = f(delta), f(lim_lo), f(lim_hi), f(centre)
        self.lo, self.hi = f(init_lo), f(init_hi)
        self.key, self.env_offset = (int(seed) ^ ADR_SEED_SALT) & M64, int(env_offset)
        J = self.J
        self.n, self.s = [0] * J, [0.0] * J
        self.expanded, self.shrunk, self.held = [0] * J, [0] * J, [0] * J
        self.ret = np.zeros(self.B, np.float64)
        self.len = np.zeros(self.B, np.int32)
        self.bnd = np.full(self.B, -1, np.int32)
        self.ep = np.zeros(self.B, np.uint32)
        self.mask = np.zeros(self.B, np.uint8)
        self.task = np.array(task, dtype=F).reshape(self.d, self.B).copy()
        # the oracle's own events
        self.events = dict(expand=0, shrink=0, hold=0, limit_clamp=0, centre_clamp=0, max_arrival=0, calls_without_done=0, boundary_episodes=0,
                           dropped_boundary_episodes=0, nan_means=0)
        self.tallied = []          # (call, lane, boundary, return) of every contribution, in the order it entered
        self.assigned = []         # (call, lane, task [d] copy, bnd) of every assignment
        self.calls = 0

    # ------------------------------------------------------------------ record
    def record(self, reward, done, apply=True):
        reward, done = np.asarray(reward, F), np.asarray(done)
        J = self.J
        blocks = (self.B + BLOCK - 1) // BLOCK
        P = [[(0, 0.0)] * J for _ in range(blocks)]
        arrivals = [0] * J
        with np.errstate(all="ignore"):
            for b in range(blocks):
                cnt, sm = [0] * J, [0.0] * J
                for i in range(b * BLOCK, min(self.B, (b + 1) * BLOCK)):
                    self.ret[i] = self.ret[i] + np.float64(reward[i])
                    self.len[i] += 1
                    a = int(self.bnd[i])
                    if done[i] != 0 and a >= 0:
                        cnt[a] += 1
                        sm[a] = sm[a] + float(self.ret[i])
                        arrivals[a] += 1
                        self.tallied.append((self.calls, i, a, float(self.ret[i])))
                P[b] = list(zip(cnt, sm))
        self.events["max_arrival"] = max(self.events["max_arrival"], max(arrivals))
        if not (done != 0).any():
            self.events["calls_without_done"] += 1
        self._fold(P, apply)
        for i in range(self.B):
            if done[i] != 0:
                self._assign(i)
                self.mask[i] = 1
            else:
                self.mask[i] = 0
        self.calls += 1

    def update(self):
        self._fold([], True)

    def _fold(self, P, apply):
        ev = self.events
        for a in range(self.J):
            for row in P:
                c, sm = row[a]
                if c > 0:
                    self.n[a] += c
                    self.s[a] = self.s[a] + sm
            if apply and self.n[a] >= self.m:
                mean = self.s[a] / float(self.n[a])
                k, upper = self.act[a >> 1], a & 1
                dl = self.delta[k]
                if mean >= self.t_hi:
                    if upper:
                        x = F(self.hi[k] + dl)
                        ev["limit_clamp"] += int(x > self.lim_hi[k])
                        self.hi[k] = min(self.lim_hi[k], x)
                    else:
                        x = F(self.lo[k] - dl)
                        ev["limit_clamp"] += int(x < self.lim_lo[k])
                        self.lo[k] = max(self.lim_lo[k], x)
                    self.expanded[a] += 1; ev["expand"] += 1
                elif mean <= self.t_lo:
                    if upper:
                        x = F(self.hi[k] - dl)
                        ev["centre_clamp"] += int(x < self.centre[k])
                        self.hi[k] = max(self.centre[k], x)
                    else:
                        x = F(self.lo[k] + dl)
                        ev["centre_clamp"] += int(x > self.centre[k])
                        self.lo[k] = min(self.centre[k], x)
                    self.shrunk[a] += 1; ev["shrink"] += 1
                else:
                    self.held[a] += 1; ev["hold"] += 1
                    ev["nan_means"] += int(mean != mean)
                self.n[a], self.s[a] = 0, 0.0

    # ------------------------------------------------------------------ assign
    def assign(self, mask=None):
        for i in range(self.B):
            on = mask is None or mask[i] != 0
            if on:
                if self.bnd[i] >= 0:
                    self.events["dropped_boundary_episodes"] += 1
                self._assign(i)
            self.mask[i] = 1 if on else 0

    def _assign(self, i):
        e = int(self.ep[i])
        self.ep[i] = np.uint32((e + 1) & 0xFFFFFFFF)
        subseq, off = self.env_offset + i, 64 * e
        u = lambda j: rng_oracle.uniform(rng_oracle.word(self.key, subseq, off + j))
        one = F(1.0)
        bnd = -1
        xi = np.zeros(self.d, F)
        for k in range(self.d):
            w = F(self.hi[k] - self.lo[k])
            f = F(one - u(4 + k))
            xi[k] = F(self.lo[k] + F(w * f))
        if F(one - u(0)) < self.p_b:
            a = min(int(F(F(one - u(1)) * F(self.J))), self.J - 1)
            k = self.act[a >> 1]
            xi[k] = self.hi[k] if a & 1 else self.lo[k]
            bnd = a
            self.events["boundary_episodes"] += 1
        self.task[:, i] = xi
        self.bnd[i] = bnd
        self.ret[i] = 0.0
        self.len[i] = 0
        self.assigned.append((self.calls, i, xi.copy(), bnd))

    # ------------------------------------------------------------------ views
    def state(self):
        return dict(lo=self.lo.copy(), hi=self.hi.copy(), n=np.array(self.n, np.int64), s=np.array(self.s, np.float64),
                    counters=np.array([self.expanded, self.shrunk, self.held], np.int64))

    def lane_state(self):
        return dict(ret=self.ret.copy(), len=self.len.copy(), bnd=self.bnd.copy(), ep=self.ep.copy())


def merge_tallies_reference(shards):
    """(n, s) of the ranks summed in rank order, in Python ints / floats"""
    J = len(shards[0][0])
    n, s = [0] * J, [0.0] * J
    for sn, ss in shards:
        for a in range(J):
            n[a] += int(sn[a])
            s[a] = s[a] + float(ss[a])
    return np.array(n, np.int64), np.array(s, np.float64)


def synthetic_calls(rng, B, calls=14, p_done=0.3):
    """`calls` record calls of caller tensors: rewards of a few units with awkward float32 patterns among them, done with probability p_done;
    call 4 has no done lane, call 7 every lane done.  (A NaN reward is placed by the test, on a lane it knows to be a boundary lane: a single
    NaN, because which of TWO NaNs an addition keeps is the hardware's choice, not the contract's.)"""
    out = []
    for c in range(calls):
        reward = rng.normal(loc=1.0, scale=2.0, size=B).astype(np.float32)
        reward[::7] = np.float32(-0.0)
        if B > 2:
            reward[1] = np.float32(1e-42)
        done = (rng.random(B) < p_done).astype(np.uint8)
        if c == 4:
            done[:] = 0
        if c == 7:
            done[:] = 1
        done[done != 0] = rng.integers(1, 256, size=int((done != 0).sum())).astype(np.uint8)   # any non-zero byte is "done"
        out.append(dict(reward=reward, done=done))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the synthetic scenario every implementation is driven through
# ------------------------------------------------------------------------------------------------------------------------------------
M_SCENARIO, T_LO, T_HI, SEED = 3, 0.0, 6.0, 20191016
# mean reward of each call: high (full tallies expand, until the limit clamps), low (they shrink, until the centre clamps), middling (they hold)
LOC = (3.0, 3.0, 3.0, 3.0, 3.0, -3.0, -3.0, -3.0, -3.0, -3.0, -3.0, 1.0, 1.0, 1.0)


def settings(centre, lim_lo, lim_hi, act, p_b=0.5):
    """Box arguments for a scenario over `centre` (the nominal task): zero-width start, a delta that reaches a limit in two moves"""
    centre, lim_lo, lim_hi = (np.asarray(x, F) for x in (centre, lim_lo, lim_hi))
    delta = (F(0.6) * np.minimum(centre - lim_lo, lim_hi - centre)).astype(F)
    delta[delta <= 0] = F(0.125)
    return dict(d=len(centre), act=list(act), p_b=p_b, m=M_SCENARIO, t_lo=T_LO, t_hi=T_HI, delta=delta, lim_lo=lim_lo, lim_hi=lim_hi, centre=centre,
                init_lo=centre.copy(), init_hi=centre.copy(), seed=SEED)


def snapshot(box):
    """state, lane state, task [d, B] and mask of an oracle Box or of anything with the same views"""
    out = dict(box.state())
    out.update(box.lane_state())
    out["task"] = np.array(box.task, np.float32).copy()
    return out


def assert_snapshots_equal(got, ref, what=""):
    for k in ("lo", "hi", "n", "s", "counters", "ret", "len", "bnd", "ep", "task"):
        assert_same_bits(got[k], ref[k], "%s %s" % (what, k))


def scenario(ref, B, seed):
    """Runs the oracle `ref` (a fresh Box) through the scenario and returns the list of operations and the oracle's snapshot behind each, to
    be replayed on an implementation with ``replay``: assign(all) | 14 records -- call 4 without a done lane, call 7 with every lane done, call 2 with a NaN reward on a boundary
    lane that finishes in it (when the oracle has one), call 5 as record(apply=False) + update() -- and a masked assign after call 9."""
    rng = np.random.default_rng(seed)
    ops, snaps = [("assign", None)], []
    ref.assign(None); snaps.append(snapshot(ref))
    for c, s in enumerate(synthetic_calls(rng, B)):
        reward = (s["reward"] + np.float32(LOC[c] - 1.0)).astype(np.float32)
        reward[::7] = np.float32(-0.0)
        done = s["done"]
        if c == 2:
            pinned = np.flatnonzero(ref.bnd >= 0)
            if len(pinned):
                i = int(pinned[len(pinned) // 2])
                reward[i] = np.float32(np.nan); done[i] = 1
        apply = c != 5
        ops.append(("record", reward, done, apply))
        ref.record(reward, done, apply); snaps.append(snapshot(ref))
        if not apply:
            ops.append(("update",)); ref.update(); snaps.append(snapshot(ref))
        if c == 9:
            mask = (rng.random(B) < 0.4).astype(np.uint8)
            mask[mask != 0] = 3
            ops.append(("assign", mask)); ref.assign(mask); snaps.append(snapshot(ref))
    return ops, snaps


def replay(impl, ops, after=None):
    """`ops` on anything with record(reward, done, apply) / update() / assign(mask); after(index, op) is called behind every operation"""
    for j, op in enumerate(ops):
        if op[0] == "record":
            impl.record(op[1], op[2], op[3])
        elif op[0] == "update":
            impl.update()
        else:
            impl.assign(op[1])
        if after:
            after(j, op)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, "%s: %s %s against %s %s" % (what, got.shape, got.dtype, ref.shape, ref.dtype)
    bad = bits(got) != bits(ref)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])
