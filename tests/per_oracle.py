"""numpy / Python-int restatement of the semantics of ``rex_per_*`` (include/rex.h) -- TEST ORACLE ONLY.

Proportional prioritised experience replay (Schaul et al. 2016): transition ``s`` is drawn with probability ``p_s / sum(p)``, a
minibatch of ``n`` is stratified (sample ``j`` falls into ``[j, j + 1) * total / n``), a new transition gets the largest priority
seen.  What this project adds is a definition that is exact to the bit:

* the sum tree is 64-ary; a node is the fp64 sum of its 64 children taken serially in index order from 0.0 (here: 64 column adds
  per level, each an IEEE fp64 addition of whole numpy columns, zeros past the end of a level);
* a new priority is valid when it is finite and > 0, anything else is stored as +0.0 and counted unless it is +-0; among several new
  values of one id in one call the largest is stored; an id outside ``[0, N)`` is counted and dropped with its value;
* sample ``j`` of draw ``draw`` uses words 2 and 3 of the Philox4x32-10 block of ``rex_rbuf_sample``:
  ``U = (u >> 11) * 2**-53``, ``x = (j + U) * (total / n)``; the descent walks a node's children with a running sum ``r`` from 0:
  ``x < r + v_k`` chooses ``k`` and continues below with ``x - r``; when nothing is chosen the last positive child is taken with
  ``x`` unchanged; when nothing is positive the id is -1;
* ``prob = float32(float64(p_id) / total)``.

Nothing here is shared with csrc/: the tree is rebuilt from the leaves after every change (the definition itself), Philox runs on numpy
uint64 columns (held to the Random123 known answers of replay_buffer_oracle.py by the tests) and the descent walks numpy columns.
"""
import numpy as np

FAN = 64
MAX_LEAVES = 2 ** 30
M32 = np.uint64(0xFFFFFFFF)


def level_sizes(N):
    """[n_1 .. n_D]"""
    N = int(N)
    if not 1 <= N <= MAX_LEAVES:
        raise ValueError("N outside [1, 2^30]")
    sizes = []
    while True:
        N = -(-N // FAN)
        sizes.append(N)
        if N == 1:
            return sizes


def tree_len(N):
    return sum(level_sizes(N))


def _children(values, nodes):
    """float64 [nodes, 64]: the children of every node of the level above ``values``, zeros past its end"""
    padded = np.zeros(nodes * FAN, np.float64)
    padded[:len(values)] = values
    return padded.reshape(nodes, FAN)


def build_levels(priority):
    """[level 1 .. level D] as float64 arrays, from float32 leaves"""
    below, levels = np.asarray(priority, np.float32).astype(np.float64), []
    for nodes in level_sizes(len(priority)):
        c = _children(below, nodes)
        s = np.zeros(nodes, np.float64)
        for k in range(FAN):
            s = s + c[:, k]
        levels.append(s)
        below = s
    return levels


def philox_words(seed, draw, j):
    """the four words of the block of samples ``j`` (an int array): uint64 arrays holding 32-bit values"""
    seed, draw = int(seed), int(draw)
    j = np.asarray(j, np.uint64)
    c0, c1 = j & M32, j >> np.uint64(32)
    c2, c3 = np.full_like(j, draw & 0xFFFFFFFF), np.full_like(j, (draw >> 32) & 0xFFFFFFFF)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def sample_x(seed, draw, n, total):
    """x of samples 0 .. n-1: float64 [n]"""
    j = np.arange(n, dtype=np.uint64)
    _, _, w2, w3 = philox_words(seed, draw, j)
    u = w2 | (w3 << np.uint64(32))
    U = (u >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return (j.astype(np.float64) + U) * (np.float64(total) / np.float64(n))


def _descend(children, x):
    """one level for all samples: (child or -1, x below)"""
    n = len(x)
    r, chosen, last, below = np.zeros(n), np.full(n, -1), np.full(n, -1), x.copy()
    for k in range(FAN):
        v = children[:, k]
        nxt = r + v
        walking = chosen < 0
        hit = walking & (x < nxt)
        below[hit] = x[hit] - r[hit]
        chosen[hit] = k
        walking &= ~hit
        r = np.where(walking, nxt, r)
        last[walking & (v > 0)] = k
    return np.where(chosen >= 0, chosen, last), below


def descent(priority, levels, x):
    """(ids int64, prob float32) of the descents that start at the root with ``x`` (float64 [n])"""
    priority = np.asarray(priority, np.float32)
    x = np.asarray(x, np.float64).copy()
    total = levels[-1][0]
    sizes = level_sizes(len(priority))
    node, ok = np.zeros(len(x), np.int64), np.ones(len(x), bool)
    for l in range(len(levels), 0, -1):
        below = levels[l - 2] if l >= 2 else priority.astype(np.float64)
        k, x = _descend(_children(below, sizes[l - 1])[node], x)
        ok &= k >= 0
        node = node * FAN + np.where(ok, k, 0)
    ids = np.where(ok, node, -1).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        prob = np.where(ok, (priority[np.where(ok, node, 0)].astype(np.float64) / total).astype(np.float32), np.float32(0)).astype(np.float32)
    return ids, prob


class Per:
    """The buffers of ``rex_per_buffers`` for T slots of B envs and the calls on them."""

    def __init__(self, T, B):
        self.T, self.B, self.N = int(T), int(B), int(T) * int(B)
        level_sizes(self.N)
        self.invalid = self.bad_ids = 0
        self.init()

    def _refresh(self):
        self.levels = build_levels(self.priority)

    @property
    def tree(self):
        return np.concatenate(self.levels)

    @property
    def total(self):
        return self.levels[-1][0]

    def init(self):
        self.priority = np.zeros(self.N, np.float32)
        self.max_priority = np.float32(1.0)
        self._refresh()

    def add(self, t):
        if not 0 <= t < self.T:
            raise ValueError("slot out of range")
        self.priority[t * self.B:(t + 1) * self.B] = self.max_priority
        self._refresh()

    def update(self, index, value):
        new = {}
        for s, v in zip(np.asarray(index, np.int64).tolist(), np.asarray(value, np.float32)):
            if not 0 <= s < self.N:
                self.bad_ids += 1
                continue
            if np.isfinite(v) and v > 0:
                self.max_priority = max(self.max_priority, v)
            else:
                self.invalid += int(not v == 0)          # NaN, inf and negative values; +-0 is a plain "never draw this"
                v = np.float32(0.0)
            new[s] = max(new.get(s, np.float32(0.0)), v)
        for s, v in new.items():
            self.priority[s] = v
        self._refresh()

    def rebuild(self):
        p = self.priority
        valid = p[np.isfinite(p) & (p > 0)]
        self.max_priority = np.float32(max(np.float32(1.0), valid.max())) if len(valid) else np.float32(1.0)
        self._refresh()

    def draw(self, n, seed, draw):
        """(ids int64 [n], prob float32 [n])"""
        return descent(self.priority, self.levels, sample_x(seed, draw, n, self.total))
