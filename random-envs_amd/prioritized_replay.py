"""PrioritizedReplayBuffer: proportional prioritised experience replay on the device.

Schaul et al. 2016 ("Prioritized Experience Replay") over the :class:`ReplayBuffer`'s storage: one float32 priority per stored
transition under a 64-ary fp64 sum tree, both tensors this object owns.  A new transition gets the largest priority seen, a minibatch
is drawn stratified and in proportion to the priorities in one HIP launch (Philox4x32-10, no host randomness, no synchronisation) and
gathered by the replay buffer's own launch, the learner's TD errors come back through :meth:`update_priorities` -- ``rex_per_*`` of
include/rex.h, csrc/priority_replay.hpp.  Every node of the tree is a serial fp64 sum in index order, so two runs agree bit for bit
and an incremental update equals a rebuild.
"""
import ctypes

from . import _native
from .replay_buffer import ReplayBuffer


class PrioritizedReplayBuffer(ReplayBuffer):
    """``PrioritizedReplayBuffer(env, n_slots, seed=0, alpha=0.6, beta=0.4, eps=1e-6)``: priorities ``(|td_error| + eps) ** alpha``,
    importance weights ``(len(self) * prob) ** -beta`` scaled to a maximum of 1."""

    def __init__(self, env, n_slots, seed=0, alpha=0.6, beta=0.4, eps=1e-6):
        super().__init__(env, n_slots, seed)
        t = self._torch
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)
        if self.alpha < 0 or self.beta < 0 or self.eps <= 0:
            raise ValueError("PrioritizedReplayBuffer: alpha and beta must be >= 0 and eps > 0")
        N = self.n_slots * self.batch
        n_tree = int(self._L.rex_per_tree_len(N))
        if n_tree < 0:
            raise ValueError(self._L.rex_last_error().decode())
        _native.check(self._L.rex_per_enable(self._h))
        self.priority = t.zeros(self.n_slots, self.batch, dtype=t.float32, device=self.device)
        self.tree = t.zeros(n_tree, dtype=t.float64, device=self.device)
        self.max_priority = t.ones(1, dtype=t.float32, device=self.device)
        self._per = _native.RexPerBuffers(self.priority.data_ptr(), self.tree.data_ptr(), self.max_priority.data_ptr(), self.n_slots)
        _native.check(self._L.rex_per_init(self._h, ctypes.byref(self._per), self._stream()))

    # ------------------------------------------------------------------ collect
    def add(self, obs_soa, action_soa, reward, done, next_obs_soa, terminal_obs_soa=None, truncated=None):
        """:meth:`ReplayBuffer.add`, then the slot's transitions take the largest priority seen so far and the tree follows."""
        slot = self.pos
        super().add(obs_soa, action_soa, reward, done, next_obs_soa, terminal_obs_soa, truncated)
        _native.check(self._L.rex_per_add(self._h, ctypes.byref(self._per), slot, self._stream()))

    # ------------------------------------------------------------------ learn
    def sample(self, batch_size, beta=None, normalize=None):
        """One minibatch drawn in proportion to the priorities, stratified (sample ``j`` comes from the ``j``-th of ``batch_size`` equal
        shares of the total), in two launches and without a synchronisation: the dict of :meth:`ReplayBuffer.sample` plus ``prob`` [n]
        float32 (priority / total) and ``weight`` [n] float32 = ``(len(self) * prob) ** -beta`` divided by its maximum over the
        minibatch.  The ids are a function of (seed, number of the draw, batch_size, j) and the priorities."""
        if len(self) == 0:
            raise RuntimeError("PrioritizedReplayBuffer.sample: the buffer is empty")
        return self._with_weight(self._launch(int(batch_size), None, None, normalize, ctypes.byref(self._per)), beta)

    def _with_weight(self, out, beta):
        t = self._torch
        b = self.beta if beta is None else float(beta)
        w = (out["prob"] * float(len(self))).pow(-b)
        w = t.where(out["prob"] > 0, w, t.zeros_like(w))          # an id of -1 (nothing to draw) weighs nothing
        out["weight"] = w / w.max().clamp_min(t.finfo(t.float32).tiny) if out["prob"].numel() else w
        return out

    def sample_nstep(self, batch_size, n_step, gamma, beta=None, normalize=None):
        """:meth:`sample` with the n-step return of :meth:`ReplayBuffer.sample_nstep` behind every id, in two launches: the same draw
        (``index`` and ``prob`` are those :meth:`sample` returns at the same draw number), then the n-step launch over its ids.  The dict
        of :meth:`sample` plus ``discount`` and ``steps``."""
        if len(self) == 0:
            raise RuntimeError("PrioritizedReplayBuffer.sample_nstep: the buffer is empty")
        return self._with_weight(self._launch(int(batch_size), None, (n_step, gamma), normalize, ctypes.byref(self._per)), beta)

    def sample_seq(self, batch_size, seq_len, beta=None, normalize=None):
        """:meth:`sample` with the sequence window of :meth:`ReplayBuffer.sample_seq` behind every id, in two launches: the same draw
        (``index`` and ``prob`` are those :meth:`sample` returns at the same draw number), then the sequence launch over its ids.  The
        dict of :meth:`ReplayBuffer.sample_seq` plus ``prob`` and ``weight``."""
        if len(self) == 0:
            raise RuntimeError("PrioritizedReplayBuffer.sample_seq: the buffer is empty")
        return self._with_weight(self._launch(int(batch_size), None, int(seq_len), normalize, ctypes.byref(self._per)), beta)

    def update_priorities(self, index, td_error):
        """Priority of transition ``index[j]`` <- ``(|td_error[j]| + eps) ** alpha`` (float32, computed by torch: a device ``powf`` would
        put a transcendental's rounding into the bit-exact contract).  ``index`` int64 [n] and ``td_error`` float32 [n] on the
        device.  Of several entries for one id the largest counts; ids out of range and values that are not finite are counted
        (:meth:`counters`)."""
        t = self._torch
        self._check_index(index)
        self._check(td_error, (index.numel(),), (t.float32,), "td_error")
        p = (td_error.abs() + self.eps).pow(self.alpha)
        _native.check(self._L.rex_per_update(self._h, ctypes.byref(self._per), self._p(index), self._p(p), index.numel(), self._stream()))

    def counters(self, clear=True):
        """``dict(invalid_priorities, bad_indices)`` met by :meth:`update_priorities` since the last clearing read.  Synchronises."""
        out = (ctypes.c_int64 * 2)()
        _native.check(self._L.rex_per_read_counters(self._h, out, int(bool(clear))))
        return dict(invalid_priorities=int(out[0]), bad_indices=int(out[1]))

    # ------------------------------------------------------------------ state
    def state_dict(self):
        """:meth:`ReplayBuffer.state_dict` plus ``priority``, ``max_priority`` and the three hyper-parameters; the tree is rebuilt on load."""
        d = super().state_dict()
        d.update(priority=self.priority.clone(), max_priority=self.max_priority.clone(), alpha=self.alpha, beta=self.beta, eps=self.eps)
        return d

    def load_state_dict(self, state):
        t = self._torch
        src = t.as_tensor(state["priority"])
        if tuple(src.shape) != tuple(self.priority.shape):
            raise ValueError("PrioritizedReplayBuffer.load_state_dict: priority has shape %s, expected %s" % (list(src.shape), list(self.priority.shape)))
        super().load_state_dict(state)
        self.priority.copy_(src)
        _native.check(self._L.rex_per_rebuild(self._h, ctypes.byref(self._per), self._stream()))
        self.max_priority.copy_(t.as_tensor(state["max_priority"]).reshape(1))      # what was SEEN, which the leaves alone may no longer show
        self.alpha, self.beta, self.eps = float(state["alpha"]), float(state["beta"]), float(state["eps"])
