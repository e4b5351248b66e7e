"""AutoDR: Automatic Domain Randomization (OpenAI et al. 2019, Algorithm 1) kept on the device.

ADR decides per EPISODE: an episode may pin one task dimension to a boundary of the current box ``[lo, hi]``, its return lands in that
boundary's buffer, a full buffer moves the boundary by ``delta`` (out when the mean return is >= ``t_high``, in when it is <=
``t_low``), and the next episode is drawn from the moved box.  With auto-reset on, the step launch has already restarted the finished
lanes, so a host spelling needs ``done.nonzero()`` -- a synchronisation -- after every step.  This layer takes in the step the env
just wrote in three HIP launches on the env's stream, without a synchronisation, atomics or host randomness (``rex_adr_*`` of
include/rex.h, csrc/adr.hpp), and stores the finished lanes' next task into the env itself.
"""
import ctypes

import numpy as np

from . import _native
from ._layer import Layer


def merge_tallies(tallies):
    """The ranks' boundary tallies -- a list of ``(n, s)``: ``n`` [J] int64, ``s`` [J] float64, in RANK ORDER -- summed in that
    order: ``n`` as integers, ``s`` as one fp64 addition per rank starting from the first rank's value.  Pure numpy on the CPU."""
    if not tallies:
        raise ValueError("merge_tallies: nothing to merge")
    n = np.array(tallies[0][0], dtype=np.int64).copy()
    s = np.array(tallies[0][1], dtype=np.float64).copy()
    with np.errstate(all="ignore"):
        for tn, ts in tallies[1:]:
            tn, ts = np.asarray(tn, np.int64), np.asarray(ts, np.float64)
            if tn.shape != n.shape or ts.shape != s.shape:
                raise ValueError("merge_tallies: tallies of different boundary counts")
            n = n + tn
            s = s + ts
    return n, s


class AutoDR(Layer):
    """``AutoDR(env, t_low, t_high, delta, ...)`` over a :class:`VecRandomEnv` (or a :class:`NormalizedVecRandomEnv`: it always
    reads the RAW reward buffer of the wrapped env) that runs with ``dr_training`` OFF and auto-reset on.

    ``dims``: the randomised task indices (default: all); ``delta``: a scalar or one value per task index; ``centre`` (default
    ``env.original_task``), ``init_low`` / ``init_high`` (default ``centre``: the paper's zero-width start) and ``limit_low`` /
    ``limit_high`` (default ``env.get_task_search_bounds()``, the box the step kernels are tested over): one value per task
    index.  Raises ``ValueError`` when the nominal task lies outside the limits.

    Making the object assigns nothing: call ``assign()`` once (after ``env.reset()``) to start every lane on a task of the box.
    Call order per step: ``env.step`` -> ``adr.record()`` -> (``log.record()``): an :class:`EpisodeLog` recorded AFTER this layer
    refreshes its shadow from the task stored here, so its records carry the task each episode ran under.  After ``env.reset()``
    or a masked reset: ``adr.assign(mask)``.  One AutoDR per env, for the env's lifetime (``rex_adr_enable`` is once per handle)."""

    def __init__(self, env, t_low, t_high, delta, p_boundary=0.5, buffer_size=240, dims=None, init_low=None, init_high=None, centre=None,
                 limit_low=None, limit_high=None, seed=0):
        super().__init__(env)
        base = self._base
        d = self.task_dim = int(base.task_dim)
        f = lambda x, name: self._vector(x, d, name)
        self.centre = f(base.original_task if centre is None else centre, "centre")
        lo, hi = base.get_task_search_bounds()
        self.limit_low, self.limit_high = f(lo if limit_low is None else limit_low, "limit_low"), f(hi if limit_high is None else limit_high, "limit_high")
        if not ((self.limit_low <= self.centre) & (self.centre <= self.limit_high)).all():
            raise ValueError("AutoDR: the nominal task (centre) lies outside the limits on task indices %s"
                             % np.flatnonzero(~((self.limit_low <= self.centre) & (self.centre <= self.limit_high))).tolist())
        init_lo, init_hi = f(self.centre if init_low is None else init_low, "init_low"), f(self.centre if init_high is None else init_high, "init_high")
        self.dims = np.arange(d, dtype=np.int32) if dims is None else np.asarray(dims, dtype=np.int32).reshape(-1)
        self.delta = f(np.full(d, delta, np.float32) if np.ndim(delta) == 0 else delta, "delta")
        self.n_boundaries = 2 * len(self.dims)
        self.t_low, self.t_high, self.p_boundary, self.buffer_size, self.seed = float(t_low), float(t_high), float(p_boundary), int(buffer_size), int(seed)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        cfg = _native.RexAdrConfig(len(self.dims), p(self.dims), self.p_boundary, self.buffer_size, self.t_low, self.t_high, p(self.delta),
                                   p(self.limit_low), p(self.limit_high), p(self.centre), p(init_lo), p(init_hi), self.seed & ((1 << 64) - 1))
        _native.check(self._L.rex_adr_enable(self._h, ctypes.byref(cfg)))
        self._clear_after_update = False

    @staticmethod
    def _vector(x, d, name):
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
        if a.size != d:
            raise ValueError("AutoDR: %s must have one value per task index (%d), got %d" % (name, d, a.size))
        return a

    # ------------------------------------------------------------------ per step
    def record(self, apply=True):
        """After ``env.step`` / ``env.step_soa``: take in the step the env just wrote (three launches, no synchronisation).
        ``apply=False`` tallies and assigns but moves no boundary (sharded runs: ``sync()`` then ``update()``)."""
        b = self._base
        self.record_buffers(b._reward, b._done, apply)

    def record_buffers(self, reward, done, apply=True):
        """The same over the caller's own ``reward`` [B] float32 and ``done`` [B] uint8 / bool device tensors (read on the env's
        stream: keep them unchanged until that work has run)."""
        t = self._torch
        self._check(reward, (self.batch,), (t.float32,), "reward")
        self._check(done, (self.batch,), (t.uint8, t.bool), "done")
        _native.check(self._L.rex_adr_record(self._h, self._p(reward), self._p(done), int(bool(apply)), self._stream()))

    def assign(self, mask=None):
        """The masked lanes (all when ``mask`` is None) start an episode on a fresh task of the box; a boundary episode in progress
        on them is dropped.  One launch, no synchronisation."""
        m = None
        if mask is not None:
            t = self._torch
            self._mask = t.as_tensor(mask).to(device=self.device, dtype=t.uint8).contiguous()   # alive until the launch has run
            if self._mask.numel() != self.batch:
                raise ValueError("AutoDR.assign: mask must have %d elements" % self.batch)
            m = self._p(self._mask)
        _native.check(self._L.rex_adr_assign(self._h, m, self._stream()))

    def update(self):
        """Every full tally moves its boundary now (one launch): after ``record(apply=False)`` and ``sync()``.  Behind a ``sync()``
        over a process group every rank but the first then clears its tallies (synchronises): what the update left below
        ``buffer_size`` is the group's, and the first rank carries it into the next ``sync()`` once."""
        _native.check(self._L.rex_adr_update(self._h, self._stream()))
        if self._clear_after_update:
            st = self.state()
            st["n"][:] = 0
            st["s"][:] = 0.0
            self.load_state(st)
            self._clear_after_update = False

    # ------------------------------------------------------------------ state
    def state(self):
        """Box, tallies and counters as numpy arrays (synchronises): ``lo``, ``hi`` [task_dim] float32; ``n`` [J] int64, ``s`` [J]
        float64; ``counters`` [3, J] int64 (expanded, shrunk, held).  Boundary ``a`` is dimension ``dims[a >> 1]``, side ``a & 1``."""
        d, J = self.task_dim, self.n_boundaries
        out = dict(lo=np.zeros(d, np.float32), hi=np.zeros(d, np.float32), n=np.zeros(J, np.int64), s=np.zeros(J, np.float64),
                   counters=np.zeros((3, J), np.int64))
        _native.check(self._L.rex_adr_get_state(self._h, *[ctypes.c_void_p(out[k].ctypes.data) for k in ("lo", "hi", "n", "s", "counters")]))
        return out

    def load_state(self, st):
        d, J = self.task_dim, self.n_boundaries
        a = [np.ascontiguousarray(st["lo"], np.float32), np.ascontiguousarray(st["hi"], np.float32), np.ascontiguousarray(st["n"], np.int64),
             np.ascontiguousarray(st["s"], np.float64), np.ascontiguousarray(st["counters"], np.int64)]
        if [x.size for x in a] != [d, d, J, J, 3 * J]:
            raise ValueError("AutoDR.load_state: state of another task or another set of dims")
        _native.check(self._L.rex_adr_set_state(self._h, *[ctypes.c_void_p(x.ctypes.data) for x in a]))

    def box(self):
        """``(lo, hi, entropy)``: the box and ``mean(log(hi - lo))`` over the active dimensions with ``hi > lo`` (``-inf`` when
        none has opened yet).  Synchronises."""
        st = self.state()
        w = (st["hi"].astype(np.float64) - st["lo"].astype(np.float64))[self.dims]
        w = w[w > 0]
        return st["lo"], st["hi"], float(np.mean(np.log(w))) if w.size else float("-inf")

    def lane_state(self):
        """Per-lane device state: ``ret`` (float64), ``len`` (int32), ``bnd`` (int32: -1 or the boundary), ``ep`` (the uint32
        assignment count of the lane, as the int32 tensor of the same bits)."""
        t, B, dev = self._torch, self.batch, self.device
        out = dict(ret=t.empty(B, dtype=t.float64, device=dev), len=t.empty(B, dtype=t.int32, device=dev), bnd=t.empty(B, dtype=t.int32, device=dev),
                   ep=t.empty(B, dtype=t.int32, device=dev))
        _native.check(self._L.rex_adr_get_lane_state(self._h, self._p(out["ret"]), self._p(out["len"]), self._p(out["bnd"]), self._p(out["ep"]), self._stream()))
        return out

    def load_lane_state(self, st):
        t, dev = self._torch, self.device
        keep = (t.as_tensor(st["ret"], dtype=t.float64, device=dev).contiguous(), t.as_tensor(st["len"], dtype=t.int32, device=dev).contiguous(),
                t.as_tensor(st["bnd"], dtype=t.int32, device=dev).contiguous(), t.as_tensor(st["ep"], dtype=t.int32, device=dev).contiguous())
        if any(k.numel() != self.batch for k in keep):
            raise ValueError("AutoDR.load_lane_state: state of another batch")
        self._lane_in = keep                        # alive until the stream-ordered copies have run
        _native.check(self._L.rex_adr_set_lane_state(self._h, *[self._p(k) for k in keep], self._stream()))

    # ------------------------------------------------------------------ sharded runs
    def sync(self, group=None):
        """Index-sharded ranks: all-gather every rank's ``(n, s)`` over ``torch.distributed`` and load their sum in rank order
        (:func:`merge_tallies`) on every rank, so a following ``update()`` moves every rank's box identically.  Without an
        initialised process group it is the identity.  Synchronises."""
        import torch.distributed as dist
        t = self._torch
        st = self.state()
        if not (dist.is_available() and dist.is_initialized()):
            return st
        J = self.n_boundaries
        flat = t.as_tensor(np.concatenate([st["n"].view(np.float64), st["s"]]))     # the counts travel as their bits
        if dist.get_backend(group) == "nccl":
            flat = flat.to(self.device)
        parts = [t.empty_like(flat) for _ in range(dist.get_world_size(group))]
        dist.all_gather(parts, flat, group=group)
        each = []
        for p in parts:
            a = p.cpu().numpy()
            each.append((a[:J].view(np.int64), a[J:]))
        st["n"], st["s"] = merge_tallies(each)
        self.load_state(st)
        self._clear_after_update = dist.get_rank(group) != 0
        return st
