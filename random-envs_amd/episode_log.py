"""EpisodeLog: the episode ledger -- which task got which return -- kept on the device.

Every domain-randomisation method consumes one datum per finished episode: the task xi it ran under and its return.  With
auto-reset and ``dr_training`` on, the step launch that finishes an episode has already stored the next episode's task, so the
pairing cannot be read back after ``step()``; and asking ``done.nonzero()`` after every step synchronises every step.  The
ledger appends (task, return, length, truncated, env, step) of every finished episode to tensors this object owns, in two HIP
launches per step on the env's stream and without a synchronisation (``rex_eplog_*`` of include/rex.h, csrc/eplog.hpp);
``drain()`` reads it whenever the outer loop wants it.
"""
import ctypes

import numpy as np

from . import _native
from ._layer import Layer

FIELDS = ("task", "episode_return", "episode_length", "truncated", "env", "step")


class EpisodeLog(Layer):
    """``EpisodeLog(env, capacity)`` over a :class:`VecRandomEnv` or a :class:`NormalizedVecRandomEnv` (it always reads the RAW
    reward buffer of the wrapped env).  Call order per step: ``env.step`` -> ``log.record()``; after anything that changes the
    task or restarts lanes from outside (``reset``, ``set_task``, ``set_random_task``, ``set_state``, ``set_full_state``):
    ``log.sync()``.  A task changed without a ``sync`` is recorded stale.

    ONE log per env: the handle holds one ledger, so making a second ``EpisodeLog`` over the same env re-registers the handle
    under the new object's tensors; every method of the displaced object then raises ``RuntimeError``.

    The launches read the tensors handed to ``record_buffers`` / ``sync`` / ``load_lane_state`` on the env's stream, which is
    torch's current stream of the device: this object keeps only the latest of them alive and otherwise relies on torch's
    stream-ordered caching allocator not handing a freed block to another stream before that work has run."""

    def __init__(self, env, capacity):
        import torch
        super().__init__(env)
        base = self._base
        self.capacity = int(capacity)
        if self.capacity <= 0:
            raise ValueError("EpisodeLog: capacity must be > 0")
        self.task_dim = int(base.task_dim)
        N, dev = self.capacity, self.device
        self.task = torch.zeros(self.task_dim, N, dtype=torch.float32, device=dev)
        self.ep_return = torch.zeros(N, dtype=torch.float64, device=dev)
        self.ep_len = torch.zeros(N, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.env_index = torch.zeros(N, dtype=torch.int64, device=dev)
        self.step_index = torch.zeros(N, dtype=torch.int64, device=dev)
        self._desc = _native.RexEplogBuffers(*[t.data_ptr() for t in (self.task, self.ep_return, self.ep_len, self.flags, self.env_index,
                                                                      self.step_index)], N)
        _native.check(self._L.rex_eplog_enable(self._h, ctypes.byref(self._desc)))
        base._episode_log = self                   # the handle's one ledger is this object's now

    def _mine(self):
        if getattr(self._base, "_episode_log", None) is not self:
            raise RuntimeError("EpisodeLog: another EpisodeLog was made over this env and owns its ledger now (one log per env)")

    # ------------------------------------------------------------------ per step
    def record(self, truncated=False):
        """After ``env.step`` / ``env.step_soa``: take in the step the env just wrote (two launches, no synchronisation).
        ``truncated=True`` also passes the env's ``TimeLimit.truncated`` buffer.  Only ``step`` writes that buffer --
        ``step_soa`` does NOT, and the env cannot tell which of the two ran last -- so the default passes no buffer (every
        ``truncated`` flag recorded is False): say ``record(truncated=True)`` after ``step``, never after ``step_soa``, where
        it would record the stale bits of the last ``step``."""
        b = self._base
        self.record_buffers(b._reward, b._done, b._trunc if truncated else None)

    def record_buffers(self, reward, done, truncated=None):
        """The same over the caller's own ``reward`` [B] float32, ``done`` [B] uint8 / bool and optional ``truncated`` [B]
        device tensors (read on the env's stream: keep them unchanged until that work has run)."""
        self._mine()
        t = self._torch
        for name, x, dt in (("reward", reward, (t.float32,)), ("done", done, (t.uint8, t.bool)), ("truncated", truncated, (t.uint8, t.bool))):
            if x is not None and (x.device != self.device or tuple(x.shape) != (self.batch,) or x.dtype not in dt or not x.is_contiguous()):
                raise ValueError("EpisodeLog: %s must be a contiguous [%d] %s tensor on %s" % (name, self.batch, dt[0], self.device))
        _native.check(self._L.rex_eplog_step(self._h, self._p(reward), self._p(done), self._p(truncated), self._stream()))

    def sync(self, mask=None, restart=True):
        """The masked lanes (all when ``mask`` is None) take the env's current task as the task of their episode; with
        ``restart`` their running return and length start again from 0.  One launch, no synchronisation."""
        self._mine()
        m = None
        if mask is not None:
            t = self._torch
            self._mask = t.as_tensor(mask).to(device=self.device, dtype=t.uint8).contiguous()   # alive until the launch has run
            if self._mask.numel() != self.batch:
                raise ValueError("EpisodeLog.sync: mask must have %d elements" % self.batch)
            m = self._p(self._mask)
        _native.check(self._L.rex_eplog_sync(self._h, m, int(bool(restart)), self._stream()))

    # ------------------------------------------------------------------ reading
    def read(self, clear=False):
        """The four counters (synchronises): ``total`` records since the last clear (dropped ones included), ``dropped`` =
        max(0, total - capacity), ``serial`` (record calls since the log was made) and ``capacity``."""
        self._mine()
        out = (ctypes.c_int64 * 4)()
        _native.check(self._L.rex_eplog_read(self._h, out, int(bool(clear))))
        return dict(total=int(out[0]), dropped=int(out[1]), serial=int(out[2]), capacity=int(out[3]))

    def drain(self, clear=True):
        """The first ``n = min(total, capacity)`` records as device tensors: ``task`` [n, task_dim] (a transposed view of the
        SoA slice, like ``get_task``), ``episode_return`` [n] float64, ``episode_length`` [n] int32, ``truncated`` [n] bool,
        ``env`` / ``step`` [n] int64, and ``dropped`` (int).  Synchronises.  ``clear=True`` empties the ledger (``step`` keeps
        counting) and returns COPIES of the slices, because the next records overwrite them; ``clear=False`` returns zero-copy
        views of the ledger's own tensors (``truncated`` excepted: it is computed from the flag bytes), valid until a later
        clearing drain lets records overwrite them."""
        c = self.read(clear=False)
        n = min(c["total"], c["capacity"])
        own = (lambda x: x.clone()) if clear else (lambda x: x)
        out = dict(task=own(self.task[:, :n]).t(), episode_return=own(self.ep_return[:n]), episode_length=own(self.ep_len[:n]),
                   truncated=(self.flags[:n] & 1).bool(), env=own(self.env_index[:n]), step=own(self.step_index[:n]), dropped=c["dropped"])
        if clear:
            self.read(clear=True)
        return out

    # ------------------------------------------------------------------ the per-lane state
    def lane_state(self):
        """Per-lane device state: running episode return (float64), length (int32) and the shadow task [task_dim, batch]."""
        self._mine()
        t, B, dev = self._torch, self.batch, self.device
        er, el = t.empty(B, dtype=t.float64, device=dev), t.empty(B, dtype=t.int32, device=dev)
        sh = t.empty(self.task_dim, B, dtype=t.float32, device=dev)
        _native.check(self._L.rex_eplog_get_lane_state(self._h, self._p(er), self._p(el), self._p(sh), self._stream()))
        return dict(ep_return=er, ep_len=el, shadow_task=sh)

    def load_lane_state(self, st):
        self._mine()
        t, dev = self._torch, self.device
        keep = (t.as_tensor(st["ep_return"], dtype=t.float64, device=dev).contiguous(), t.as_tensor(st["ep_len"], dtype=t.int32, device=dev).contiguous(),
                t.as_tensor(st["shadow_task"], dtype=t.float32, device=dev).contiguous())
        if keep[0].numel() != self.batch or keep[1].numel() != self.batch or tuple(keep[2].shape) != (self.task_dim, self.batch):
            raise ValueError("EpisodeLog.load_lane_state: state of another batch or task")
        self._lane_in = keep                        # alive until the stream-ordered copies have run
        _native.check(self._L.rex_eplog_set_lane_state(self._h, self._p(keep[0]), self._p(keep[1]), self._p(keep[2]), self._stream()))


def merge_logs(drained):
    """Merge what the shards of an index-sharded run drained (a list of dicts as :meth:`EpisodeLog.drain` returns them; torch
    tensors or numpy arrays): concatenated, then sorted STABLY by ``(step, env)``.  Shards stepped in lockstep (one ``record`` per
    step on each, none of them dropping records) merge into exactly the table one handle over the global batch would have
    written.  Pure numpy / torch on the CPU; returns CPU torch tensors when it was given tensors, numpy arrays otherwise."""
    if not drained:
        raise ValueError("merge_logs: nothing to merge")
    is_torch = any(hasattr(d["step"], "cpu") for d in drained)
    as_np = lambda x: x.detach().cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    cat = {k: np.concatenate([as_np(d[k]) for d in drained], axis=0) for k in FIELDS}
    order = np.lexsort((cat["env"], cat["step"]))            # last key first; lexsort is stable
    out = {k: np.ascontiguousarray(v[order]) for k, v in cat.items()}
    if is_torch:
        import torch
        out = {k: torch.from_numpy(v) for k, v in out.items()}
    out["dropped"] = int(sum(int(d.get("dropped", 0)) for d in drained))
    return out
