"""RolloutBuffer: the on-policy rollout buffer on the device.

The layer every on-policy loop places above ``step()`` -- stable-baselines3's ``RolloutBuffer`` -- over tensors this object
owns, in the SoA layout of the kernels (``obs [T, obs_dim, B]``, ``action [T, act_dim, B]``, the rest ``[T, B]``): one HIP
launch stores a step (time-limit bootstrap included), one computes GAE(lambda), two the advantage statistics, one gathers
a minibatch into the row-major ``[n, dim]`` layout a policy network reads (``rex_rollout_*`` of include/rex.h,
csrc/rollout.hpp).
"""
import ctypes

from . import _native
from ._layer import Layer


class RolloutBuffer(Layer):
    """``RolloutBuffer(env, n_steps)`` over a :class:`VecRandomEnv` or a :class:`NormalizedVecRandomEnv`."""

    def __init__(self, env, n_steps, gamma=0.99, gae_lambda=0.95):
        import torch
        super().__init__(env)
        base = self._base
        self.n_steps, self.gamma, self.gae_lambda = int(n_steps), float(gamma), float(gae_lambda)
        if self.n_steps <= 0:
            raise ValueError("RolloutBuffer: n_steps must be > 0")
        _native.check(self._L.rex_rollout_enable(self._h))
        T, B = self.n_steps, self.batch
        f32 = dict(dtype=torch.float32, device=self.device)
        self.obs = torch.zeros(T, self.obs_dim, B, **f32)
        self.action = torch.zeros(T, self.act_dim, B, dtype=torch.int32 if base.dims.discrete_action else torch.float32, device=self.device)
        self.reward, self.value, self.log_prob = torch.zeros(T, B, **f32), torch.zeros(T, B, **f32), torch.zeros(T, B, **f32)
        self.advantage, self.returns = torch.zeros(T, B, **f32), torch.zeros(T, B, **f32)
        self.done = torch.zeros(T, B, dtype=torch.uint8, device=self.device)
        self._desc = _native.RexRolloutBuffers(*[t.data_ptr() for t in (self.obs, self.action, self.reward, self.value, self.log_prob,
                                                                        self.advantage, self.returns, self.done)], T)
        self.pos = 0

    @property
    def full(self):
        return self.pos == self.n_steps

    def reset(self):
        self.pos = 0

    # ------------------------------------------------------------------ collect
    def add(self, obs_soa, action_soa, reward, done, value, log_prob, truncated=None, terminal_value=None):
        """Store one step in ONE launch: ``obs_soa`` [obs_dim, B] (the observation the action was computed from),
        ``action_soa`` [act_dim, B], ``reward`` / ``value`` / ``log_prob`` [B] float32, ``done`` [B] uint8 or bool.  With
        ``truncated`` [B] and ``terminal_value`` [B] (only together) the lanes that hit the time limit store
        ``reward + gamma * terminal_value`` (SB3's bootstrap).  The inputs are read on the env's stream: keep them unchanged
        until that work has run, as with ``step_soa``."""
        t = self._torch
        if self.pos >= self.n_steps:
            raise RuntimeError("RolloutBuffer.add: the buffer is full (%d steps); call reset()" % self.n_steps)
        if (truncated is None) != (terminal_value is None):
            raise ValueError("RolloutBuffer.add: truncated and terminal_value go together")
        B, byte = self.batch, (t.uint8, t.bool)
        self._check(obs_soa, (self.obs_dim, B), (t.float32,), "obs_soa")
        self._check(action_soa, (self.act_dim, B), (self.action.dtype,), "action_soa")
        for name, x in (("reward", reward), ("value", value), ("log_prob", log_prob)):
            self._check(x, (B,), (t.float32,), name)
        self._check(done, (B,), byte, "done")
        if truncated is not None:
            self._check(truncated, (B,), byte, "truncated")
            self._check(terminal_value, (B,), (t.float32,), "terminal_value")
        _native.check(self._L.rex_rollout_add(self._h, ctypes.byref(self._desc), self.pos, self._p(obs_soa), self._p(action_soa), self._p(reward),
                                              self._p(done), self._p(value), self._p(log_prob), self._p(truncated), self._p(terminal_value),
                                              self.gamma, self._stream()))
        self.pos += 1

    def compute_returns_and_advantage(self, last_value, normalize=False):
        """GAE(lambda) over the stored steps in one launch (``last_value`` [B]: the value of the observation after the last
        step; the final ``dones`` are the last stored ``done``), then the advantage statistics; ``normalize=True`` also
        rewrites ``advantage`` as ``(A - mean) / (std + 1e-8)``."""
        if not self.full:
            raise RuntimeError("RolloutBuffer: %d of %d steps stored" % (self.pos, self.n_steps))
        self._check(last_value, (self.batch,), (self._torch.float32,), "last_value")
        _native.check(self._L.rex_rollout_gae(self._h, ctypes.byref(self._desc), self._p(last_value), self.gamma, self.gae_lambda, self._stream()))
        _native.check(self._L.rex_rollout_adv_stats(self._h, ctypes.byref(self._desc), int(bool(normalize)), self._stream()))

    def advantage_stats(self):
        """n, mean, M2 (fp64) of the advantages as the last ``compute_returns_and_advantage`` found them (before it normalised
        them), their unbiased std, and the non-finite elements left out.  Synchronises."""
        out = (ctypes.c_double * 4)()
        _native.check(self._L.rex_rollout_get_adv_stats(self._h, out))
        n, mean, m2, bad = (float(v) for v in out)
        return dict(n=int(n), mean=mean, m2=m2, std=(m2 / (n - 1)) ** 0.5 if n > 1 else float("nan"), nonfinite=int(bad))

    def bad_indices(self, clear=True):
        """Sample ids outside [0, T * B) the gathers met since the last clearing read (their outputs are zeros).  Synchronises."""
        return self._read_counter(self._L.rex_rollout_read_bad_indices, clear)

    # ------------------------------------------------------------------ learn
    def gather(self, index):
        """One minibatch for the flat sample ids ``index`` (int64 on the device, ``s = t * B + b``) in one launch: a dict of
        ``obs`` [n, obs_dim], ``action`` [n, act_dim] (row-major) and ``advantage`` / ``returns`` / ``value`` / ``log_prob`` [n]."""
        t = self._torch
        self._check_index(index)
        n = index.numel()
        f32 = dict(dtype=t.float32, device=self.device)
        out = dict(obs=t.empty(n, self.obs_dim, **f32), action=t.empty(n, self.act_dim, dtype=self.action.dtype, device=self.device),
                   advantage=t.empty(n, **f32), returns=t.empty(n, **f32), value=t.empty(n, **f32), log_prob=t.empty(n, **f32))
        _native.check(self._L.rex_rollout_gather(self._h, ctypes.byref(self._desc), self._p(index), n, self._p(out["obs"]), self._p(out["action"]),
                                                 self._p(out["advantage"]), self._p(out["returns"]), self._p(out["value"]),
                                                 self._p(out["log_prob"]), self._stream()))
        out["index"] = index
        return out

    def permutation(self, generator=None, shuffle=True, tile=1):
        """The sample ids of one epoch: a ``torch.randperm`` on the device over whole runs of ``tile`` consecutive ids (a run
        is ``tile`` neighbouring envs of one step, so its reads are coalesced); a last, shorter run keeps its place in the
        shuffle."""
        t = self._torch
        N, k = self.n_steps * self.batch, int(tile)
        if k < 1:
            raise ValueError("RolloutBuffer: tile must be >= 1")
        runs = (N + k - 1) // k
        order = t.randperm(runs, generator=generator, device=self.device) if shuffle else t.arange(runs, device=self.device)
        if k == 1:
            return order
        ids = (order.unsqueeze(1) * k + t.arange(k, device=self.device).unsqueeze(0)).reshape(-1)
        return ids[ids < N].contiguous() if runs * k != N else ids

    def minibatches(self, batch_size, generator=None, shuffle=True, tile=1):
        """Yield the minibatches of one epoch (dicts as :meth:`gather` returns them), one gather launch each; the last,
        shorter one included.  ``generator``: a ``torch.Generator`` of the env's device."""
        if not self.full:
            raise RuntimeError("RolloutBuffer: %d of %d steps stored" % (self.pos, self.n_steps))
        ids = self.permutation(generator, shuffle, tile)
        for s in range(0, ids.numel(), int(batch_size)):
            yield self.gather(ids[s:s + int(batch_size)])

    def views(self):
        """The stored tensors as zero-copy ``[T, B, dim]`` / ``[T, B]`` views."""
        return dict(obs=self.obs.transpose(1, 2), action=self.action.transpose(1, 2), reward=self.reward, value=self.value, log_prob=self.log_prob,
                    advantage=self.advantage, returns=self.returns, done=self.done)
