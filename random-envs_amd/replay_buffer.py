"""ReplayBuffer: the off-policy replay buffer on the device.

The layer every off-policy loop (SAC, TD3, DDPG, and every domain-randomisation loop that reuses data across distribution
updates) places above ``step()`` -- stable-baselines3's ``ReplayBuffer`` -- over tensors this object owns.  Storage is a ring
of ``n_slots`` time slots over the env's batch, TRANSITION-MAJOR (``obs`` / ``next_obs [T, B, obs_dim]``, ``action
[T, B, act_dim]``, ``reward`` / ``done`` / ``timeout [T, B]``): one HIP launch transposes a step out of the SoA buffers
``step_soa_full`` returns (terminal observations go into ``next_obs`` on the finished lanes), one launch draws the ids of a
minibatch on the device (Philox4x32-10, no host randomness, no synchronisation) and copies the whole rows into the row-major
``[n, dim]`` layout a network reads, normalised with the running statistics of a ``NormalizedVecRandomEnv`` on request
(``rex_rbuf_*`` of include/rex.h, csrc/replay_buffer.hpp).  ``sample_nstep`` / ``gather_nstep`` form an n-step return behind every id
in the same single launch (csrc/nstep_replay.hpp); ``sample_seq`` / ``gather_seq`` copy a window of consecutive steps behind every id,
padded and masked, in one launch too (csrc/seq_replay.hpp).
"""
import ctypes

from . import _native
from ._layer import Layer

_FIELDS = ("obs", "next_obs", "action", "reward", "done", "timeout")


class ReplayBuffer(Layer):
    """``ReplayBuffer(env, n_slots, seed=0)`` over a :class:`VecRandomEnv` or a :class:`NormalizedVecRandomEnv`; it holds
    ``n_slots * env.batch`` transitions."""

    def __init__(self, env, n_slots, seed=0):
        import torch
        super().__init__(env)
        base = self._base
        self._normalized = base is not env
        self.n_slots, self.seed = int(n_slots), int(seed) & 0xFFFFFFFFFFFFFFFF
        if self.n_slots <= 0:
            raise ValueError("ReplayBuffer: n_slots must be > 0")
        _native.check(self._L.rex_rbuf_enable(self._h))
        T, B = self.n_slots, self.batch
        f32 = dict(dtype=torch.float32, device=self.device)
        self.obs, self.next_obs = torch.zeros(T, B, self.obs_dim, **f32), torch.zeros(T, B, self.obs_dim, **f32)
        self.action = torch.zeros(T, B, self.act_dim, dtype=torch.int32 if base.dims.discrete_action else torch.float32, device=self.device)
        self.reward = torch.zeros(T, B, **f32)
        self.done, self.timeout = torch.zeros(T, B, dtype=torch.uint8, device=self.device), torch.zeros(T, B, dtype=torch.uint8, device=self.device)
        self._desc = _native.RexRbufBuffers(*[getattr(self, k).data_ptr() for k in _FIELDS], T)
        self.pos, self.full, self.draws = 0, False, 0

    def _normalise_flag(self, normalize):
        return int(self._normalized if normalize is None else bool(normalize))

    def __len__(self):
        """Transitions stored."""
        return (self.n_slots if self.full else self.pos) * self.batch

    # ------------------------------------------------------------------ collect
    def add(self, obs_soa, action_soa, reward, done, next_obs_soa, terminal_obs_soa=None, truncated=None):
        """Store one transition per env in ONE launch: ``obs_soa`` [obs_dim, B] (the observation the action was computed
        from), ``action_soa`` [act_dim, B], ``reward`` [B] float32, ``done`` [B] uint8 or bool, ``next_obs_soa`` [obs_dim, B]
        (what the step returned, i.e. after the auto-reset).  With ``terminal_obs_soa`` [obs_dim, B] the finished lanes store
        it as their ``next_obs``; with ``truncated`` [B] the time-limit ends are kept apart, so ``sample`` returns ``done = 0``
        for them.  Store RAW values when sampling with ``normalize``.  The inputs are read on the env's stream: keep them
        unchanged until that work has run, as with ``step_soa``."""
        t = self._torch
        B, byte = self.batch, (t.uint8, t.bool)
        self._check(obs_soa, (self.obs_dim, B), (t.float32,), "obs_soa")
        self._check(action_soa, (self.act_dim, B), (self.action.dtype,), "action_soa")
        self._check(reward, (B,), (t.float32,), "reward")
        self._check(done, (B,), byte, "done")
        self._check(next_obs_soa, (self.obs_dim, B), (t.float32,), "next_obs_soa")
        if terminal_obs_soa is not None:
            self._check(terminal_obs_soa, (self.obs_dim, B), (t.float32,), "terminal_obs_soa")
        if truncated is not None:
            self._check(truncated, (B,), byte, "truncated")
        _native.check(self._L.rex_rbuf_add(self._h, ctypes.byref(self._desc), self.pos, self._p(obs_soa), self._p(action_soa), self._p(reward),
                                           self._p(done), self._p(next_obs_soa), self._p(terminal_obs_soa), self._p(truncated), self._stream()))
        self.pos += 1
        if self.pos == self.n_slots:
            self.pos, self.full = 0, True

    # ------------------------------------------------------------------ learn
    def _launch(self, n, index, window, normalize, per=None):
        """The one call site of the sample family.  ``index`` None: the ids are drawn (``draws`` goes up), uniformly, or by the priorities
        behind ``per`` (a :class:`PrioritizedReplayBuffer`'s description, by reference); else they are gathered.  ``window``: None, the
        ``(n_step, gamma)`` of an n-step return, or the int ``seq_len`` of a sequence.  Allocates and returns the output dict.  The
        pointers every entry point of a kind takes are formed once; each call below names the entry point's own extra outputs beside
        them, in the order of include/rex.h."""
        t, dev, p, L = self._torch, self.device, self._p, self._L
        f32 = t.float32
        seq = isinstance(window, int)
        obs_rows, rows = ((window + 1,), (window,)) if seq else ((), ())     # a sequence: [n, L + 1] observation rows, [n, L] of the rest
        obs = t.empty(n, *obs_rows, self.obs_dim, dtype=f32, device=dev)
        act = t.empty(n, *rows, self.act_dim, dtype=self.action.dtype, device=dev)
        rew, done = t.empty(n, *rows, dtype=f32, device=dev), t.empty(n, *rows, dtype=f32, device=dev)
        if seq:
            mask, length = t.empty(n, window, dtype=f32, device=dev), t.empty(n, dtype=t.int32, device=dev)
            out = {"obs": obs, "action": act, "reward": rew, "done": done, "mask": mask, "length": length}
            outs = (p(obs), p(act), p(rew), p(done), p(mask), p(length))
        else:
            nxt = t.empty(n, self.obs_dim, dtype=f32, device=dev)
            out = {"obs": obs, "next_obs": nxt, "action": act, "reward": rew, "done": done}
            five = (p(obs), p(nxt), p(act), p(rew), p(done))
        h, desc, norm, stream = self._h, ctypes.byref(self._desc), self._normalise_flag(normalize), self._stream()
        if index is None:
            ids = out["index"] = t.empty(n, dtype=t.int64, device=dev)
            size, seed, draw = self.n_slots if self.full else self.pos, self.seed, self.draws
            if per is not None:
                prob = out["prob"] = t.empty(n, dtype=f32, device=dev)
        if window is None:
            if index is not None:
                rc = L.rex_rbuf_gather(h, desc, p(index), n, norm, *five, stream)
            elif per is None:
                rc = L.rex_rbuf_sample(h, desc, size, n, seed, draw, norm, *five, p(ids), stream)
            else:
                rc = L.rex_per_sample(h, desc, per, n, seed, draw, norm, *five, p(ids), p(prob), stream)
        elif seq:
            head = self._head()
            if index is not None:
                rc = L.rex_rbuf_gather_seq(h, desc, p(index), n, head, window, norm, *outs, stream)
            elif per is None:
                rc = L.rex_rbuf_sample_seq(h, desc, size, head, n, seed, draw, window, norm, *outs, p(ids), stream)
            else:
                rc = L.rex_per_sample_seq(h, desc, per, n, head, seed, draw, window, norm, *outs, p(ids), p(prob), stream)
        else:
            head, n_step, gamma = self._head(), int(window[0]), float(window[1])
            disc = out["discount"] = t.empty(n, dtype=f32, device=dev)
            steps = out["steps"] = t.empty(n, dtype=t.int32, device=dev)
            if index is not None:
                rc = L.rex_rbuf_gather_nstep(h, desc, p(index), n, head, n_step, gamma, norm, *five, p(disc), p(steps), stream)
            elif per is None:
                rc = L.rex_rbuf_sample_nstep(h, desc, size, head, n, seed, draw, n_step, gamma, norm, *five, p(disc), p(steps), p(ids), stream)
            else:
                rc = L.rex_per_sample_nstep(h, desc, per, n, head, seed, draw, n_step, gamma, norm, *five, p(disc), p(steps), p(ids), p(prob), stream)
        _native.check(rc)
        if index is None:
            self.draws += 1
        else:
            out["index"] = index
        return out

    def sample(self, batch_size, normalize=None):
        """One minibatch of ``batch_size`` transitions drawn uniformly with replacement from those stored, in ONE launch and
        without a synchronisation: a dict of ``obs`` / ``next_obs`` [n, obs_dim], ``action`` [n, act_dim] (row-major),
        ``reward`` [n], ``done`` [n] float32 (``done and not timeout``) and ``index`` [n] int64 (``s = t * B + b``).  The ids are
        a function of (seed, number of the draw, fill level, batch, j).  ``normalize=None`` means "yes iff the env is a
        ``NormalizedVecRandomEnv``": observations and rewards then come back normalised with its running statistics as
        they stand."""
        if self.pos == 0 and not self.full:
            raise RuntimeError("ReplayBuffer.sample: the buffer is empty")
        return self._launch(int(batch_size), None, None, normalize)

    def gather(self, index, normalize=None):
        """The same launch for the caller's ids ``index`` (int64 on the device): prioritised schemes, tests.  An id outside
        ``[0, n_slots * batch)`` gives zeros and is counted (:meth:`bad_indices`)."""
        self._check_index(index)
        return self._launch(index.numel(), index, None, normalize)

    # ------------------------------------------------------------------ learn, n-step
    def _head(self):
        """The slot written most recently: where every n-step window stops at the latest."""
        return (self.pos - 1) % self.n_slots

    def sample_nstep(self, batch_size, n_step, gamma, normalize=None):
        """:meth:`sample` with an n-step return behind every id, still in ONE launch: the window of transition ``s`` follows its env
        through the ring for at most ``n_step`` (1 .. 32) steps and ends early at a done, a time limit or the newest slot.  ``obs`` and
        ``action`` are those of the first step, ``next_obs`` and ``done`` those of the last, ``reward`` is ``r_0 + gamma r_1 + ... +
        gamma^(m-1) r_(m-1)`` (fp64 sum, one rounding), ``discount`` [n] float32 is ``gamma^m`` -- what the target value is multiplied
        by -- and ``steps`` [n] int32 is ``m``.  The ids are those :meth:`sample` draws at the same draw number, and the two methods
        share that number.  With ``normalize`` the return is normalised once, as a reward is."""
        if self.pos == 0 and not self.full:
            raise RuntimeError("ReplayBuffer.sample_nstep: the buffer is empty")
        return self._launch(int(batch_size), None, (n_step, gamma), normalize)

    def gather_nstep(self, index, n_step, gamma, normalize=None):
        """The same launch for the caller's ids, as :meth:`gather` is to :meth:`sample`.  An id out of range gives zeros (``discount``
        and ``steps`` included) and is counted (:meth:`bad_indices`)."""
        self._check_index(index)
        return self._launch(index.numel(), index, (n_step, gamma), normalize)

    # ------------------------------------------------------------------ learn, sequences
    def sample_seq(self, batch_size, seq_len, normalize=None):
        """:meth:`sample` with a window of up to ``seq_len`` (1 .. 64) consecutive steps of the same env behind every id, still in ONE
        launch: what a recurrent or history-fed learner trains on.  The window follows the env through the ring and ends early at a
        done, a time limit or the newest slot (the rule of :meth:`sample_nstep`); ``length`` [n] int32 is its number of steps ``m``.
        Batch-first: ``obs`` [n, L + 1, obs_dim] holds the observations of the steps and, in row ``m``, the observation to bootstrap
        from (``obs[:, :-1]`` / ``obs[:, 1:]`` are obs / next_obs of every valid step); ``action`` [n, L, act_dim]; ``reward``, ``done``
        (``done and not timeout``) and ``mask`` (1 on the valid steps) [n, L] float32; ``index`` [n] int64.  Everything past a window's
        end is zero.  The ids are those :meth:`sample` draws at the same draw number, and the methods share that number.  With
        ``normalize`` the written observation rows and every reward are normalised as :meth:`sample` normalises them."""
        if self.pos == 0 and not self.full:
            raise RuntimeError("ReplayBuffer.sample_seq: the buffer is empty")
        return self._launch(int(batch_size), None, int(seq_len), normalize)

    def gather_seq(self, index, seq_len, normalize=None):
        """The same launch for the caller's ids, as :meth:`gather` is to :meth:`sample`.  An id out of range gives zeros (``length``
        included) and is counted (:meth:`bad_indices`)."""
        self._check_index(index)
        return self._launch(index.numel(), index, int(seq_len), normalize)

    def bad_indices(self, clear=True):
        """Ids out of range the gathers met since the last clearing read (their outputs are zeros).  Synchronises."""
        return self._read_counter(self._L.rex_rbuf_read_bad_indices, clear)

    # ------------------------------------------------------------------ state
    def state_dict(self):
        """Everything a resume needs: ``pos``, ``full``, ``seed``, ``draws`` and clones of the stored tensors.  A buffer restored
        from it continues the same sample stream."""
        d = dict(pos=self.pos, full=self.full, seed=self.seed, draws=self.draws)
        d.update({k: getattr(self, k).clone() for k in _FIELDS})
        return d

    def load_state_dict(self, state):
        for k in _FIELDS:
            src = self._torch.as_tensor(state[k])
            if tuple(src.shape) != tuple(getattr(self, k).shape):
                raise ValueError("ReplayBuffer.load_state_dict: %s has shape %s, expected %s" % (k, list(src.shape), list(getattr(self, k).shape)))
            getattr(self, k).copy_(src)
        self.pos, self.full, self.seed, self.draws = int(state["pos"]), bool(state["full"]), int(state["seed"]), int(state["draws"])

    def views(self):
        """The stored tensors (zero-copy): ``obs`` / ``next_obs`` [T, B, obs_dim], ``action`` [T, B, act_dim], the rest [T, B]."""
        return {k: getattr(self, k) for k in _FIELDS}
