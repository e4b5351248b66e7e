"""HistoryStack: the acting-time history window -- the last K (observation, previous action) frames of every env -- on the device.

``ReplayBuffer.sample_seq`` gives a learner the windows a recurrent or history-fed network trains on; this is the other half of
that loop: at acting time the same network needs the last ``k`` frames of every env after every ``step()``.  The usual torch way
(shift, write, zero the finished lanes) is several torch kernels between two step launches and rewrites the whole history each
step.  Here the history is a MIRRORED RING in tensors this object owns: every env steps in lockstep, so one ring position serves
the batch; a push writes the new frame twice, ``k`` rows apart, and the window is a strided view that never needs a shift
(``rex_hist_*`` of include/rex.h, csrc/hist.hpp).  One HIP launch per push, on the env's stream, without a synchronisation.
"""
import ctypes

from . import _native
from ._layer import Layer

MAX_K = 64


class HistoryStack(Layer):
    """``HistoryStack(env, k, with_action=True)`` over a :class:`VecRandomEnv` (either layout) or a
    :class:`NormalizedVecRandomEnv`.  Call order: ``env.reset(mask)`` -> ``hist.reset(mask)``; ``env.step(a)`` (or
    ``step_soa_full``) -> ``hist.push(a)``; then ``hist.window()`` is what the policy reads for its next action.

    A frame is the observation row followed by the action that led to it, ``(obs_t, a_{t-1})``, ``W = obs_dim + act_dim`` wide
    (``obs_dim`` without action); a CartPole action is stored as ``float(a)``.  The first frame of an episode carries a zero action.
    Owned tensors: ``frames`` [B, 2k, W], ``length`` [B] int32 (valid frames of the window, saturating at ``k``) and
    ``terminal_window`` [B, k, W] -- on the lanes a push found done, the window the finished episode would have seen, ending with
    ``(terminal_observation, action)``: what a history-fed critic bootstraps a time-limit end from.  Its other rows keep what
    they held (the rule of ``terminal_observation`` in row-major mode).

    The launches read the tensors handed to ``push`` / ``push_buffers`` / ``reset`` on the env's stream, which is torch's current
    stream of the device: keep them unchanged until that work has run, as with ``step_soa``."""

    def __init__(self, env, k, with_action=True):
        import torch
        super().__init__(env)
        base = self._base
        self.k, self.with_action = int(k), bool(with_action)
        if not 1 <= self.k <= MAX_K:
            raise ValueError("HistoryStack: k must be in [1, %d]" % MAX_K)
        self._normalized = base is not env
        self._rows = bool(getattr(base, "row_major", False))
        self._discrete = bool(base.dims.discrete_action)
        self.width = self.obs_dim + (self.act_dim if self.with_action else 0)
        B, K, W, dev = self.batch, self.k, self.width, self.device
        self.frames = torch.empty(B, 2 * K, W, dtype=torch.float32, device=dev)
        self.length = torch.empty(B, dtype=torch.int32, device=dev)
        self.terminal_window = torch.zeros(B, K, W, dtype=torch.float32, device=dev)
        self._desc = _native.RexHistBuffers(self.frames.data_ptr(), self.length.data_ptr(), K, int(self.with_action))
        self.count = 0                              # ring positions taken so far (pushes, and a reset before the first of them): the next is count % k
        _native.check(self._L.rex_hist_init(self._h, ctypes.byref(self._desc), self._stream()))

    def _slot(self):
        """The slot of the most recent push."""
        return (self.count - 1) % self.k if self.count else 0

    def _action_shape(self, rows):
        B, A = self.batch, self.act_dim
        if self._discrete:
            return (B,) if rows else (A, B)
        return (B, A) if rows else (A, B)

    # ------------------------------------------------------------------ per step
    def reset(self, mask=None):
        """After ``env.reset(mask)``: the masked lanes (all when ``mask`` is None) start over -- their window is the observation the
        reset returned (with a zero action) under ``k - 1`` zero rows, ``length`` 1.  The other lanes and the ring position stay.
        One launch."""
        env, base, t = self.env, self._base, self._torch
        if self._rows:
            obs = base._obs_rows
        else:
            obs = env._nobs if self._normalized and env.norm_obs else base._obs
        m = None
        if mask is not None:
            self._mask = t.as_tensor(mask).to(device=self.device, dtype=t.uint8).contiguous()   # alive until the launch has run
            if self._mask.numel() != self.batch:
                raise ValueError("HistoryStack.reset: mask must have %d elements" % self.batch)
            m = self._p(self._mask)
        _native.check(self._L.rex_hist_reset(self._h, ctypes.byref(self._desc), self._slot(), m, self._p(obs), int(self._rows), self._stream()))
        self.count = max(self.count, 1)             # before the first push the reset's frame takes slot 0: the next push goes to slot 1

    def push(self, action=None):
        """After ``env.step`` / ``step_soa_full``: take in the step the env just wrote, in ONE launch.  It reads the buffers that
        call returned -- the env's SoA buffers, or its row-major ones under ``row_major=True``; over a ``NormalizedVecRandomEnv``
        with ``norm_obs`` the normalised observation buffers.  ``action`` is read by pointer when it is a contiguous device
        tensor of the layout's shape and dtype ([act_dim, B], or [B, act_dim] / CartPole [B] int32 in row-major mode); otherwise
        (``None``, numpy, another shape) the env's own action buffer is read.  ``step`` fills that buffer whenever it copies the
        action; ``step_soa`` / ``step_soa_full`` and a row-major ``step`` handed a fitting tensor read the caller's tensor by pointer
        and do NOT, so pass that same tensor here.  ``terminal_window`` is meaningful after calls that write the terminal
        observation (``step``, ``step_soa_full``)."""
        env, base, t = self.env, self._base, self._torch
        if self._rows:
            obs, done, term, own = base._obs_rows, base._done_b, base._term_rows, base._act_rows
        else:
            norm = self._normalized and env.norm_obs
            obs, term = (env._nobs, env._nterm) if norm else (base._obs, base._term_obs)
            done, own = base._done, base._act
        a = None
        if self.with_action:
            fits = (isinstance(action, t.Tensor) and action.device == own.device and action.dtype == own.dtype and action.is_contiguous()
                    and tuple(action.shape) == tuple(own.shape))
            a = action if fits else own
        self._launch(obs, a, done, term, self._rows)

    def push_buffers(self, obs, action, done, terminal_obs=None, rows=False):
        """The same over the caller's own device tensors: ``obs`` (and ``terminal_obs``) [obs_dim, B] float32 -- [B, obs_dim] with
        ``rows=True`` --, ``action`` [act_dim, B] / [B, act_dim] float32 (CartPole: int32, [B] with ``rows=True``; ignored without
        action), ``done`` [B] uint8 / bool or None.  Without ``terminal_obs`` the ``terminal_window`` is not written."""
        t = self._torch
        B, D = self.batch, self.obs_dim
        shape = (B, D) if rows else (D, B)
        self._check(obs, shape, (t.float32,), "obs")
        if self.with_action:
            if action is None:
                raise ValueError("HistoryStack: with_action needs an action")
            self._check(action, self._action_shape(rows), (t.int32 if self._discrete else t.float32,), "action")
        if done is not None:
            self._check(done, (B,), (t.uint8, t.bool), "done")
        if terminal_obs is not None:
            self._check(terminal_obs, shape, (t.float32,), "terminal_obs")
        self._launch(obs, action if self.with_action else None, done, terminal_obs, rows)

    def _launch(self, obs, action, done, term, rows):
        p = self._p
        _native.check(self._L.rex_hist_push(self._h, ctypes.byref(self._desc), self.count % self.k, p(obs), p(action), p(done), p(term),
                                            p(self.terminal_window) if term is not None else None, int(bool(rows)), self._stream()))
        self.count += 1

    # ------------------------------------------------------------------ reading
    def window(self):
        """The current window [B, k, W], oldest frame first, newest last, the first ``k - length`` rows zero: a ZERO-COPY strided view
        (strides ``(2kW, W, 1)``) of ``frames``.  IT MOVES EVERY PUSH: the view taken before a push shows, after it, the window
        shifted the wrong way round -- take it again after every ``push``, or use :meth:`materialize` for a fixed address."""
        c = self._slot()
        return self.frames[:, c + 1:c + self.k + 1, :]

    def flat(self):
        """:meth:`window` flattened to [B, k * W]: a zero-copy view too (strides ``(2kW, 1)``), and it moves every push as well."""
        c = self._slot()
        return self.frames.view(self.batch, 2 * self.k * self.width)[:, (c + 1) * self.width:(c + 1 + self.k) * self.width]

    def materialize(self, out=None):
        """The window copied into a contiguous [B, k, W] tensor (``out``, or a fresh one) in one launch: for callers that need a
        contiguous tensor or a fixed address (a captured graph's input)."""
        t = self._torch
        shape = (self.batch, self.k, self.width)
        if out is None:
            out = t.empty(*shape, dtype=t.float32, device=self.device)
        else:
            self._check(out, shape, (t.float32,), "out")
        _native.check(self._L.rex_hist_window(self._h, ctypes.byref(self._desc), self._slot(), self._p(out), self._stream()))
        return out

    def mask(self):
        """[B, k] float32, 1 on the valid rows of :meth:`window` (its last ``length`` rows).  Computed with torch from ``length``: off the
        hot path."""
        t = self._torch
        first = (self.k - self.length).unsqueeze(1)
        return (t.arange(self.k, device=self.device).unsqueeze(0) >= first).to(t.float32)

    # ------------------------------------------------------------------ state
    def state(self):
        """Everything an exact resume needs: clones of ``frames``, ``length`` and ``terminal_window``, and the push counter."""
        return dict(frames=self.frames.clone(), length=self.length.clone(), terminal_window=self.terminal_window.clone(), count=self.count)

    def load_state(self, state):
        t = self._torch
        for k in ("frames", "length", "terminal_window"):
            src = t.as_tensor(state[k])
            if tuple(src.shape) != tuple(getattr(self, k).shape):
                raise ValueError("HistoryStack.load_state: %s has shape %s, expected %s" % (k, list(src.shape), list(getattr(self, k).shape)))
            getattr(self, k).copy_(src)
        self.count = int(state["count"])
