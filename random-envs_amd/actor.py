"""DeviceActor: an MLP policy acting on the device in one launch -- both towers, the Gaussian draw, its log-probability and the value.

Every other part of an RL loop around ``step()`` is one or a few launches here; a torch ``MlpPolicy`` between two steps is about fifteen
eager launches for the usual two 64-wide towers.  This layer runs stable-baselines3's default continuous-action ``MlpPolicy`` (two
separate towers of up to three hidden layers of up to 64 units, ``tanh`` or ``relu``, a state-independent ``log_std``) as ONE HIP launch
on the env's stream (``rex_actor_act`` of include/rex.h, csrc/actor.hpp), without an allocation or a synchronisation.  Inference only:
the learner stays in torch on the SAME parameters -- the launch reads ``data_ptr()`` of the live tensors at every call, so an in-place
optimiser step is seen by the next ``act`` without a copy.  Only ``std = exp(log_std)`` is a copy of the layer's: call :meth:`refresh`
after the learner has moved ``log_std``.
"""
import ctypes

from . import _native
from ._layer import Layer

MAX_HIDDEN, MAX_WIDTH, MAX_IN = _native.ACTOR_MAX_HIDDEN, 64, 1024
ACTIVATIONS = {"tanh": 0, "relu": 1}


class DeviceActor(Layer):
    """``DeviceActor(env, pi=[(W, b), ...], vf=[(W, b), ...] or None, log_std=..., activation="tanh", seed=0, in_dim=None)`` over a
    :class:`VecRandomEnv` (either layout) or a :class:`NormalizedVecRandomEnv` with continuous actions.

    A tower is a list of ``(weight, bias)`` pairs, hidden layers first and the head last, each a contiguous float32 device tensor
    shaped as ``nn.Linear`` keeps them (``weight`` [out, in], ``bias`` [out]): one to three hidden layers of width 1..64, a ``pi``
    head of ``act_dim`` rows and a ``vf`` head of one row.  Either tower may be ``None``.  ``in_dim`` defaults to the env's
    ``obs_dim``; a flattened :class:`HistoryStack` window made contiguous is as legal an input.  The tensors are NOT copied: keep
    them alive and update them in place.

    ``act(obs)`` accepts what the env returned: a contiguous [B, in_dim] tensor (``row_major=True``), a contiguous [in_dim, B] one (the SoA
    buffers of ``step_soa``), or the [B, in_dim] transposed view of an SoA buffer that ``reset`` / ``step`` of the other envs return; the
    action comes back in the same layout, ready for ``step`` / ``step_soa``.  Actions are not clipped: the step kernels clamp ``ctrl`` themselves.
    The noise of call number ``draw`` for env ``i`` depends on ``(seed, env_offset + i, draw)`` only, so a run does not depend on
    how the batch is sharded."""

    def __init__(self, env, pi=None, vf=None, log_std=None, activation="tanh", seed=0, in_dim=None):
        import torch
        super().__init__(env)
        if self._base.dims.discrete_action:
            raise _native.RexError("DeviceActor: %s has discrete actions (the categorical head is out of scope)" % self._base.kind)
        if activation not in ACTIVATIONS:
            raise ValueError("DeviceActor: activation must be one of %s" % sorted(ACTIVATIONS))
        if pi is None and vf is None:
            raise ValueError("DeviceActor: at least one of pi and vf is required")
        self.activation, self.seed = activation, int(seed)
        self.in_dim = self.obs_dim if in_dim is None else int(in_dim)
        if not 1 <= self.in_dim <= MAX_IN:
            raise ValueError("DeviceActor: in_dim must be in [1, %d]" % MAX_IN)
        B, A, dev = self.batch, self.act_dim, self.device
        self._pi, self._vf = self._tower(pi, A, "pi"), self._tower(vf, 1, "vf")
        self.log_std = None
        if pi is not None:
            if log_std is None:
                raise ValueError("DeviceActor: pi needs log_std")
            self._check(log_std, (A,), (torch.float32,), "log_std")
            self.log_std = log_std
            self.std = torch.empty(A, dtype=torch.float32, device=dev)
            self.refresh()
        f32 = dict(dtype=torch.float32, device=dev)
        # outputs the actor owns: the action in both layouts (the one matching the input is written), logp, value, noise
        self._action = {True: torch.zeros(B, A, **f32), False: torch.zeros(A, B, **f32)} if pi is not None else None
        self._logp = torch.zeros(B, **f32) if pi is not None else None
        self._value = torch.zeros(B, **f32) if vf is not None else None
        self._noise = None
        self.draw = 0                      # calls of act() so far: the next call's draw number
        self._net = _native.RexActorNet(self.in_dim, ACTIVATIONS[activation],
                                        ctypes.pointer(self._pi[0]) if self._pi else None, ctypes.pointer(self._vf[0]) if self._vf else None,
                                        self._p(self.log_std) if pi is not None else None, self._p(self.std) if pi is not None else None,
                                        self.seed & ((1 << 64) - 1))
        self._net_vf = _native.RexActorNet(self.in_dim, ACTIVATIONS[activation], None, ctypes.pointer(self._vf[0]) if self._vf else None, None, None, 0)

    def _tower(self, layers, head_out, name):
        """(the ctypes description, the tensors it points into) of a list of (W, b) pairs, or None"""
        t = self._torch
        if layers is None:
            return None
        layers = [(W, b) for W, b in layers]
        n_hidden = len(layers) - 1
        if not 1 <= n_hidden <= MAX_HIDDEN:
            raise ValueError("DeviceActor: %s must have 1 to %d hidden layers and a head (got %d layers)" % (name, MAX_HIDDEN, len(layers)))
        desc = _native.RexActorTower()
        desc.n_hidden = n_hidden
        fan_in = self.in_dim
        for l, (W, b) in enumerate(layers):
            out = head_out if l == n_hidden else int(W.shape[0]) if W.dim() == 2 else -1
            if l < n_hidden and not 1 <= out <= MAX_WIDTH:
                raise ValueError("DeviceActor: %s layer %d must be 1 to %d units wide" % (name, l, MAX_WIDTH))
            self._check(W, (out, fan_in), (t.float32,), "%s weight %d" % (name, l))     # a non-contiguous parameter is an error, not a silent copy
            self._check(b, (out,), (t.float32,), "%s bias %d" % (name, l))
            desc.W[l], desc.b[l] = W.data_ptr(), b.data_ptr()
            if l < n_hidden:
                desc.width[l] = out
            fan_in = out
        return desc, layers

    @classmethod
    def from_policy(cls, env, policy, seed=0, in_dim=None):
        """From a stable-baselines3 ``ActorCriticPolicy`` (duck-typed: ``mlp_extractor.policy_net`` / ``value_net`` -- sequences of
        ``Linear`` modules and activations --, ``action_net``, ``value_net``, ``log_std``).  The live parameters are used, not copies."""
        def linears(seq, head):
            mods = [m for m in seq if hasattr(m, "weight") and hasattr(m, "bias")] + [head]
            return [(m.weight.data, m.bias.data) for m in mods]

        def activation_of(seq):
            names = {type(m).__name__.lower() for m in seq if not hasattr(m, "weight")}
            if len(names) != 1 or not names <= set(ACTIVATIONS):
                raise ValueError("DeviceActor.from_policy: the towers must use one activation out of %s (found %s)" % (sorted(ACTIVATIONS), sorted(names)))
            return names.pop()
        ext = policy.mlp_extractor
        act = activation_of(list(ext.policy_net) + list(ext.value_net))
        return cls(env, pi=linears(ext.policy_net, policy.action_net), vf=linears(ext.value_net, policy.value_net), log_std=policy.log_std.data,
                   activation=act, seed=seed, in_dim=in_dim)

    # ------------------------------------------------------------------ acting
    def refresh(self):
        """``std <- exp(log_std)`` (one torch launch): call it after the learner has moved ``log_std``."""
        if self.log_std is not None:
            self._torch.exp(self.log_std, out=self.std)

    def _layout(self, obs, who):
        """(the contiguous tensor the launch reads, rows, viewed): [B, in_dim] contiguous is row-major; [in_dim, B] contiguous is SoA; the
        [B, in_dim] transposed VIEW of an SoA buffer -- what ``reset`` / ``step`` of the SoA envs return -- is read as that buffer
        (``viewed``: the action goes back as the same kind of view).  A square contiguous input reads as row-major."""
        t = self._torch
        if not isinstance(obs, t.Tensor):
            raise ValueError("DeviceActor.%s: obs must be a device tensor" % who)
        B, D = self.batch, self.in_dim
        if obs.dim() == 2 and tuple(obs.shape) == (B, D) and not obs.is_contiguous() and obs.t().is_contiguous():
            obs, rows, viewed = obs.t(), False, True
        else:
            rows, viewed = tuple(obs.shape) != (D, B) or B == D, False
        self._check(obs, (B, D) if rows else (D, B), (t.float32,), "obs")
        return obs, rows, viewed

    def act(self, obs, deterministic=False, noise=False):
        """``(action, logp, value)`` for ``obs`` in tensors the actor owns (overwritten by the next call): ``action`` in the layout of
        ``obs``, ``logp`` and ``value`` [B] (``value`` is None without a ``vf`` tower).  One launch; the call takes draw number
        ``self.draw`` and advances it (a deterministic call draws nothing and advances it all the same).  ``noise=True`` also keeps the standard normals drawn in ``self.noise`` [B, act_dim]."""
        if self._pi is None:
            raise ValueError("DeviceActor.act: no pi tower (use value())")
        t = self._torch
        obs, rows, viewed = self._layout(obs, "act")
        if noise and self._noise is None:
            self._noise = t.zeros(self.batch, self.act_dim, dtype=t.float32, device=self.device)
        action = self._action[rows]
        _native.check(self._L.rex_actor_act(self._h, ctypes.byref(self._net), self._p(obs), int(rows), self.draw, int(bool(deterministic)),
                                            self._p(action), self._p(self._logp), self._p(self._value), self._p(self._noise) if noise else None,
                                            self._stream()))
        self.draw += 1
        return (action.t() if viewed else action), self._logp, self._value

    @property
    def noise(self):
        return self._noise

    def value(self, obs):
        """The ``vf`` tower alone on ``obs`` (the bootstrap call on ``terminal_observation``), into the owned ``value`` tensor."""
        if self._vf is None:
            raise ValueError("DeviceActor.value: no vf tower")
        obs, rows, _ = self._layout(obs, "value")
        _native.check(self._L.rex_actor_act(self._h, ctypes.byref(self._net_vf), self._p(obs), int(rows), 0, 1, None, None, self._p(self._value), None,
                                            self._stream()))
        return self._value

    # ------------------------------------------------------------------ state
    def state_dict(self):
        """What an exact resume needs besides the parameters (which belong to the caller): the draw counter and the seed."""
        return {"draw": self.draw, "seed": self.seed}

    def load_state_dict(self, state):
        self.draw, self.seed = int(state["draw"]), int(state["seed"])
        self._net.seed = self.seed & ((1 << 64) - 1)
