"""NormalizedVecRandomEnv: running observation / reward normalisation and episode statistics on the device.

The layer every RL loop places directly above ``step()`` -- stable-baselines3's ``VecNormalize`` and ``VecMonitor`` -- as an
opt-in post-pass of two HIP launches per step on the caller's stream (``rex_norm_*`` of include/rex.h,
csrc/vecnorm.hpp).  The wrapped env's buffers keep the raw values (``get_original_obs`` / ``get_original_reward``); the
normalised values live in buffers of the wrapper.  The running statistics are a first-class state: ``stats`` /
``load_stats`` / ``save`` / ``load``, and ``merge_stats`` / ``sync_stats`` for index-sharded ranks.
"""
import ctypes

import numpy as np

from . import _native
from ._layer import _p

PRIOR_COUNT = 1e-4      # RunningMeanStd's initial pseudo-count (mean 0, var 1)


def _chan(a, b):
    """(count, mean, M2) of the union of two sets of rows, fp64, elementwise; rows with no samples on one side pass through."""
    na, ma, sa = a
    nb, mb, sb = b
    tot = na + nb
    safe = np.where(tot > 0, tot, 1.0)
    d = mb - ma
    return tot, ma + d * nb / safe, sa + sb + d * d * na * nb / safe


def _unchan(t, b):
    """Inverse of :func:`_chan`: what was merged INTO ``b`` to give ``t`` (rows where nothing was: count 0)."""
    nt, mt, st = t
    nb, mb, sb = b
    nd = nt - nb
    has = nd > 0
    safe = np.where(has, nd, 1.0)
    md = np.where(has, (nt * mt - nb * mb) / safe, mb)
    d = md - mb
    sd = st - sb - d * d * nb * nd / np.where(nt > 0, nt, 1.0)
    return np.where(has, nd, 0.0), md, np.where(has, np.maximum(sd, 0.0), 0.0)


def _triple(s):
    c = np.asarray(s["count"], dtype=np.float64)
    return c, np.asarray(s["mean"], dtype=np.float64), np.asarray(s["var"], dtype=np.float64) * c


def initial_stats(rows):
    """The statistic before any data: count 1e-4, mean 0, var 1 for every row."""
    return dict(count=np.full(rows, PRIOR_COUNT), mean=np.zeros(rows), var=np.ones(rows))


def merge_stats(stats_list, base=None):
    """Fixed-order Chan merge, in fp64, of the statistics of several shards that all started from ``base`` (default: the
    initial statistic): ``base + sum_k (stats_k - base)``, the shards taken in list order.  What every shard shares --
    the 1e-4 prior, or everything up to the last synchronisation -- is counted once, so the result equals the statistic
    of one unsharded stream over the same data up to fp64 rounding.  Pure numpy: usable on the CPU.
    Each entry is a dict of ``count`` / ``mean`` / ``var`` arrays of one length (rows)."""
    if not stats_list:
        raise ValueError("merge_stats: nothing to merge")
    rows = np.asarray(stats_list[0]["count"]).size
    b = _triple(initial_stats(rows) if base is None else base)
    acc = b
    for s in stats_list:
        if np.asarray(s["count"]).size != rows:
            raise ValueError("merge_stats: statistics of different sizes")
        acc = _chan(acc, _unchan(_triple(s), b))
    n, m, s2 = acc
    return dict(count=n, mean=m, var=s2 / n)


class NormalizedVecRandomEnv:
    """``VecNormalize`` + ``VecMonitor`` over a :class:`VecRandomEnv`, computed on the device.

    ``reset`` / ``step`` / ``step_soa`` return normalised observations and rewards; ``info["episode_return"]`` (float64)
    and ``info["episode_length"]`` (int32) are ``[batch]`` tensors valid where ``done``.  Everything else is delegated to
    the wrapped env."""

    def __init__(self, env, gamma=0.99, clip_obs=10.0, clip_reward=10.0, epsilon=1e-8, norm_obs=True, norm_reward=True, training=True):
        import torch
        if getattr(env, "row_major", False):
            raise ValueError("NormalizedVecRandomEnv needs an env in the default layout: its kernels read the env's SoA [obs_dim, batch] buffers, "
                             "which a row_major=True env's step() does not write")
        self._torch = torch
        self.env = env
        self.gamma, self.clip_obs, self.clip_reward, self.epsilon = float(gamma), float(clip_obs), float(clip_reward), float(epsilon)
        self.norm_obs, self.norm_reward = bool(norm_obs), bool(norm_reward)
        self._training = bool(training)
        self._L, self._h = env._L, env._h
        cfg = _native.RexNormConfig(self.gamma, self.epsilon, self.clip_obs, self.clip_reward, int(self.norm_obs), int(self.norm_reward),
                                    int(self._training))
        _native.check(self._L.rex_norm_enable(self._h, ctypes.byref(cfg)))
        B, D, dev = env.batch, env.dims.obs_dim, env.device
        self.rows = D + 1
        self._nobs = torch.zeros(D, B, dtype=torch.float32, device=dev)
        self._nterm = torch.zeros(D, B, dtype=torch.float32, device=dev)
        self._nreward = torch.zeros(B, dtype=torch.float32, device=dev)
        self._ep_return = torch.zeros(B, dtype=torch.float64, device=dev)
        self._ep_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self._base = initial_stats(self.rows)      # what every rank shared at the last sync_stats

    def __getattr__(self, name):                   # everything else: the wrapped env
        if name in ("env", "_torch"):
            raise AttributeError(name)
        return getattr(self.env, name)

    # ------------------------------------------------------------------ switches
    @property
    def training(self):
        return self._training

    @training.setter
    def training(self, flag):
        self.set_training(flag)

    def set_training(self, flag):
        """Freeze (False) or resume (True) the running statistics; the outputs follow the statistics either way."""
        self._training = bool(flag)
        _native.check(self._L.rex_norm_set_training(self._h, int(self._training)))

    # ------------------------------------------------------------------ gym protocol
    _p = staticmethod(_p)

    def reset(self, mask=None):
        env = self.env
        env.reset(mask)
        m = env._mask_ptr(mask)
        _native.check(self._L.rex_norm_reset(self._h, m, self._p(env._obs), self._p(self._nobs), env._stream()))
        return (self._nobs if self.norm_obs else env._obs).t()

    def _norm_step(self, with_term):
        env = self.env
        _native.check(self._L.rex_norm_step(
            self._h, self._p(env._obs), self._p(env._reward), self._p(env._done), self._p(env._term_obs) if with_term else None,
            self._p(self._nobs), self._p(self._nreward), self._p(self._nterm) if with_term else None,
            self._p(self._ep_return), self._p(self._ep_len), env._stream()))

    def step(self, action):
        _, _, done, info = self.env.step(action)
        self._norm_step(True)
        info = dict(info)
        if self.norm_obs:
            info["terminal_observation"] = self._nterm.t()
        info["episode_return"], info["episode_length"] = self._ep_return, self._ep_len
        return ((self._nobs if self.norm_obs else self.env._obs).t(), self._nreward if self.norm_reward else self.env._reward,
                done, info)

    def step_soa(self, action_soa):
        """Zero-copy hot path: the wrapped env's ``step_soa`` plus the two normalisation launches; returns the SoA normalised
        obs / reward and the done buffer (episode totals: :meth:`episode_buffers`, aggregates: :meth:`episode_summary`)."""
        _, _, done = self.env.step_soa(action_soa)
        self._norm_step(False)
        return (self._nobs if self.norm_obs else self.env._obs, self._nreward if self.norm_reward else self.env._reward, done)

    def get_original_obs(self):
        """The raw observations of the last reset / step, [batch, obs_dim] (the wrapped env's buffer)."""
        return self.env._obs.t()

    def get_original_reward(self):
        return self.env._reward

    def episode_buffers(self):
        """(episode_return float64 [batch], episode_length int32 [batch]): totals of the episode a lane finished last."""
        return self._ep_return, self._ep_len

    def episode_summary(self, clear=True):
        """Device aggregates since the last clearing read (synchronises): episodes finished, their mean return and length,
        and the non-finite input elements that were left out of the statistics."""
        out = (ctypes.c_double * 4)()
        _native.check(self._L.rex_norm_read_episodes(self._h, out, int(bool(clear))))
        n = int(out[0])
        return dict(episodes=n, return_sum=float(out[1]), length_sum=int(out[2]), mean_return=float(out[1]) / n if n else float("nan"),
                    mean_length=float(out[2]) / n if n else float("nan"), nonfinite=int(out[3]))

    # ------------------------------------------------------------------ the statistics as a state
    def stats(self):
        """dict of float64 numpy arrays ``count`` / ``mean`` / ``var`` with obs_dim + 1 rows (the last: the discounted return)."""
        buf = np.zeros(3 * self.rows, dtype=np.float64)
        _native.check(self._L.rex_norm_get_stats(self._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        R = self.rows
        return dict(count=buf[:R].copy(), mean=buf[R:2 * R].copy(), var=buf[2 * R:].copy())

    def load_stats(self, stats):
        buf = np.ascontiguousarray(np.concatenate([np.asarray(stats[k], dtype=np.float64).reshape(-1) for k in ("count", "mean", "var")]))
        if buf.size != 3 * self.rows:
            raise ValueError("load_stats: expected %d rows, got %d values" % (self.rows, buf.size))
        _native.check(self._L.rex_norm_set_stats(self._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))

    def lane_state(self):
        """Per-lane device state: discounted return, running episode return (float64) and episode length (int32)."""
        t, B, dev = self._torch, self.env.batch, self.env.device
        ret = t.empty(B, dtype=t.float64, device=dev); er = t.empty(B, dtype=t.float64, device=dev)
        el = t.empty(B, dtype=t.int32, device=dev)
        _native.check(self._L.rex_norm_get_lane_state(self._h, self._p(ret), self._p(er), self._p(el), self.env._stream()))
        return dict(ret=ret, ep_return=er, ep_len=el)

    def load_lane_state(self, st):
        t, dev = self._torch, self.env.device
        keep = (t.as_tensor(st["ret"], dtype=t.float64, device=dev).contiguous(), t.as_tensor(st["ep_return"], dtype=t.float64, device=dev).contiguous(),
                t.as_tensor(st["ep_len"], dtype=t.int32, device=dev).contiguous())
        assert all(k.numel() == self.env.batch for k in keep)
        self._lane_in = keep                        # alive until the stream-ordered copies have run
        _native.check(self._L.rex_norm_set_lane_state(self._h, self._p(keep[0]), self._p(keep[1]), self._p(keep[2]), self.env._stream()))

    def save(self, path):
        """Statistics, per-lane state and configuration to an ``.npz`` file."""
        s, ls = self.stats(), self.lane_state()
        if not str(path).endswith(".npz"):
            path = str(path) + ".npz"
        np.savez(path, count=s["count"], mean=s["mean"], var=s["var"], ret=ls["ret"].cpu().numpy(), ep_return=ls["ep_return"].cpu().numpy(),
                 ep_len=ls["ep_len"].cpu().numpy(), base_count=self._base["count"], base_mean=self._base["mean"], base_var=self._base["var"],
                 config=np.array([self.gamma, self.epsilon, self.clip_obs, self.clip_reward]))
        return path

    def load(self, path, lanes=True):
        """Inverse of :meth:`save`; ``lanes=False`` takes the statistics only (e.g. into an evaluation env of another batch)."""
        with np.load(path) as z:
            self.load_stats(z)
            self._base = dict(count=z["base_count"].copy(), mean=z["base_mean"].copy(), var=z["base_var"].copy())
            if lanes:
                self.load_lane_state(dict(ret=z["ret"], ep_return=z["ep_return"], ep_len=z["ep_len"]))

    def sync_stats(self, group=None):
        """Index-sharded ranks: all-gather every rank's statistics over ``torch.distributed``, merge them in rank order
        (:func:`merge_stats` against what the ranks shared at the last call) and load the result on every rank, which
        therefore all hold the same bits.  Without an initialised process group it is the identity."""
        import torch.distributed as dist
        t = self._torch
        mine = self.stats()
        if not (dist.is_available() and dist.is_initialized()):
            self._base = mine
            return mine
        flat = t.as_tensor(np.concatenate([mine["count"], mine["mean"], mine["var"]]))
        if dist.get_backend(group) == "nccl":
            flat = flat.to(self.env.device)
        parts = [t.empty_like(flat) for _ in range(dist.get_world_size(group))]
        dist.all_gather(parts, flat, group=group)
        R = self.rows
        each = []
        for p in parts:
            a = p.cpu().numpy()
            each.append(dict(count=a[:R], mean=a[R:2 * R], var=a[2 * R:]))
        merged = merge_stats(each, base=self._base)
        self.load_stats(merged)
        self._base = merged
        return merged
