"""fp64 numpy restatement of the semantics of ``rex_norm_*`` (include/rex.h) -- TEST ORACLE ONLY.

It restates the published behaviour of stable-baselines3 (v2.x):

* ``RunningMeanStd`` (stable_baselines3/common/running_mean_std.py): ``__init__(epsilon=1e-4)`` gives mean 0, var 1,
  count 1e-4; ``update(arr)`` takes ``np.mean(arr, 0)``, ``np.var(arr, 0)`` (population) and ``arr.shape[0]`` into
  ``update_from_moments``: delta = bm - mean; tot = count + bc; mean += delta*bc/tot;
  M2 = var*count + bv*bc + delta^2*count*bc/tot; var = M2/tot.
* ``VecNormalize`` (stable_baselines3/common/vec_env/vec_normalize.py): ``step_wait`` updates ``obs_rms`` with the
  observations just returned (post auto-reset) when training, then ``_update_reward`` (returns = returns*gamma +
  reward; ret_rms.update(returns)) when training, normalises obs (``clip((obs - mean)/sqrt(var + eps), +-clip_obs)``),
  reward (``clip(reward/sqrt(ret_rms.var + eps), +-clip_reward)``) and ``infos[i]["terminal_observation"]``, and
  finally ``returns[dones] = 0``.  ``reset`` zeroes the returns and, when training, updates ``obs_rms`` with the reset
  observations.  Defaults: gamma 0.99, epsilon 1e-8, both clips 10.
* ``VecMonitor`` (stable_baselines3/common/vec_env/vec_monitor.py): ``episode_returns += rewards``,
  ``episode_lengths += 1``; a done env reports ``{"r": return, "l": length}`` and both restart from 0.

Additions of this project (include/rex.h): the statistics are kept per observation ROW with a count of their own, a
non-finite element is left out of its row's batch moments and counted, a masked reset updates with the masked lanes only,
and three aggregates (episodes, sum of returns, sum of lengths) accumulate between reads.  Arrays are SoA: obs is
``[obs_dim, B]``.
"""
import numpy as np


def update_from_moments(count, mean, var, bc, bm, bv):
    """RunningMeanStd.update_from_moments for one row; a batch without finite elements (bc == 0) changes nothing."""
    if bc == 0:
        return count, mean, var
    delta = bm - mean
    tot = count + bc
    new_mean = mean + delta * bc / tot
    m2 = var * count + bv * bc + delta * delta * count * bc / tot
    return tot, new_mean, m2 / tot


class VecNormOracle:
    def __init__(self, obs_dim, batch, gamma=0.99, epsilon=1e-8, clip_obs=10.0, clip_reward=10.0, norm_obs=True,
                 norm_reward=True, training=True):
        self.D, self.B = int(obs_dim), int(batch)
        self.gamma, self.epsilon, self.clip_obs, self.clip_reward = float(gamma), float(epsilon), float(clip_obs), float(clip_reward)
        self.norm_obs, self.norm_reward, self.training = bool(norm_obs), bool(norm_reward), bool(training)
        R = self.D + 1                        # the last row is the discounted return
        self.count = np.full(R, 1e-4)
        self.mean = np.zeros(R)
        self.var = np.ones(R)
        self.ret = np.zeros(self.B)
        self.ep_return = np.zeros(self.B)
        self.ep_len = np.zeros(self.B, dtype=np.int64)
        self.episodes, self.sum_return, self.sum_length, self.nonfinite = 0, 0.0, 0, 0

    # ------------------------------------------------------------------ statistics
    def _update_row(self, r, x):
        x = np.asarray(x, dtype=np.float64)
        ok = np.isfinite(x)
        self.nonfinite += int(x.size - ok.sum())
        x = x[ok]
        if x.size == 0:
            return
        self.count[r], self.mean[r], self.var[r] = update_from_moments(self.count[r], self.mean[r], self.var[r], x.size,
                                                                       np.mean(x), np.var(x))

    def _norm_obs(self, obs):
        m, v = self.mean[:self.D, None], self.var[:self.D, None]
        with np.errstate(invalid="ignore"):
            return np.clip((np.asarray(obs, dtype=np.float64) - m) / np.sqrt(v + self.epsilon), -self.clip_obs, self.clip_obs)

    def stats(self):
        return dict(count=self.count.copy(), mean=self.mean.copy(), var=self.var.copy())

    # ------------------------------------------------------------------ protocol
    def reset(self, obs, mask=None):
        """obs [D, B] raw; returns the normalised observations (fp64; rows of unmasked lanes are meaningless)."""
        obs = np.asarray(obs, dtype=np.float64)
        m = np.ones(self.B, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
        self.ret[m] = 0.0
        self.ep_return[m] = 0.0
        self.ep_len[m] = 0
        if self.norm_obs:
            if self.training:
                for r in range(self.D):
                    self._update_row(r, obs[r, m])
            return self._norm_obs(obs)
        return obs

    def step(self, obs, reward, done, term_obs=None):
        """Raw obs [D, B], reward [B], done [B], term_obs [D, B] -> dict of fp64 results."""
        obs = np.asarray(obs, dtype=np.float64)
        reward = np.asarray(reward, dtype=np.float64)
        done = np.asarray(done).astype(bool)
        if self.training and self.norm_obs:
            for r in range(self.D):
                self._update_row(r, obs[r])
        if self.training and self.norm_reward:
            self.ret = self.ret * self.gamma + reward
            self._update_row(self.D, self.ret)
        out = {}
        out["obs"] = self._norm_obs(obs) if self.norm_obs else obs
        with np.errstate(invalid="ignore"):
            out["reward"] = (np.clip(reward / np.sqrt(self.var[self.D] + self.epsilon), -self.clip_reward, self.clip_reward)
                             if self.norm_reward else reward)
        if term_obs is not None:
            out["term_obs"] = self._norm_obs(term_obs) if self.norm_obs else np.asarray(term_obs, dtype=np.float64)
        self.ret[done] = 0.0
        # VecMonitor
        self.ep_return = self.ep_return + reward
        self.ep_len = self.ep_len + 1
        out["ep_return"] = self.ep_return.copy()
        out["ep_len"] = self.ep_len.copy()
        self.episodes += int(done.sum())
        self.sum_return += float(np.sum(self.ep_return[done]))
        self.sum_length += int(np.sum(self.ep_len[done]))
        self.ep_return[done] = 0.0
        self.ep_len[done] = 0
        out["done"] = done
        return out


def f32_ulp_distance(a, b):
    """|a - b| in units of fp32 ulps (ordered-integer distance) of two float32 arrays; 0 where both are NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
    ia = a.view(np.int32).astype(np.int64); ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia); ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    return np.where(np.isnan(a) & np.isnan(b), 0, d)
