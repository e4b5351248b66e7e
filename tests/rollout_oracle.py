"""numpy fp64 restatement of the rollout buffer (TEST ORACLE): stable-baselines3's RolloutBuffer.add with the time-limit
bootstrap of collect_rollouts, compute_returns_and_advantage, the advantage statistics PPO normalises with, and get() as
fancy indexing -- written from the formulas, over the SoA layout: obs [T, obs_dim, B], action [T, act_dim, B], the rest [T, B]."""
import numpy as np

F32, F64 = np.float32, np.float64


def bootstrap_reward(reward, truncated, terminal_value, gamma):
    """reward + gamma * V(terminal_obs) on the truncated lanes: a product and a sum in fp64, rounded once to fp32"""
    r = np.asarray(reward, dtype=F32).copy()
    m = np.asarray(truncated).astype(bool)
    prod = F64(gamma) * np.asarray(terminal_value, dtype=F32).astype(F64)
    r[m] = (r.astype(F64) + prod).astype(F32)[m]
    return r


def gae(reward, value, done, last_value, gamma, lam):
    """advantage, returns [T, B] float32; done[t] is the flag step t returned"""
    reward, value = np.asarray(reward, dtype=F32).astype(F64), np.asarray(value, dtype=F32).astype(F64)
    T, B = reward.shape
    gamma, gl = F64(gamma), F64(gamma) * F64(lam)
    adv, ret = np.zeros((T, B), dtype=F32), np.zeros((T, B), dtype=F32)
    A = np.zeros(B, dtype=F64)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            nnt = np.where(np.asarray(done[t]) != 0, F64(0), F64(1))
            nv = np.asarray(last_value, dtype=F32).astype(F64) if t == T - 1 else value[t + 1]
            delta = (reward[t] + (gamma * nv) * nnt) - value[t]
            A = delta + (gl * nnt) * A
            adv[t] = A.astype(F32)
            ret[t] = (A + value[t]).astype(F32)
    return adv, ret


def adv_stats(adv):
    """n, mean, M2 over the finite elements (two-pass, fp64), and the number left out"""
    x = np.asarray(adv, dtype=F32).astype(F64).ravel()
    ok = np.isfinite(x)
    y = x[ok]
    n = y.size
    mean = y.mean() if n else 0.0
    m2 = float(((y - mean) ** 2).sum()) if n else 0.0
    return dict(n=n, mean=float(mean), m2=m2, nonfinite=int(x.size - n))


def normalised(adv, st):
    """(A - mean) / (std + 1e-8) in fp64 with the unbiased deviation (not rounded)"""
    with np.errstate(all="ignore"):
        sd = np.sqrt(F64(st["m2"]) / F64(st["n"] - 1))
        return (np.asarray(adv, dtype=F32).astype(F64) - st["mean"]) / (sd + 1e-8)


def gather(bufs, index):
    """bufs: dict of the SoA arrays; index: flat ids s = t * B + b, all in range.  Row-major [n, dim] / [n] outputs."""
    T, B = bufs["reward"].shape
    idx = np.asarray(index, dtype=np.int64)
    t, b = idx // B, idx % B
    out = {k: bufs[k][t, b] for k in ("advantage", "returns", "value", "log_prob")}
    out["obs"] = bufs["obs"][t, :, b]
    out["action"] = bufs["action"][t, :, b]
    return out


def f32_ulp_distance(a, b):
    """distance in units in the last place between float32 arrays (NaN against NaN: 0)"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia); ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    d = np.abs(ia - ib)
    return np.where(np.isnan(a) & np.isnan(b), 0, np.where(np.isnan(a) | np.isnan(b), 1 << 40, d))
