"""numpy / Python-int restatement of the semantics of ``rex_rbuf_*`` (include/rex.h) -- TEST ORACLE ONLY.

It restates the published behaviour of stable-baselines3 (v2.x):

* ``ReplayBuffer.add`` (stable_baselines3/common/buffers.py) stores ``obs``, ``next_obs``, ``action``, ``reward``, ``done`` and
  ``timeouts = [info.get("TimeLimit.truncated", False) ...]`` at ``pos``; ``OffPolicyAlgorithm._store_transition``
  (common/off_policy_algorithm.py) first replaces ``next_obs[i]`` by ``infos[i]["terminal_observation"]`` where ``dones[i]``.
* ``ReplayBuffer.sample`` draws ``np.random.randint(0, upper_bound, size=batch_size)`` (with replacement) and ``_get_samples``
  returns the rows, ``dones * (1 - timeouts)`` and, given a ``VecNormalize``, ``normalize_obs`` / ``normalize_reward`` of them:
  ``clip((obs - mean) / sqrt(var + epsilon), +-clip_obs)``, ``clip(reward / sqrt(ret_var + epsilon), +-clip_reward)``.

Additions of this project: the ids come from a counter-based generator -- Philox4x32-10 (Salmon et al., SC11; the Random123 library
publishes its known-answer vectors) with key ``(lo32(seed), hi32(seed))`` and counter ``(lo32(j), hi32(j), lo32(draw), hi32(draw))``,
``u = w0 | w1 << 32``, id ``= (u * N) >> 64`` in exact integer arithmetic -- storage is transition-major with id ``s = t * B + b``, and
an id out of range yields zeros and is counted.  Everything but the normalisation is a copy, so it is compared bit for bit; the
normalisation is evaluated in fp64 by numpy's own expression order and compared within 1 fp32 ulp.
"""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85

# Random123's known-answer vectors for philox4x32 with 10 rounds: (counter, key) -> output
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """One block with Python ints."""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def sample_bits(seed, draw, j):
    seed, draw, j = int(seed), int(draw), int(j)
    w = philox4x32_10((j & M32, j >> 32, draw & M32, (draw >> 32) & M32), (seed & M32, (seed >> 32) & M32))
    return w[0] | (w[1] << 32)


def sample_ids(seed, draw, size, B, n):
    """ids of samples 0 .. n-1 of draw number ``draw`` over ``size`` valid slots of ``B`` envs: int64 [n]"""
    N = int(size) * int(B)
    return np.array([(sample_bits(seed, draw, j) * N) >> 64 for j in range(n)], dtype=np.int64)


def empty_buffers(T, B, D, A, act_dtype=np.float32):
    return dict(obs=np.zeros((T, B, D), np.float32), next_obs=np.zeros((T, B, D), np.float32), action=np.zeros((T, B, A), act_dtype),
                reward=np.zeros((T, B), np.float32), done=np.zeros((T, B), np.uint8), timeout=np.zeros((T, B), np.uint8))


def add(bufs, t, obs, action, reward, done, next_obs, terminal_obs=None, truncated=None):
    """SoA inputs ([dim, B] / [B]) into slot t of the transition-major buffers, in place."""
    T = bufs["obs"].shape[0]
    if not 0 <= t < T:
        raise ValueError("slot %d outside [0, %d)" % (t, T))
    fin = np.asarray(done) != 0
    nxt = np.asarray(next_obs).T
    if terminal_obs is not None:
        nxt = np.where(fin[:, None], np.asarray(terminal_obs).T, nxt)
    bufs["obs"][t] = np.asarray(obs).T
    bufs["next_obs"][t] = nxt
    bufs["action"][t] = np.asarray(action).T
    bufs["reward"][t] = reward
    bufs["done"][t] = fin
    bufs["timeout"][t] = 0 if truncated is None else (np.asarray(truncated) != 0)


def normalise(x, mean, var, epsilon, clip):
    """VecNormalize's expression in fp64"""
    with np.errstate(invalid="ignore"):
        return np.clip((np.asarray(x, dtype=np.float64) - mean) / np.sqrt(var + epsilon), -clip, clip)


def gather(bufs, index, norm=None):
    """(outputs, bad): rows of the ids ``index``; zeros for an id outside [0, T * B).  ``norm``: None or a dict of ``mean`` / ``var``
    (float64 [D + 1], the return row last), ``norm_obs``, ``norm_reward``, ``epsilon``, ``clip_obs``, ``clip_reward`` -- the normalised outputs
    are then float64."""
    T, B, D = bufs["obs"].shape
    index = np.asarray(index, dtype=np.int64)
    ok = (index >= 0) & (index < T * B)
    s = np.where(ok, index, 0)
    flat = {k: v.reshape((T * B,) + v.shape[2:]) for k, v in bufs.items()}
    out = {k: flat[k][s].copy() for k in ("obs", "next_obs", "action", "reward")}
    out["done"] = ((flat["done"][s] != 0) & (flat["timeout"][s] == 0)).astype(np.float32)
    if norm is not None:
        if norm["norm_obs"]:
            for k in ("obs", "next_obs"):
                out[k] = normalise(out[k], norm["mean"][None, :D], norm["var"][None, :D], norm["epsilon"], norm["clip_obs"])
        if norm["norm_reward"]:
            out["reward"] = normalise(out["reward"], 0.0, norm["var"][D], norm["epsilon"], norm["clip_reward"])
    for k in out:
        out[k][~ok] = 0
    return out, int((~ok).sum())


def sample(bufs, size, n, seed, draw, norm=None):
    B = bufs["obs"].shape[1]
    ids = sample_ids(seed, draw, size, B, n)
    out, bad = gather(bufs, ids, norm)
    assert bad == 0
    out["index"] = ids
    return out
