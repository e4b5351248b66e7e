"""numpy restatement of the n-step semantics of include/rex.h (rex_rbuf_gather_nstep and its siblings) -- TEST ORACLE ONLY.

The definition is the loop of the header, evaluated per sample in numpy ``float64`` SCALAR operations (each one IEEE operation, no
contraction) over the buffers of ``replay_buffer_oracle.empty_buffers``:

    s_k = ((t0 + k) mod T) * B + b;  step k is the last (m = k + 1) at the first of: done or timeout at s_k, t_k == head, k == n_step - 1
    acc = reward[s_0];  g = gamma;   for k = 1 .. m-1:  acc = acc + g * reward[s_k];  g = g * gamma

Beside the outputs it returns ``m``, the last id of every window, which of the three conditions ended it and whether it wrapped from slot
``T - 1`` to slot 0, so a test can assert that its inputs exercise every ending.  Everything but the normalisation is compared bit for
bit; normalised values are float64 here and compared within 1 fp32 ulp (replay_buffer_oracle.normalise).
"""
import numpy as np

import replay_buffer_oracle as rb

END_EPISODE, END_HEAD, END_FULL = 0, 1, 2          # the first condition that held, in the header's order


def gather_nstep(bufs, index, head, n_step, gamma, norm=None):
    """(outputs, info): outputs obs / next_obs / action / reward / done / discount / steps for the ids ``index`` (zeros for an id outside
    [0, T * B)); info = dict(m, last, ending, wrapped, bad).  ``norm`` as in replay_buffer_oracle.gather."""
    T, B, D = bufs["obs"].shape
    assert 1 <= n_step <= 32 and 0 <= head < T and np.isfinite(gamma) and 0.0 <= gamma <= 1.0
    index = np.asarray(index, dtype=np.int64)
    n = len(index)
    flat = {k: v.reshape((T * B,) + v.shape[2:]) for k, v in bufs.items()}
    out = dict(obs=np.zeros((n, D), np.float32), next_obs=np.zeros((n, D), np.float32), action=np.zeros((n,) + flat["action"].shape[1:], flat["action"].dtype),
               reward=np.zeros(n, np.float32), done=np.zeros(n, np.float32), discount=np.zeros(n, np.float32), steps=np.zeros(n, np.int32))
    info = dict(m=np.zeros(n, np.int64), last=np.full(n, -1, np.int64), ending=np.full(n, -1, np.int64), wrapped=np.zeros(n, bool), bad=0)
    gamma = np.float64(gamma)
    for j, s in enumerate(int(v) for v in index):
        if not 0 <= s < T * B:
            info["bad"] += 1
            continue
        t0, b = divmod(s, B)
        acc, g, k = np.float64(flat["reward"][s]), gamma, 0
        while True:
            t_k = (t0 + k) % T
            s_k = t_k * B + b
            if k > 0:
                acc = acc + g * np.float64(flat["reward"][s_k])
                g = g * gamma
                info["wrapped"][j] |= t_k == 0
            if flat["done"][s_k] != 0 or flat["timeout"][s_k] != 0:
                ending = END_EPISODE
            elif t_k == head:
                ending = END_HEAD
            elif k == n_step - 1:
                ending = END_FULL
            else:
                k += 1
                continue
            break
        m = k + 1
        out["obs"][j], out["action"][j], out["next_obs"][j] = flat["obs"][s], flat["action"][s], flat["next_obs"][s_k]
        out["reward"][j] = np.float32(acc)
        out["done"][j] = 1.0 if (flat["done"][s_k] != 0 and flat["timeout"][s_k] == 0) else 0.0
        out["discount"][j], out["steps"][j] = np.float32(g), m
        info["m"][j], info["last"][j], info["ending"][j] = m, s_k, ending
    if norm is not None:
        ok = info["m"] > 0
        if norm["norm_obs"]:
            for k in ("obs", "next_obs"):
                out[k] = rb.normalise(out[k], norm["mean"][None, :D], norm["var"][None, :D], norm["epsilon"], norm["clip_obs"])
                out[k][~ok] = 0
        if norm["norm_reward"]:
            out["reward"] = rb.normalise(out["reward"], 0.0, norm["var"][D], norm["epsilon"], norm["clip_reward"])
            out["reward"][~ok] = 0
    return out, info


def sample_nstep(bufs, size, head, n, seed, draw, n_step, gamma, norm=None):
    T, B = bufs["obs"].shape[:2]
    assert 1 <= size <= T and (size == T or head == size - 1)
    ids = rb.sample_ids(seed, draw, size, B, n)
    out, info = gather_nstep(bufs, ids, head, n_step, gamma, norm)
    assert info["bad"] == 0
    out["index"] = ids
    return out, info
