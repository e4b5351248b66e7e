"""numpy restatement of the sequence-window semantics of include/rex.h (rex_rbuf_gather_seq and its siblings) -- TEST ORACLE ONLY.

The definition is the loop of the header, evaluated per sample over the buffers of ``replay_buffer_oracle.empty_buffers``:

    s_k = ((t0 + k) mod T) * B + b;  step k is the last (m = k + 1) at the first of: done or timeout at s_k, t_k == head, k == L - 1
    obs[j, k] = obs[s_k], action[j, k] = action[s_k], reward[j, k] = reward[s_k], done[j, k] = done and not timeout at s_k,
    mask[j, k] = 1 for k < m;  obs[j, m] = next_obs[s_(m-1)];  everything else 0;  length[j] = m

Beside the outputs it returns ``m``, the ids of every window's steps, which of the three conditions ended it and whether it wrapped from
slot ``T - 1`` to slot 0, so a test can assert that its inputs exercise every ending.  Everything but the normalisation is compared bit
for bit; normalised values are float64 here and compared within 1 fp32 ulp (replay_buffer_oracle.normalise).
"""
import numpy as np

import replay_buffer_oracle as rb

END_EPISODE, END_HEAD, END_FULL = 0, 1, 2          # the first condition that held, in the header's order
MAX_LEN = 64


def gather_seq(bufs, index, head, seq_len, norm=None):
    """(outputs, info): outputs obs [n, L + 1, D] / action [n, L, A] / reward / done / mask [n, L] / length [n] for the ids ``index`` (zeros
    for an id outside [0, T * B)); info = dict(m, steps [n, L] (ids, -1 past the end), ending, wrapped, bad).  ``norm`` as in
    replay_buffer_oracle.gather."""
    T, B, D = bufs["obs"].shape
    L = int(seq_len)
    assert 1 <= L <= MAX_LEN and 0 <= head < T
    index = np.asarray(index, dtype=np.int64)
    n = len(index)
    flat = {k: v.reshape((T * B,) + v.shape[2:]) for k, v in bufs.items()}
    A = flat["action"].shape[1]
    out = dict(obs=np.zeros((n, L + 1, D), np.float32), action=np.zeros((n, L, A), flat["action"].dtype), reward=np.zeros((n, L), np.float32),
               done=np.zeros((n, L), np.float32), mask=np.zeros((n, L), np.float32), length=np.zeros(n, np.int32))
    info = dict(m=np.zeros(n, np.int64), steps=np.full((n, L), -1, np.int64), ending=np.full(n, -1, np.int64), wrapped=np.zeros(n, bool), bad=0)
    for j, s in enumerate(int(v) for v in index):
        if not 0 <= s < T * B:
            info["bad"] += 1
            continue
        t0, b = divmod(s, B)
        k = 0
        while True:
            t_k = (t0 + k) % T
            s_k = t_k * B + b
            if k > 0:
                info["wrapped"][j] |= t_k == 0
            info["steps"][j, k] = s_k
            out["obs"][j, k], out["action"][j, k], out["reward"][j, k] = flat["obs"][s_k], flat["action"][s_k], flat["reward"][s_k]
            out["done"][j, k] = 1.0 if (flat["done"][s_k] != 0 and flat["timeout"][s_k] == 0) else 0.0
            out["mask"][j, k] = 1.0
            if flat["done"][s_k] != 0 or flat["timeout"][s_k] != 0:
                ending = END_EPISODE
            elif t_k == head:
                ending = END_HEAD
            elif k == L - 1:
                ending = END_FULL
            else:
                k += 1
                continue
            break
        m = k + 1
        out["obs"][j, m] = flat["next_obs"][s_k]
        out["length"][j] = m
        info["m"][j], info["ending"][j] = m, ending
    if norm is not None:
        rows = np.arange(L + 1)[None, :] <= info["m"][:, None]                 # the written rows of obs: the steps and row m
        rows &= (info["m"] > 0)[:, None]
        steps = out["mask"] != 0
        if norm["norm_obs"]:
            out["obs"] = rb.normalise(out["obs"], norm["mean"][None, None, :D], norm["var"][None, None, :D], norm["epsilon"], norm["clip_obs"])
            out["obs"][~rows] = 0
        if norm["norm_reward"]:
            out["reward"] = rb.normalise(out["reward"], 0.0, norm["var"][D], norm["epsilon"], norm["clip_reward"])
            out["reward"][~steps] = 0
    return out, info


def sample_seq(bufs, size, head, n, seed, draw, seq_len, norm=None):
    T, B = bufs["obs"].shape[:2]
    assert 1 <= size <= T and (size == T or head == size - 1)
    ids = rb.sample_ids(seed, draw, size, B, n)
    out, info = gather_seq(bufs, ids, head, seq_len, norm)
    assert info["bad"] == 0
    out["index"] = ids
    return out, info
