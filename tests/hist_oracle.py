"""Numpy restatement of rex_hist_init / push / reset / window (TEST INFRASTRUCTURE), written from the rules of include/rex.h with an
EXPLICIT SHIFT and no ring: ``win`` [B, K, W] is every lane's window, oldest frame first, and a push moves every row up by one.  Inputs
are batch-major ([B, dim]); every comparison against it is to identical bits (views as uint32)."""
import numpy as np


def frame_of(obs, action, with_action, zero=None):
    """[B, W] frames (obs, action): ``action`` converted to float32 (the cart-pole's ints), zeros on the lanes ``zero`` flags."""
    obs = np.asarray(obs, np.float32)
    if not with_action:
        return obs.copy()
    act = np.zeros((obs.shape[0], 0), np.float32) if action is None else np.asarray(action).reshape(obs.shape[0], -1).astype(np.float32)
    if zero is not None:
        act = np.where(np.asarray(zero, bool)[:, None], np.float32(0), act)
    return np.concatenate([obs, act], axis=1)


class HistOracle:
    def __init__(self, B, K, obs_dim, act_dim, with_action=True):
        self.B, self.K, self.with_action = B, K, bool(with_action)
        self.W = obs_dim + (act_dim if with_action else 0)
        self.act_dim = act_dim
        self.win = np.zeros((B, K, self.W), np.float32)
        self.length = np.zeros(B, np.int32)
        self.pushes = 0

    def push(self, obs, action, done=None, terminal_obs=None, term_out=None):
        """term_out [B, K, W] is updated in place on the done lanes when terminal_obs is given"""
        B, K = self.B, self.K
        done = np.zeros(B, bool) if done is None else np.asarray(done).astype(bool)
        if term_out is not None and terminal_obs is not None:
            last = frame_of(terminal_obs, action, self.with_action)
            for b in np.nonzero(done)[0]:
                term_out[b, :K - 1] = self.win[b, 1:]
                term_out[b, K - 1] = last[b]
        self.win[done] = 0
        self.length[done] = 0
        frame = frame_of(obs, action, self.with_action, zero=done)
        for k in range(K - 1):                      # the shift
            self.win[:, k] = self.win[:, k + 1]
        self.win[:, K - 1] = frame
        self.length = np.minimum(self.length + 1, K).astype(np.int32)
        self.pushes += 1

    def reset(self, mask, obs):
        m = np.ones(self.B, bool) if mask is None else np.asarray(mask).astype(bool)
        frame = frame_of(obs, np.zeros((self.B, self.act_dim), np.float32), self.with_action)
        self.win[m] = 0
        self.win[m, self.K - 1] = frame[m]
        self.length[m] = 1

    def window(self):
        return self.win.copy()

    def mask(self):
        return (np.arange(self.K)[None, :] >= (self.K - self.length)[:, None]).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ring_window(frames, pushes, K):
    """the strided view of the ring [B, 2K, W] after ``pushes`` pushes"""
    c = (pushes - 1) % K if pushes else 0
    return frames[:, c + 1:c + K + 1, :]
