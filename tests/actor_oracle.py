"""fp64 numpy restatement of rex_actor_act (include/rex.h) with a running error bound per output -- TEST ORACLE ONLY.

Nothing here shares code with csrc/actor.hpp: the towers are matmuls, the activation is ``np.tanh`` / ``np.maximum``, the noise is
``rng_oracle.Stream``.  Every output comes with a bound on what correct fp32 arithmetic in the contract's order may differ by:

* a layer with ``n`` inputs adds ``(n + 2) * 2^-24 * (sum |W||x| + |b|)`` (n fused multiply-adds, each rounded once, on top of the exact dot
  product) plus ``sum |W| * err_in`` (the error carried in);
* tanh and relu are 1-Lipschitz, so they pass the carried error on and add ``T * 2^-24``, ``T`` being the recorded bound of ``tanh32`` in
  ulp (|tanh| <= 1, so an ulp is at most ``2^-24``);
* ``action = mean + std * eps`` adds one rounding of its magnitude; ``logp`` the roundings of its ``2 act_dim + 2`` operations.
"""
import numpy as np

import rng_oracle

U = 2.0 ** -24
T_ULP = 1.5                      # include/rex.h, DESIGN.md section 2: the exhaustive sweep's worst case (1.371 ulp), rounded up
ACTOR_SALT = 0xA0761D6478BD642F
DRAW_WORDS = 32
HALF_LOG_2PI = float(np.float32(0.91893853))
SEED = (1 << 33) + 11


def make_tower(rng, in_dim, widths, head_out, scale=1.0):
    """[(W, b), ...] float32, hidden layers then the head: uniform(-1, 1) * scale / sqrt(fan_in), biases uniform(-0.5, 0.5)"""
    layers, n = [], in_dim
    for m in list(widths) + [head_out]:
        layers.append(((rng.uniform(-1, 1, (m, n)) * scale / np.sqrt(n)).astype(np.float32), rng.uniform(-0.5, 0.5, m).astype(np.float32)))
        n = m
    return layers


# the cases the host twin and the device are both held on: name -> (env id, B, in_dim, act_dim, widths, activation)
CASES = {
    "hopper_64x64_tanh": ("RandomHopper-v0", 200, 11, 3, (64, 64), "tanh"),
    "hopper_33_relu": ("RandomHopper-v0", 200, 11, 3, (33,), "relu"),
    "hopper_64_17_64_tanh": ("RandomHopper-v0", 200, 11, 3, (64, 17, 64), "tanh"),
    "humanoid_64x64_tanh": ("RandomHumanoid-v0", 70, 376, 17, (64, 64), "tanh"),
}


def make_case(name):
    """dict(pi, vf, log_std, obs [B, in_dim], ...) of a named case, seeded by the name"""
    env_id, B, in_dim, A, widths, activation = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 77)
    return dict(env_id=env_id, B=B, in_dim=in_dim, act_dim=A, widths=widths, activation=activation,
                pi=make_tower(rng, in_dim, widths, A, 2.0), vf=make_tower(rng, in_dim, widths, 1, 2.0),
                log_std=rng.uniform(-1.5, 0.3, A).astype(np.float32), obs=(rng.standard_normal((B, in_dim)) * 1.5).astype(np.float32))


def tower(layers, x, activation):
    """(y, err) [B, out] of a tower on x [B, in] (fp64 holding fp32 values)"""
    x = np.asarray(x, np.float64)
    err = np.zeros_like(x)
    for l, (W, b) in enumerate(layers):
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        n = W.shape[1]
        y = x @ W.T + b
        mag = np.abs(x) @ np.abs(W).T + np.abs(b)
        err = (n + 2) * U * mag + err @ np.abs(W).T
        if l < len(layers) - 1:
            y = np.tanh(y) if activation == "tanh" else np.maximum(y, 0.0)
            err = err + T_ULP * U
        x = y
    return x, err


def eps(seed, env_offset, B, act_dim, draw):
    """[B, act_dim] fp64: rocRAND's normals of call `draw`, as Stream.normal() pairs them"""
    out = np.zeros((B, act_dim))
    for i in range(B):
        st = rng_oracle.Stream((int(seed) ^ ACTOR_SALT) & rng_oracle.M64, env_offset + i, (DRAW_WORDS * int(draw)) & rng_oracle.M64)
        for k in range(act_dim):
            out[i, k] = st.normal()
    return out


def act(case_or_pi, vf=None, log_std=None, obs=None, activation="tanh", eps_in=None):
    """dict of (value, bound) pairs: mean, value, and with ``eps_in`` [B, act_dim] also action and logp; absent towers give None"""
    if isinstance(case_or_pi, dict):
        c = case_or_pi
        pi, vf, log_std, obs, activation = c["pi"], c["vf"], c["log_std"], c["obs"], c["activation"]
    else:
        pi = case_or_pi
    out = dict(mean=None, value=None, action=None, logp=None)
    if vf is not None:
        v, e = tower(vf, obs, activation)
        out["value"] = (v[:, 0], e[:, 0])
    if pi is not None:
        m, e = tower(pi, obs, activation)
        out["mean"] = (m, e)
        if eps_in is not None:
            ls = np.asarray(log_std, np.float64)
            z = np.asarray(eps_in, np.float64)
            std = np.exp(ls)
            A = len(ls)
            a = m + std * z
            out["action"] = (a, e + 2 * U * (np.abs(m) + np.abs(std * z)) + U * np.abs(std * z))     # (the last term: std itself is an fp32 rounding of exp)
            S = (z * z).sum(1)
            c = ls.sum() + A * HALF_LOG_2PI
            mag = 0.5 * S + np.abs(ls).sum() + A * HALF_LOG_2PI
            out["logp"] = (-0.5 * S - c, (2 * A + 2) * U * mag)
    return out
