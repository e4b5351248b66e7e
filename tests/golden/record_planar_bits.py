"""Records tests/golden/planar_fp32_bits.npz: the fp32 bits of the planar engine's host build along seeded rollouts.

The fixture pins the ARITHMETIC of the Newton solvers: a change that only moves work around (computes a value later, or only
on the path that reads it) must reproduce every word.  Record it from the commit whose results are to be kept -- run

    python tests/golden/record_planar_bits.py

there, and commit the .npz; tests/test_newton_lazy_sums_host.py replays it with replay() below.

Per kind (hopper, half-cheetah, walker2d): 128 envs from the reset distribution, xi = nominal * U(0.8, 1.2), one action sequence
U(-1, 1) of 24 env-steps; stepped by the fp32 host harness (host_step) with the feet-only solver allowed (fast 1), switched off
(fast 0: every solve on the unrolled general instantiation) and switched off with the general path on the list solver of the
two-lanes-per-env kernels (set_rolled(2)), under five line-search schedules (ls_max, ls_free): the model's default, (3, 0), (3, 2), (1, 4), (3, 24).
qpos / qvel of every 4th step are kept as uint32 words.  All inputs are stored as float32, which the harness reads exactly.
Schedules 1.. are stored XORed with schedule 0 (they agree in most words, so the compressed file stays small).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

KINDS = ("hopper", "halfcheetah", "walker2d")
NQ = {"hopper": 6, "halfcheetah": 9, "walker2d": 9}
NU = {"hopper": 3, "halfcheetah": 6, "walker2d": 6}
FRAME_SKIP = {"hopper": 4, "halfcheetah": 5, "walker2d": 4}
SCHEDULES = ((-1, -1), (3, 0), (3, 2), (1, 4), (3, 24))   # (ls_max, ls_free); -1: the model's default
MODES = ((1, 0), (0, 0), (0, 2))   # (set_fast, set_rolled)
N_ENVS, N_STEPS, EVERY = 128, 24, 4
PATH = os.path.join(HERE, "planar_fp32_bits.npz")


def make_inputs(kind, seed):
    from random_envs_amd.specs import SPECS
    rng = np.random.RandomState(seed)
    nq, nu = NQ[kind], NU[kind]
    nom = np.array(SPECS[kind].nominal_task)
    xi = nom[None, :] * rng.uniform(0.8, 1.2, (N_ENVS, len(nom)))
    if kind == "halfcheetah":
        q = rng.uniform(-0.1, 0.1, (N_ENVS, nq)); v = 0.1 * rng.randn(N_ENVS, nq)
    else:
        q = rng.uniform(-0.005, 0.005, (N_ENVS, nq)); v = rng.uniform(-0.005, 0.005, (N_ENVS, nq))
        q[:, 1] += 1.25
    act = rng.uniform(-1, 1, (N_STEPS, N_ENVS, nu))
    return [x.astype(np.float32) for x in (q, v, xi, act)]


def replay(kind, q0, v0, xi, act):
    """-> qpos bits, qvel bits [mode, schedule, recorded step, env, nq] (uint32) and the number of capped solves"""
    from host_harness.build import host_step, set_fast, set_line_search, set_rolled
    nrec = N_STEPS // EVERY
    qb = np.zeros((len(MODES), len(SCHEDULES), nrec) + q0.shape, np.uint32); vb = np.zeros_like(qb)
    capped = 0
    try:
        for fi, (fast, gen) in enumerate(MODES):
            set_fast(fast); set_rolled(gen)
            for si, (ls_max, ls_free) in enumerate(SCHEDULES):
                set_line_search(ls_max, ls_free)
                q, v = q0.astype(np.float64), v0.astype(np.float64)
                for s in range(N_STEPS):
                    q, v, cap = host_step(kind, True, q, v, act[s].astype(np.float64), xi.astype(np.float64), FRAME_SKIP[kind])
                    capped += int(cap.sum())
                    if (s + 1) % EVERY == 0:
                        r = (s + 1) // EVERY - 1
                        q32, v32 = q.astype(np.float32), v.astype(np.float32)
                        assert (q32 == q).all() and (v32 == v).all()   # the fp32 harness hands back fp32 values
                        qb[fi, si, r] = q32.view(np.uint32); vb[fi, si, r] = v32.view(np.uint32)
    finally:
        set_fast(1); set_rolled(0); set_line_search(-1, -1)
    return qb, vb, capped


def pack(bits):
    out = bits.copy(); out[:, 1:] ^= bits[:, :1]; return out


def unpack(stored):
    out = stored.copy(); out[:, 1:] ^= stored[:, :1]; return out


def main():
    out = {}
    for k, kind in enumerate(KINDS):
        q0, v0, xi, act = make_inputs(kind, 100 + k)
        qb, vb, capped = replay(kind, q0, v0, xi, act)
        assert capped == 0, (kind, capped)
        out.update({kind + "_q0": q0, kind + "_v0": v0, kind + "_xi": xi, kind + "_act": act,
                    kind + "_qbits": pack(qb), kind + "_vbits": pack(vb)})
        print(kind, "words differing from schedule 0:", int((pack(qb)[:, 1:] != 0).sum() + (pack(vb)[:, 1:] != 0).sum()))
    np.savez_compressed(PATH, **out)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
