"""Records tests/golden/planar_decisions_bits.npz: the fp32 bits of the planar engine's host build along seeded rollouts whose start
states and solver knobs reach every wave-uniform decision of forward() and of the Newton solvers.

The fixture pins the arithmetic under changes of CONTROL FLOW only (the dispatch of forward(), the loop control of the Newton solvers, one
branch into the correction block, Ma rebuilt at the end of a correction trip instead of at the top of the next pass).  Record it from the
commit whose results are to be kept -- run

    python tests/golden/record_decisions_bits.py

there, and commit the .npz; tests/test_wave_decisions_host.py replays it with replay() below.  It adds to planar_fp32_bits.npz (reset
neighbourhood, default corr / warm) what that fixture does not hold:

  knobs   corr 0 / 1 / 2, warm start off, `fast` off (unrolled general instantiation and the list solver), the rolled row-list solver, and
          the line-search schedules (3, 0) and (3, 2) beside the default -- CASES below;
  states  32 envs per kind, mixed: lanes 0-9 from the reset distribution; lanes 10-15 with the root 1 m above the reset height and zero action
          (free flight, forward() mode 0, until they land); lanes 16-27 with the trunk pitched about +-1.2 rad at low height (the body lies down:
          capsules other than the feet on the floor, general modes 1 / 2); lanes 28-31 pitched with a folded leg (hopper: a
          capsule-capsule self pair passes the cull).

16 env-steps of one action sequence U(-1, 1) per kind; xi = nominal * U(0.8, 1.2); qpos / qvel of every 4th step are kept as uint32 words,
cases 1.. XORed with case 0.  `mode` holds, per case / step / env, the solver instantiation that forward() enters at the step's start state.
The harness (tests/host_harness/decisions_host.cpp) is plain x86-64 g++ -O2 with the engine's own sincos_poly: the bits do not depend on
the machine.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)
from host_harness.build import build_so  # noqa: E402

KINDS = ("hopper", "halfcheetah", "walker2d")
KIND_ID = {"hopper": 1, "halfcheetah": 2, "walker2d": 3}
NQ = {"hopper": 6, "halfcheetah": 9, "walker2d": 9}
NU = {"hopper": 3, "halfcheetah": 6, "walker2d": 6}
FRAME_SKIP = {"hopper": 4, "halfcheetah": 5, "walker2d": 4}
# (fast, gen, corr, warm, ls_max, ls_free); -1: the model's default (fast 1, corr 2, warm 1 with RK4, ls 3 / 4)
CASES = ((-1, 0, -1, -1, -1, -1),   # the defaults
         (-1, 0, 0, -1, -1, -1), (-1, 0, 1, -1, -1, -1), (-1, 0, 2, -1, -1, -1),   # corr 0 / 1 / 2
         (-1, 0, -1, 0, -1, -1),                                                   # warm start off
         (0, 0, -1, -1, -1, -1), (0, 2, -1, -1, -1, -1),                           # fast off: unrolled general / list solver on every solve
         (0, 2, 0, -1, -1, -1), (0, 2, 1, -1, -1, -1), (0, 2, -1, 0, -1, -1),      # the list solver: corr 0 / 1, warm off
         (-1, 2, -1, -1, -1, -1), (-1, 1, -1, -1, -1, -1),                         # fast on, general modes on the list / rolled solver
         (-1, 0, -1, -1, 3, 0), (-1, 0, -1, -1, 3, 2), (-1, 2, -1, -1, 3, 0), (0, 2, -1, -1, 3, 2),   # searching from pass 0 / from pass 2
         (-1, 0, 1, 0, 3, 0))                                                      # everything off its default at once
N_ENVS, N_STEPS, EVERY = 32, 16, 4
FREE = slice(10, 16)      # lanes that start 1 m up
LYING = slice(16, 32)     # lanes that start pitched at low height
PATH = os.path.join(HERE, "planar_decisions_bits.npz")
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("decisions_host", "decisions_host.cpp"))
    return _lib


def step(kind, case, q, v, a, xi):
    """one env-step of the fp32 host engine under `case` -> qpos, qvel (float32), capped, mode at the start state (int32)"""
    n = q.shape[0]
    q, v, a, xi = [np.ascontiguousarray(x, np.float32) for x in (q, v, a, xi)]
    qo, vo = np.empty_like(q), np.empty_like(v)
    cap, mode = np.zeros(n, np.int32), np.zeros(n, np.int32)
    kn = np.array(case, np.int32)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    rc = lib().dh_step(KIND_ID[kind], n, FRAME_SKIP[kind], kn.ctypes.data_as(ip), *[x.ctypes.data_as(fp) for x in (q, v, a, xi, qo, vo)],
                       cap.ctypes.data_as(ip), mode.ctypes.data_as(ip))
    assert rc == 0
    return qo, vo, cap, mode


def make_inputs(kind, seed):
    from random_envs_amd.specs import SPECS
    rng = np.random.RandomState(seed)
    nq, nu = NQ[kind], NU[kind]
    nom = np.array(SPECS[kind].nominal_task)
    xi = nom[None, :] * rng.uniform(0.8, 1.2, (N_ENVS, len(nom)))
    if kind == "halfcheetah":
        q = rng.uniform(-0.1, 0.1, (N_ENVS, nq)); v = 0.1 * rng.randn(N_ENVS, nq)
        low = -0.35     # root z is an offset from the model's 0.7
    else:
        q = rng.uniform(-0.005, 0.005, (N_ENVS, nq)); v = rng.uniform(-0.005, 0.005, (N_ENVS, nq))
        q[:, 1] += 1.25
        low = 0.45
    q[FREE, 1] += 1.0
    nl = LYING.stop - LYING.start
    q[LYING, 1] = low + rng.uniform(-0.05, 0.05, nl)
    q[LYING, 2] = np.where(np.arange(nl) % 2 == 0, 1.0, -1.0) * (1.2 + rng.uniform(-0.1, 0.1, nl))
    if kind == "hopper":   # folded leg: thigh and knee near their -150 deg limits bring leg and foot to the torso
        q[28:32, 3] = rng.uniform(-2.5, -2.2, 4); q[28:32, 4] = rng.uniform(-2.5, -2.2, 4)
    else:
        q[28:32, 3] = rng.uniform(-0.5, -0.3, 4)
    act = rng.uniform(-1, 1, (N_STEPS, N_ENVS, nu))
    act[:, FREE] = 0.0   # no motor swings a limb into a joint limit: these lanes have no row until they land
    return [x.astype(np.float32) for x in (q, v, xi, act)]


def replay(kind, q0, v0, xi, act):
    """-> qpos bits, qvel bits [case, recorded step, env, nq] (uint32), mode [case, step, env] (int8), number of capped solves"""
    nrec = N_STEPS // EVERY
    qb = np.zeros((len(CASES), nrec) + q0.shape, np.uint32); vb = np.zeros_like(qb)
    modes = np.zeros((len(CASES), N_STEPS, q0.shape[0]), np.int8)
    capped = 0
    for ci, case in enumerate(CASES):
        q, v = q0, v0
        for s in range(N_STEPS):
            q, v, cap, mode = step(kind, case, q, v, act[s], xi)
            capped += int(cap.sum()); modes[ci, s] = mode
            if (s + 1) % EVERY == 0:
                r = (s + 1) // EVERY - 1
                qb[ci, r] = q.view(np.uint32); vb[ci, r] = v.view(np.uint32)
    return qb, vb, modes, capped


def pack(bits):
    out = bits.copy(); out[1:] ^= bits[:1]; return out


def unpack(stored):
    out = stored.copy(); out[1:] ^= stored[:1]; return out


def main():
    out = {}
    for k, kind in enumerate(KINDS):
        q0, v0, xi, act = make_inputs(kind, 300 + k)
        qb, vb, modes, capped = replay(kind, q0, v0, xi, act)
        assert capped == 0, (kind, capped)
        assert np.isfinite(qb.view(np.float32)).all() and np.isfinite(vb.view(np.float32)).all(), kind
        out.update({kind + "_q0": q0, kind + "_v0": v0, kind + "_xi": xi, kind + "_act": act,
                    kind + "_qbits": pack(qb), kind + "_vbits": pack(vb), kind + "_mode": modes})
        print(kind, "start-state modes per case [mode 0, 1, 2, 3]:", [np.bincount(m.ravel(), minlength=4).tolist() for m in modes])
        print(kind, "words differing from case 0:", int((pack(qb)[1:] != 0).sum() + (pack(vb)[1:] != 0).sum()))
    np.savez_compressed(PATH, **out)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
