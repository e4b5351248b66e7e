"""Records tests/golden/humanoid_fp32_bits.npz: the fp32 bits of the humanoid engines' host builds on a handful of states.

The fixture pins the ARITHMETIC of the host instantiations of humanoid_engine.hpp and humanoid_pair.hpp (the device code has the
assembly comparison of profiles/isa_same.py; the host builds have this): a change that only moves declarations around or writes a
shared piece once must reproduce every word.  Record it from the commit whose results are to be kept -- run

    python tests/golden/record_humanoid_bits.py

there, and commit the .npz; tests/test_humanoid_bits_host.py replays it with replay() below.  `--pool` prints the row count of every
candidate state in every series instead (for choosing PICK again after a change that is meant to move results).

Series, all fp32: `hh` = hh_step_rows (humanoid_host.cpp, one lane per env), `hd` = the same from the -DREX_PGS_CHECK_HOST build (the
device's sweep schedule on the host), `hp` = hp_step (humanoid_pair_host.cpp, two lanes per env), and `hpr` = hp_reset on seeded draws.
Per step series: qpos_out, qvel_out, obs, reward, xout as uint32 words, done, and nrows = the constraint rows of the step's last
forward evaluation.  `hd` and `hp` are stored XORed with `hh` (they agree in most leading bits, so the compressed file stays small).

States (PICK, at most 16, from a seeded pool): standing, after-reset, states along seeded random-action rollouts into ground contact,
and the lying / crumpled constructions of test_forward_dynamics_pile_ups and test_pile_ups_all_solver_paths.  They are chosen so that
the last evaluation of EVERY step series reaches every size of the dual solve (rows <= 4, 5-8, 9-10, 11-12, 13-14, 15-16, 17-18,
19-21), the scratch-row solve_pgs (> 21 rows) and the no-row path (0): coverage() is asserted here and again by the replay test.
All inputs are stored as float32, which the harnesses read exactly.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, "humanoid_fp32_bits.npz")
SERIES = ("hh", "hd", "hp")
FIELDS = ("qpos", "qvel", "obs", "reward", "xout")      # uint32 words; done (uint8) and nrows (int32) beside them
QPOS0 = np.array([0, 0, 1.4, 1, 0, 0, 0] + [0] * 17, dtype=float)
LEVELS = ((1, 4), (5, 8), (9, 10), (11, 12), (13, 14), (15, 16), (17, 18), (19, 21))   # row counts of the eight dual sizes
N_ROLL, ROLL_STEPS = 4, 60      # envs and env-steps of the seeded random-action rollouts
# indices into pool(): standing (2 rows), after-reset (0); rollout states with 8, 9, 12, 13, 16 and 24 rows; of the first pile-up
# construction 21 and 77 rows; of the second 17 and 77
PICK = (0, 1, 45, 189, 83, 96, 88, 179, 341, 242, 429, 463)
N_RESET = 4   # envs of the hp_reset series (one path: no rows, no solver), xi of the first N_RESET states


def _libs():
    from host_harness.build import build_so
    return (ctypes.CDLL(build_so("humanoid_host", "humanoid_host.cpp")),
            ctypes.CDLL(build_so("humanoid_host_devsched", "humanoid_host.cpp", ["-DREX_PGS_CHECK_HOST"])),
            ctypes.CDLL(build_so("humanoid_pair_host", "humanoid_pair_host.cpp", ["-pthread"])))


_D = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(_D)


def step(fn, f32, q, v, a, xi):
    """one env step of hh_step_rows / hp_step on [n, rows] inputs (xprev absent: the harness takes it from a forward at the state)"""
    n = len(q)
    qs, vs, as_, xs = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).T) for x in (q, v, a, xi)]
    qo = np.zeros_like(qs); vo = np.zeros_like(vs); obs = np.zeros((376, n)); r = np.zeros(n); d = np.zeros(n, dtype=np.uint8)
    xo = np.zeros((14, n)); ov = np.zeros(n, dtype=np.int32); nr = np.zeros(n, dtype=np.int32)
    I = ctypes.POINTER(ctypes.c_int)
    fn(int(f32), n, _p(qs), _p(vs), _p(as_), _p(xs), None, _p(qo), _p(vo), _p(obs), _p(r), d.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
       _p(xo), ov.ctypes.data_as(I), nr.ctypes.data_as(I))
    assert ov.sum() == 0
    return dict(qpos=qo.T.copy(), qvel=vo.T.copy(), obs=obs.T.copy(), reward=r, xout=xo.T.copy(), done=d, nrows=nr)


def reset(hp, f32, draws, xi):
    n = len(xi)
    ds, xs = np.ascontiguousarray(np.asarray(draws, dtype=np.float64).T), np.ascontiguousarray(np.asarray(xi, dtype=np.float64).T)
    qo = np.zeros((24, n)); vo = np.zeros((23, n)); obs = np.zeros((376, n)); xo = np.zeros((14, n))
    hp.hp_reset(int(f32), n, _p(ds), _p(xs), _p(qo), _p(vo), _p(obs), _p(xo))
    return dict(qpos=qo.T.copy(), qvel=vo.T.copy(), obs=obs.T.copy(), xout=xo.T.copy())


def pool(hh):
    """the candidate states [n, 24 + 23 + 17 + 30] as float32: standing, after-reset, the rollouts (stepped by the fp32 hh build), the
    two pile-up constructions"""
    from random_envs_amd.specs import SPECS
    nom = np.array(SPECS["humanoid"].nominal_task)
    f = lambda *xs: [np.asarray(x, dtype=np.float32).astype(np.float64) for x in xs]
    out = [np.concatenate([QPOS0, np.zeros(23), np.zeros(17), nom])[None]]
    rng = np.random.RandomState(200)
    out.append(np.concatenate([QPOS0 + rng.uniform(-.01, .01, 24), rng.uniform(-.01, .01, 23), rng.uniform(-.4, .4, 17), nom * rng.uniform(.8, 1.2, 30)])[None])
    n = N_ROLL
    rng = np.random.RandomState(201)
    q, v, xi = f(QPOS0 + rng.uniform(-.01, .01, (n, 24)), rng.uniform(-.01, .01, (n, 23)), nom * rng.uniform(.8, 1.2, (n, 30)))
    for s in range(ROLL_STEPS):
        a, = f(rng.uniform(-1, 1, (n, 17)))
        out.append(np.concatenate([q, v, a, xi], axis=1))
        o = step(hh.hh_step_rows, 1, q, v, a, xi)
        q, v = o["qpos"], o["qvel"]
    rng = np.random.RandomState(5)      # test_forward_dynamics_pile_ups (test_humanoid_host.py)
    for k in range(160):
        q = QPOS0.copy(); q[7:] += rng.uniform(-1.2, 1.2, 17); q[2] = rng.uniform(0.05, 0.6)
        qq = np.array([1, 0, 0, 0]) + rng.uniform(-1, 1, 4); q[3:7] = qq / np.linalg.norm(qq)
        out.append(np.concatenate([q, rng.uniform(-1, 1, 23), rng.uniform(-.4, .4, 17), nom * rng.uniform(.9, 1.1, 30)])[None])
    n = 64; rng = np.random.RandomState(5)   # test_pile_ups_all_solver_paths (test_humanoid_pair_host.py)
    q = np.tile(QPOS0, (n, 1)); q[:, 7:] += rng.uniform(-1.2, 1.2, (n, 17)); q[:, 2] = rng.uniform(0.05, 0.6, n)
    qq = np.array([1, 0, 0, 0]) + rng.uniform(-1, 1, (n, 4)); q[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    out.append(np.concatenate([q, rng.uniform(-1, 1, (n, 23)), rng.uniform(-.4, .4, (n, 17)), nom * rng.uniform(.9, 1.1, (n, 30))], axis=1))
    return np.concatenate(out).astype(np.float32)


def split(states):
    s = np.asarray(states, dtype=np.float64)
    return s[:, :24], s[:, 24:47], s[:, 47:64], s[:, 64:]


def coverage(nrows):
    """the solver paths the row counts reach: 'none', 'scratch', and one name per dual size"""
    seen = set()
    for n in np.asarray(nrows).ravel():
        seen.add("none" if n == 0 else "scratch" if n > LEVELS[-1][1] else next("%d-%d" % l for l in LEVELS if l[0] <= n <= l[1]))
    return seen


ALL_PATHS = {"none", "scratch"} | {"%d-%d" % l for l in LEVELS}


def bits(x):
    x32 = np.asarray(x).astype(np.float32)
    assert (x32 == x).all() or np.isnan(x).any()      # the fp32 harnesses hand back fp32 values
    return x32.view(np.uint32)


def replay(states, draws):
    """-> {series_field: array}: the words of every series, unpacked (hd and hp as themselves, not XORed)"""
    hh, hd, hp = _libs()
    q, v, a, xi = split(states)
    out = {}
    for name, fn in zip(SERIES, (hh.hh_step_rows, hd.hh_step_rows, hp.hp_step)):
        o = step(fn, 1, q, v, a, xi)
        for k in FIELDS:
            out[name + "_" + k] = bits(o[k])
        out[name + "_done"] = o["done"]; out[name + "_nrows"] = o["nrows"]
    o = reset(hp, 1, np.asarray(draws, dtype=np.float64), xi[:len(draws)])
    for k in ("qpos", "qvel", "obs", "xout"):
        out["hpr_" + k] = bits(o[k])
    return out


def pack(words):
    out = dict(words)
    for name in SERIES[1:]:
        for k in FIELDS:
            out[name + "_" + k] = words[name + "_" + k] ^ words["hh_" + k]
    return out


unpack = pack      # XOR with the (unchanged) hh words is its own inverse


def main():
    hh = _libs()[0]
    cand = pool(hh)
    if "--pool" in sys.argv:
        q, v, a, xi = split(cand)
        hh, hd, hp = _libs()
        nr = [step(fn, 1, q, v, a, xi)["nrows"] for fn in (hh.hh_step_rows, hd.hh_step_rows, hp.hp_step)]
        for i in range(len(cand)):
            print(i, nr[0][i], nr[1][i], nr[2][i])
        return
    states = cand[list(PICK)]
    assert len(states) <= 16
    draws = np.random.RandomState(202).uniform(0, 1, (N_RESET, 47)).astype(np.float32)
    words = replay(states, draws)
    for name in SERIES:
        assert coverage(words[name + "_nrows"]) == ALL_PATHS, (name, sorted(ALL_PATHS - coverage(words[name + "_nrows"])))
        print(name, "rows of the last evaluation:", words[name + "_nrows"].tolist())
    np.savez_compressed(PATH, states=states, draws=draws, **pack(words))
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
