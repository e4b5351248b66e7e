"""Python-int / numpy restatement of the device random streams of csrc/device_rng.hpp -- TEST ORACLE ONLY.

It says, for one lane, WHICH WORD OF WHICH PHILOX STREAM BECOMES WHICH NUMBER.  Nothing here shares code with the kernels or with rocRAND:
the generator is ``replay_buffer_oracle.philox4x32_10`` (Python ints, held to Random123's known-answer vectors), the conversions restate
rocRAND's published expressions, and the consumers restate the reference's ``reset_model`` / ``sample_task`` plus the draw order the kernels
document.  tests/test_rng_oracle_host.py holds this file to rocRAND's own engine compiled for the host.

The stream map (device_rng.hpp):

* key ``(lo32(seed), hi32(seed))``, counter ``(lo32(offset >> 2), hi32(offset >> 2), lo32(subseq), hi32(subseq))``, draw ``j`` of a stream is
  word ``(offset + j) & 3`` of block ``(offset + j) >> 2``;
* subsequence = GLOBAL env index ``env_offset + i``;
* offset = ``episode * 2^32`` + a region: ``[0, 256)`` init-state noise, ``[256, 512)`` xi draws, ``512 + 64 t`` the observation noise of step t;
* ``rex_sample_task``: key ``seed ^ SAMPLE_SEED_SALT``, offset ``256 * draw_index``.

Conversions (rocrand_uniform.h, rocrand_normal.h): ``uniform`` is fp32 arithmetic and restated in fp32, bit for bit; ``normal2`` takes the fp32
``u`` and ``v`` rocRAND forms and evaluates Box-Muller in fp64 (the engine's own logf / sinf / cosf are what a test allows a tolerance for).
Everything behind a conversion (scaling, redraw rules, Cholesky product, denormalisation) is fp64 arithmetic over the fp32 PARAMETER values
the host layer uploads, so the oracle carries no rounding of its own beyond the conversion's.
"""
import functools
import math

import numpy as np

from replay_buffer_oracle import M32, philox4x32_10

# the layout of device_rng.hpp: philox_episode(ep) = ep * EP_STRIDE + INIT_BASE, philox_task(ep) = ... + XI_BASE, philox_step(ep, t) = ... + STEP_BASE + t * STEP_STRIDE
EP_STRIDE = 1 << 32
INIT_BASE, XI_BASE, STEP_BASE, STEP_STRIDE = 0, 256, 512, 64
INIT_WORDS, XI_WORDS, STEP_WORDS, SAMPLE_WORDS = 256, 256, 64, 256     # the budget of each region
SAMPLE_SEED_SALT = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1

_F = np.float32
_INV32 = _F(2.3283064e-10)        # ROCRAND_2POW32_INV
_INV32_2PI = _F(1.46291807e-09)   # ROCRAND_2POW32_INV_2PI

try:                                   # an fp64 inverse normal CDF
    from scipy.special import ndtri as _ndtri
except Exception:                      # pragma: no cover
    import statistics
    _ndtri = statistics.NormalDist().inv_cdf
PHI_M2, PHI_P2 = 0.022750131948179195, 0.9772498680518208   # Phi(-2), Phi(2)


@functools.lru_cache(maxsize=1 << 16)
def _block(seed, subseq, blk):
    return philox4x32_10((blk & M32, (blk >> 32) & M32, subseq & M32, (subseq >> 32) & M32), (seed & M32, (seed >> 32) & M32))


def word(seed, subseq, offset):
    """The 32-bit word the engine returns first after rocrand_init(seed, subseq, offset)."""
    seed, subseq, offset = int(seed) & M64, int(subseq) & M64, int(offset) & M64
    return _block(seed, subseq, offset >> 2)[offset & 3]


def uniform(w):
    """rocRAND's uniform_distribution(unsigned): (0, 1], fp32, two roundings behind the int -> float conversion."""
    return _INV32 + _F(int(w)) * _INV32


@functools.lru_cache(maxsize=1 << 16)
def normal2(w0, w1):
    """rocRAND's box_muller(x, y) with fp32 u, v and fp64 transcendentals: (.x = s sin v, .y = s cos v)."""
    u = float(_INV32 + _F(int(w0)) * _INV32)
    v = float(_INV32_2PI + _F(int(w1)) * _INV32_2PI)
    s = math.sqrt(-2.0 * math.log(u))
    return s * math.sin(v), s * math.cos(v)


@functools.lru_cache(maxsize=1 << 16)
def normal_scale(w0):
    """s = sqrt(-2 ln u) of the pair whose first word is w0 (what an error bound of a normal scales with)"""
    return math.sqrt(-2.0 * math.log(float(_INV32 + _F(int(w0)) * _INV32)))


class Stream:
    """The engine's draw sequence from (seed, subseq, offset): uniform() takes one word; normal() takes two and keeps rocrand_normal's
    pairing -- .x now, the saved .y at the next normal() call, whatever uniform() calls come in between."""

    def __init__(self, seed, subseq, offset):
        self.seed, self.subseq, self.offset = int(seed) & M64, int(subseq) & M64, int(offset)
        self.words_used = 0
        self._saved = None
        self.last_scale = None       # s of the Box-Muller pair the last normal() came from

    def next_word(self):
        w = word(self.seed, self.subseq, self.offset + self.words_used)
        self.words_used += 1
        return w

    def uniform(self):
        return uniform(self.next_word())

    def normal(self):
        if self._saved is not None:
            y, self._saved = self._saved, None
            return y
        w0, w1 = self.next_word(), self.next_word()
        x, y = normal2(w0, w1)
        self._saved, self.last_scale = y, normal_scale(w0)
        return x


# ------------------------------------------------------------------------------------------------------------------------------------
# init-state noise: reset_model of the five kinds (random_cartpole.py:226-229, random_hopper.py:112-120, random_half_cheetah.py:123-131,
# random_walker2d.py:144-153, random_humanoid.py:219-234) in the kernels' documented draw order.  The fp32 constants are the kernels'.
# ------------------------------------------------------------------------------------------------------------------------------------
INIT_KINDS = {   # kind: (nq, nv, c, {row of init_qpos: value})
    "cartpole": (2, 2, float(_F(0.05)), {}),
    "hopper": (6, 6, float(_F(0.005)), {1: 1.25}),
    "walker2d": (9, 9, float(_F(0.005)), {1: 1.25}),
    "halfcheetah": (9, 9, float(_F(0.1)), {}),
    "humanoid": (24, 23, float(_F(0.01)), {2: 1.4, 3: 1.0}),
}


def init_qpos(kind):
    nq, _, _, rows = INIT_KINDS[kind]
    q0 = np.zeros(nq)
    for k, val in rows.items():
        q0[k] = val
    return q0


def _sym(st, c):
    return c * (2.0 * (1.0 - float(st.uniform())) - 1.0)


def init_state(kind, seed, subseq, episode):
    """(qpos, qvel, words_used) in fp64 of the reset of `episode` (the value s.episode holds AFTER the reset)."""
    nq, nv, c, _ = INIT_KINDS[kind]
    st = Stream(seed, subseq, int(episode) * EP_STRIDE + INIT_BASE)
    q, v = init_qpos(kind), np.zeros(nv)
    if kind == "cartpole":      # U(-0.05, 0.05)^4 stored as x, x_dot, theta, theta_dot; qpos = (x, theta), qvel = (x_dot, theta_dot)
        d = [float(-_F(0.05)) + float(_F(0.1)) * (1.0 - float(st.uniform())) for _ in range(4)]
        q[:] = (d[0], d[2]); v[:] = (d[1], d[3])
    elif kind in ("hopper", "walker2d"):      # word 2 k -> qpos[k], word 2 k + 1 -> qvel[k]
        for k in range(nv):
            q[k] += _sym(st, c)
            v[k] = _sym(st, c)
    elif kind == "halfcheetah":               # uniform qpos[k], then 0.1 * normal for qvel[k]: words (qpos[2p], pair, pair, qpos[2p+1])
        for k in range(nv):
            q[k] += _sym(st, c)
            v[k] = float(_F(0.1)) * st.normal()
    elif kind == "humanoid":                  # q[0..23], then v[0..22]
        for k in range(nq):
            q[k] += _sym(st, c)
        for k in range(nv):
            v[k] = _sym(st, c)
    else:
        raise KeyError(kind)
    return q, v, st.words_used


def init_words(kind):
    """words one reset takes from the init region (no data-dependent draws)"""
    return init_state(kind, 1, 0, 1)[2]


# ------------------------------------------------------------------------------------------------------------------------------------
# RandomEnv.sample_task (random_env.py:148-220; truncnorm: the intended rule)
# ------------------------------------------------------------------------------------------------------------------------------------
def dr_params(dr_type, distr, lower_bounds=None, search_bounds=None):
    """The distribution block as the host layer uploads it (dr.py / vec_env._push_dr): every parameter rounded to fp32, the fullgaussian
    covariance as the fp32 of its fp64 lower Cholesky factor.  `distr`: the argument of set_dr_distribution."""
    f = lambda x: np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)
    dr = {"type": dr_type}
    if dr_type in ("uniform", "truncnorm", "gaussian"):
        p = f(distr).reshape(-1, 2)
        dr["a"], dr["b"] = p[:, 0].copy(), p[:, 1].copy()
        dr["dim"] = len(p)
    elif dr_type == "fullgaussian":
        dr["a"] = f(distr["mean"])
        dr["dim"] = len(dr["a"])
        dr["chol"] = f(np.linalg.cholesky(np.asarray(distr["cov"], dtype=np.float64)))
        lo, hi = search_bounds
        dr["lo"], dr["hi"] = f(lo), f(hi)
    else:
        raise ValueError("Unknown dr_type:" + str(dr_type))
    dr["lower"] = f(lower_bounds) if lower_bounds is not None else np.zeros(dr["dim"])
    return dr


def truncnorm2(u):
    """truncated standard normal on [-2, 2] by inverse CDF of the uniform u"""
    return min(max(float(_ndtri(PHI_M2 + float(u) * (PHI_P2 - PHI_M2))), -2.0), 2.0)


def xi_words_worst(dr_type, dim):
    """worst-case words one sample_task call takes from its region"""
    if dr_type == "uniform":
        return dim
    if dr_type == "truncnorm":
        return 3 * dim
    if dr_type == "gaussian":         # three normals per dim, each pair of normals two words: never more than one word per normal + 1
        return 3 * dim + (3 * dim) % 2
    if dr_type == "fullgaussian":
        return 2 * ((dim + 1) // 2)
    raise ValueError(dr_type)


def sample_task(dr, seed, subseq, offset):
    """One lane's xi in TASK order.  Returns a dict: xi [dim] fp64; redraws [dim] (0, 1 or 2); clamped [dim] (truncnorm: set to the lower
    bound, gaussian: set to 0.1 and counted, fullgaussian: a clip acted); margin [dim]: the smallest distance of a compared draw from its
    threshold, in units of the dimension's stdev (inf where nothing is compared); scale [dim]: the largest Box-Muller s among the normals
    that entered (0 where none did); words_used."""
    d, t = dr["dim"], dr["type"]
    xi, red, clamp = np.zeros(d), np.zeros(d, dtype=np.int64), np.zeros(d, dtype=bool)
    margin, scale = np.full(d, np.inf), np.zeros(d)
    st = Stream(seed, subseq, offset)
    if t == "uniform":                 # lo + (hi - lo) (1 - u)
        for k in range(d):
            xi[k] = dr["a"][k] + (dr["b"][k] - dr["a"][k]) * (1.0 - float(st.uniform()))
    elif t in ("truncnorm", "gaussian"):
        for k in range(d):
            m, s = dr["a"][k], dr["b"][k]
            floor = dr["lower"][k] if t == "truncnorm" else float(_F(0.1))

            def draw():
                if t == "truncnorm":
                    return m + s * truncnorm2(st.uniform())
                z = st.normal()
                scale[k] = max(scale[k], st.last_scale)
                return m + s * z
            obs = draw()
            margin[k] = abs(obs - floor) / s
            while obs < floor and red[k] < 2:          # at most two redraws are kept
                obs = draw(); red[k] += 1
                margin[k] = min(margin[k], abs(obs - floor) / s)
            if obs < floor:
                obs, clamp[k] = floor, True
            xi[k] = obs
    elif t == "fullgaussian":          # mean + L z in the normalised [0, 4]^d box, clip, denormalise; z replayed from the region's start per row
        for k in range(d):
            sz = Stream(seed, subseq, offset)
            acc = dr["a"][k]
            for j in range(k + 1):
                acc += dr["chol"][k, j] * sz.normal()
                scale[k] = max(scale[k], sz.last_scale)
            st.words_used = max(st.words_used, sz.words_used)
            clamp[k] = acc < 0.0 or acc > 4.0
            acc = min(max(acc, 0.0), 4.0)
            xi[k] = acc * (dr["hi"][k] - dr["lo"][k]) * 0.25 + dr["lo"][k]
    else:
        raise ValueError('sampling value of random env needs to be set before using sample_task() or set_random_task()')
    return dict(xi=xi, redraws=red, clamped=clamp, margin=margin, scale=scale, words_used=st.words_used)


def reset_xi(dr, seed, subseq, episode):
    """sample_task at the xi region of `episode`"""
    return sample_task(dr, seed, subseq, int(episode) * EP_STRIDE + XI_BASE)


def sample_task_draw(dr, seed, subseq, draw_index):
    """what rex_sample_task returns for draw number draw_index (a stream family of its own)"""
    return sample_task(dr, (int(seed) ^ SAMPLE_SEED_SALT) & M64, subseq, int(draw_index) * SAMPLE_WORDS)


def obs_noise(seed, subseq, episode, t, n):
    """(normals [n] fp64, scales [n]): the n standard normals of the observation of step t (t = 0: the reset observation)"""
    st = Stream(seed, subseq, int(episode) * EP_STRIDE + STEP_BASE + int(t) * STEP_STRIDE)
    z, s = np.zeros(n), np.zeros(n)
    for k in range(n):
        z[k] = st.normal(); s[k] = st.last_scale
    return z, s


def obs_noise_words(n):
    return 2 * ((n + 1) // 2)
