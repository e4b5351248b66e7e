"""Every random number the kernels draw, per lane, against tests/rng_oracle.py: which word of which Philox stream becomes which number.

The statistical tests (test_gpu_reset_dr.py, test_gpu_surface.py) pass with a draw taken from the wrong region, the wrong subsequence, the wrong
step or one redraw too many; test_gpu_fused_reset_bits.py compares two kernels that share the stream constants and the sample_task body.  Here
the reference is independent: Python-int Philox, rocRAND's conversions restated (and held to rocRAND's own engine on the host by
test_rng_oracle_host.py), reset_model / sample_task restated from the reference.

Shapes: batch 200 = four 64-lane blocks with a ragged last one, and an odd number of pairs (4) in the last wave of the two-lanes-per-env kernels
(200 envs = 400 lanes = 6 waves + 16 lanes).  seed = 2^33 + 11 and env_offset = 2^32 + 7 have bits above 32 in the key and in the subsequence;
episodes 4 and 5 (init-state case) put a bit above 32 into the block counter.  Episodes and step counts are read from get_full_state().

Tolerances.  Uniform draws are a fixed fp32 expression of at most four roundings behind the word: atol = 4 * 2^-24 * (|offset| + scale) (a
wrong word misses by about `scale`, 10^3 times that at least).  Where a normal or truncnorm2 enters, the device evaluates logf, __sincosf and
normcdfinvf, whose error nobody states; it was MEASURED on the MI355X over this file's own lanes against the fp64 oracle (largest absolute
error per quantity, product kernels), and each tolerance is 8 x that maximum, to absorb inputs the 200 lanes did not visit:

    quantity                              unit                    measured max     tolerance (8 x)   cap (1 % of the draw's scale)
    half-cheetah qvel (0.1 * normal)      absolute                1.395e-07        1.116e-06         1.0e-03
    truncnorm xi                          stdev of the dim        1.407e-06        1.126e-05         1.0e-02
    gaussian xi                           stdev of the dim        1.408e-06        1.126e-05         1.0e-02
    fullgaussian xi                       normalised [0, 4] box   1.514e-06        1.211e-05         2.2e-03
    observation noise                     noise_std               2.416e-05        1.933e-04         1.0e-02

(The noise figure is mostly the fp32 rounding of observation + noise: 2^-24 |obs| / noise_std.)  Every test prints its own maximum
("RNGERR ...", pytest -s), and the module the largest of the run.

Threshold lanes.  A redraw or clamp decision whose oracle draw lies closer to its bound than the tolerance cannot be predicted: such a
lane-dimension is left out of the comparison and of the gaussian_fail equality.  At most 1 % of a case's lane-dimensions may be left out and each
of "0 redraws", "1", "2" and "clamped" must keep at least 3 compared lane-dimensions; both are asserted (and, for the exclusion radius at its cap,
by test_rng_oracle_host.py without a GPU).
"""
import ctypes
import functools

import numpy as np
import pytest

import rng_oracle as R

pytestmark = pytest.mark.gpu

B = 200
SEED = (1 << 33) + 11
ENV_OFFSETS = [0, (1 << 32) + 7]
EPS = 2.0 ** -24

# 1 % of the draw's scale: 0.1 (half-cheetah qvel), sigma, the smallest normalised stdev of the fullgaussian cases (cov = A A^T + 0.05 I), noise_std
CAP = dict(cheetah_qvel=1e-3, truncnorm=1e-2, gaussian=1e-2, fullgaussian=1e-2 * 0.05 ** 0.5, noise=1e-2)
# the largest error measured on the MI355X (module docstring) and 8 x it
MEASURED = dict(cheetah_qvel=1.395e-07, truncnorm=1.407e-06, gaussian=1.408e-06, fullgaussian=1.514e-06, noise=2.416e-05)
TOL = {k: 8 * v for k, v in MEASURED.items()}
assert all(TOL[k] <= CAP[k] for k in CAP)

KIND_IDS = {"cartpole": "RandomCartPole-v0", "hopper": "RandomHopper-v0", "halfcheetah": "RandomHalfCheetah-v0", "walker2d": "RandomWalker2d-v0",
            "humanoid": "RandomHumanoid-v0"}
_seen = {}


def _record(name, value):
    _seen[name] = max(_seen.get(name, 0.0), float(value))
    print("RNGERR %s %.3e" % (name, value))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_seen):
        print("RNGERR-MAX %s %.3e (tolerance %.3e)" % (k, _seen[k], TOL.get(k, float("nan"))))


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64)


def _lanes(env):
    """(episode, t) of every env as Python-int arrays, read from the handle"""
    st = env.get_full_state()
    return st["episode"].cpu().numpy().view(np.uint32).astype(np.int64), st["t"].cpu().numpy().astype(np.int64)


def _make(eid, off, **kw):
    import random_envs_amd as rex
    return rex.make(eid, batch=B, seed=SEED, env_offset=off, **kw)


@functools.lru_cache(maxsize=None)
def _init(kind, subseq, ep):
    return R.init_state(kind, SEED, subseq, ep)[:2]


def check_init_state(kind, off, q, v, ep, lanes=None, tag=()):
    """qpos / qvel [B, .] of the lanes `lanes` against init_state at their episodes"""
    nq, nv, c, _ = R.INIT_KINDS[kind]
    q0 = R.init_qpos(kind)
    lanes = range(B) if lanes is None else lanes
    ref = [_init(kind, off + i, int(ep[i])) for i in lanes]
    rq, rv = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
    idx = np.array(list(lanes))
    eq = np.abs(q[idx] - rq); tq = 4 * EPS * (np.abs(q0) + c)
    assert (eq <= tq[None]).all(), tag + ("qpos", float((eq / tq[None]).max()), np.argwhere(eq > tq[None])[:5].tolist())
    ev = np.abs(v[idx] - rv)
    if kind == "halfcheetah":
        _record("cheetah_qvel", ev.max())
        assert ev.max() <= TOL["cheetah_qvel"], tag + ("qvel", float(ev.max()))
    else:
        assert (ev <= 4 * EPS * c).all(), tag + ("qvel", float(ev.max() / (4 * EPS * c)), np.argwhere(ev > 4 * EPS * c)[:5].tolist())


# ------------------------------------------------------------------------------------------------------------------- (a) init state
@pytest.mark.parametrize("off", ENV_OFFSETS)
@pytest.mark.parametrize("kind", sorted(KIND_IDS))
def test_init_state_is_the_oracles_words(kind, off):
    """reset(), then four masked resets over the lanes with bit j of their index set: lane i ends in episode 1 + popcount(i & 15), 1..5"""
    import torch
    env = _make(KIND_IDS[kind], off, autoreset=False)
    env.reset()
    for j in range(-1, 4):
        if j >= 0:
            env.reset(mask=((torch.arange(B) >> j) & 1).to(torch.uint8))
        ep, t = _lanes(env)
        want = 1 + np.array([bin(i & ((1 << (j + 1)) - 1)).count("1") for i in range(B)])
        assert np.array_equal(ep, want) and not t.any(), (kind, off, j)
        q, v = env.get_state()
        check_init_state(kind, off, _np(q), _np(v), ep, tag=(kind, off, "after masked reset %d" % j))
    assert set(ep.tolist()) == {1, 2, 3, 4, 5}
    env.close()


# ------------------------------------------------------------------------------------------------------------------- (b) xi at reset
NEAR = (0, 1, 2)      # the dimensions whose mean sits next to the bound
XI_IDS = ["RandomHopper-v0", "RandomWalker2d-v0", "RandomHumanoid-v0", "RandomCartPole-v0", "RandomWalker2dUnmodeled-v0", "RandomHumanoidUnmodeled-v0"]
MODES = ["uniform", "truncnorm", "gaussian", "fullgaussian"]


def dr_case(spec, mode):
    """(dr_type, the argument of set_dr_distribution, the oracle's distribution block) of a case; parameters that reach every branch"""
    nom = np.asarray(spec.nominal_task, dtype=np.float64); d = len(nom)
    lower = np.asarray(spec.lower_bounds, dtype=np.float64)
    b = np.asarray(spec.search_bounds, dtype=np.float64)
    if mode == "uniform":
        dr_type, distr = "uniform", np.stack([0.9 * nom, 1.1 * nom], 1).ravel().tolist()
    elif mode == "truncnorm":             # mean = lower + 0.5 sigma on three dimensions: P(below) = 0.2994 per draw
        std = 0.1 * nom; mean = nom.copy()
        mean[list(NEAR)] = lower[list(NEAR)] + 0.5 * std[list(NEAR)]
        dr_type, distr = "truncnorm", np.stack([mean, std], 1).ravel().tolist()
    elif mode == "gaussian":              # mean 0.15, sigma 0.1 on three dimensions: P(< 0.1) = 0.3085 per draw
        std = 0.1 * nom; mean = nom.copy()
        mean[list(NEAR)] = 0.15; std[list(NEAR)] = 0.1
        dr_type, distr = "gaussian", np.stack([mean, std], 1).ravel().tolist()
    elif mode == "gaussian_wide":         # test_gpu_fused_reset_bits.py's: the redraw rule fires on the light bodies, the models stay steppable
        dr_type, distr = "gaussian", np.stack([nom, 0.4 * nom], 1).ravel().tolist()
    elif mode == "fullgaussian":          # both clips act: means 0.2 and 3.8 on two dimensions each
        A = np.random.RandomState(0).randn(d, d) * 0.1
        mean = np.full(d, 2.0); mean[:2] = 0.2; mean[2:4] = 3.8
        dr_type, distr = "fullgaussian", {"mean": mean, "cov": A @ A.T + 0.05 * np.eye(d)}
    else:
        raise AssertionError(mode)
    return dr_type, distr, R.dr_params(dr_type, distr, lower_bounds=lower, search_bounds=(b[:, 0], b[:, 1]))


def xi_tolerance(dr, radius=None):
    """(atol [dim] of a compared xi, the radius inside which a threshold decision is left out, in the unit of sample_task's margin)"""
    t = dr["type"]
    if t == "uniform":
        return 4 * EPS * (np.maximum(np.abs(dr["a"]), np.abs(dr["b"])) + np.abs(dr["b"] - dr["a"])), 0.0
    if t == "fullgaussian":
        return TOL["fullgaussian"] * (dr["hi"] - dr["lo"]) / 4, 0.0
    return TOL[t] * dr["b"], (TOL[t] if radius is None else radius)


def branch_census(outs, radius):
    """(compared [n, dim] bool, counts of compared lane-dimensions per branch) of oracle draws under an exclusion radius"""
    margin = np.array([o["margin"] for o in outs]); red = np.array([o["redraws"] for o in outs]); cl = np.array([o["clamped"] for o in outs])
    keep = margin >= radius
    return keep, {"0 redraws": int((keep & (red == 0)).sum()), "1 redraw": int((keep & (red == 1)).sum()),
                  "2 redraws": int((keep & (red == 2) & ~cl).sum()), "clamped": int((keep & cl).sum())}


def check_xi(dr, xi_dev, outs, tag, populated=True):
    """device xi rows [n, dim] against the oracle's draws `outs`; returns the (lowest, highest) number of gaussian clamps the device may count"""
    atol, radius = xi_tolerance(dr)
    ref = np.array([o["xi"] for o in outs])
    keep, census = branch_census(outs, radius)
    err = np.abs(xi_dev - ref)
    if dr["type"] in ("truncnorm", "gaussian"):
        assert (~keep).sum() <= 0.01 * keep.size, tag + ("threshold lane-dimensions", int((~keep).sum()))
        if populated:
            assert min(census.values()) >= 3, tag + (census,)
        _record(dr["type"], (err / dr["b"][None])[keep].max())
    elif dr["type"] == "fullgaussian":
        clip = np.array([o["clamped"] for o in outs])
        mid = 0.5 * (dr["lo"] + dr["hi"])[None]
        lo_hit = int((clip & (ref < mid)).sum()); hi_hit = int((clip & (ref > mid)).sum())
        if populated:
            assert lo_hit >= 3 and hi_hit >= 3, tag + (lo_hit, hi_hit)
        _record("fullgaussian", (err * 4 / (dr["hi"] - dr["lo"])[None]).max())
    bad = keep & (err > atol[None])
    assert not bad.any(), tag + ("xi", np.argwhere(bad)[:5].tolist(), float((err / atol[None])[keep].max()))
    if dr["type"] != "gaussian":
        return 0, 0
    cl = np.array([o["clamped"] for o in outs])
    sure = int((keep & cl).sum())
    return sure, sure + int((~keep).sum())


def _xi_case(eid, mode):
    from random_envs_amd import registry
    return dr_case(registry.spec(eid), mode)


@pytest.mark.parametrize("off", ENV_OFFSETS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("eid", XI_IDS)
def test_xi_at_reset(eid, mode, off):
    import torch
    from random_envs_amd import _native
    dr_type, distr, dr = _xi_case(eid, mode)
    env = _make(eid, off, autoreset=False)
    tag = (eid, mode, off)
    cart = env.kind == "cartpole"
    frozen = None
    if env.unmodeled and env.kind == "humanoid":      # body masses as the kernels hold them: cinert[b][9] of the observation = mass of body b
        def masses():
            o = torch.empty(376, B, device="cuda")
            _native.check(_native.lib().rex_get_obs(env._h, ctypes.c_void_p(o.data_ptr()), env._stream()))
            return _np(o.t())[:, [45 + 10 * b + 9 for b in range(1, 14)]]
        frozen = masses()
        from random_envs_amd.specs import SPECS
        full_nom = np.asarray(SPECS["humanoid"].nominal_task)[:13].astype(np.float32).astype(np.float64)
        assert np.allclose(frozen[:, :4], 0.8 * full_nom[None, :4], rtol=1e-6) and np.allclose(frozen[:, 4:], full_nom[None, 4:], rtol=1e-6), tag
    env.set_dr_distribution(dr_type, distr)
    env.set_dr_training(True)
    fails = env.counters()["gaussian_fail"]
    third = (torch.arange(B) % 3 == 0).to(torch.uint8)
    for mask in (None, third):
        ep0, _ = _lanes(env)
        before = _np(env.get_task())
        if cart:                       # CartPole.reset() never resamples: set_random_task is its sampling call
            env.set_random_task(mask)
        else:
            env.reset(mask=mask)
        ep, _ = _lanes(env)
        hit = np.ones(B, dtype=bool) if mask is None else third.numpy().astype(bool)
        assert np.array_equal(ep, ep0 + hit), tag
        xi = _np(env.get_task())
        assert xi.shape == (B, dr["dim"]) and np.array_equal(xi[~hit], before[~hit]), tag
        lanes = np.where(hit)[0]
        outs = [R.reset_xi(dr, SEED, off + int(i), int(ep[i])) for i in lanes]
        lo, hi = check_xi(dr, xi[lanes], outs, tag + ("all" if mask is None else "every third",), populated=mask is None)
        now = env.counters()["gaussian_fail"]
        assert lo <= now - fails <= hi, tag + ("gaussian_fail", now - fails, lo, hi)
        fails = now
    if frozen is not None:             # frozen rows keep their values; task columns 0..8 are the masses of bodies 5..13
        m = masses()
        assert np.array_equal(m[:, :4], frozen[:, :4]) and np.allclose(m[:, 4:], xi[:, :9], rtol=1e-6), tag
    if env.unmodeled:
        assert dr["dim"] == len(env.original_task) < {"walker2d": 13, "humanoid": 30}[env.kind]
    env.close()


# ------------------------------------------------------------------------------------------------------------------- (c) fused auto-reset
def _fused_case(eid, kind, shape, mode, off, fall):
    import torch
    dr_type, distr, dr = _xi_case(eid, mode)
    env = _make(eid, off, autoreset=True)
    got = env.set_launch_shape(**shape)
    assert all(got[k] == v for k, v in shape.items()), (shape, got)
    tag = (eid, mode, off, str(shape))
    env.set_dr_distribution(dr_type, distr); env.set_dr_training(True)
    env.reset()
    q, v = env.get_state()
    q = q.clone(); v = v.clone()
    fallen = np.arange(B) % 3 == 0
    fall(q, torch.as_tensor(fallen))
    env.set_state(q, v)
    ep0, t0 = _lanes(env)
    xi0 = env.get_task().clone()
    fails = env.counters()["gaussian_fail"]
    obs, r, d, info = env.step(torch.zeros(B, env.dims.act_dim))
    obs = _np(obs)
    assert np.array_equal(d.cpu().numpy(), fallen), tag + ("done",)
    ep, t = _lanes(env)
    assert np.array_equal(ep, ep0 + fallen) and np.array_equal(t, np.where(fallen, 0, t0 + 1)), tag
    xi = env.get_task()
    assert torch.equal(xi[~torch.as_tensor(fallen)], xi0[~torch.as_tensor(fallen)]), tag + ("xi of the running envs",)
    lanes = np.where(fallen)[0]
    qn, vn = env.get_state(); qn, vn = _np(qn), _np(vn)
    check_init_state(kind, off, qn, vn, ep, lanes=lanes.tolist(), tag=tag)
    if kind == "hopper":               # the new episode's observation: concat(qpos[1:], qvel) of the new state, bit for bit
        assert np.array_equal(obs[lanes], np.concatenate([qn[lanes, 1:], vn[lanes]], 1)), tag + ("obs",)
    outs = [R.reset_xi(dr, SEED, off + int(i), int(ep[i])) for i in lanes]
    lo, hi = check_xi(dr, _np(xi)[lanes], outs, tag, populated=False)
    now = env.counters()["gaussian_fail"]
    assert lo <= now - fails <= hi, tag + ("gaussian_fail", now - fails, lo, hi)
    env.close()


PLANAR_SHAPES = {"pair": dict(lanes=64, pair=True, rolled=False), "one-lane": dict(lanes=64, pair=False, rolled=False)}
HUM_SHAPES = {"pair": dict(lanes=64, hum_pair=True), "one-lane-64": dict(lanes=64, hum_pair=False), "one-lane-32": dict(lanes=32, hum_pair=False)}


@pytest.mark.parametrize("off", ENV_OFFSETS)
@pytest.mark.parametrize("mode", ["uniform", "gaussian_wide"])
@pytest.mark.parametrize("shape", sorted(PLANAR_SHAPES))
def test_hopper_fused_reset_draws_the_reset_streams(shape, mode, off):
    """every third env starts with the torso pitched past the 0.2 rad of the done rule (random_hopper.py:92): one step ends its episode"""
    def fall(q, m):
        q[m, 2] = 0.5
    _fused_case("RandomHopper-v0", "hopper", PLANAR_SHAPES[shape], mode, off, fall)


@pytest.mark.parametrize("off", ENV_OFFSETS)
@pytest.mark.parametrize("shape", sorted(HUM_SHAPES))
def test_humanoid_auto_reset_draws_the_reset_streams(shape, off):
    """every third env starts with its torso at 0.9 < 1.0 (random_humanoid.py:176-177): one step ends its episode"""
    def fall(q, m):
        q[m, 2] = 0.9
    _fused_case("RandomHumanoid-v0", "humanoid", HUM_SHAPES[shape], "gaussian_wide", off, fall)


# ------------------------------------------------------------------------------------------------------------------- (d) observation noise
NOISE_IDS = {"hopper": ("RandomHopperNoisy-v0", "RandomHopper-v0", 11), "halfcheetah": ("RandomHalfCheetahNoisy-v0", "RandomHalfCheetah-v0", 17),
             "walker2d": ("RandomWalker2dNoisy-v0", "RandomWalker2d-v0", 17), "humanoid": ("RandomHumanoidNoisy-v0", "RandomHumanoid-v0", 45)}
NOISE_CASES = [(k, s) for k in ("hopper", "halfcheetah", "walker2d") for s in sorted(PLANAR_SHAPES)] + [("humanoid", "pair"), ("humanoid", "one-lane-64")]


@pytest.mark.parametrize("off", ENV_OFFSETS)
@pytest.mark.parametrize("kind,shape", NOISE_CASES)
def test_observation_noise_is_the_step_region_of_the_stream(kind, shape, off):
    import torch
    noisy_id, plain_id, n = NOISE_IDS[kind]
    sh = (HUM_SHAPES if kind == "humanoid" else PLANAR_SHAPES)[shape]
    twins = []
    for eid in (noisy_id, plain_id):
        env = _make(eid, off, autoreset=False)
        got = env.set_launch_shape(**sh)
        assert all(got[k] == v for k, v in sh.items()), (sh, got)
        twins.append(env)
    noisy, plain = twins
    assert noisy.noisy and not plain.noisy
    std = float(np.sqrt(np.float32(noisy.noise_level)))
    tag = (kind, shape, off)

    def check(o_noisy, o_plain, lanes, what):
        a, b = noisy.get_full_state(), plain.get_full_state()
        for k in ("qpos", "qvel", "t", "episode", "done"):
            x, y = a[k], b[k]
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), tag + (what, "twin states differ", k)
        ep, t = _lanes(noisy)
        diff = _np(o_noisy) - _np(o_plain)
        assert not diff[:, n:].any(), tag + (what, "noise on a row that takes none")
        ref = np.array([R.obs_noise(SEED, off + int(i), int(ep[i]), int(t[i]), n)[0] for i in lanes])
        err = np.abs(diff[lanes, :n] - std * ref) / std
        _record("noise", err.max())
        assert err.max() <= TOL["noise"], tag + (what, float(err.max()), np.argwhere(err > TOL["noise"])[:5].tolist())
        return ep, t

    everyone = np.arange(B)
    ep, t = check(noisy.reset().clone(), plain.reset().clone(), everyone, "reset")
    assert (ep == 1).all() and not t.any()
    g = torch.Generator().manual_seed(3)
    for step in range(3):
        act = torch.rand(B, noisy.dims.act_dim, generator=g) * 0.2 - 0.1
        on = noisy.step(act)[0].clone(); op = plain.step(act)[0].clone()
        ep, t = check(on, op, everyone, "step %d" % (step + 1))
        assert (t == step + 1).all() and (ep == 1).all()
    third = (torch.arange(B) % 3 == 0).to(torch.uint8)
    hit = np.where(third.numpy())[0]
    ep, t = check(noisy.reset(mask=third).clone(), plain.reset(mask=third).clone(), hit, "masked reset")    # (the other lanes' rows are not rewritten)
    assert (ep[hit] == 2).all() and not t[hit].any() and (t[np.arange(B) % 3 != 0] == 3).all()
    act = torch.rand(B, noisy.dims.act_dim, generator=g) * 0.2 - 0.1
    on = noisy.step(act)[0].clone(); op = plain.step(act)[0].clone()
    ep, t = check(on, op, everyone, "step behind the masked reset")
    assert set(t.tolist()) == {1, 4} and set(ep.tolist()) == {1, 2}
    noisy.close(); plain.close()


# ------------------------------------------------------------------------------------------------------------------- (e) env.sample_task()
@pytest.mark.parametrize("off", ENV_OFFSETS)
@pytest.mark.parametrize("eid,mode", [("RandomHopper-v0", "gaussian"), ("RandomWalker2dUnmodeled-v0", "truncnorm"), ("RandomHumanoid-v0", "fullgaussian"),
                                      ("RandomCartPole-v0", "uniform")])
def test_sample_task_draws_its_own_stream_family(eid, mode, off):
    import torch
    dr_type, distr, dr = _xi_case(eid, mode)
    env = _make(eid, off, autoreset=False)
    env.set_dr_distribution(dr_type, distr); env.set_dr_training(True)
    env.reset()
    task0 = env.get_task().clone(); ep0, t0 = _lanes(env); c0 = env.counters()
    lo = hi = 0
    for k in range(3):
        xi = _np(env.sample_task())
        assert xi.shape == (B, dr["dim"])
        outs = [R.sample_task_draw(dr, SEED, off + i, k) for i in range(B)]
        a, b = check_xi(dr, xi, outs, (eid, mode, off, "draw %d" % k), populated=True)
        lo += a; hi += b
    c1 = env.counters(); ep1, t1 = _lanes(env)
    assert torch.equal(env.get_task(), task0) and np.array_equal(ep0, ep1) and np.array_equal(t0, t1)
    assert lo <= c1["gaussian_fail"] - c0["gaussian_fail"] <= hi, (eid, mode, off, c0, c1, lo, hi)
    assert all(c1[k] == c0[k] for k in c0 if k != "gaussian_fail")
    env.close()
