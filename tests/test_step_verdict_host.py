"""The restated step verdict (tests/verdict_reference.py: reward, done, time limit, the non-finite rule -- written from the reference's env
files) held to the ORACLE's mjo_env_step on the oracle's own fp64 end states, on inputs that land on the thresholds of the done rule.

    coverage      every ladder, on the oracle's output alone: >= 20 lanes on each side of its threshold, >= 2 within 2e-5 of it (the eps the
                  suite grants a `done` mismatch), every end state finite, every OTHER clause >= 1e-3 from firing
    agreement     done equal, reward equal to fp64 rounding, every lane of every ladder (+ rollout states under U(-1.2, 1.2) actions; CartPole
                  at every fp32 value within 4 ulp of its four thresholds and at the four double thresholds themselves)
    misreadings   six ways of misreading the rules, each switched on in the restatement, each seen to DISAGREE with the oracle: the inputs
                  above tell them apart
    rehearsal     the poisoned inputs of tests/test_gpu_step_verdict.py (NaN / inf in the state, NaN / inf in the action) through the fp32
                  host instantiations of the engines FIRST: every solver form returns, and what it returns is recorded"""
import ctypes

import numpy as np
import pytest

import verdict_reference as vr
from verdict_reference import POISONS, poison
from oracle_bindings import DIMS, _p, oracle_cartpole_step, rollout_states

PLANAR = ("hopper", "walker2d", "halfcheetah")


def _reward_bound(*terms):
    """fp64 rounding of a sum of len(terms) terms, each itself a product or quotient: a few ulp of the sum of magnitudes"""
    return 8 * 2.0 ** -52 * sum(np.abs(t) for t in terms)


def _restate(kind, q0, o, a, xi, **kw):
    if kind == "humanoid":
        return vr.humanoid_verdict(o["com_before"], o["com_after"], o["qpos"], o["qvel"], a, **kw)
    return vr.planar_verdict(kind, q0[:, 0], o["qpos"], o["qvel"], a, **kw)


def _terms(kind, ref):
    if kind == "humanoid":
        return ref["reward_linvel"], ref["reward_quadctrl"], ref["reward_alive"]
    return ref["reward_run"], ref["reward_ctrl"], ref["reward_alive"]


@pytest.fixture(scope="module")
def random_steps():
    """per kind: rollout states (humanoid: reset poses dropped a little) under actions beyond the control range, stepped by the oracle"""
    out = {}
    for kind in PLANAR:
        q, v, xi = rollout_states(kind, 256, steps_max=40, seed=21)
        a = np.random.RandomState(2).uniform(-1.2, 1.2, (256, DIMS[kind]["nu"]))
        out[kind] = (q, v, a, xi, vr.oracle_step(kind, q, v, a, xi))
    rng = np.random.RandomState(3)
    q, v = vr._reset_state("humanoid", rng, 48); q[:, 2] -= rng.uniform(0, 0.45, 48)
    a = rng.uniform(-0.6, 0.6, (48, 17)); xi = np.tile(vr._nominal("humanoid"), (48, 1)) * rng.uniform(0.8, 1.2, (48, 30))
    out["humanoid"] = (q, v, a, xi, vr.oracle_step("humanoid", q, v, a, xi))
    return out


@pytest.mark.parametrize("kind", ["hopper", "walker2d", "humanoid"])
def test_every_ladder_meets_the_coverage_conditions(kind):
    lads = vr.ladders(kind)
    assert len(lads) == {"hopper": 15, "walker2d": 4, "humanoid": 2}[kind]
    for lad in lads:
        c = vr.ladder_coverage(lad)
        print(kind, lad["name"], c)
        assert vr.coverage_ok(c), (kind, lad["name"], c)
        assert len(lad["qpos"]) == vr.N_LADDER and vr.N_LADDER % 32 != 0
        for key in ("qpos", "qvel", "action", "xi"):      # what the kernel reads is what the oracle read
            assert np.array_equal(lad[key], lad[key].astype(np.float32).astype(np.float64)), key
        # both outcomes in the ORACLE's own done, and the clause the restatement names is the watched one
        assert lad["oracle"]["done"].any() and not lad["oracle"]["done"].all()
    assert vr.ladders("halfcheetah") == []                # random_half_cheetah.py:108: no threshold to stand on


@pytest.mark.parametrize("kind", ["hopper", "walker2d", "halfcheetah", "humanoid"])
def test_restatement_equals_the_oracle(kind, random_steps):
    """done equal and reward equal to fp64 rounding, on the oracle's own end states: every lane of every ladder and of the random steps"""
    sets = [(l["name"], l["qpos"], l["qvel"], l["action"], l["xi"], l["oracle"], l["clause_index"]) for l in vr.ladders(kind)]
    q, v, a, xi, o = random_steps[kind]
    sets.append(("random", q, v, a, xi, o, None))
    for name, q, v, a, xi, o, ci in sets:
        ref = _restate(kind, q, o, a, xi)
        assert np.array_equal(ref["done"], o["done"]), (kind, name, np.where(ref["done"] != o["done"])[0][:8])
        assert np.array_equal(ref["terminated"], o["done"]) and not ref["truncated"].any() and not ref["nonfinite"].any()
        err = np.abs(ref["reward"] - o["reward"]); bound = _reward_bound(*_terms(kind, ref))
        print(kind, name, "max |dreward| %.2e (bound %.2e), done %d of %d" % (err.max(), bound.min(), o["done"].sum(), len(err)))
        assert (err <= bound).all(), (kind, name, err.max())
        if ci is not None:                                 # on a ladder the watched clause is the one that fires, alone
            assert set(np.unique(ref["clause"])) == {-1, ci}, (kind, name, np.unique(ref["clause"]))


def _cartpole_inputs():
    state, action, xi, names = vr.cartpole_ladder()
    exact = np.zeros((4, 4)); exact[0, 0] = vr.X_THRESHOLD; exact[1, 0] = -vr.X_THRESHOLD
    exact[2, 2] = vr.THETA_THRESHOLD; exact[3, 2] = -vr.THETA_THRESHOLD            # fp64 only: ON the thresholds
    state = np.concatenate([state, exact]); action = np.concatenate([action, [0, 1, 0, 1]]); xi = np.concatenate([xi, xi[:4]])
    return state, action, xi, names + ["x_hi", "x_lo", "th_hi", "th_lo"]


def test_cartpole_restatement_equals_the_oracle():
    state, action, xi, names = _cartpole_inputs()
    nxt, r, d = oracle_cartpole_step(state, action, xi)
    assert np.array_equal(nxt[:, [0, 2]], state[:, [0, 2]])          # x_dot = theta_dot = 0: the watched coordinates do not move
    ref = vr.cartpole_verdict(nxt, np.zeros(len(d), bool))
    assert np.array_equal(ref["done"], d) and np.array_equal(ref["reward"], r)
    # fl32(2.4) and fl32(12 * 2 pi / 360) both lie ABOVE the double thresholds: the middle one of the 9 values and the 4 beyond it are past it;
    # a state ON the double threshold is not
    assert float(np.float32(vr.X_THRESHOLD)) > vr.X_THRESHOLD and float(np.float32(vr.THETA_THRESHOLD)) > vr.THETA_THRESHOLD
    assert d[:36].reshape(4, 9).sum(1).tolist() == [5, 5, 5, 5] and not d[36:].any()
    for i in np.where(d)[0]:
        assert vr.CLAUSES["cartpole"][ref["clause"][i]] == names[i]
    # steps_beyond_done (random_cartpole.py:207-222) through mjo_cartpole_step itself: reward 1 on the step that ends the episode, 0 after it
    from oracle_bindings import lib
    L = lib()
    for i in (0, 8, 20, 35):
        s = np.ascontiguousarray(state[i]); x = np.ascontiguousarray(xi[i]); o = np.zeros(4); rr = ctypes.c_double(); dd = ctypes.c_int()
        sbd = ctypes.c_int(-1); got = []
        for _ in range(2):
            L.mjo_cartpole_step(_p(s), int(action[i]), _p(x), _p(o), ctypes.byref(rr), ctypes.byref(dd), ctypes.byref(sbd))
            got.append((rr.value, bool(dd.value)))
        was = [False, got[0][1]]
        for k in range(2):
            ref1 = vr.cartpole_verdict(state[i][None], np.array([was[k]]))
            assert (float(ref1["reward"][0]), bool(ref1["done"][0])) == got[k], (i, k, got)


def test_time_limit_and_flags_of_the_restatement():
    """gym's TimeLimit on top of the rule: truncated only on the step that reaches max_episode_steps WITHOUT terminating; endless clears
    terminated on finite states only; the read-only replay never truncates"""
    lad = vr.ladders("walker2d")[0]; o = lad["oracle"]; q0 = lad["qpos"]
    last = vr.MAX_EPISODE_STEPS - 1
    r = vr.planar_verdict("walker2d", q0[:, 0], o["qpos"], o["qvel"], lad["action"], t=last)
    assert np.array_equal(r["terminated"], o["done"]) and np.array_equal(r["truncated"], ~o["done"]) and r["done"].all()
    assert not vr.planar_verdict("walker2d", q0[:, 0], o["qpos"], o["qvel"], lad["action"], t=last - 1)["truncated"].any()
    assert not vr.planar_verdict("walker2d", q0[:, 0], o["qpos"], o["qvel"], lad["action"], t=last, time_limit=False)["truncated"].any()
    assert not vr.planar_verdict("walker2d", q0[:, 0], o["qpos"], o["qvel"], lad["action"], t=last, readonly=True)["truncated"].any()
    e = vr.planar_verdict("walker2d", q0[:, 0], o["qpos"], o["qvel"], lad["action"], t=last, endless=True)
    assert not e["terminated"].any() and e["truncated"].all()
    # the contract of the non-finite lane, every kind, endless or not, on the last step of the time limit or not
    for kind in ("hopper", "walker2d", "halfcheetah", "humanoid"):
        d = DIMS[kind]
        for bad, where in ((np.nan, "v"), (np.inf, "q"), (-np.inf, "q")):
            q = np.zeros((3, d["nq"])); v = np.zeros((3, d["nv"])); q[:, 1 if kind != "humanoid" else 2] = 1.2
            (q if where == "q" else v)[1, 5] = bad
            for endless in (False, True):
                kw = dict(t=last, endless=endless)
                r = (vr.humanoid_verdict(np.zeros(3), np.zeros(3), q, v, np.zeros((3, d["nu"])), **kw) if kind == "humanoid"
                     else vr.planar_verdict(kind, np.zeros(3), q, v, np.zeros((3, d["nu"])), **kw))
                assert r["nonfinite"].tolist() == [False, True, False] and r["terminated"].tolist() == [False, True, False]
                assert r["truncated"].tolist() == [True, False, True] and r["clause"].tolist() == [-1, 0, -1]
    s = np.zeros((2, 4)); s[1, 3] = np.nan
    r = vr.cartpole_verdict(s, np.zeros(2, bool), t=3)
    assert r["terminated"].tolist() == [False, True] and r["nonfinite"].tolist() == [False, True] and not r["truncated"].any()


def _disagrees(kind, sets, misread):
    for q, v, a, xi, o in sets:
        ref = _restate(kind, q, o, a, xi, misread=misread)
        if not np.array_equal(ref["done"], o["done"]):
            return "done"
        if (np.abs(ref["reward"] - o["reward"]) > 100 * _reward_bound(*_terms(kind, ref))).any():
            return "reward"
    return None


def test_misreadings_fail(random_steps):
    """each named misreading, switched on in the restatement, disagrees with the oracle on the inputs above (and the true reading does not:
    test_restatement_equals_the_oracle)"""
    by_kind = {k: [(l["qpos"], l["qvel"], l["action"], l["xi"], l["oracle"]) for l in vr.ladders(k)] + [random_steps[k]]
               for k in ("hopper", "walker2d", "halfcheetah", "humanoid")}
    seen = {}
    seen["walker_0p7"] = _disagrees("walker2d", by_kind["walker2d"], "walker_0p7")
    seen["one_sided_ang"] = _disagrees("hopper", by_kind["hopper"], "one_sided_ang")
    seen["velocity_from_2"] = _disagrees("hopper", by_kind["hopper"], "velocity_from_2")
    seen["cheetah_alive_bonus"] = _disagrees("halfcheetah", by_kind["halfcheetah"], "cheetah_alive_bonus")
    for kind in ("hopper", "walker2d", "halfcheetah", "humanoid"):
        seen["clipped_ctrl_cost/" + kind] = _disagrees(kind, by_kind[kind], "clipped_ctrl_cost")
    state, action, xi, _ = _cartpole_inputs()
    nxt, r, d = oracle_cartpole_step(state, action, xi)
    ref = vr.cartpole_verdict(nxt, np.zeros(len(d), bool), misread="nonstrict")
    seen["nonstrict"] = None if np.array_equal(ref["done"], d) else "done"
    print(seen)
    assert set(k.split("/")[0] for k in seen) == set(vr.MISREADINGS)
    assert all(seen.values()), seen
    assert seen["walker_0p7"] == seen["one_sided_ang"] == seen["velocity_from_2"] == seen["nonstrict"] == "done"
    # which ladders catch them: the one-sided pitch only the -0.2 ladder, the velocity slice only the root-x and root-z velocity ladders
    names = [l["name"] for l in vr.ladders("hopper")]
    caught = [n for n, s in zip(names, by_kind["hopper"]) if _disagrees("hopper", [s], "one_sided_ang")]
    assert caught == ["ang@-0.2"], caught
    caught = [n for n, s in zip(names, by_kind["hopper"]) if _disagrees("hopper", [s], "velocity_from_2")]
    assert caught == ["qvel0@+100", "qvel0@-100", "qvel1@+100", "qvel1@-100"], caught


# ---- rehearsal of the poisoned inputs on the host engines ------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", PLANAR)
def test_poisoned_inputs_through_the_fp32_planar_host_engine(kind):
    """ph_step, fp32, in every form of the general solver (unrolled, rolled row list, LIST) with and without the feet-only path: the call
    returns (no solver loop is held open by a lane whose comparisons are all false), a poisoned STATE ends non-finite, a poisoned ACTION leaves
    the state finite (the actuator clamps the force: fmin / fmax drop a NaN) and the healthy lanes do not notice their neighbours"""
    from host_harness import build as hb
    d = DIMS[kind]; rng = np.random.RandomState(0); n = 6
    q, v, xi = rollout_states(kind, n, steps_max=30, seed=4)
    a = rng.uniform(-1, 1, (n, d["nu"]))
    try:
        for gen in (0, 1, 2):
            for fast in (1, 0):
                hb.set_rolled(gen); hb.set_fast(fast)
                q0, v0, _ = hb.host_step(kind, 1, q, v, a, xi, d["frame_skip"])
                for what in POISONS:
                    qq, vv, aa = poison(kind, q, v, a, what, [1, 4])
                    qo, vo, cap = hb.host_step(kind, 1, qq, vv, aa, xi, d["frame_skip"])
                    fin = np.isfinite(qo).all(1) & np.isfinite(vo).all(1)
                    print(kind, "gen", gen, "fast", fast, what, "finite", fin.astype(int).tolist(), "capped", cap.tolist())
                    assert fin[[0, 2, 3, 5]].all() and np.array_equal(qo[[0, 2, 3, 5]], q0[[0, 2, 3, 5]])
                    assert fin[[1, 4]].all() == what.endswith("action") and fin[[1, 4]].any() == what.endswith("action")
    finally:
        hb.set_rolled(0); hb.set_fast(1)


def test_poisoned_inputs_through_the_fp32_humanoid_host_engines():
    """hh_step (one lane per env) and hp_step (two lanes per env: two lock-stepped threads), fp32: both return on every poisoned input; a
    poisoned state ends non-finite, a poisoned action leaves it finite"""
    from host_harness.build import build_so
    UB = ctypes.POINTER(ctypes.c_ubyte); I = ctypes.POINTER(ctypes.c_int)
    hh = ctypes.CDLL(build_so("humanoid_host", "humanoid_host.cpp"))
    hp = ctypes.CDLL(build_so("humanoid_pair_host", "humanoid_pair_host.cpp", ["-pthread"]))
    rng = np.random.RandomState(1); n = 3
    q, v = vr._reset_state("humanoid", rng, n); q[:, 2] -= 0.35      # feet on the floor
    a = rng.uniform(-.4, .4, (n, 17)); xi = np.tile(vr._nominal("humanoid"), (n, 1))
    for what in POISONS:
        qq, vv, aa = poison("humanoid", q, v, a, what, [1])
        qs, vs, as_, xs = [np.ascontiguousarray(x.T) for x in (qq, vv, aa, xi)]
        for name in ("one lane", "pair"):
            qo = np.zeros_like(qs); vo = np.zeros_like(vs); obs = np.zeros((376, n)); r = np.zeros(n); dd = np.zeros(n, dtype=np.uint8)
            xo = np.zeros((14, n)); ov = np.zeros(n, dtype=np.int32); nr = np.zeros(n, dtype=np.int32)
            if name == "pair":
                hp.hp_step(1, n, _p(qs), _p(vs), _p(as_), _p(xs), None, _p(qo), _p(vo), _p(obs), _p(r), dd.ctypes.data_as(UB), _p(xo),
                           ov.ctypes.data_as(I), nr.ctypes.data_as(I))
            else:
                hh.hh_step(1, n, _p(qs), _p(vs), _p(as_), _p(xs), None, _p(qo), _p(vo), _p(obs), _p(r), dd.ctypes.data_as(UB), _p(xo),
                           ov.ctypes.data_as(I))
            fin = np.isfinite(qo).all(0) & np.isfinite(vo).all(0)
            print("humanoid", name, what, "finite", fin.astype(int).tolist(), "reward", r.tolist(), "overflow", ov.tolist())
            assert fin[[0, 2]].all() and fin[1] == what.endswith("action")
