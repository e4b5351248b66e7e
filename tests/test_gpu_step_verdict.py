"""The tail of the four step kernels -- reward and `info` terms, terminated / TimeLimit.truncated / done, the terminal observation, the
`nonfinite` counter and the restart of the lane -- held to tests/verdict_reference.py (the rules restated from the reference's env files)
applied to the kernel's OWN stored state, so the physics error drops out, on inputs that land on the thresholds (the ladders of
verdict_reference.py; tests/test_step_verdict_host.py holds restatement and ladders to the oracle).

The stored state is get_state() after the step; with the auto-reset on, a finished row's is read from `terminal_observation` (qpos[1:] and
qvel of the planar kinds, z first for the humanoid, all four values for CartPole).

Exempt from the exact comparison are only the lanes whose stored value sits within one fp32 ulp of a double threshold that fp32 does not
hold (0.7, 0.8, 0.2, 2.4, 12 * 2 pi / 360): there the kernel's fp32 constant and the reference's double can legitimately disagree --
walker2d at z == 0.8f is one.  They are counted and printed.

Every assertion runs over the INSTANTIATIONS of the tail (CONFIGS below x SoA / row-major x auto-reset off / fused / unfused), not over
the workload's sizes.  The tests named *nonfinite* poison lanes on purpose (NaN / inf in the state or in the action -- what a diverged policy
or a bad checkpoint produces) and run after the CPU rehearsal of the same inputs in tests/test_step_verdict_host.py."""
import numpy as np
import pytest

import verdict_reference as vr
from oracle_bindings import DIMS, oracle_cartpole_step, rollout_states
from parity_util import create_knobs

pytestmark = pytest.mark.gpu

IDS = {"hopper": "RandomHopper-v0", "walker2d": "RandomWalker2d-v0", "halfcheetah": "RandomHalfCheetah-v0", "humanoid": "RandomHumanoid-v0",
       "cartpole": "RandomCartPole-v0"}
ALIVE = {"hopper": 1.0, "walker2d": 1.0, "halfcheetah": 0.0}
CTRL_COST = {"hopper": 1e-3, "walker2d": 1e-3, "halfcheetah": 0.1}
LAST = vr.MAX_EPISODE_STEPS - 1
TOL_QPOS, TOL_QVEL_REL = 2e-5, 2e-4          # tests/test_gpu_planar.py

# the instantiations of the tail: (kind, create-time knobs)
CONFIGS = [("hopper", {}), ("hopper", dict(REX_PAIR=0)), ("hopper", dict(REX_ROLLED=1, REX_PAIR=0)),
           ("walker2d", {}), ("walker2d", dict(REX_PAIR=0)), ("halfcheetah", {}), ("halfcheetah", dict(REX_PAIR=0)),
           ("humanoid", dict(REX_HUM_PAIR=1)), ("humanoid", dict(REX_HUM_PAIR=0))]
CONFIG_IDS = ["%s-%s" % (k, "-".join("%s%s" % (n[4:].lower(), v) for n, v in sorted(kn.items())) or "default") for k, kn in CONFIGS]


def _resets(kind, knobs):
    """auto-reset variants of a configuration: off, on as the configuration has it, and -- where a knob unfuses it -- on and unfused"""
    out = [("off", False, {}, False), ("on", True, {}, False)]
    if kind == "humanoid" and knobs.get("REX_HUM_PAIR") == 1:
        out.append(("unfused", True, dict(REX_HUM_FUSED_RESET=0), False))
    if kind == "walker2d":
        out.append(("unfused", True, dict(REX_FUSED_DERIVE=0), True))      # (under DR: only then does the knob unfuse the reset)
    return out


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _make(kind, n, knobs, row_major, autoreset, time_limit=True, endless=False, dr=False, seed=7):
    import random_envs_amd as rex
    with create_knobs(**knobs):
        env = rex.make(IDS[kind], batch=n, seed=seed, autoreset=autoreset, time_limit=time_limit, row_major=row_major)
    if endless:
        env.set_endless(True)
    if dr:
        nom = np.asarray(env.original_task, dtype=np.float64)
        env.set_dr_distribution("uniform", np.stack([0.9 * nom, 1.1 * nom], 1).ravel().tolist()); env.set_dr_training(True)
    return env


def _load(env, torch, q, v, xi, t):
    """task, state and the per-lane step counter (set_counters_state through set_full_state)"""
    env.set_task(np.asarray(xi, dtype=np.float32))
    env.set_state(np.asarray(q, dtype=np.float32), np.asarray(v, dtype=np.float32))
    st = env.get_full_state()
    st["t"] = torch.full_like(st["t"], int(t)); st["done"] = torch.zeros_like(st["done"])
    env.set_full_state(st)


def _step(env, torch, a):
    """one step; everything the caller gets, as numpy copies"""
    act = torch.as_tensor(np.asarray(a), dtype=torch.int32 if env.kind == "cartpole" else torch.float32).to(env.device)
    obs, r, d, info = env.step(act.contiguous())
    out = dict(obs=obs.float().cpu().numpy().copy(), reward=r.cpu().numpy().copy(), done=d.cpu().numpy().astype(bool).copy(),
               truncated=info["TimeLimit.truncated"].cpu().numpy().astype(bool).copy(), term=info["terminal_observation"].cpu().numpy().copy())
    for name in env.INFO_TERMS[env.kind]:
        out[name] = info[name].cpu().numpy().copy()
    qq, vv = env.get_state()
    out["qpos"] = qq.cpu().numpy().copy(); out["qvel"] = vv.cpu().numpy().copy()
    return out


def _stored(kind, out, autoreset):
    """the post-step state the tail judged: get_state(), and on rows the auto-reset has already restarted the terminal observation (the
    coordinates it does not hold -- root x; the humanoid's x, y -- are zeroed: no rule reads them)"""
    q = out["qpos"].astype(np.float64).copy(); v = out["qvel"].astype(np.float64).copy()
    if autoreset and out["done"].any():
        rows = np.where(out["done"])[0]; term = out["term"][rows].astype(np.float64)
        if kind == "cartpole":
            q[rows] = term[:, [0, 2]]; v[rows] = term[:, [1, 3]]
        else:
            skip = 2 if kind == "humanoid" else 1
            nq = q.shape[1]
            q[rows, :skip] = 0.0; q[rows, skip:] = term[:, :nq - skip]; v[rows] = term[:, nq - skip:nq - skip + v.shape[1]]
    return q, v


def _verdict(kind, q, v, a, t, was_done=None, **flags):
    if kind == "cartpole":
        s = np.stack([q[:, 0], v[:, 0], q[:, 1], v[:, 1]], 1)
        return vr.cartpole_verdict(s, np.zeros(len(q), bool) if was_done is None else was_done, t=t, time_limit=flags.get("time_limit", True))
    if kind == "humanoid":
        return vr.humanoid_verdict(np.zeros(len(q)), np.zeros(len(q)), q, v, a, t=t, **flags)
    return vr.planar_verdict(kind, np.zeros(len(q)), q, v, a, t=t, **flags)


def _ties(kind, q, v):
    """lanes within one fp32 ulp of a double threshold that fp32 does not hold"""
    m = vr.clause_margins(kind, q, v)
    tie = np.zeros(len(q), bool)
    if kind == "hopper":
        cols = {0.7: [m.shape[1] - 2], 0.2: [m.shape[1] - 1]}
    elif kind == "walker2d":
        cols = {0.8: [0]}
    elif kind == "cartpole":
        cols = {vr.X_THRESHOLD: [0, 1], vr.THETA_THRESHOLD: [2, 3]}
    else:
        cols = {}
    for thr, cc in cols.items():
        assert float(np.float32(thr)) != thr
        for c in cc:
            tie |= np.abs(m[:, c]) <= float(np.spacing(np.float32(thr)))
    return tie


def _assert_verdict(tag, kind, out, ref, tie):
    """terminated and TimeLimit.truncated equal to the restated rule, every lane but the ties"""
    term = out["done"] & ~out["truncated"]
    ok = ~tie
    bad_t = np.where((term != ref["terminated"]) & ok)[0]; bad_u = np.where((out["truncated"] != ref["truncated"]) & ok)[0]
    assert bad_t.size == 0, "%s: terminated differs from the restated rule in lanes %s (clauses %s)" % (tag, bad_t[:10], ref["clause"][bad_t[:10]])
    assert bad_u.size == 0, "%s: TimeLimit.truncated differs from the restated rule in lanes %s" % (tag, bad_u[:10])
    assert not (out["truncated"] & term).any()
    return int(tie.sum())


def _batch(kind, extra=200, seed=31):
    """every ladder of `kind` in one ragged batch + `extra` rollout states under U(-1.2, 1.2) actions (the humanoid: reset poses dropped a
    little, U(-0.6, 0.6)); the oracle's step of all of it"""
    lads = vr.ladders(kind)
    rng = np.random.RandomState(seed); d = DIMS[kind]
    if kind == "humanoid":
        extra = 48
        q, v = vr._reset_state(kind, rng, extra); q[:, 2] -= rng.uniform(0, 0.45, extra)
        a = rng.uniform(-0.6, 0.6, (extra, 17)); xi = np.tile(vr._nominal(kind), (extra, 1)) * rng.uniform(0.8, 1.2, (extra, 30))
    else:
        q, v, xi = rollout_states(kind, extra, steps_max=40, seed=seed)
        a = rng.uniform(-1.2, 1.2, (extra, d["nu"]))
    q, v, a, xi = [vr._r32(x) for x in (q, v, a, xi)]
    q[:, 0] = 0.0
    o = vr.oracle_step(kind, q, v, a, xi)
    if lads:
        lq, lv, la, lx, sl = vr.concat_ladders(lads)
        lq = lq.copy(); lq[:, 0] = 0.0
        q = np.concatenate([lq, q]); v = np.concatenate([lv, v]); a = np.concatenate([la, a]); xi = np.concatenate([lx, xi])
        o = {k: np.concatenate([np.concatenate([l["oracle"][k] for l in lads]), o[k]]) for k in ("qpos", "qvel", "done")}
    else:
        sl = []
    return dict(q=q, v=v, a=a, xi=xi, oracle=o, slices=sl, ladders=lads)


_BATCHES = {}


def batch_of(kind):
    if kind not in _BATCHES:
        _BATCHES[kind] = _batch(kind)
    return _BATCHES[kind]


def _f32_steps(x, k):
    """x (float32, non-zero) moved by k fp32 values away from zero (k < 0: towards it)"""
    return (np.asarray(x, dtype=np.float32).view(np.int32) + np.asarray(k, dtype=np.int32)).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------- ladders on the device
@pytest.mark.parametrize("row_major", [False, True], ids=["soa", "rows"])
@pytest.mark.parametrize("kind,knobs", CONFIGS, ids=CONFIG_IDS)
def test_done_rule_on_the_ladders(torch, kind, knobs, row_major):
    """terminated / truncated against the restated rule on the kernel's own state, every lane; done against the oracle where the oracle is
    more than 2e-5 from every threshold; both outcomes on every ladder; the time limit, endless and time_limit=False on the same lanes"""
    b = batch_of(kind); n = len(b["q"]); o = b["oracle"]
    o_margin = np.abs(vr.clause_margins(kind, o["qpos"], o["qvel"])).min(1) if b["ladders"] else np.full(n, np.inf)
    base = None
    for rname, autoreset, extra, dr in _resets(kind, knobs):
        kn = dict(knobs, **extra)
        for mode, t, flags in (("plain", 0, {}), ("last step", LAST, {}), ("last step, endless", LAST, dict(endless=True)),
                               ("last step, no time limit", LAST, dict(time_limit=False))):
            tag = "%s %s %s reset=%s [%s]" % (kind, kn, "rows" if row_major else "soa", rname, mode)
            env = _make(kind, n, kn, row_major, autoreset, dr=dr, **flags)
            _load(env, torch, b["q"], b["v"], b["xi"], t)
            out = _step(env, torch, b["a"])
            c = env.counters(); env.close()
            q, v = _stored(kind, out, autoreset)
            assert np.isfinite(q).all() and np.isfinite(v).all() and c["nonfinite"] == 0, tag
            ref = _verdict(kind, q, v, b["a"], t, **flags)
            ties = _assert_verdict(tag, kind, out, ref, _ties(kind, q, v))
            term = out["done"] & ~out["truncated"]
            per = [(l["name"], int(term[s].sum()), int((~term[s]).sum())) for l, s in zip(b["ladders"], b["slices"])]
            print("%s: %d exempt tie lanes; terminated / not per ladder %s" % (tag, ties, per))
            if mode == "plain":
                far = o_margin > vr.EPS_DONE
                assert np.array_equal(out["done"][far], o["done"][far]), (tag, np.where(out["done"][far] != o["done"][far])[0][:10])
                assert not out["truncated"].any(), tag
                for name, yes, no in per:                                    # both outcomes on every ladder, in the kernel's own output
                    assert yes >= 1 and no >= 1, (tag, name, yes, no)
            elif mode == "last step":
                assert out["done"].all() and np.array_equal(out["truncated"], ~term), tag
                assert term.any() == bool(b["ladders"]) and out["truncated"].any(), tag       # both groups (the half-cheetah never terminates)
            elif mode == "last step, endless":
                assert not term.any() and out["truncated"].all(), tag
            else:
                assert not out["truncated"].any() and np.array_equal(out["done"], term), tag
            # one tail, whatever restarts the lane: reward, done and truncated bits do not depend on the auto-reset
            if rname == "off":
                base = dict(base or {}, **{mode: out})
            else:
                ref_out = base[mode]
                assert np.array_equal(out["done"], ref_out["done"]) and np.array_equal(out["truncated"], ref_out["truncated"]), tag
                assert np.array_equal(out["reward"].view(np.int32), ref_out["reward"].view(np.int32)), tag
                rows = out["done"]                                           # the terminal observation is the stepped one, bit for bit
                assert np.array_equal(out["term"][rows].view(np.int32), ref_out["obs"][rows].view(np.int32)), tag


@pytest.mark.parametrize("kind,knobs", [c for c in CONFIGS if c[0] != "halfcheetah"], ids=[i for i in CONFIG_IDS if "cheetah" not in i])
def test_the_flip_itself_on_consecutive_fp32_values(torch, kind, knobs):
    """Around the flip each coarse ladder showed: the bracket narrowed until 250 CONSECUTIVE fp32 values of the pre-step coordinate span it;
    on those the kernel shows both outcomes and every lane obeys the restated rule on its own stored state.  A flip that falls outside fails."""
    lads = vr.ladders(kind); nl = len(lads); N = vr.N_LADDER
    coords = [(0 if l["coord"][0] == "q" else 1, l["coord"][1]) for l in lads]

    def run(values):                                                         # values [nl][N] float32 of each ladder's coordinate
        q, v, a, xi, sl = vr.concat_ladders(lads)
        q = q.copy(); v = v.copy(); q[:, 0] = 0.0
        for k, (s, (w, idx)) in enumerate(zip(sl, coords)):
            (q, v)[w][s, idx] = values[k].astype(np.float64)
        env = _make(kind, len(q), knobs, False, False)
        _load(env, torch, q, v, xi, 0)
        out = _step(env, torch, a); env.close()
        qq, vv = _stored(kind, out, False)
        ref = _verdict(kind, qq, vv, a, 0)
        ties = _assert_verdict("%s %s fine" % (kind, knobs), kind, out, ref, _ties(kind, qq, vv))
        return [out["done"][s] for s in sl], ties

    vals = [(l["qpos"], l["qvel"])[w][:, idx].astype(np.float32) for l, (w, idx) in zip(lads, coords)]
    for rnd in range(6):
        done, ties = run(vals)
        consecutive = all(np.all(np.abs(np.diff(x.view(np.int32).astype(np.int64))) == 1) for x in vals)
        width = []
        for k in range(nl):
            flips = np.where(done[k][1:] != done[k][:-1])[0]
            assert flips.size, "%s %s %s: no flip on the ladder of round %d (%d of %d done)" % (kind, knobs, lads[k]["name"], rnd, done[k].sum(), N)
            lo, hi = vals[k][flips[0]], vals[k][flips[0] + 1]
            gap = abs(int(hi.view(np.int32)) - int(lo.view(np.int32)))
            width.append(gap)
            inner = lo if abs(lo) < abs(hi) else hi                        # the bracket's end nearer zero; steps count away from zero
            if gap <= N - 1:                                                 # consecutive values, the bracket in the middle
                steps = np.arange(N) - (N - 1 - gap) // 2
            else:
                steps = np.round(np.linspace(0, gap, N)).astype(np.int64)
            vals[k] = _f32_steps(np.full(N, inner, dtype=np.float32), steps)
        print("%s %s round %d: consecutive=%s, bracket widths in fp32 values %s, %d exempt tie lanes" % (kind, knobs, rnd, consecutive, width, ties))
        if consecutive:                                                      # (the flip asserted above was seen on 250 consecutive values)
            break
    else:
        raise AssertionError("%s %s: the brackets did not narrow to consecutive fp32 values: %s" % (kind, knobs, width))


# ---------------------------------------------------------------------------------------------------------------- reward
@pytest.mark.parametrize("row_major", [False, True], ids=["soa", "rows"])
@pytest.mark.parametrize("kind,knobs", [c for c in CONFIGS if c[0] != "humanoid"], ids=[i for i in CONFIG_IDS if "humanoid" not in i])
def test_planar_reward_is_the_restated_formula(torch, kind, knobs, row_major):
    """root x = 0 before the step: reward = q0_after / dt + alive - c sum(a^2) in fp64 from the stored fp32 q0_after and the fp32 RAW action,
    within (NU + 8) 2^-24 (|q0 / dt| + alive + c sum(a^2)) -- one rounding per fp32 operation of the tail (NU products, NU - 1 sums, the division,
    the product with c, two sums) plus the two rounded constants dt and c, and contraction to FMA only removes roundings.  The info rows
    within 4 ulp each."""
    b = batch_of(kind); n = len(b["q"]); nu = DIMS[kind]["nu"]
    env = _make(kind, n, knobs, row_major, False)
    _load(env, torch, b["q"], b["v"], b["xi"], 0)
    out = _step(env, torch, b["a"]); env.close()
    ref = vr.planar_verdict(kind, np.zeros(n), out["qpos"].astype(np.float64), out["qvel"].astype(np.float64), b["a"])
    scale = np.abs(ref["reward_run"]) + ALIVE[kind] + np.abs(ref["reward_ctrl"])
    err = np.abs(out["reward"].astype(np.float64) - ref["reward"])
    print("%s %s: max reward error %.2f of the bound, |a| max %.2f" % (kind, knobs, (err / ((nu + 8) * 2.0 ** -24 * scale)).max(), np.abs(b["a"]).max()))
    assert np.abs(b["a"]).max() > 1.1                                        # the raw action, beyond the control range
    assert (err <= (nu + 8) * 2.0 ** -24 * scale).all(), (kind, knobs, np.argmax(err / scale), (err / scale).max())
    for name in ("reward_run", "reward_ctrl"):
        e = np.abs(out[name].astype(np.float64) - ref[name]); ulp = np.spacing(np.abs(ref[name]).astype(np.float32)).astype(np.float64)
        assert (e <= 4 * ulp).all(), (kind, knobs, name, (e / ulp).max())


@pytest.mark.parametrize("row_major", [False, True], ids=["soa", "rows"])
@pytest.mark.parametrize("hum_pair", [1, 0])
def test_humanoid_reward_is_the_sum_of_its_info_rows(torch, hum_pair, row_major):
    b = batch_of("humanoid"); n = len(b["q"])
    env = _make("humanoid", n, dict(REX_HUM_PAIR=hum_pair), row_major, False)
    _load(env, torch, b["q"], b["v"], b["xi"], 0)
    out = _step(env, torch, b["a"]); env.close()
    rows = [out[k].astype(np.float64) for k in ("reward_linvel", "reward_quadctrl", "reward_alive", "reward_impact")]
    err = np.abs(out["reward"].astype(np.float64) - sum(rows))
    assert (err <= 8 * 2.0 ** -24 * sum(np.abs(r) for r in rows)).all(), err.max()
    assert (out["reward_alive"] == 5.0).all() and (out["reward_impact"] == 0.0).all()
    # the control cost is the RAW action's (random_humanoid.py:167: data.ctrl is not clamped), 4 ulp as for the planar rows
    quad = -0.1 * (b["a"] ** 2).sum(1)
    assert (np.abs(rows[1] - quad) <= 4 * np.spacing(np.abs(quad).astype(np.float32))).all() and np.abs(b["a"]).max() > 0.5


@pytest.mark.parametrize("kind,knobs", [c for c in CONFIGS if c[0] != "humanoid"], ids=[i for i in CONFIG_IDS if "humanoid" not in i])
def test_translation_of_the_root(torch, kind, knobs):
    """the step is integrated from x = 0: from x = 0 and from x = 1e4 the same reward and observation bits, and the stored q[0] is
    fl32(x_before + dx) with the dx of the run from 0"""
    b = batch_of(kind); n = len(b["q"]); outs = []
    for x0 in (0.0, 1e4):
        q = b["q"].copy(); q[:, 0] = x0
        env = _make(kind, n, knobs, False, False)
        _load(env, torch, q, b["v"], b["xi"], 0)
        outs.append(_step(env, torch, b["a"])); env.close()
    z, far = outs
    assert np.array_equal(z["reward"].view(np.int32), far["reward"].view(np.int32)) and np.array_equal(z["obs"].view(np.int32), far["obs"].view(np.int32))
    assert np.array_equal(z["done"], far["done"])
    assert np.array_equal(far["qpos"][:, 0], (np.float32(1e4) + z["qpos"][:, 0]).astype(np.float32))
    assert np.array_equal(far["qpos"][:, 1:], z["qpos"][:, 1:]) and np.array_equal(far["qvel"], z["qvel"])


# ---------------------------------------------------------------------------------------------------------------- replay, CartPole
@pytest.mark.parametrize("kind,knobs", CONFIGS, ids=CONFIG_IDS)
def test_replay_gives_the_same_terminated_and_touches_nothing(torch, kind, knobs):
    """rex_replay, the read-only path: the same terminated as a step of the same lanes, never truncated (the handle sits on its last step),
    all four counters as they were"""
    b = batch_of(kind); n = len(b["q"])
    env = _make(kind, n, knobs, False, False)
    _load(env, torch, b["q"], b["v"], b["xi"], LAST)
    before = env.counters(); st0 = env.get_full_state()
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32).T)).to(env.device)
    obs, r, d = env.replay_soa(dev(b["q"]), dev(b["v"]), dev(b["xi"]), dev(b["a"]))
    obs = obs.t().cpu().numpy().copy(); d = d.cpu().numpy().astype(bool).copy(); r = r.cpu().numpy().copy()
    assert env.counters() == before
    st1 = env.get_full_state()
    for k in ("qpos", "qvel", "t", "episode", "done"):
        assert torch.equal(st0[k], st1[k]), k
    out = _step(env, torch, b["a"]); env.close()
    term = out["done"] & ~out["truncated"]
    assert out["done"].all() and np.array_equal(d, term), (kind, knobs, np.where(d != term)[0][:10])
    assert np.array_equal(r.view(np.int32), out["reward"].view(np.int32)) and np.array_equal(obs.view(np.int32), out["obs"].view(np.int32))
    print("%s %s: replay terminated %d of %d, step truncated %d" % (kind, knobs, d.sum(), n, out["truncated"].sum()))


@pytest.mark.parametrize("autoreset", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("row_major", [False, True], ids=["soa", "rows"])
def test_cartpole_at_every_fp32_value_around_its_thresholds(torch, row_major, autoreset):
    state, action, xi, names = vr.cartpole_ladder(); n = len(state)
    nxt, r_o, d_o = oracle_cartpole_step(state, action, xi)
    for mode, t, tl in (("plain", 0, True), ("last step", LAST, True), ("last step, no time limit", LAST, False)):
        env = _make("cartpole", n, {}, row_major, autoreset, time_limit=tl)
        _load(env, torch, state[:, [0, 2]], state[:, [1, 3]], xi, t)
        out = _step(env, torch, action)
        q, v = _stored("cartpole", out, autoreset)
        assert np.array_equal(q, state[:, [0, 2]])                           # x_dot = theta_dot = 0: exact
        ref = _verdict("cartpole", q, v, None, t, time_limit=tl)
        tie = _ties("cartpole", q, v)
        ties = _assert_verdict("cartpole %s" % mode, "cartpole", out, ref, tie)
        term = out["done"] & ~out["truncated"]
        print("cartpole rows=%s reset=%s [%s]: %d exempt tie lanes, terminated per threshold %s" % (row_major, autoreset, mode, ties, term.reshape(4, 9).sum(1).tolist()))
        assert 4 <= ties <= 8 and (term.reshape(4, 9).sum(1) >= 4).all() and ((~term).reshape(4, 9).sum(1) >= 4).all()
        assert np.array_equal(term[~tie], d_o[~tie])                         # (the oracle's margin on the other lanes is >= 1 ulp > 0: no eps needed)
        assert (out["reward"] == 1.0).all() and env.counters()["nonfinite"] == 0
        if mode == "last step":
            assert out["done"].all() and out["truncated"][~term].all()
        if not autoreset and mode == "plain":                                # two consecutive steps from a state past the threshold: 1 then 0
            out2 = _step(env, torch, action)                                 # (the first step's push moves the cart: some lanes come back inside)
            q2, v2 = _stored("cartpole", out2, False)
            ref2 = _verdict("cartpole", q2, v2, None, t + 1, was_done=term, time_limit=tl)
            ok2 = ~_ties("cartpole", q2, v2)
            assert np.array_equal(out2["reward"][ok2], ref2["reward"][ok2].astype(np.float32))
            again = term & ref2["terminated"] & ok2
            assert again.sum() >= 8 and (out2["reward"][again] == 0.0).all() and (out2["reward"][~term & ok2] == 1.0).all()
        env.close()


# ---------------------------------------------------------------------------------------------------------------- the non-finite contract
NF_B = 130                                                                   # two 64-lane blocks and a ragged tail
NF_LANES = np.array([0, 40, 129] + list(range(64, 128)))                     # lane 0 of a block, mid-wave, the last env, one whole wave (two of 32 envs)


def _nf_inputs(kind):
    rng = np.random.RandomState(9); d = DIMS[kind] if kind != "cartpole" else dict(nq=2, nv=2, nu=1)
    if kind == "cartpole":
        q = rng.uniform(-0.05, 0.05, (NF_B, 2)); v = rng.uniform(-0.05, 0.05, (NF_B, 2)); a = rng.randint(0, 2, NF_B)
        xi = np.tile(np.array([9.8, 1.0, 0.1, 0.5]), (NF_B, 1))
    elif kind == "humanoid":
        q, v = vr._reset_state(kind, rng, NF_B); q[:, 2] -= rng.uniform(0, 0.3, NF_B)
        a = rng.uniform(-0.4, 0.4, (NF_B, 17)); xi = np.tile(vr._nominal(kind), (NF_B, 1))
    else:
        q, v, xi = rollout_states(kind, NF_B, steps_max=30, seed=12)
        keep = ~vr.oracle_step(kind, vr._r32(q), vr._r32(v), np.zeros((NF_B, d["nu"])), vr._r32(xi))["done"]
        q[~keep], v[~keep] = q[keep][0], v[keep][0]                          # (healthy lanes that do not end on their own)
        a = rng.uniform(-0.3, 0.3, (NF_B, d["nu"]))
    q, v, xi = [vr._r32(x) for x in (q, v, xi)]
    if kind != "cartpole":
        a = vr._r32(a); q[:, 0] = 0.0
    cases = {}
    for what in ("nan_qvel", "inf_qpos", "nan_action", "inf_action"):
        if kind == "cartpole":
            if what.endswith("action"):
                continue                                                     # (an int32 action holds neither)
            qq, vv = q.copy(), v.copy()
            if what == "nan_qvel":
                vv[NF_LANES, 1] = np.nan
            else:
                qq[NF_LANES, 0] = np.inf
            cases[what] = (qq, vv, a)
        else:
            cases[what] = vr.poison(kind, q, v, a, what, NF_LANES)
    return q, v, a, xi, cases


NF_CONFIGS = CONFIGS + [("cartpole", {})]
NF_IDS = CONFIG_IDS + ["cartpole-default"]


@pytest.mark.parametrize("row_major", [False, True], ids=["soa", "rows"])
@pytest.mark.parametrize("kind,knobs", NF_CONFIGS, ids=NF_IDS)
def test_nonfinite_lane_ends_is_counted_and_restarts(torch, kind, knobs, row_major):
    """Whenever the stored post-step state holds a non-finite element: terminated = 1 and truncated = 0 (also under endless, also on the last
    step of the time limit); counters()["nonfinite"] grows by exactly the number of such lanes in that step; with the auto-reset on the lane's
    next observation is finite and bit-equal to a masked reset of the same lane and episode on a twin env; without it the lane stays done and is
    counted once per step.  A non-finite action that leaves the state finite is not counted and does not end the lane, and the reward follows
    the restated formula (the sum of squares of a NaN is NaN in the reference too)."""
    q0, v0, a0, xi, cases = _nf_inputs(kind)
    for what, (q, v, a) in cases.items():
        for endless in ((False, True) if kind != "cartpole" else (False,)):
            flags = dict(endless=True) if endless else {}
            for rname, autoreset, extra, dr in _resets(kind, knobs):
                kn = dict(knobs, **extra)
                tag = "%s %s %s reset=%s %s endless=%s" % (kind, kn, "rows" if row_major else "soa", rname, what, endless)
                env = _make(kind, NF_B, kn, row_major, autoreset, dr=dr, **flags)
                _load(env, torch, q, v, xi, LAST)
                c0 = env.counters()
                out = _step(env, torch, a)
                c1 = env.counters()
                if not autoreset:
                    sq, sv = out["qpos"].astype(np.float64), out["qvel"].astype(np.float64)
                    bad = ~(np.isfinite(sq).all(1) & np.isfinite(sv).all(1))
                    off = dict(out=out, bad=bad)
                else:
                    bad = off["bad"]                                         # (the same kernel on the same inputs: the `off` run's lanes)
                    sq, sv = _stored(kind, out, True)
                term = out["done"] & ~out["truncated"]
                delta = c1["nonfinite"] - c0["nonfinite"]
                print("%s: %d lanes with a non-finite stored state, nonfinite counter +%d, terminated %d, truncated %d, solver_capped %d"
                      % (tag, bad.sum(), delta, term.sum(), out["truncated"].sum(), c1["solver_capped"]))
                if what in ("nan_qvel", "inf_qpos"):
                    assert np.array_equal(np.where(bad)[0], np.sort(NF_LANES)), (tag, np.where(bad)[0])
                assert term[bad].all() and not out["truncated"][bad].any(), (tag, np.where(bad & ~term)[0][:10])
                assert delta == bad.sum(), (tag, delta, int(bad.sum()))
                # the finite lanes: the restated rule on their own state (they sit on the last step: truncated unless terminated)
                ref = _verdict(kind, np.where(bad[:, None], np.nan, sq), sv, a if kind != "cartpole" else None, LAST, **flags)
                _assert_verdict(tag, kind, out, ref, _ties(kind, np.nan_to_num(sq), np.nan_to_num(sv)))
                if kind in ALIVE and not autoreset:                          # reward of the finite lanes: the restated formula, NaN where it is NaN
                    rr = vr.planar_verdict(kind, np.zeros(NF_B), sq, sv, a)["reward"]; ok = ~bad
                    scale = np.abs(sq[:, 0] / vr.DT[kind]) + ALIVE[kind] + CTRL_COST[kind] * (np.asarray(a, dtype=np.float64) ** 2).sum(1)
                    got = out["reward"].astype(np.float64)
                    assert np.array_equal(np.isnan(got[ok]), np.isnan(rr[ok])), tag
                    fin = ok & np.isfinite(rr)
                    assert (np.abs(got[fin] - rr[fin]) <= (DIMS[kind]["nu"] + 8) * 2.0 ** -24 * scale[fin]).all(), tag
                    assert np.array_equal(got[ok & ~fin], rr[ok & ~fin], equal_nan=True), tag
                if autoreset:
                    assert np.array_equal(out["done"], off["out"]["done"]) and np.array_equal(out["truncated"], off["out"]["truncated"]), tag
                    assert np.isfinite(out["obs"]).all(), tag
                    twin = _make(kind, NF_B, kn, row_major, False, dr=dr, **flags)
                    _load(twin, torch, q, v, xi, LAST)
                    _step(twin, torch, a)
                    robs = twin.reset(mask=torch.as_tensor(out["done"].astype(np.uint8))).cpu().numpy().copy()
                    rows = out["done"]
                    if kind == "humanoid" and rname == "on" and kn.get("REX_HUM_PAIR") == 1:
                        # the fused restart runs the pair engine, the masked reset the one-lane engine: same draws, same state bits (below), the
                        # qpos / qvel slice of the observation bit-equal, the derived blocks to the 2e-5 tests/test_gpu_humanoid.py holds them to
                        assert np.array_equal(out["obs"][rows][:, :45].view(np.int32), robs[rows][:, :45].view(np.int32)), tag
                        e = np.abs(out["obs"][rows].astype(np.float64) - robs[rows]).max(1) / (1 + np.abs(robs[rows]).max(1))
                        assert e.max() < 2e-5, (tag, e.max())
                    else:
                        assert np.array_equal(out["obs"][rows].view(np.int32), robs[rows].view(np.int32)), tag
                    tq, tv = twin.get_state(); twin.close()
                    assert np.array_equal(out["qpos"].view(np.int32), tq.cpu().numpy().view(np.int32)), tag
                    assert np.array_equal(out["qvel"].view(np.int32), tv.cpu().numpy().view(np.int32)), tag
                # two further steps with healthy actions: restarted lanes are healthy; without the auto-reset a bad lane stays bad, stays done
                # and is counted once per step
                for k in range(2):
                    c_before = env.counters()["nonfinite"]
                    nxt = _step(env, torch, a0)
                    still = ~(np.isfinite(nxt["qpos"]).all(1) & np.isfinite(nxt["qvel"]).all(1))
                    assert env.counters()["nonfinite"] - c_before == still.sum(), (tag, k)
                    if autoreset:
                        assert not still.any() and np.isfinite(nxt["obs"]).all() and np.isfinite(nxt["reward"]).all(), (tag, k)
                    else:
                        assert np.array_equal(still, bad) and nxt["done"][bad].all() and not nxt["truncated"][bad].any(), (tag, k)
                env.close()


@pytest.mark.parametrize("kind", ["hopper", "walker2d", "halfcheetah"])
def test_nonfinite_lanes_do_not_reach_their_neighbours(torch, kind):
    """REX_FAST=0 with one lane per env is lane-independent (tests/test_gpu_launch_shapes.py): every healthy lane bit-equal to the same batch with
    the poisoned lanes replaced by a healthy state.  In the default configuration the healthy lanes stay within the fp32 tolerances of that
    run and their done obeys the restated rule."""
    q0, v0, a0, xi, cases = _nf_inputs(kind)
    healthy = np.setdiff1d(np.arange(NF_B), NF_LANES)

    def run(knobs, q, v, a):
        env = _make(kind, NF_B, knobs, False, False)
        _load(env, torch, q, v, xi, 0)
        out = _step(env, torch, a); c = env.counters(); env.close()
        return out, c

    clean, _ = run(dict(REX_FAST=0, REX_PAIR=0), q0, v0, a0)
    for what, (q, v, a) in cases.items():
        slow, c_slow = run(dict(REX_FAST=0, REX_PAIR=0), q, v, a)
        for k in ("qpos", "qvel", "obs", "reward"):
            assert np.array_equal(slow[k][healthy].view(np.int32), clean[k][healthy].view(np.int32)), (kind, what, k)
        assert np.array_equal(slow["done"][healthy], clean["done"][healthy])
        dflt, c_dflt = run({}, q, v, a)
        eq = np.abs(dflt["qpos"][healthy].astype(np.float64) - clean["qpos"][healthy]).max(1)
        vs = 1 + np.abs(clean["qvel"][healthy]).max(1)
        ev = np.abs(dflt["qvel"][healthy].astype(np.float64) - clean["qvel"][healthy]).max(1) / vs
        print("%s %s: healthy lanes max |dqpos| %.2e |dqvel|rel %.2e; solver_capped REX_FAST=0 %d, default %d"
              % (kind, what, eq.max(), ev.max(), c_slow["solver_capped"], c_dflt["solver_capped"]))
        assert eq.max() <= TOL_QPOS and ev.max() <= TOL_QVEL_REL, (kind, what, eq.max(), ev.max())
        sq, sv = dflt["qpos"].astype(np.float64)[healthy], dflt["qvel"].astype(np.float64)[healthy]
        ref = vr.planar_verdict(kind, np.zeros(len(healthy)), sq, sv, np.asarray(a)[healthy])
        sub = {k: dflt[k][healthy] for k in ("done", "truncated")}
        _assert_verdict("%s %s healthy" % (kind, what), kind, sub, ref, _ties(kind, sq, sv))
