"""Automatic domain randomisation, CPU half: the kernels' own arithmetic, its order, the addressing and the draws (the __host__ __device__
functions of csrc/adr.hpp, driven block by block in grid order by tests/host_harness/adr_host.cpp) against the numpy / Python-int
restatement of the contract in tests/adr_oracle.py.  Every state word, every lane word and every xi row is held to IDENTICAL BITS behind
every call of the scenario."""
import os
import subprocess

import numpy as np
import pytest

import adr_oracle as oracle
from adr_oracle import assert_same_bits, assert_snapshots_equal
from host_harness import adr as host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "host_harness")
SIZES = [1, 63, 64, 257, 4097]
FROZEN = np.float32(7.5)           # what the rows outside the task hold: no assignment may touch them

pytestmark = pytest.mark.skipif(host.rocm_include() is None, reason="rocRAND headers (rocrand/rocrand_kernel.h) not found under ROCM_PATH or /opt/rocm")

# kind: (task rows d, active task indices, task row -> row of the full xi block, rows of the full block)
KINDS = {
    "hopper": (4, list(range(4)), list(range(4)), 4),
    "hopper_unmodeled": (3, list(range(3)), [1, 2, 3], 4),                       # the torso mass is frozen
    "walker2d_masses": (13, list(range(7)), list(range(13)), 13),                # masses only: lengths and friction stay at the centre
    "humanoid": (30, list(range(30)), list(range(30)), 30),                      # J = 60
}


def _settings(kind, p_b=0.5):
    d, act, row_map, full = KINDS[kind]
    rng = np.random.default_rng(d)
    centre = rng.uniform(1.0, 5.0, size=d).astype(np.float32)
    cfg = oracle.settings(centre, (centre * np.float32(0.5)).astype(np.float32), (centre * np.float32(2.0)).astype(np.float32), act, p_b)
    return cfg, row_map, full


def run_both(kind, B, p_b=0.5, env_offset=0, seed=None):
    cfg, row_map, full = _settings(kind, p_b)
    d = cfg["d"]
    task0 = np.tile(cfg["centre"][:, None], (1, B)).astype(np.float32)
    xi = np.full((full, B), FROZEN, np.float32)
    xi[np.asarray(row_map)] = task0
    ref = oracle.Box(B, task=task0, env_offset=env_offset, **cfg)
    ops, snaps = oracle.scenario(ref, B, B if seed is None else seed)
    impl = host.HostBox(B, xi_full=xi, row_map=row_map, env_offset=env_offset, **cfg)

    def after(j, op):
        assert_snapshots_equal(oracle.snapshot(impl), snaps[j], "%s B=%d behind operation %d (%s)" % (kind, B, j, op[0]))
        assert_same_bits(impl.mask, _mask_of(op, B), "mask behind operation %d" % j) if op[0] != "update" else None
    oracle.replay(impl, ops, after)
    frozen = [r for r in range(full) if r not in row_map]
    assert (impl.xi[frozen] == FROZEN).all()
    return impl, ref, ops


def _mask_of(op, B):
    flags = op[2] if op[0] == "record" else op[1]
    return np.ones(B, np.uint8) if flags is None else (np.asarray(flags) != 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------- the contract, every size
@pytest.mark.parametrize("B", SIZES)
def test_hopper_equals_the_oracle_bit_for_bit(B):
    impl, ref, ops = run_both("hopper", B, env_offset=(1 << 33) if B == 63 else 0)     # a global index past 2^32 reaches the subsequence's high word
    ev = ref.events
    print("B=%d events: %s" % (B, ev))
    assert ev["calls_without_done"] >= 1 and any(op[0] == "record" and np.asarray(op[2]).all() for op in ops)
    assert any(op[0] == "update" for op in ops) and sum(op[0] == "assign" for op in ops) == 2
    if B >= 257:       # conditions on the oracle's own run, not measurements: the scenario contains what it is meant to exercise
        assert ev["expand"] >= 1 and ev["shrink"] >= 1 and ev["hold"] >= 1, ev
        assert ev["limit_clamp"] >= 1 and ev["centre_clamp"] >= 1, ev
        assert ev["max_arrival"] > oracle.M_SCENARIO, ev
        assert ev["nan_means"] >= 1 and ev["dropped_boundary_episodes"] >= 1, ev      # the NaN reward reached a mean; the masked assign dropped pinned episodes
        assert np.isnan(np.array([r for _, _, _, r in ref.tallied])).sum() == 1
        assert (ref.lo < ref.centre).any() or (ref.hi > ref.centre).any() or ev["shrink"] >= 1


@pytest.mark.parametrize("kind,B", [("hopper_unmodeled", 63), ("hopper_unmodeled", 257), ("walker2d_masses", 257), ("humanoid", 257), ("humanoid", 65)])
def test_other_tasks_equal_the_oracle_bit_for_bit(kind, B):
    impl, ref, _ = run_both(kind, B)
    d, act, _, _ = KINDS[kind]
    ev = ref.events
    print("%s B=%d events: %s" % (kind, B, ev))
    assert ev["boundary_episodes"] >= 1 and ev["expand"] + ev["shrink"] + ev["hold"] >= 1
    inactive = [k for k in range(d) if k not in act]
    assert_same_bits(impl.lo[inactive], ref.centre[inactive], "inactive lower bounds"); assert_same_bits(impl.hi[inactive], ref.centre[inactive], "inactive upper bounds")
    if inactive:
        assert (impl.task[inactive] == ref.centre[inactive][:, None]).all()          # the rows outside `act` stay at the centre of a zero-width start


@pytest.mark.parametrize("p_b", [0.0, 1.0])
def test_never_and_always_a_boundary_episode(p_b):
    impl, ref, _ = run_both("hopper", 257, p_b=p_b)
    if p_b == 0.0:
        assert (impl.bnd == -1).all() and not impl.n.any() and not impl.counters.any() and ref.events["boundary_episodes"] == 0
        assert_same_bits(impl.lo, ref.centre, "an untouched box"); assert_same_bits(impl.hi, ref.centre, "an untouched box")
    else:
        assert (impl.bnd >= 0).all() and (impl.bnd < 8).all() and ref.events["boundary_episodes"] == len(ref.assigned)
        assert len(np.unique(impl.bnd)) == 8                                          # every boundary is drawn


def test_argument_check():
    cfg, _, _ = _settings("hopper")
    base = {k: cfg[k] for k in ("d", "act", "p_b", "m", "t_lo", "t_hi", "delta", "lim_lo", "lim_hi", "centre", "init_lo", "init_hi")}
    assert host.check(**base) is None
    bad = lambda **kw: host.check(**dict(base, **kw))
    assert "n_act" in bad(act=[]) and "n_act" in bad(act=[0, 1, 2, 3, 3])
    assert "act" in bad(act=[1, 0]) and "act" in bad(act=[0, 0]) and "act" in bad(act=[0, 4]) and "act" in bad(act=[-1, 2])
    assert "m must" in bad(m=0)
    for p in (-0.1, 1.5, float("nan")):
        assert "p_b" in bad(p_b=p)
    assert "t_lo" in bad(t_lo=2.0, t_hi=1.0) and "t_lo" in bad(t_lo=float("nan"))
    z = base["delta"].copy(); z[2] = 0
    assert "delta" in bad(delta=z) and bad(delta=z, act=[0, 1, 3]) is None            # an inactive dimension's delta is not read
    for name, scale in (("lim_lo", 1.5), ("lim_hi", 0.9), ("init_lo", 1.1), ("init_hi", 0.9), ("init_hi", 2.5), ("init_lo", 0.4)):
        v = base[name].copy(); v[1] = np.float32(base["centre"][1] * scale)
        assert "lim_lo <= lo" in bad(**{name: v}), name
    assert bad(t_lo=1.0, t_hi=1.0) is None and bad(p_b=0.0) is None and bad(p_b=1.0) is None


# ------------------------------------------------------------------------------------------------- sharded runs
@pytest.mark.parametrize("split", [(64, 64), (1, 127)])
def test_merged_shard_tallies_then_update_give_the_unsharded_box(split):
    """Index-sharded ranks record with apply=False, merge their tallies in rank order (merge_tallies) and update: every rank then holds the
    box one handle over the global batch would hold; every rank but the first then clears its tallies, as AutoDR.update does behind a sync.  Returns here are small integers, so the fp64 sums do not depend on how the lanes
    are grouped (the contract fixes the order WITHIN a handle; across ranks the sum is in rank order)."""
    from random_envs_amd import merge_tallies
    B = 128
    cfg, row_map, full = _settings("hopper")
    task0 = np.tile(cfg["centre"][:, None], (1, B)).astype(np.float32)
    whole = oracle.Box(B, task=task0, **cfg)
    shards, lo = [], 0
    for n in split:
        shards.append((lo, lo + n, host.HostBox(n, xi_full=task0[:, lo:lo + n].copy(), env_offset=lo, **cfg))); lo += n
    whole.assign(None)
    for a, b, sh in shards:
        sh.assign(None)
    rng = np.random.default_rng(17)
    for c in range(10):
        reward = rng.integers(-4, 12, size=B).astype(np.float32)
        done = (rng.random(B) < 0.4).astype(np.uint8)
        whole.record(reward, done, apply=False); whole.update()
        for a, b, sh in shards:
            sh.record(reward[a:b], done[a:b], apply=False)
        n, s = merge_tallies([(sh.n, sh.s) for _, _, sh in shards])
        assert_same_bits(n, oracle.merge_tallies_reference([(sh.n, sh.s) for _, _, sh in shards])[0], "merged counts")
        assert_same_bits(s, oracle.merge_tallies_reference([(sh.n, sh.s) for _, _, sh in shards])[1], "merged sums")
        for a, b, sh in shards:
            sh.n[:], sh.s[:] = n, s
            sh.update()
            assert_same_bits(sh.lo, whole.lo, "call %d lower bounds" % c); assert_same_bits(sh.hi, whole.hi, "call %d upper bounds" % c)
            assert_same_bits(sh.counters, whole.state()["counters"], "call %d counters" % c)
            assert not sh.n[n >= cfg["m"]].any()
            assert_same_bits(sh.task, whole.task[:, a:b], "call %d tasks" % c)          # the global env index keys the draws
            if a > 0:
                sh.n[:], sh.s[:] = 0, 0.0                                              # what the update left is the group's: the first rank carries it (AutoDR.update)
    assert whole.events["expand"] >= 1 and whole.events["shrink"] + whole.events["hold"] >= 1
    with pytest.raises(ValueError):
        merge_tallies([])


# ------------------------------------------------------------------------------------------------- sanitizers
def test_host_functions_stay_inside_exactly_sized_buffers_under_sanitizers(tmp_path):
    """tests/host_harness/adr_sanitize_main.cpp: a program of its own (the sanitizer runtimes are linked into it; nothing is preloaded)"""
    exe = str(tmp_path / "adr_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
                          + host.build_flags() + ["-o", exe, os.path.join(HARNESS, "adr_sanitize_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "B=4097 d=30 J=60" in run.stdout and "B=4097 d=3 J=6" in run.stdout
