"""The on-device actor's arithmetic without a GPU: the host twin (csrc/actor.hpp under g++ -ffp-contract=off, tests/host_harness/actor_host.cpp)
against the fp64 oracle's running bound on the cases the device is held on, tanh32 against fp64 tanh, the argument check, and the twin under
sanitizers.  tests/test_gpu_actor.py then holds the kernel to the twin bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import actor_oracle as oracle
from host_harness import actor as host

HARNESS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_harness")


def _within(got, ref, what):
    val, bound = ref
    err = np.abs(np.asarray(got, np.float64) - val)
    worst = float((err / bound).max())
    print("%s: worst error %.3e, %.3f of its bound" % (what, float(err.max()), worst))
    assert np.isfinite(err).all() and (err <= bound).all(), what


@pytest.mark.parametrize("rows", [True, False])
@pytest.mark.parametrize("name", sorted(oracle.CASES))
def test_twin_stays_within_the_oracles_bound(name, rows):
    c = oracle.make_case(name)
    obs = c["obs"] if rows else np.ascontiguousarray(c["obs"].T)
    z = oracle.eps(oracle.SEED, 5, c["B"], c["act_dim"], 3).astype(np.float32)
    ref = oracle.act(c, eps_in=z)
    det = host.act(c["pi"], c["vf"], c["log_std"], obs, c["act_dim"], c["activation"], rows)
    sto = host.act(c["pi"], c["vf"], c["log_std"], obs, c["act_dim"], c["activation"], rows, eps=z)
    lay = (lambda a: a) if rows else (lambda a: a.T)
    _within(det["mean"], ref["mean"], "mean"); _within(det["value"], ref["value"], "value")
    assert np.array_equal(lay(det["action"]).view(np.uint32), det["mean"].view(np.uint32))       # deterministic: action = mean
    c_norm = ref["logp"][0] + 0.5 * (z.astype(np.float64) ** 2).sum(1)
    _within(det["logp"], (c_norm, ref["logp"][1]), "deterministic logp")
    _within(lay(sto["action"]), ref["action"], "action"); _within(sto["logp"], ref["logp"], "logp")
    assert np.array_equal(sto["mean"].view(np.uint32), det["mean"].view(np.uint32)) and np.array_equal(sto["value"].view(np.uint32), det["value"].view(np.uint32))


def test_twin_bits_do_not_depend_on_the_layout_or_the_absent_tower():
    c = oracle.make_case("hopper_64_17_64_tanh")
    a = host.act(c["pi"], c["vf"], c["log_std"], c["obs"], 3)
    b = host.act(c["pi"], c["vf"], c["log_std"], np.ascontiguousarray(c["obs"].T), 3, rows=False)
    assert np.array_equal(a["mean"].view(np.uint32), b["mean"].view(np.uint32)) and np.array_equal(a["value"].view(np.uint32), b["value"].view(np.uint32))
    only_pi, only_vf = host.act(c["pi"], None, c["log_std"], c["obs"], 3), host.act(None, c["vf"], None, c["obs"], 3)
    assert only_pi["value"] is None and only_vf["mean"] is None
    assert np.array_equal(only_pi["mean"].view(np.uint32), a["mean"].view(np.uint32)) and np.array_equal(only_vf["value"].view(np.uint32), a["value"].view(np.uint32))


@pytest.mark.parametrize("rows", [True, False])
def test_a_nan_input_under_each_activation(rows):
    """The contract's two clauses meet here (include/rex.h): a layer is a chain of fmaf, relu is fmaxf(x, 0).  Under tanh a NaN input makes
    the lane's mean and value NaN; under relu every first-layer unit it reaches becomes fmaxf(NaN, 0) = 0, so the lane comes out FINITE and
    equal to what all-zero first-layer activations give.  logp depends on the noise and log_std alone.  No other lane changes either way."""
    for name in ("hopper_64x64_tanh", "hopper_33_relu"):
        c = oracle.make_case(name)
        obs = c["obs"].copy()
        obs[70, 4] = np.nan
        lay = (lambda a: a) if rows else (lambda a: np.ascontiguousarray(a.T))
        z = oracle.eps(oracle.SEED, 0, c["B"], 3, 1).astype(np.float32)
        clean = host.act(c["pi"], c["vf"], c["log_std"], lay(c["obs"]), 3, c["activation"], rows, eps=z)
        bad = host.act(c["pi"], c["vf"], c["log_std"], lay(obs), 3, c["activation"], rows, eps=z)
        keep = np.arange(c["B"]) != 70
        for k in ("mean", "value", "logp"):
            assert np.array_equal(bad[k][keep].view(np.uint32), clean[k][keep].view(np.uint32)), (name, k)
        assert np.array_equal(bad["logp"].view(np.uint32), clean["logp"].view(np.uint32))
        if c["activation"] == "tanh":
            assert np.isnan(bad["mean"][70]).all() and np.isnan(bad["value"][70])
        else:
            zero = [(np.zeros_like(c["pi"][0][0]), np.zeros_like(c["pi"][0][1]))]
            dead = host.act(zero + c["pi"][1:], [(np.zeros_like(c["vf"][0][0]), np.zeros_like(c["vf"][0][1]))] + c["vf"][1:], c["log_std"], lay(c["obs"]), 3, "relu", rows)
            assert np.isfinite(bad["mean"][70]).all() and np.isfinite(bad["value"][70])
            assert np.array_equal(bad["mean"][70].view(np.uint32), dead["mean"][70].view(np.uint32)) and bad["value"][70] == dead["value"][70]


# ------------------------------------------------------------------------------------------------- tanh32
BP = np.float32(0.625)


def _ulps(x):
    x = np.asarray(x, np.float32)
    ref = np.tanh(x.astype(np.float64))
    return np.abs(host.tanh(x).astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def test_tanh32_stays_within_the_recorded_bound_on_the_subsample():
    """every 4 099th fp32 in [-10, 10], both neighbours of each breakpoint and the breakpoints, 0, +-denormal"""
    assert oracle.T_ULP <= 4.0                                   # the cap: a wrong coefficient misses by hundreds of ulp
    top = int(np.float32(10.0).view(np.uint32))
    pos = np.arange(0, top + 1, 4099, dtype=np.uint32).view(np.float32)
    edges = []
    for e in (BP, np.float32(10.0)):
        edges += [np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(20))]
    x = np.concatenate([pos, -pos, np.array(edges, np.float32), -np.array(edges, np.float32),
                        np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39], np.float32)])
    err = _ulps(x)
    k = int(np.argmax(err))
    print("tanh32: %d values, worst %.4f ulp at x = %r (T = %.2f)" % (len(x), err[k], float(x[k]), oracle.T_ULP))
    assert err.max() <= oracle.T_ULP
    assert len(pos) > 260000


def test_tanh32_special_values_symmetry_and_saturation():
    y = host.tanh(np.array([np.inf, -np.inf, 20.0, -20.0, 1e30, 0.0, -0.0, np.nan], np.float32))
    assert list(y[:5]) == [1.0, -1.0, 1.0, -1.0, 1.0] and np.isnan(y[7])
    assert y[5:7].view(np.uint32).tolist() == [0, 0x80000000]                        # +-0 keep their sign
    x = np.random.default_rng(3).uniform(0, 12, 100000).astype(np.float32)
    assert np.array_equal(host.tanh(-x).view(np.uint32), (-host.tanh(x)).view(np.uint32))      # exactly odd
    assert (np.abs(host.tanh(x)) <= 1.0).all()
    d = np.array([1e-45, 1e-40, 1.1754942e-38], np.float32)
    assert np.array_equal(host.tanh(d).view(np.uint32), d.view(np.uint32))           # denormals come back as they are


def test_exhaustive_sweep_of_a_slice_agrees_with_the_recorded_bound():
    """The recorded T comes from the sweep of ALL 1 092 616 193 fp32 in [0, 10] (profiles/actor_tanh_sweep.py: 1.371 ulp at x = 0.63022083);
    this runs the same function over the 2^20 values around that worst case."""
    worst_x = np.float32(0.6302208304405212)
    b = int(worst_x.view(np.uint32))
    lo, hi = (np.uint32(b - (1 << 19)).view(np.float32), np.uint32(b + (1 << 19)).view(np.float32))
    worst, where = host.tanh_sweep(lo, hi)
    print("sweep [%r, %r]: %.6f ulp at %r" % (float(lo), float(hi), worst, where))
    assert 1.3 < worst <= oracle.T_ULP


# ------------------------------------------------------------------------------------------------- the argument check
def test_argument_check_rules_and_their_order():
    assert host.check() is None
    assert host.check(pi=None, has_log_std=False, has_std=False, has_action=False) is None        # vf alone
    assert host.check(vf=None, has_value=False) is None                                          # pi alone
    assert host.check(pi=(1, 1, 0, 0, -1), vf=(3, 64, 17, 64, -1), in_dim=1024, activation=1) is None
    assert "null net" in host.check(null_net=True, pi=None, vf=None)
    assert "both towers" in host.check(pi=None, vf=None, in_dim=0)
    for d in (0, -3, 1025):
        assert "in_dim" in host.check(in_dim=d, activation=7)
    assert "activation" in host.check(activation=2, pi=(0, 64, 64, 0, -1))
    for t in ((0, 64, 64, 0, -1), (4, 64, 64, 64, -1)):
        assert "pi: n_hidden" in host.check(pi=t, vf=t) and "vf: n_hidden" in host.check(vf=t, has_log_std=False)
    for t in ((2, 64, 0, 0, -1), (2, 65, 64, 0, -1), (3, 64, 64, -1, -1)):
        assert "pi: a width" in host.check(pi=t) and "vf: a width" in host.check(vf=t)
    assert host.check(pi=(1, 64, 999, -5, -1)) is None                                           # widths past n_hidden are not read
    for l in (0, 1, 2, 8, 9, 10):
        assert "pi: null W or b" in host.check(pi=(2, 64, 64, 0, l), has_std=False) and "vf: null W or b" in host.check(vf=(2, 64, 64, 0, l))
    assert host.check(pi=(2, 64, 64, 0, 3)) is None                                              # a layer past the head is not read
    for kw in (dict(has_log_std=False), dict(has_std=False), dict(has_action=False)):
        assert "pi needs" in host.check(has_value=False, **kw)
        assert host.check(pi=None, **kw) is None
    assert "vf needs" in host.check(has_value=False, draw=-1)
    assert "negative draw" in host.check(draw=-1, has_in=False)
    assert "null input" in host.check(has_in=False)
    assert host.check(draw=(1 << 62)) is None


# ------------------------------------------------------------------------------------------------- sanitizers
def test_host_functions_stay_inside_exactly_sized_buffers_under_sanitizers(tmp_path):
    """tests/host_harness/actor_sanitize_main.cpp: a program of its own (the sanitizer runtimes are linked into it; nothing is preloaded)"""
    exe = str(tmp_path / "actor_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
                          + host.build_flags() + ["-o", exe, os.path.join(HARNESS, "actor_sanitize_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "in=376 act=17 widths=64,17,64 rows=0" in run.stdout and "in=1 act=1 widths=1 rows=1" in run.stdout


# ------------------------------------------------------------------------------------------------- the code object
def test_the_kernel_compiles_without_scratch_or_spilled_vector_registers(tmp_path):
    """The kernel leans on the compiler keeping 64 accumulators and 64 prefetched inputs in registers and the weights in scalar registers
    (csrc/actor.hpp says which barriers hold that in place): csrc/actor.hpp alone, compiled for gfx950 with build()'s flags, read with
    profiles/kmeta.py.  No GPU needed."""
    import sys
    import __graft_entry__ as g
    root = os.path.dirname(os.path.dirname(HARNESS))
    src, obj = tmp_path / "actor_only.hip", tmp_path / "actor_only.co"
    src.write_text('#include <hip/hip_runtime.h>\n#include "%s"\n' % os.path.join(root, "random-envs_amd", "csrc", "actor.hpp"))
    flags = [f for f in g.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", str(obj), str(src)],
                          stderr=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(root, "profiles", "kmeta.py"), str(obj)], capture_output=True, text=True, check=True).stdout
    line = [l for l in out.splitlines() if "actor_kernel" in l]
    print(out)
    assert len(line) == 1
    f = line[0].split()
    meta = {f[k]: f[k + 1] for k in range(1, len(f) - 1, 2)}
    assert meta["spill"] == "0" and meta["scratch"] == "0" and meta["agpr"] == "0"
    assert int(meta["vgpr"]) <= 256 and int(meta["lds"]) == 4 * 64 * 65
