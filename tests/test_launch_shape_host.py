"""The launch-shape rule without a GPU: csrc/launch_shape.hpp (compiled with g++ by tests/host_harness/shape_host.cpp) against
sharding.shape_for_batch, the Python restatement that pinned shards rely on for bit-reproducibility, for SIMD counts no single card
shows; the precedence of the tuning knobs, the shape request / report of the C-ABI and the reset plan of a step as literal tables."""
import ctypes
import itertools

import pytest

from host_harness.build import build_so

KINDS = {"cartpole": 0, "hopper": 1, "halfcheetah": 2, "walker2d": 3, "humanoid": 4}
KNOBS = ("REX_LANES", "REX_PAIR", "REX_ROLLED", "REX_HUM_PAIR", "REX_HUM_FUSED_RESET", "REX_FUSED_DERIVE", "REX_FAST")
FIELDS = ("lanes", "pair_lanes", "pair", "rolled", "hum_pair", "hum_fused_reset", "fused_derive")
REX_OK, REX_ERR_ARG = 0, -1
DR_NONE, DR_UNIFORM = 0, 1
RS_RESAMPLE, RS_DERIVE, RS_REFRESH = 1, 2, 4

_lib = None


def harness():
    """tests/host_harness/shape_host.cpp built with g++ (rebuilt when it or a header is newer)"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_so("shape_host", "shape_host.cpp", ["-Wall", "-Werror"]))
        vp, ll, i32 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
        _lib.sh_why.restype = ctypes.c_char_p
        _lib.sh_choose.argtypes = [i32, ll, i32, vp, vp, vp]
        _lib.sh_apply.argtypes = [i32, vp, vp, vp]
        _lib.sh_reset_plan.argtypes = [i32, i32, i32, i32, i32, vp, vp]
        _lib.sh_reset_plan.restype = None
        _lib.sh_grid.argtypes = [vp, ll, vp]
        _lib.sh_grid.restype = None
    return _lib


def _i32(values):
    return (ctypes.c_int32 * len(values))(*values)


def choose(kind, batch, simds, **knobs):
    """(rc, message, the seven fields, what rex_get_launch_shape reports) of choose_launch_shape with the given knobs set"""
    assert set(knobs) <= set(KNOBS)
    flat = []
    for name in KNOBS:
        flat += [1, int(knobs[name])] if name in knobs else [0, 0]
    fields, report = _i32([0] * 7), _i32([0] * 4)
    rc = harness().sh_choose(KINDS[kind], batch, simds, _i32(flat), fields, report)
    return rc, harness().sh_why().decode(), dict(zip(FIELDS, fields)), reported(report)


def reported(report):
    return dict(lanes=report[0], pair=bool(report[1]), rolled=bool(report[2]), hum_pair=bool(report[3]))


def apply(kind, fields, lanes=-1, pair=-1, rolled=-1, hum_pair=-1):
    """(rc, message, fields afterwards, report afterwards) of apply_shape_request on a shape given as the seven fields"""
    f, report = _i32([fields[k] for k in FIELDS]), _i32([0] * 4)
    rc = harness().sh_apply(KINDS[kind], _i32([int(lanes), int(pair), int(rolled), int(hum_pair)]), f, report)
    return rc, harness().sh_why().decode(), dict(zip(FIELDS, f)), reported(report)


def batches(simds):
    out = [1, 2, 63, 64, 65, 4095, 4096, 4097, 524287, 524288, 2 ** 20]
    for m in (8, 16, 32, 64):
        out += [m * simds - 1, m * simds, m * simds + 1]
    return sorted(set(out))


@pytest.mark.parametrize("simds", [64, 1024, 1216])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_rule_agrees_with_its_python_restatement(kind, simds):
    """choose_launch_shape with no knob set reports what sharding.shape_for_batch says, at every threshold of the rule and its neighbours:
    every batch of tests/test_gpu_api.py::test_launch_shape_follows_the_batch, and the SIMD counts that test cannot see on one card."""
    from random_envs_amd import sharding
    for batch in batches(simds):
        rc, why, fields, report = choose(kind, batch, simds)
        assert rc == REX_OK, (kind, simds, batch, why)
        assert report == sharding.shape_for_batch(kind, batch, simds), (kind, simds, batch, fields)


def test_knob_precedence():
    """The order in which the knobs bear on the shape, literally (simds = 1 024: an MI355X)."""
    S = 1024
    rc, _, f, rep = choose("hopper", 256, S, REX_PAIR=0, REX_ROLLED=1, REX_LANES=64)
    assert rc == REX_OK and rep == dict(lanes=64, pair=False, rolled=True, hum_pair=False)
    assert choose("hopper", 256, S)[3]["pair"] is True
    assert choose("hopper", 256, S, REX_FAST=0)[3]["pair"] is False          # the strict-lane-independence mode: one lane per env ...
    assert choose("hopper", 256, S, REX_FAST=0, REX_PAIR=1)[3]["pair"] is True   # ... unless REX_PAIR asks for the pair kernel
    assert choose("hopper", 256, S, REX_FAST=1)[3]["pair"] is True
    _, _, f, rep = choose("hopper", 256, S, REX_PAIR=1, REX_ROLLED=1)         # pair clears rolled
    assert (f["pair"], f["rolled"]) == (1, 0) and rep["pair"] and not rep["rolled"]
    _, _, f, rep = choose("hopper", 128 * S, S, REX_PAIR=1)                   # ... the batch's own rolled as well
    assert (f["pair"], f["rolled"]) == (1, 0)
    _, _, f, rep = choose("walker2d", 256, S, REX_PAIR=0, REX_ROLLED=1)       # the rolled kernel exists for the hopper only
    assert f["rolled"] == 0 and not rep["rolled"]
    rc, why, _, _ = choose("hopper", 256, S, REX_LANES=48)
    assert rc == REX_ERR_ARG and why == "REX_LANES must be 8, 16, 32 or 64 (got 48)"
    for bad in (4, 128, 65, 7):
        assert choose("walker2d", 256, S, REX_LANES=bad)[0] == REX_ERR_ARG
    for kind in KINDS:                                                        # REX_LANES sets both widths, whatever the batch gave
        for batch in (256, 8 * S, 128 * S):
            rc, _, f, _ = choose(kind, batch, S, REX_LANES=16)
            assert rc == REX_OK and (f["lanes"], f["pair_lanes"]) == (16, 16)
    assert choose("walker2d", 8 * S, S, REX_LANES=0)[2]["pair_lanes"] == 16   # REX_LANES=0 is no request: the batch's widths
    for kind in KINDS:                                                        # fused_derive: below 524 288 envs, and as REX_FUSED_DERIVE says
        assert choose(kind, 524287, S)[2]["fused_derive"] == 1 and choose(kind, 524288, S)[2]["fused_derive"] == 0
        assert choose(kind, 524288, S, REX_FUSED_DERIVE=1)[2]["fused_derive"] == 1
        assert choose(kind, 64, S, REX_FUSED_DERIVE=0)[2]["fused_derive"] == 0
    _, _, f, rep = choose("humanoid", 64, S)
    assert (f["hum_pair"], f["hum_fused_reset"]) == (1, 1) and rep["hum_pair"]
    _, _, f, rep = choose("humanoid", 64, S, REX_HUM_PAIR=0)
    assert (f["hum_pair"], f["hum_fused_reset"]) == (0, 1) and not rep["hum_pair"]
    _, _, f, rep = choose("humanoid", 64, S, REX_HUM_FUSED_RESET=0)
    assert (f["hum_pair"], f["hum_fused_reset"]) == (1, 0) and rep["hum_pair"]


def test_shape_requests():
    """apply_shape_request / report_shape: the round trip and the refusals of
    tests/test_gpu_api.py::test_stray_knobs_are_refused_and_shapes_are_pinned_through_the_abi, -1 keeps a field, a lanes request sets
    both widths, a refused request changes nothing."""
    S = 1024
    _, _, f, rep = choose("hopper", 256, S)
    assert rep == dict(lanes=64, pair=True, rolled=False, hum_pair=False)
    rc, _, f, rep = apply("hopper", f, lanes=64, pair=False)
    assert rc == REX_OK and rep == dict(lanes=64, pair=False, rolled=False, hum_pair=False) and (f["lanes"], f["pair_lanes"]) == (64, 64)
    rc, _, f, rep = apply("hopper", f, rolled=True)
    assert rc == REX_OK and rep == dict(lanes=64, pair=False, rolled=True, hum_pair=False)
    rc, _, g, rep = apply("hopper", f)                                        # all -1: nothing changes
    assert rc == REX_OK and g == f and rep == dict(lanes=64, pair=False, rolled=True, hum_pair=False)
    for bad, msg in ((dict(lanes=48), "rex_set_launch_shape: lanes must be 8, 16, 32 or 64 (got 48)"),
                     (dict(pair=True), "rex_set_launch_shape: the rolled kernel is a one-lane-per-env kernel (pair and rolled exclude each other)"),
                     (dict(hum_pair=True), "rex_set_launch_shape: hum_pair is a shape of the humanoid")):
        rc, why, g, _ = apply("hopper", f, **bad)
        assert rc == REX_ERR_ARG and why == msg and g == f, bad
    _, _, w, _ = choose("walker2d", 64, S)
    rc, why, g, _ = apply("walker2d", w, rolled=True)
    assert rc == REX_ERR_ARG and why == "rex_set_launch_shape: the rolled kernel exists for the hopper only" and g == w
    for kind in ("cartpole", "humanoid"):
        _, _, c, _ = choose(kind, 64, S)
        rc, why, g, _ = apply(kind, c, pair=True)
        assert rc == REX_ERR_ARG and why == "rex_set_launch_shape: two lanes per env (pair) is a shape of the planar chains" and g == c
    for kind in ("cartpole", "hopper", "halfcheetah", "walker2d"):
        _, _, c, _ = choose(kind, 64, S)
        assert apply(kind, c, hum_pair=True)[0] == REX_ERR_ARG
    _, _, hm, _ = choose("humanoid", 64, S)
    rc, _, g, rep = apply("humanoid", hm, hum_pair=False)
    assert rc == REX_OK and g["hum_pair"] == 0 and not rep["hum_pair"]
    # a lanes request sets both widths; without one a walker2d batch keeps the two it was created with
    _, _, w, rep = choose("walker2d", 8 * S, S)
    assert (w["lanes"], w["pair_lanes"]) == (32, 16) and rep["lanes"] == 16
    rc, _, g, rep = apply("walker2d", w, pair=False)
    assert rc == REX_OK and (g["lanes"], g["pair_lanes"]) == (32, 16) and rep == dict(lanes=32, pair=False, rolled=False, hum_pair=False)
    rc, _, g, rep = apply("walker2d", w, lanes=8)
    assert rc == REX_OK and (g["lanes"], g["pair_lanes"]) == (8, 8) and rep["lanes"] == 8


def _plan_oracle(kind, variant, autoreset, dr_training, dr_type, fused_derive, hum_pair, hum_fused_reset):
    """the expression at the top of rex_step (and the resample line of rex_reset) as it stood before reset_plan, restated"""
    resample_on_reset = 1 if (dr_training and kind != "cartpole") else 0
    walker_dr = kind == "walker2d" and resample_on_reset and dr_type != DR_NONE
    fused = 1 if (autoreset and (kind == "hopper" or kind == "halfcheetah" or (kind == "walker2d" and (not walker_dr or fused_derive)) or
                                 (kind == "humanoid" and hum_pair and hum_fused_reset))) else 0
    rs = RS_RESAMPLE if resample_on_reset else 0
    if walker_dr and fused_derive:
        rs |= RS_DERIVE | (RS_REFRESH if variant else 0)
    return [fused, rs, resample_on_reset]


def test_reset_plan_truth_table():
    """reset_plan over every combination of its inputs.  Cart-pole: never fused, never resampled.  Walker2d under DR: fused only with
    fused_derive, and then RS_DERIVE, plus RS_REFRESH for the Unmodeled id."""
    lib = harness()
    n = 0
    for kind, variant, autoreset, dr_training, dr_type, fused_derive, hum_pair, hum_fused_reset in itertools.product(
            sorted(KINDS), (0, 1), (0, 1), (0, 1), (DR_NONE, DR_UNIFORM), (0, 1), (0, 1), (0, 1)):
        fields = dict(lanes=32, pair_lanes=64, pair=1, rolled=0, hum_pair=hum_pair, hum_fused_reset=hum_fused_reset, fused_derive=fused_derive)
        out = _i32([0] * 3)
        lib.sh_reset_plan(KINDS[kind], variant, autoreset, dr_training, dr_type, _i32([fields[k] for k in FIELDS]), out)
        want = _plan_oracle(kind, variant, autoreset, dr_training, dr_type, fused_derive, hum_pair, hum_fused_reset)
        assert list(out) == want, (kind, variant, autoreset, dr_training, dr_type, fields)
        if kind == "cartpole":
            assert list(out) == [0, 0, 0]
        if kind == "walker2d" and autoreset and dr_training and dr_type == DR_UNIFORM:
            assert list(out) == ([1, RS_RESAMPLE | RS_DERIVE | (RS_REFRESH if variant else 0), 1] if fused_derive else [0, RS_RESAMPLE, 1])
        n += 1
    assert n == 5 * 128


def test_one_lane_launches_cover_the_batch():
    """LaunchShape::grid / block: blocks of `lanes` lanes, the last one partial"""
    lib = harness()
    for lanes in (8, 16, 32, 64):
        for B in (1, lanes - 1, lanes, lanes + 1, 1000, 2 ** 20, 2 ** 31 + 5):
            out = _i32([0] * 2)
            lib.sh_grid(_i32([lanes, 64, 1, 0, 1, 1, 1]), B, out)
            assert out[1] == lanes and (out[0] - 1) * lanes < B <= out[0] * lanes, (lanes, B, list(out))
