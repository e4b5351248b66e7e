"""ctypes binding of the C-ABI declared in include/rex.h (librex_hip.so).

The library is loaded lazily and loudly: if it is missing or cannot be loaded (no ROCm runtime,
not built), every entry point raises -- the product path never falls back to CPU code.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("REX_LIB", "librex_hip.so"))   # REX_LIB: A/B builds while tuning

# every symbol include/rex.h declares (tests check the built library exports all of them)
SYMBOLS = [
    "rex_get_dims", "rex_create", "rex_destroy", "rex_set_dr", "rex_set_dr_training", "rex_set_flags",
    "rex_set_autoreset", "rex_seed", "rex_reset", "rex_step", "rex_get_state", "rex_set_state",
    "rex_get_task", "rex_set_task", "rex_set_random_task", "rex_get_obs", "rex_step_count",
    "rex_get_counters", "rex_enable_timing", "rex_read_timing", "rex_last_error", "rex_version",
    "rex_get_counters_state", "rex_set_counters_state", "rex_sample_task", "rex_set_info_buffer", "rex_export_lane", "rex_get_aux", "rex_set_aux", "rex_replay",
    "rex_get_launch_shape", "rex_set_launch_shape",
    "rex_norm_enable", "rex_norm_set_training", "rex_norm_reset", "rex_norm_step", "rex_norm_get_stats", "rex_norm_set_stats",
    "rex_norm_get_lane_state", "rex_norm_set_lane_state", "rex_norm_read_episodes",
    "rex_rollout_enable", "rex_rollout_add", "rex_rollout_gae", "rex_rollout_adv_stats", "rex_rollout_get_adv_stats", "rex_rollout_gather",
    "rex_rollout_read_bad_indices",
    "rex_eplog_enable", "rex_eplog_step", "rex_eplog_sync", "rex_eplog_read", "rex_eplog_get_lane_state", "rex_eplog_set_lane_state",
    "rex_rbuf_enable", "rex_rbuf_add", "rex_rbuf_sample", "rex_rbuf_gather", "rex_rbuf_read_bad_indices",
    "rex_per_tree_len", "rex_per_enable", "rex_per_init", "rex_per_add", "rex_per_update", "rex_per_rebuild", "rex_per_draw", "rex_per_sample",
    "rex_per_read_counters",
    "rex_rbuf_gather_nstep", "rex_rbuf_sample_nstep", "rex_per_sample_nstep",
    "rex_rbuf_gather_seq", "rex_rbuf_sample_seq", "rex_per_sample_seq",
    "rex_rows_enable", "rex_reset_rows", "rex_step_rows",
    "rex_hist_init", "rex_hist_push", "rex_hist_reset", "rex_hist_window",
    "rex_adr_enable", "rex_adr_record", "rex_adr_assign", "rex_adr_update", "rex_adr_get_state", "rex_adr_set_state",
    "rex_adr_get_lane_state", "rex_adr_set_lane_state",
    "rex_actor_act",
]

ENV_KINDS = {"cartpole": 0, "hopper": 1, "halfcheetah": 2, "walker2d": 3, "humanoid": 4}
DR_TYPES = {None: 0, "uniform": 1, "truncnorm": 2, "gaussian": 3, "fullgaussian": 4}


class RexDims(ctypes.Structure):
    _fields_ = [("nq", ctypes.c_int), ("nv", ctypes.c_int), ("act_dim", ctypes.c_int), ("obs_dim", ctypes.c_int),
                ("task_dim", ctypes.c_int), ("frame_skip", ctypes.c_int), ("max_episode_steps", ctypes.c_int),
                ("discrete_action", ctypes.c_int), ("dt", ctypes.c_float), ("act_low", ctypes.c_float),
                ("act_high", ctypes.c_float), ("n_info", ctypes.c_int), ("n_aux", ctypes.c_int)]


class RexNormConfig(ctypes.Structure):
    _fields_ = [("gamma", ctypes.c_double), ("epsilon", ctypes.c_double), ("clip_obs", ctypes.c_double),
                ("clip_reward", ctypes.c_double), ("norm_obs", ctypes.c_int), ("norm_reward", ctypes.c_int),
                ("training", ctypes.c_int)]


class RexRolloutBuffers(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("obs", "action", "reward", "value", "log_prob", "advantage", "returns", "done")] + [("T", ctypes.c_int64)]


class RexEplogBuffers(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("task", "ep_return", "ep_len", "flags", "env", "step")] + [("capacity", ctypes.c_int64)]


class RexRbufBuffers(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("obs", "next_obs", "action", "reward", "done", "timeout")] + [("T", ctypes.c_int64)]


class RexPerBuffers(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("priority", "tree", "max_priority")] + [("T", ctypes.c_int64)]


class RexHistBuffers(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_void_p), ("length", ctypes.c_void_p), ("K", ctypes.c_int), ("with_action", ctypes.c_int)]


class RexAdrConfig(ctypes.Structure):
    _fields_ = [("n_act", ctypes.c_int32), ("act", ctypes.c_void_p), ("p_b", ctypes.c_float), ("m", ctypes.c_int64), ("t_lo", ctypes.c_double),
                ("t_hi", ctypes.c_double)] + [(k, ctypes.c_void_p) for k in ("delta", "lim_lo", "lim_hi", "centre", "init_lo", "init_hi")] + [("seed", ctypes.c_uint64)]


ACTOR_MAX_HIDDEN = 3


class RexActorTower(ctypes.Structure):
    _fields_ = [("n_hidden", ctypes.c_int), ("width", ctypes.c_int * ACTOR_MAX_HIDDEN), ("W", ctypes.c_void_p * (ACTOR_MAX_HIDDEN + 1)),
                ("b", ctypes.c_void_p * (ACTOR_MAX_HIDDEN + 1))]


class RexActorNet(ctypes.Structure):
    _fields_ = [("in_dim", ctypes.c_int), ("activation", ctypes.c_int), ("pi", ctypes.POINTER(RexActorTower)), ("vf", ctypes.POINTER(RexActorTower)),
                ("log_std", ctypes.c_void_p), ("std", ctypes.c_void_p), ("seed", ctypes.c_uint64)]


class RexError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RexError("librex_hip.so not built (%s missing): run `python -c 'import __graft_entry__ as g; "
                       "g.build()'` -- there is no CPU fallback" % LIB_PATH)
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 missing
        raise RexError("cannot load %s: %s" % (LIB_PATH, e))
    vp, i32, i64, u64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float
    fp = ctypes.POINTER(ctypes.c_float)
    L.rex_get_dims.argtypes = [i32, i32, ctypes.POINTER(RexDims)]
    L.rex_create.argtypes = [i32, i32, i64, i32, u64, i64, ctypes.POINTER(vp)]
    L.rex_destroy.argtypes = [vp]
    L.rex_set_dr.argtypes = [vp, i32, fp, i32, fp]
    L.rex_set_dr_training.argtypes = [vp, i32]
    L.rex_set_flags.argtypes = [vp, i32, i32, f32]
    L.rex_set_autoreset.argtypes = [vp, i32, i32]
    L.rex_seed.argtypes = [vp, u64]
    L.rex_reset.argtypes = [vp, vp, vp, vp]
    L.rex_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.rex_rows_enable.argtypes = [vp]
    L.rex_reset_rows.argtypes = [vp, vp, vp, vp]
    L.rex_step_rows.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.rex_get_state.argtypes = [vp, vp, vp, vp]
    L.rex_set_state.argtypes = [vp, vp, vp, vp]
    L.rex_get_task.argtypes = [vp, vp, vp]
    L.rex_set_task.argtypes = [vp, vp, vp]
    L.rex_set_random_task.argtypes = [vp, vp, vp]
    L.rex_get_obs.argtypes = [vp, vp, vp]
    L.rex_step_count.argtypes = [vp]
    L.rex_step_count.restype = i64
    L.rex_get_counters.argtypes = [vp, ctypes.POINTER(i64)]
    L.rex_get_launch_shape.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.rex_set_launch_shape.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.rex_enable_timing.argtypes = [vp, i32]
    L.rex_read_timing.argtypes = [vp, fp, i32]
    L.rex_get_counters_state.argtypes = [vp, vp, vp, vp, vp]
    L.rex_set_counters_state.argtypes = [vp, vp, vp, vp, vp]
    L.rex_sample_task.argtypes = [vp, vp, u64, vp]
    L.rex_set_info_buffer.argtypes = [vp, vp]
    L.rex_export_lane.argtypes = [vp, i64, fp, fp, fp]
    L.rex_replay.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rex_get_aux.argtypes = [vp, vp, vp]
    L.rex_set_aux.argtypes = [vp, vp, vp]
    dp = ctypes.POINTER(ctypes.c_double)
    L.rex_norm_enable.argtypes = [vp, ctypes.POINTER(RexNormConfig)]
    L.rex_norm_set_training.argtypes = [vp, i32]
    L.rex_norm_reset.argtypes = [vp, vp, vp, vp, vp]
    L.rex_norm_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rex_norm_get_stats.argtypes = [vp, dp]
    L.rex_norm_set_stats.argtypes = [vp, dp]
    L.rex_norm_get_lane_state.argtypes = [vp, vp, vp, vp, vp]
    L.rex_norm_set_lane_state.argtypes = [vp, vp, vp, vp, vp]
    L.rex_norm_read_episodes.argtypes = [vp, dp, i32]
    bp, f64 = ctypes.POINTER(RexRolloutBuffers), ctypes.c_double
    L.rex_rollout_enable.argtypes = [vp]
    L.rex_rollout_add.argtypes = [vp, bp, i64, vp, vp, vp, vp, vp, vp, vp, vp, f64, vp]
    L.rex_rollout_gae.argtypes = [vp, bp, vp, f64, f64, vp]
    L.rex_rollout_adv_stats.argtypes = [vp, bp, i32, vp]
    L.rex_rollout_get_adv_stats.argtypes = [vp, dp]
    L.rex_rollout_gather.argtypes = [vp, bp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    L.rex_rollout_read_bad_indices.argtypes = [vp, ctypes.POINTER(i64), i32]
    L.rex_eplog_enable.argtypes = [vp, ctypes.POINTER(RexEplogBuffers)]
    L.rex_eplog_step.argtypes = [vp, vp, vp, vp, vp]
    L.rex_eplog_sync.argtypes = [vp, vp, i32, vp]
    L.rex_eplog_read.argtypes = [vp, ctypes.POINTER(i64), i32]
    L.rex_eplog_get_lane_state.argtypes = [vp, vp, vp, vp, vp]
    L.rex_eplog_set_lane_state.argtypes = [vp, vp, vp, vp, vp]
    rp = ctypes.POINTER(RexRbufBuffers)
    L.rex_rbuf_enable.argtypes = [vp]
    L.rex_rbuf_add.argtypes = [vp, rp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rex_rbuf_sample.argtypes = [vp, rp, i64, i64, u64, u64, i32, vp, vp, vp, vp, vp, vp, vp]
    L.rex_rbuf_gather.argtypes = [vp, rp, vp, i64, i32, vp, vp, vp, vp, vp, vp]
    L.rex_rbuf_read_bad_indices.argtypes = [vp, ctypes.POINTER(i64), i32]
    pp = ctypes.POINTER(RexPerBuffers)
    L.rex_per_tree_len.argtypes = [i64]
    L.rex_per_tree_len.restype = i64
    L.rex_per_enable.argtypes = [vp]
    L.rex_per_init.argtypes = [vp, pp, vp]
    L.rex_per_add.argtypes = [vp, pp, i64, vp]
    L.rex_per_update.argtypes = [vp, pp, vp, vp, i64, vp]
    L.rex_per_rebuild.argtypes = [vp, pp, vp]
    L.rex_per_draw.argtypes = [vp, pp, i64, u64, u64, vp, vp, vp]
    L.rex_per_sample.argtypes = [vp, rp, pp, i64, u64, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rex_per_read_counters.argtypes = [vp, ctypes.POINTER(i64), i32]
    L.rex_rbuf_gather_nstep.argtypes = [vp, rp, vp, i64, i64, i32, f64, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rex_rbuf_sample_nstep.argtypes = [vp, rp, i64, i64, i64, u64, u64, i32, f64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rex_per_sample_nstep.argtypes = [vp, rp, pp, i64, i64, u64, u64, i32, f64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rex_rbuf_gather_seq.argtypes = [vp, rp, vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.rex_rbuf_sample_seq.argtypes = [vp, rp, i64, i64, i64, u64, u64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rex_per_sample_seq.argtypes = [vp, rp, pp, i64, i64, u64, u64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    hp = ctypes.POINTER(RexHistBuffers)
    L.rex_hist_init.argtypes = [vp, hp, vp]
    L.rex_hist_push.argtypes = [vp, hp, i64, vp, vp, vp, vp, vp, i32, vp]
    L.rex_hist_reset.argtypes = [vp, hp, i64, vp, vp, i32, vp]
    L.rex_hist_window.argtypes = [vp, hp, i64, vp, vp]
    L.rex_adr_enable.argtypes = [vp, ctypes.POINTER(RexAdrConfig)]
    L.rex_adr_record.argtypes = [vp, vp, vp, i32, vp]
    L.rex_adr_assign.argtypes = [vp, vp, vp]
    L.rex_adr_update.argtypes = [vp, vp]
    L.rex_adr_get_state.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rex_adr_set_state.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rex_adr_get_lane_state.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rex_adr_set_lane_state.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rex_actor_act.argtypes = [vp, ctypes.POINTER(RexActorNet), vp, i32, i64, i32, vp, vp, vp, vp, vp]
    L.rex_last_error.restype = ctypes.c_char_p
    L.rex_version.restype = ctypes.c_char_p
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = lib().rex_last_error().decode()
        if rc == -1:
            raise ValueError(msg)
        raise RexError("rex error %d: %s" % (rc, msg))


def exported_symbols():
    """Names from SYMBOLS that the built library exports (no GPU needed: dlsym only)."""
    if not os.path.exists(LIB_PATH):
        raise RexError("librex_hip.so not built")
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    return [s for s in SYMBOLS if s in names]
