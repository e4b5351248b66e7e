"""Records tests/golden/abi_errors.json: what the host argument checks of the C-ABI answer -- (return code, rex_last_error()) per case.

The checks sit behind REX_ENTER, so only a GPU run reaches them.  Record the fixture from the commit whose answers are to be kept -- run

    python tests/golden/record_abi_errors.py

on the MI355X there, and commit the .json; tests/test_gpu_abi_errors.py replays cases() below and compares exactly.  A change that only moves
or merges host code must leave every pair as it is, the FIRST error of a call with two bad arguments included (the "a+b" cases pin the order of
the checks).

Every case returns before any kernel launch: its arguments are ones a check rejects, or n == 0 (REX_OK without a launch; the message of an OK
call is not part of the contract and is recorded as "").  Even so every non-null device pointer points into one zeroed 1 MiB device block, far
larger than anything a batch of 4 with T = 4 addresses, so a case that did launch would stay inside it.

Handles (batch 4, autoreset off): H hopper with rex_rbuf / rex_per / rex_rollout enabled and NO rex_norm_enable (the normalise cases); N hopper
with rex_norm and rex_per only (the norm argument cases, and the second REX_NEEDS of the prioritised calls); Z hopper with no layer (the REX_NEEDS
cases); C cart-pole (misaligned rows, unsupported calls).  rex_eplog_enable launches, so no handle enables the ledger.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, "abi_errors.json")
B, T = 4, 4
NAN = float("nan")

# the sample family: argument names in the order of include/rex.h.  rb / pb: the two buffer descriptions; every other name that DEFAULTS does not
# hold is a device pointer
SAMPLE = {
    "rex_rbuf_sample": "rb size n seed draw normalise obs next_obs action reward done index_out stream",
    "rex_rbuf_gather": "rb index n normalise obs next_obs action reward done stream",
    "rex_per_sample": "rb pb n seed draw normalise obs next_obs action reward done index_out prob_out stream",
    "rex_rbuf_gather_nstep": "rb index n head n_step gamma normalise obs next_obs action reward done discount steps stream",
    "rex_rbuf_sample_nstep": "rb size head n seed draw n_step gamma normalise obs next_obs action reward done discount steps index_out stream",
    "rex_per_sample_nstep": "rb pb n head seed draw n_step gamma normalise obs next_obs action reward done discount steps index_out prob_out stream",
    "rex_rbuf_gather_seq": "rb index n head seq_len normalise obs action reward done mask length stream",
    "rex_rbuf_sample_seq": "rb size head n seed draw seq_len normalise obs action reward done mask length index_out stream",
    "rex_per_sample_seq": "rb pb n head seed draw seq_len normalise obs action reward done mask length index_out prob_out stream",
}
# a call that passes every check and, with n == 0, returns REX_OK without launching: a full ring (size == T), so any head in [0, T) is allowed
DEFAULTS = dict(rb="ok", pb="ok", size=T, n=0, seed=1, draw=0, normalise=0, head=T - 1, n_step=3, gamma=0.99, seq_len=3, stream=None)


class Ctx:
    """the library, the four handles and the device block every pointer points into"""

    def __init__(self):
        import torch
        from random_envs_amd import _native
        assert torch.cuda.is_available()
        self.N = _native
        self.L = L = _native.lib()
        self.block = torch.zeros(1 << 18, dtype=torch.float32, device="cuda")
        self.P = self.block.data_ptr()
        assert self.P % 16 == 0
        self.handles = []
        self.H, self.Nh, self.Z, self.C = (self._create(k) for k in (1, 1, 1, 0))
        for fn, h in (("rex_rbuf_enable", self.H), ("rex_per_enable", self.H), ("rex_rollout_enable", self.H), ("rex_norm_enable", self.Nh),
                      ("rex_per_enable", self.Nh)):
            rc = getattr(L, fn)(*((h, None) if fn == "rex_norm_enable" else (h,)))
            assert rc == 0, (fn, L.rex_last_error())
        torch.cuda.synchronize()

    def _create(self, kind):
        h = ctypes.c_void_p()
        assert self.L.rex_create(kind, 0, B, 0, 0, 0, ctypes.byref(h)) == 0, self.L.rex_last_error()
        assert self.L.rex_set_autoreset(h, 0, 1) == 0
        self.handles.append(h)
        return h

    def close(self):
        for h in self.handles:
            self.L.rex_destroy(h)
        self.handles = []

    def desc(self, cls, how, t_field="T"):
        """a buffer description: "ok", None (a null description), "null_ptr" (its second pointer null), or an int for its T / capacity"""
        if how is None:
            return None
        d = cls()
        for name, _ in cls._fields_[:-1]:
            setattr(d, name, self.P)
        setattr(d, t_field, how if isinstance(how, int) else T)
        if how == "null_ptr":
            setattr(d, cls._fields_[1][0], None)
        return ctypes.byref(d)

    def sample(self, fn, h, **over):
        a = dict(DEFAULTS, **over)
        args = []
        for name in SAMPLE[fn].split():
            if name == "rb":
                args.append(self.desc(self.N.RexRbufBuffers, a["rb"]))
            elif name == "pb":
                args.append(self.desc(self.N.RexPerBuffers, a["pb"]))
            else:
                args.append(a.get(name, self.P))
        return getattr(self.L, fn)(h, *args)


def _sample_cases(c):
    for fn, names in SAMPLE.items():
        names = names.split()
        per, gather, uniform = "pb" in names, "index" in names, "size" in names
        nstep, seq = "n_step" in names, "seq_len" in names
        window = dict(head=-1)
        def S(fn=fn, h=c.H, **kw):
            return lambda: c.sample(fn, h, **kw)
        yield fn + "/not_enabled", S(h=c.Z)
        if per:
            yield fn + "/per_but_no_rbuf", S(h=c.Nh)
        yield fn + "/n0_ok", S()
        for how in (None, "null_ptr", 0):
            yield fn + "/rb_%s" % how, S(rb=how)
            if per:
                yield fn + "/pb_%s" % how, S(pb=how)
        if per:
            yield fn + "/pb_too_many", S(pb=1 << 30)
            yield fn + "/T_disagree", S(pb=T - 1)
            yield fn + "/pb_None+rb_None", S(pb=None, rb=None)
        if uniform:
            yield fn + "/size_0", S(size=0)
            yield fn + "/size_T+1", S(size=T + 1)
        yield fn + "/n_-1", S(n=-1)
        if gather:
            yield fn + "/n_1_null_index", S(n=1, index=None)
        if per:
            yield fn + "/n_1_null_index_out", S(n=1, index_out=None)
            yield fn + "/n_1_null_prob_out", S(n=1, prob_out=None)
        if nstep or seq:
            yield fn + "/head_-1", S(head=-1)
            yield fn + "/head_T", S(head=T)
        if nstep:
            for v in (0, 33):
                yield fn + "/n_step_%d" % v, S(n_step=v)
            for v in (1.5, NAN, -0.5):
                yield fn + "/gamma_%s" % v, S(gamma=v)
            yield fn + "/n_step_0+gamma_nan+head_-1", S(n_step=0, gamma=NAN, head=-1)
            yield fn + "/gamma_nan+head_-1", S(gamma=NAN, head=-1)
        if seq:
            for v in (0, 65):
                yield fn + "/seq_len_%d" % v, S(seq_len=v)
            yield fn + "/seq_len_0+head_-1", S(seq_len=0, head=-1)
        if uniform and (nstep or seq):
            yield fn + "/ring_not_full", S(size=2, head=0)
            yield fn + "/ring_not_full_ok", S(size=2, head=1)
            yield fn + "/size_0+ring", S(size=0, head=2)
            yield fn + "/ring+n_-1", S(size=2, head=0, n=-1)
        yield fn + "/normalise_without_norm", S(normalise=1)
        if nstep or seq:   # the order of the checks: description, window, id source, normalise
            yield fn + "/rb_None+window", S(rb=None, **window)
            yield fn + "/rb_0+window", S(rb=0, **window)
            if per:
                yield fn + "/T_disagree+window", S(pb=T - 1, **window)
            if uniform:
                yield fn + "/window+size_0", S(size=0, **window)
            yield fn + "/window+n_-1", S(n=-1, **window)
            yield fn + "/window+normalise", S(normalise=1, **window)
        if uniform:
            yield fn + "/size_0+n_-1", S(size=0, n=-1)
        yield fn + "/n_-1+normalise", S(n=-1, normalise=1)
        yield fn + "/rb_None+n_-1", S(rb=None, n=-1)


def _layer_cases(c):
    L, P, H, Nh, Z, C = c.L, c.P, c.H, c.Nh, c.Z, c.C
    RO, RB, PB, EL = c.N.RexRolloutBuffers, c.N.RexRbufBuffers, c.N.RexPerBuffers, c.N.RexEplogBuffers
    ro = lambda how="ok": c.desc(RO, how)   # noqa: E731
    rb = lambda how="ok": c.desc(RB, how)   # noqa: E731
    pb = lambda how="ok": c.desc(PB, how)   # noqa: E731
    i64x4 = (ctypes.c_int64 * 4)()
    dbl = (ctypes.c_double * 64)()        # host memory of 3 * (obs_dim + 1) = 36 doubles and more, all 0: no row has count > 0
    flt = (ctypes.c_float * 16)()

    # ---- rollout
    def add(h, d, t=0, src=(P,) * 6, trunc=P, tv=P):
        return L.rex_rollout_add(h, d, t, *src, trunc, tv, 0.99, None)
    yield "rex_rollout_add/not_enabled", lambda: add(Z, ro())
    for how in (None, "null_ptr", 0):
        yield "rex_rollout_add/buf_%s" % how, lambda how=how: add(H, ro(how))
        yield "rex_rollout_gae/buf_%s" % how, lambda how=how: L.rex_rollout_gae(H, ro(how), P, 0.99, 0.95, None)
        yield "rex_rollout_adv_stats/buf_%s" % how, lambda how=how: L.rex_rollout_adv_stats(H, ro(how), 1, None)
        yield "rex_rollout_gather/buf_%s" % how, lambda how=how: L.rex_rollout_gather(H, ro(how), P, 0, P, P, P, P, P, P, None)
    yield "rex_rollout_add/slot_-1", lambda: add(H, ro(), t=-1)
    yield "rex_rollout_add/slot_T", lambda: add(H, ro(), t=T)
    for k in range(6):
        yield "rex_rollout_add/null_input_%d" % k, lambda k=k: add(H, ro(), src=tuple(None if j == k else P for j in range(6)))
    yield "rex_rollout_add/truncated_alone", lambda: add(H, ro(), tv=None)
    yield "rex_rollout_add/terminal_value_alone", lambda: add(H, ro(), trunc=None)
    yield "rex_rollout_add/buf_None+slot_-1", lambda: add(H, ro(None), t=-1)
    yield "rex_rollout_add/slot_-1+null_input", lambda: add(H, ro(), t=-1, src=(None,) * 6)
    yield "rex_rollout_gae/not_enabled", lambda: L.rex_rollout_gae(Z, ro(), P, 0.99, 0.95, None)
    yield "rex_rollout_gae/null_last_value", lambda: L.rex_rollout_gae(H, ro(), None, 0.99, 0.95, None)
    yield "rex_rollout_adv_stats/not_enabled", lambda: L.rex_rollout_adv_stats(Z, ro(), 1, None)
    yield "rex_rollout_get_adv_stats/not_enabled", lambda: L.rex_rollout_get_adv_stats(Z, dbl)
    yield "rex_rollout_get_adv_stats/null_out", lambda: L.rex_rollout_get_adv_stats(H, None)
    yield "rex_rollout_gather/not_enabled", lambda: L.rex_rollout_gather(Z, ro(), P, 0, P, P, P, P, P, P, None)
    yield "rex_rollout_gather/n_-1", lambda: L.rex_rollout_gather(H, ro(), P, -1, P, P, P, P, P, P, None)
    yield "rex_rollout_gather/n_1_null_index", lambda: L.rex_rollout_gather(H, ro(), None, 1, P, P, P, P, P, P, None)
    yield "rex_rollout_gather/n0_ok", lambda: L.rex_rollout_gather(H, ro(), None, 0, P, P, P, P, P, P, None)
    yield "rex_rollout_read_bad_indices/not_enabled", lambda: L.rex_rollout_read_bad_indices(Z, i64x4, 0)
    yield "rex_rollout_read_bad_indices/null_out", lambda: L.rex_rollout_read_bad_indices(H, None, 0)

    # ---- vecnorm
    bad_cfg = c.N.RexNormConfig(-1.0, 1e-8, 10.0, 10.0, 1, 1, 1)
    nan_cfg = c.N.RexNormConfig(0.99, NAN, 10.0, 10.0, 1, 1, 1)
    zero_clip = c.N.RexNormConfig(0.99, 1e-8, 0.0, 10.0, 1, 1, 1)
    for name, cfg in (("gamma_-1", bad_cfg), ("epsilon_nan", nan_cfg), ("clip_obs_0", zero_clip)):
        yield "rex_norm_enable/" + name, lambda cfg=cfg: L.rex_norm_enable(Z, ctypes.byref(cfg))   # refused before anything is allocated: Z stays without the layer
    step = lambda h, **kw: L.rex_norm_step(h, *[kw.get(k, P) for k in ("obs_in", "reward_in", "done", "term_in", "obs_out", "reward_out", "term_out",   # noqa: E731
                                                                      "ep_return", "ep_len")], None)
    yield "rex_norm_set_training/null_handle", lambda: L.rex_norm_set_training(None, 1)
    yield "rex_norm_set_training/not_enabled", lambda: L.rex_norm_set_training(Z, 1)
    yield "rex_norm_reset/not_enabled", lambda: L.rex_norm_reset(Z, None, P, P, None)
    yield "rex_norm_reset/obs_in_alone", lambda: L.rex_norm_reset(Nh, None, P, None, None)
    yield "rex_norm_reset/obs_out_alone", lambda: L.rex_norm_reset(Nh, None, None, P, None)
    yield "rex_norm_step/not_enabled", lambda: step(Z)
    yield "rex_norm_step/null_reward_in", lambda: step(Nh, reward_in=None)
    yield "rex_norm_step/null_done", lambda: step(Nh, done=None)
    yield "rex_norm_step/obs_in_alone", lambda: step(Nh, obs_out=None)
    yield "rex_norm_step/term_in_alone", lambda: step(Nh, term_out=None)
    yield "rex_norm_step/term_without_obs", lambda: step(Nh, obs_in=None, obs_out=None)
    yield "rex_norm_step/null_done+obs_in_alone", lambda: step(Nh, done=None, obs_out=None)
    yield "rex_norm_get_stats/not_enabled", lambda: L.rex_norm_get_stats(Z, dbl)
    yield "rex_norm_get_stats/null_out", lambda: L.rex_norm_get_stats(Nh, None)
    yield "rex_norm_set_stats/not_enabled", lambda: L.rex_norm_set_stats(Z, dbl)
    yield "rex_norm_set_stats/null_in", lambda: L.rex_norm_set_stats(Nh, None)
    yield "rex_norm_set_stats/count_0", lambda: L.rex_norm_set_stats(Nh, dbl)
    for fn in ("rex_norm_get_lane_state", "rex_norm_set_lane_state"):
        yield fn + "/not_enabled", lambda fn=fn: getattr(L, fn)(Z, P, P, P, None)
        for k in range(3):
            yield fn + "/null_%d" % k, lambda fn=fn, k=k: getattr(L, fn)(Nh, *[None if j == k else P for j in range(3)], None)
    yield "rex_norm_read_episodes/not_enabled", lambda: L.rex_norm_read_episodes(Z, dbl, 0)
    yield "rex_norm_read_episodes/null_out", lambda: L.rex_norm_read_episodes(Nh, None, 0)

    # ---- episode ledger (never enabled here: its enable launches)
    for how in (None, "null_ptr", 0, -3):
        yield "rex_eplog_enable/buf_%s" % how, lambda how=how: L.rex_eplog_enable(Z, c.desc(EL, how, "capacity"))
    yield "rex_eplog_step/not_enabled", lambda: L.rex_eplog_step(Z, P, P, P, None)
    yield "rex_eplog_sync/not_enabled", lambda: L.rex_eplog_sync(Z, None, 0, None)
    yield "rex_eplog_read/not_enabled", lambda: L.rex_eplog_read(Z, i64x4, 0)
    yield "rex_eplog_get_lane_state/not_enabled", lambda: L.rex_eplog_get_lane_state(Z, P, P, P, None)
    yield "rex_eplog_set_lane_state/not_enabled", lambda: L.rex_eplog_set_lane_state(Z, P, P, P, None)

    # ---- replay buffer: add and the counter
    def radd(h, d, t=0, src=(P,) * 5):
        obs, action, reward, done, next_obs = src
        return L.rex_rbuf_add(h, d, t, obs, action, reward, done, next_obs, None, None, None)
    yield "rex_rbuf_add/not_enabled", lambda: radd(Z, rb())
    for how in (None, "null_ptr", 0):
        yield "rex_rbuf_add/buf_%s" % how, lambda how=how: radd(H, rb(how))
    yield "rex_rbuf_add/slot_-1", lambda: radd(H, rb(), t=-1)
    yield "rex_rbuf_add/slot_T", lambda: radd(H, rb(), t=T)
    for k in range(5):
        yield "rex_rbuf_add/null_input_%d" % k, lambda k=k: radd(H, rb(), src=tuple(None if j == k else P for j in range(5)))
    yield "rex_rbuf_add/buf_0+slot_T", lambda: radd(H, rb(0), t=T)
    yield "rex_rbuf_read_bad_indices/not_enabled", lambda: L.rex_rbuf_read_bad_indices(Z, i64x4, 0)
    yield "rex_rbuf_read_bad_indices/null_out", lambda: L.rex_rbuf_read_bad_indices(H, None, 0)

    # ---- prioritised replay
    yield "rex_per_tree_len/N_0", lambda: L.rex_per_tree_len(0)
    yield "rex_per_tree_len/N_2^30+1", lambda: L.rex_per_tree_len((1 << 30) + 1)
    calls = {"rex_per_init": lambda h, d: L.rex_per_init(h, d, None), "rex_per_add": lambda h, d: L.rex_per_add(h, d, 0, None),
             "rex_per_update": lambda h, d: L.rex_per_update(h, d, P, P, 0, None), "rex_per_rebuild": lambda h, d: L.rex_per_rebuild(h, d, None),
             "rex_per_draw": lambda h, d: L.rex_per_draw(h, d, 0, 1, 0, P, P, None)}
    for fn, call in calls.items():
        yield fn + "/not_enabled", lambda call=call: call(Z, pb())
        for how in (None, "null_ptr", 0, 1 << 30):
            yield fn + "/buf_%s" % how, lambda call=call, how=how: call(H, pb(how))
    yield "rex_per_add/slot_-1", lambda: L.rex_per_add(H, pb(), -1, None)
    yield "rex_per_add/slot_T", lambda: L.rex_per_add(H, pb(), T, None)
    yield "rex_per_update/n_-1", lambda: L.rex_per_update(H, pb(), P, P, -1, None)
    yield "rex_per_update/n_1_null_index", lambda: L.rex_per_update(H, pb(), None, P, 1, None)
    yield "rex_per_update/n_1_null_priority", lambda: L.rex_per_update(H, pb(), P, None, 1, None)
    yield "rex_per_update/n0_ok", lambda: L.rex_per_update(H, pb(), None, None, 0, None)
    yield "rex_per_draw/n_-1", lambda: L.rex_per_draw(H, pb(), -1, 1, 0, P, P, None)
    yield "rex_per_draw/n_1_null_index_out", lambda: L.rex_per_draw(H, pb(), 1, 1, 0, None, P, None)
    yield "rex_per_draw/n_1_null_prob_out", lambda: L.rex_per_draw(H, pb(), 1, 1, 0, P, None, None)
    yield "rex_per_draw/n0_ok", lambda: L.rex_per_draw(H, pb(), 0, 1, 0, None, None, None)
    yield "rex_per_read_counters/not_enabled", lambda: L.rex_per_read_counters(Z, i64x4, 0)
    yield "rex_per_read_counters/null_out", lambda: L.rex_per_read_counters(H, None, 0)

    # ---- row-major calls
    def srows(h, **kw):
        return L.rex_step_rows(h, *[kw.get(k, P) for k in ("action", "obs", "reward", "done", "trunc", "term")], None)
    yield "rex_reset_rows/null_handle", lambda: L.rex_reset_rows(None, None, P, None)
    yield "rex_reset_rows/null_obs_rows", lambda: L.rex_reset_rows(H, None, None, None)
    yield "rex_reset_rows/cartpole_misaligned", lambda: L.rex_reset_rows(C, None, P + 4, None)
    yield "rex_reset_rows/cartpole_null_obs_rows", lambda: L.rex_reset_rows(C, None, None, None)
    yield "rex_step_rows/null_handle", lambda: srows(None)
    for k in ("action", "obs", "reward", "done"):
        yield "rex_step_rows/null_%s" % k, lambda k=k: srows(H, **{k: None})
    yield "rex_step_rows/cartpole_misaligned_obs", lambda: srows(C, obs=P + 4)
    yield "rex_step_rows/cartpole_misaligned_term", lambda: srows(C, term=P + 8)
    yield "rex_step_rows/cartpole_null_done+misaligned_obs", lambda: srows(C, done=None, obs=P + 4)

    # ---- the env calls
    yield "rex_step/null_handle", lambda: L.rex_step(None, P, P, P, P, None, None, None)
    for k in range(4):
        yield "rex_step/null_%d" % k, lambda k=k: L.rex_step(H, *[None if j == k else P for j in range(4)], None, None, None)
    yield "rex_replay/cartpole", lambda: L.rex_replay(C, *(P,) * 7, None)
    for k in range(7):
        yield "rex_replay/null_%d" % k, lambda k=k: L.rex_replay(H, *[None if j == k else P for j in range(7)], None)
    yield "rex_replay/cartpole+null", lambda: L.rex_replay(C, None, *(P,) * 6, None)
    yield "rex_reset/null_handle", lambda: L.rex_reset(None, None, P, None)
    yield "rex_set_random_task/no_dr", lambda: L.rex_set_random_task(H, None, None)
    yield "rex_sample_task/null_out", lambda: L.rex_sample_task(H, None, 0, None)
    yield "rex_sample_task/no_dr", lambda: L.rex_sample_task(H, P, 0, None)
    fp = ctypes.POINTER(ctypes.c_float)
    yield "rex_set_dr/n_params", lambda: L.rex_set_dr(Z, 1, ctypes.cast(flt, fp), 3, None)
    yield "rex_set_dr/null_params", lambda: L.rex_set_dr(Z, 2, None, 8, None)
    yield "rex_set_dr/fullgaussian_n_params", lambda: L.rex_set_dr(Z, 4, ctypes.cast(flt, fp), 8, None)
    yield "rex_set_dr/unknown_type", lambda: L.rex_set_dr(Z, 9, ctypes.cast(flt, fp), 8, None)
    yield "rex_set_dr/null_handle", lambda: L.rex_set_dr(None, 0, None, 0, None)
    for fn in ("rex_get_state", "rex_set_state"):
        yield fn + "/null_qpos", lambda fn=fn: getattr(L, fn)(H, None, P, None)
        yield fn + "/null_qvel", lambda fn=fn: getattr(L, fn)(H, P, None, None)
    for fn in ("rex_get_task", "rex_set_task", "rex_get_obs"):
        yield fn + "/null", lambda fn=fn: getattr(L, fn)(H, None, None)
        yield fn + "/null_handle", lambda fn=fn: getattr(L, fn)(None, P, None)
    yield "rex_get_counters/null_out", lambda: L.rex_get_counters(H, None)
    for fn in ("rex_get_counters_state", "rex_set_counters_state"):
        for k in range(3):
            yield fn + "/null_%d" % k, lambda fn=fn, k=k: getattr(L, fn)(H, *[None if j == k else P for j in range(3)], None)
    for fn in ("rex_get_aux", "rex_set_aux"):
        yield fn + "/null", lambda fn=fn: getattr(L, fn)(H, None, None)
        yield fn + "/hopper_has_none", lambda fn=fn: getattr(L, fn)(H, P, None)
    yield "rex_set_info_buffer/cartpole", lambda: L.rex_set_info_buffer(C, P)
    yield "rex_set_info_buffer/null_handle", lambda: L.rex_set_info_buffer(None, P)
    f = ctypes.cast(flt, fp)
    yield "rex_export_lane/null_qpos", lambda: L.rex_export_lane(H, 0, None, f, f)
    yield "rex_export_lane/null_xi", lambda: L.rex_export_lane(H, 0, f, f, None)
    yield "rex_export_lane/lane_-1", lambda: L.rex_export_lane(H, -1, f, f, f)
    yield "rex_export_lane/lane_B", lambda: L.rex_export_lane(H, B, f, f, f)
    yield "rex_export_lane/null+lane_B", lambda: L.rex_export_lane(H, B, None, f, f)
    yield "rex_get_launch_shape/null_out", lambda: L.rex_get_launch_shape(H, None)
    yield "rex_set_launch_shape/null_shape", lambda: L.rex_set_launch_shape(H, None)
    yield "rex_read_timing/null_out", lambda: L.rex_read_timing(H, None, 4)
    yield "rex_enable_timing/null_handle", lambda: L.rex_enable_timing(None, 1)


def cases(c):
    """(name, call) in a fixed order; a call returns the entry point's return code"""
    yield from _sample_cases(c)
    yield from _layer_cases(c)


def run(c):
    """-> [{"name", "rc", "error"}] in the order of cases(); error is "" for REX_OK"""
    out = []
    for name, call in cases(c):
        rc = int(call())
        out.append({"name": name, "rc": rc, "error": c.L.rex_last_error().decode() if rc else ""})
    return out


def main():
    import __graft_entry__ as g
    g.build()
    c = Ctx()
    try:
        got = run(c)
    finally:
        c.close()
    names = [r["name"] for r in got]
    assert len(set(names)) == len(names)
    with open(PATH, "w") as f:
        json.dump(got, f, indent=0)
        f.write("\n")
    print(PATH, len(got), "cases,", sum(1 for r in got if r["rc"] == 0), "of them REX_OK")


if __name__ == "__main__":
    main()
