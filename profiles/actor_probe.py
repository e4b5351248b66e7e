#!/usr/bin/env python3
"""Measurements of the on-device actor: writes profiles/actor_times.json.

Workloads: hopper, half-cheetah and humanoid at 32 768 envs, make(id, row_major=True), uniform DR of +-10 %, dr_training and auto-reset on,
settled for 200 steps under the policy; the policy is stable-baselines3's default MlpPolicy shape: two separate tanh towers of 64 - 64, a
state-independent log_std.  Candidates, in ONE process with the profiler off, alternated inside every repetition:
  device_act     DeviceActor.act(obs): one launch
  torch_act      the same network in eager torch on preallocated outputs: six addmm(out=), four tanh_(), exp(log_std), normal_(), addcmul for
                 the action, and the Normal log-prob as mul / sum / mul_ / sub_ with the constant kept on the device
  step           env.step(action) on 16 preallocated actions in turn, U(-1, 1) x the actuator range as in bench.py (open loop: one FIXED
                 action drives the humanoid into a regime four times as expensive as the loop's and says nothing about it)
  loop_device    act -> step with DeviceActor (the action tensor is read by the step kernel by pointer)
  loop_torch     act -> step with the torch spelling
Per repetition and candidate: a device-event pair around LAUNCHES consecutive calls, divided by LAUNCHES; REPS repetitions, so REPS * LAUNCHES
(>= 1000) timed calls per figure; median [min - max] over the repetitions is the figure and its spread.  A call whose kernels are shorter
than the host's enqueue is timed at the enqueue rate: the figures are what a loop pays per call, not kernel durations.  Before timing, both
actors' mean and value must lie within the fp64 oracle's bound (tests/actor_oracle.py) on the settled observations.

    python3 profiles/actor_probe.py [--out profiles/actor_times.json] [--kinds hopper,halfcheetah,humanoid]

A measurement path that finds no GPU fails: nothing is estimated."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WORKLOADS = {"hopper": "RandomHopper-v0", "halfcheetah": "RandomHalfCheetah-v0", "humanoid": "RandomHumanoid-v0"}
BATCH, WIDTHS = 32768, (64, 64)
LAUNCHES, REPS, WARM = 100, 10, 20


class TorchActor:
    """what a user writes today, with every output preallocated"""

    def __init__(self, torch, pi, vf, log_std, B, A, device):
        self.t, self.pi, self.vf, self.log_std = torch, pi, vf, log_std
        z = lambda *s: torch.zeros(*s, device=device)
        self.hp, self.hv = [z(B, W.shape[0]) for W, _ in pi[:-1]], [z(B, W.shape[0]) for W, _ in vf[:-1]]
        self.mean, self.value, self.eps, self.action, self.sq, self.logp = z(B, A), z(B, 1), z(B, A), z(B, A), z(B, A), z(B)
        self.std, self.c = z(A), z(())
        self.half_log_2pi = A * 0.9189385332046727

    def _tower(self, layers, bufs, head_out, x):
        t = self.t
        for (W, b), buf in zip(layers[:-1], bufs):
            t.addmm(b, x, W.t(), out=buf)
            buf.tanh_()
            x = buf
        W, b = layers[-1]
        t.addmm(b, x, W.t(), out=head_out)

    def forward(self, obs):
        self._tower(self.pi, self.hp, self.mean, obs)
        self._tower(self.vf, self.hv, self.value, obs)

    def act(self, obs):
        t = self.t
        self.forward(obs)
        t.exp(self.log_std, out=self.std)
        self.eps.normal_()
        t.addcmul(self.mean, self.eps, self.std, out=self.action)
        t.mul(self.eps, self.eps, out=self.sq)
        t.sum(self.sq, 1, out=self.logp)
        t.sum(self.log_std, 0, out=self.c)
        self.logp.mul_(-0.5).sub_(self.c).sub_(self.half_log_2pi)
        return self.action, self.logp, self.value


def timed(torch, fn, reps_out):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(LAUNCHES):
        fn(k)
    e1.record()
    e1.synchronize()
    reps_out.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)                           # us per call


def measure(kind):
    import numpy as np
    import torch
    import actor_oracle as oracle
    import random_envs_amd as rex
    if not torch.cuda.is_available():
        raise SystemExit("actor_probe: no GPU")
    env = rex.make(WORKLOADS[kind], batch=BATCH, seed=0, row_major=True)
    nom = np.array(env.original_task)
    env.set_dr_distribution("uniform", np.stack([0.9 * nom, 1.1 * nom], 1).ravel().tolist())
    env.set_dr_training(True)
    obs = env.reset()
    D, A, dev = int(env.dims.obs_dim), int(env.dims.act_dim), env.device
    rng = np.random.default_rng(0)
    pi_np, vf_np = oracle.make_tower(rng, D, WIDTHS, A, 0.5), oracle.make_tower(rng, D, WIDTHS, 1, 0.5)
    up = lambda layers: [(torch.as_tensor(W).to(dev), torch.as_tensor(b).to(dev)) for W, b in layers]
    pi, vf = up(pi_np), up(vf_np)
    log_std = torch.full((A,), -1.0, device=dev)
    actor = rex.DeviceActor(env, pi=pi, vf=vf, log_std=log_std, seed=0)
    ref = TorchActor(torch, pi, vf, log_std, BATCH, A, dev)
    for _ in range(200):
        obs, _, _, _ = env.step(actor.act(obs)[0])
    settled = obs.clone()
    # both actors against the fp64 oracle's bound on the settled observations
    x = settled.cpu().numpy()
    finite = np.isfinite(x).all(1)
    want = {"mean": oracle.tower(pi_np, x[finite], "tanh"), "value": oracle.tower(vf_np, x[finite], "tanh")}
    mean, _, value = actor.act(settled, deterministic=True)
    ref.forward(settled)
    got = {"device": {"mean": mean.cpu().numpy()[finite], "value": value.cpu().numpy()[finite, None]},
           "torch": {"mean": ref.mean.cpu().numpy()[finite], "value": ref.value.cpu().numpy()[finite]}}
    agreement = {}
    for who, outs in got.items():
        for k, arr in outs.items():
            val, bound = want[k]
            err = np.abs(arr.astype(np.float64) - val)
            agreement["%s_%s" % (who, k)] = {"max_abs_error": float(err.max()), "worst_share_of_bound": float((err / bound).max())}
            if not (err <= bound).all():
                raise SystemExit("actor_probe: %s %s leaves the oracle's bound on %s" % (who, k, kind))
    gen = torch.Generator().manual_seed(0)
    amp = float(env.dims.act_high)
    acts = [((torch.rand(BATCH, A, generator=gen) * 2 - 1) * amp).to(dev).contiguous() for _ in range(16)]
    state = {"obs": settled}

    def loop_device(k):
        state["obs"] = env.step(actor.act(state["obs"])[0])[0]

    def loop_torch(k):
        state["obs"] = env.step(ref.act(state["obs"])[0])[0]

    fns = (("device_act", lambda k: actor.act(settled)), ("torch_act", lambda k: ref.act(settled)), ("step", lambda k: env.step(acts[k % 16])),
           ("loop_device", loop_device), ("loop_torch", loop_torch))
    runs = {name: [] for name, _ in fns}
    for name, fn in fns:
        for k in range(WARM):
            fn(k)
    torch.cuda.synchronize()
    for rep in range(REPS):
        for name, fn in fns:
            timed(torch, fn, runs[name])
    us = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for k, v in runs.items()}
    fma = 2 * (D * WIDTHS[0] + WIDTHS[0] * WIDTHS[1]) + WIDTHS[1] * (A + 1)
    rec = {"env": WORKLOADS[kind], "batch": BATCH, "in_dim": D, "act_dim": A, "widths": list(WIDTHS), "finite_rows_checked": int(finite.sum()),
           "calls_per_figure": LAUNCHES * REPS, "agreement_with_fp64_oracle": agreement, "fma_per_env": fma, "us_per_call": us,
           "torch_over_device_act": us["torch_act"]["median"] / us["device_act"]["median"],
           "device_act_over_step": us["device_act"]["median"] / us["step"]["median"],
           "loop_torch_over_loop_device": us["loop_torch"]["median"] / us["loop_device"]["median"],
           "device_act_beats_torch_by_more_than_the_spread": us["device_act"]["max"] < us["torch_act"]["min"],
           "device_act_gflops_at_median": 2.0 * fma * BATCH / us["device_act"]["median"] * 1e-3}
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_times.json"))
    ap.add_argument("--kinds", default="hopper,halfcheetah,humanoid")
    args = ap.parse_args()
    out = {"method": __doc__.split("\n\n")[1]}
    for kind in args.kinds.split(","):
        out[kind] = measure(kind)
        json.dump(out, open(args.out, "w"), indent=1)
        print("[probe] %s: %s" % (kind, json.dumps({k: v for k, v in out[kind].items() if k != "us_per_call"})), flush=True)
        print("[probe] %s: %s" % (kind, json.dumps({k: [round(v[s], 2) for s in ("median", "min", "max")] for k, v in out[kind]["us_per_call"].items()})), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
