#!/usr/bin/env python3
"""Measurements of the history stack: writes profiles/hist_times.json.

Workloads: hopper 32 768 envs with K = 50 and humanoid 4 096 envs with K = 16, frames with action, uniform DR of +-10 %, dr_training and
auto-reset on (the training configuration), settled for 300 steps; then 16 consecutive steps are recorded (observation, action, done,
terminal observation: the env's natural done rate) and every candidate replays those 16 inputs in turn.  Candidates, in ONE process with the
profiler off, alternated inside every repetition:
  push_no_done     HistoryStack.push_buffers with a done buffer of zeros
  push_natural     ... with the recorded done flags and terminal observations (terminal_window written)
  materialize      HistoryStack.materialize into a preallocated tensor
  torch_pingpong   the same semantics in torch on preallocated ping-pong buffers [B, K, W]: one fused where() that shifts by one row and zeroes the
                   done lanes, the frame write (two transposing copies, the action masked), the length update.  It does NOT produce the
                   terminal window, which is to its advantage.
  step             env.step_soa, the step kernel of the same run
Per repetition and candidate: a device-event pair around LAUNCHES consecutive calls, divided by LAUNCHES; REPS repetitions, so REPS * LAUNCHES
(>= 1000) timed launches per figure; median [min - max] over the repetitions is the figure and its spread.  A call whose kernel is shorter than
the host's enqueue is timed at the enqueue rate: the figures are what a loop pays per call, not kernel durations.  Before timing, the torch
spelling and the stack are run side by side on the recorded inputs and must agree bit for bit.

    python3 profiles/hist_probe.py [--out profiles/hist_times.json]

A measurement path that finds no GPU fails: nothing is estimated."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOADS = {"hopper": ("RandomHopper-v0", 32768, 50), "humanoid": ("RandomHumanoid-v0", 4096, 16)}
LAUNCHES, REPS, WARM, SNAPSHOTS = 100, 12, 30, 16


class TorchStack:
    """what a user writes today: preallocated ping-pong shift + zero of the done lanes, frame write, length update"""

    def __init__(self, torch, B, K, D, A, device):
        self.t, self.K, self.D = torch, K, D
        self.buf = [torch.zeros(B, K, D + A, device=device), torch.zeros(B, K, D + A, device=device)]
        self.length = torch.zeros(B, dtype=torch.int32, device=device)
        self.zero = torch.zeros((), device=device)
        self.cur = 0

    def push(self, obs_soa, act_soa, done):
        t, src, dst = self.t, self.buf[self.cur], self.buf[1 - self.cur]
        d = done.bool()
        t.where(d[:, None, None], self.zero, src[:, 1:], out=dst[:, :-1])          # shift by one row, the done lanes cleared
        dst[:, -1, :self.D].copy_(obs_soa.t())
        t.where(d[:, None], self.zero, act_soa.t(), out=dst[:, -1, self.D:])
        self.length.masked_fill_(d, 0).add_(1).clamp_(max=self.K)
        self.cur = 1 - self.cur

    def window(self):
        return self.buf[self.cur]


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
    import random_envs_amd as rex
    if not torch.cuda.is_available():
        raise SystemExit("hist_probe: no GPU")
    env_id, B, K = WORKLOADS[kind]
    env = rex.make(env_id, batch=B, seed=0)
    nom = np.array(env.original_task)
    env.set_dr_distribution("uniform", np.stack([0.9 * nom, 1.1 * nom], 1).ravel().tolist())
    env.set_dr_training(True)
    env.reset()
    D, A = int(env.dims.obs_dim), int(env.dims.act_dim)
    g = torch.Generator().manual_seed(0)
    amp = float(env.dims.act_high)
    acts = [((torch.rand(A, B, generator=g) * 2 - 1) * amp).cuda().contiguous() for _ in range(SNAPSHOTS)]
    for k in range(300):
        env.step_soa(acts[k % SNAPSHOTS])
    snaps = []
    for k in range(SNAPSHOTS):
        obs, _, done, _, term = env.step_soa_full(acts[k])
        snaps.append((obs.clone(), acts[k], done.clone(), term.clone()))
    no_done = torch.zeros(B, dtype=torch.uint8, device=env.device)
    hist = rex.HistoryStack(env, K)
    ref = TorchStack(torch, B, K, D, A, env.device)
    out = torch.empty(B, K, D + A, device=env.device)
    # the two spellings agree bit for bit on the recorded inputs (2 K + 3 pushes: the ring wraps twice)
    for k in range(2 * K + 3):
        o, a, d, tm = snaps[k % SNAPSHOTS]
        hist.push_buffers(o, a, d, tm)
        ref.push(o, a, d)
    same = bool(torch.equal(hist.window().contiguous().view(torch.int32), ref.window().view(torch.int32))) and bool(torch.equal(hist.length, ref.length))
    same = same and bool(torch.equal(hist.materialize(out).view(torch.int32), ref.window().view(torch.int32)))
    if not same:
        raise SystemExit("hist_probe: the torch spelling and the stack differ on %s" % kind)
    done_rate = float(torch.stack([s[2].float().mean() for s in snaps]).mean())

    def push_no_done(k):
        o, a, _, _ = snaps[k % SNAPSHOTS]
        hist.push_buffers(o, a, no_done)

    def push_natural(k):
        o, a, d, tm = snaps[k % SNAPSHOTS]
        hist.push_buffers(o, a, d, tm)

    def torch_pingpong(k):
        o, a, d, _ = snaps[k % SNAPSHOTS]
        ref.push(o, a, d)

    fns = (("push_no_done", push_no_done), ("push_natural", push_natural), ("materialize", lambda k: hist.materialize(out)),
           ("torch_pingpong", torch_pingpong), ("step", lambda k: env.step_soa(acts[k % SNAPSHOTS])))
    runs = {name: [] for name, _ in fns}
    for name, fn in fns:
        for k in range(WARM):
            fn(k)
    torch.cuda.synchronize()
    for rep in range(REPS):
        for name, fn in fns:
            timed(torch, fn, runs[name])
    W = D + A
    rec = {"env": env_id, "batch": B, "K": K, "W": W, "done_rate_per_step": done_rate, "launches_per_figure": LAUNCHES * REPS, "bit_identical_to_torch": same,
           "us_per_call": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for k, v in runs.items()},
           "bytes_per_step": {"push_written": 2 * W * 4 * B, "push_read": W * 4 * B, "shift_read_and_written": (2 * K - 1) * W * 4 * B}}
    us = rec["us_per_call"]
    rec["torch_over_push_natural"] = us["torch_pingpong"]["median"] / us["push_natural"]["median"]
    rec["torch_over_push_no_done"] = us["torch_pingpong"]["median"] / us["push_no_done"]["median"]
    rec["push_natural_over_step"] = us["push_natural"]["median"] / us["step"]["median"]
    rec["byte_ratio_written_shift_over_push"] = (2 * K - 1) / 2.0
    rec["push_beats_torch_by_more_than_the_spread"] = us["push_natural"]["max"] < us["torch_pingpong"]["min"] and us["push_no_done"]["max"] < us["torch_pingpong"]["min"]
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_times.json"))
    args = ap.parse_args()
    out = {"method": __doc__.split("\n\n")[1]}
    for kind in ("hopper", "humanoid"):
        out[kind] = measure(kind)
        json.dump(out, open(args.out, "w"), indent=1)
        print("[probe] %s: %s" % (kind, json.dumps({k: v for k, v in out[kind].items() if k != "us_per_call"})), flush=True)
        print("[probe] %s: %s" % (kind, json.dumps({k: [round(v[s], 2) for s in ("median", "min", "max")] for k, v in out[kind]["us_per_call"].items()})), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
