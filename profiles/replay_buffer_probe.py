#!/usr/bin/env python3
"""Measurements of the device-side replay buffer (replay buffer section): writes profiles/replay_buffer_times.json.

Workloads: hopper 32 768 envs x T = 64 slots and humanoid 32 768 envs x T = 8 slots, minibatches of 4 096.  For each of add, sample and
sample with normalisation:
  (a) the stream time per call (HIP events around a loop of launches after a warm-up, profiler off, one child process per workload) of the
      rex_rbuf_* launch and of a torch restatement of the same work in the same process -- SoA storage [dim][T][B]; add: six copies and a
      where() that puts the terminal observations into next_obs; sample: randint, index_select of every field, the dones arithmetic, the
      transposing .contiguous() of the row fields, and for the normalised line the VecNormalize arithmetic in fp32 -- and their ratio;
  (b) the GPU time per call of the rb_* kernels from ``rocprofv3 --kernel-trace --stats``, in profiled child processes of their own
      (nothing else traced).

    python3 profiles/replay_buffer_probe.py                 # everything (needs a GPU and rocprofv3), writes the JSON
    python3 profiles/replay_buffer_probe.py payload ...     # what a child process runs

A measurement that could not be taken is recorded as null with the reason: nothing is estimated.  A failed child process ends the run."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOADS = {"hopper": ("RandomHopper-v0", 32768, 64), "humanoid": ("RandomHumanoid-v0", 32768, 8)}
OPS = ("add", "sample", "sample_norm")
KERNELS = {"add": "rb_add_kernel", "sample": "rb_sample_kernel", "sample_norm": "rb_sample_kernel"}
ITERS, WARM = 2000, 100
MINIBATCH = 4096


def setup(kind):
    import torch
    import random_envs_amd as rex
    env_id, batch, T = WORKLOADS[kind]
    env = rex.make(env_id, batch=batch, seed=0)
    w = rex.NormalizedVecRandomEnv(env)
    w.reset()
    g = torch.Generator().manual_seed(0)
    amp = float(env.dims.act_high)
    acts = [((torch.rand(env.dims.act_dim, batch, generator=g) * 2 - 1) * amp).cuda().contiguous() for _ in range(4)]
    for a in acts:                                             # the statistics leave their initial values
        w.step_soa(a)
    w.set_training(False)
    buf = rex.ReplayBuffer(w, T)
    obs, reward, done, trunc, term = env.step_soa_full(acts[0])
    prev = obs.clone()
    for t in range(T):
        buf.add(prev, acts[0], reward, done, obs, term, trunc)
    torch.cuda.synchronize()
    return torch, env, w, acts, buf, (prev, acts[0], reward, done, obs, term, trunc)


def torch_restatement(torch, env, w, T):
    """the same buffer out of torch calls over SoA storage: what a user of step_soa writes today"""
    B, D, A, dev = env.batch, env.dims.obs_dim, env.dims.act_dim, env.device
    f32 = dict(dtype=torch.float32, device=dev)
    s = dict(obs=torch.zeros(D, T, B, **f32), next_obs=torch.zeros(D, T, B, **f32), action=torch.zeros(A, T, B, **f32), reward=torch.zeros(T, B, **f32),
             done=torch.zeros(T, B, dtype=torch.uint8, device=dev), timeout=torch.zeros(T, B, dtype=torch.uint8, device=dev))
    st = w.stats()
    mean = torch.as_tensor(st["mean"][:D], **f32)
    std = torch.as_tensor((st["var"][:D] + w.epsilon) ** 0.5, **f32)
    ret_std = float((st["var"][D] + w.epsilon) ** 0.5)

    def add(t, obs, act, reward, done, next_obs, term, trunc):
        s["obs"][:, t].copy_(obs); s["action"][:, t].copy_(act); s["reward"][t].copy_(reward); s["done"][t].copy_(done); s["timeout"][t].copy_(trunc)
        s["next_obs"][:, t].copy_(torch.where(done.bool(), term, next_obs))

    def sample(n, size, normalise):
        idx = torch.randint(0, size * B, (n,), device=dev)
        obs = s["obs"].view(D, T * B).index_select(1, idx).t().contiguous()
        nxt = s["next_obs"].view(D, T * B).index_select(1, idx).t().contiguous()
        act = s["action"].view(A, T * B).index_select(1, idx).t().contiguous()
        rew = s["reward"].view(-1).index_select(0, idx)
        done = s["done"].view(-1).index_select(0, idx).float() * (1.0 - s["timeout"].view(-1).index_select(0, idx).float())
        if normalise:
            obs = torch.clamp((obs - mean) / std, -w.clip_obs, w.clip_obs)
            nxt = torch.clamp((nxt - mean) / std, -w.clip_obs, w.clip_obs)
            rew = torch.clamp(rew / ret_std, -w.clip_reward, w.clip_reward)
        return obs, nxt, act, rew, done, idx

    return add, sample


def payload(args):
    torch, env, w, acts, buf, step = setup(args.kind)
    T = buf.n_slots
    e_add, e_sample = torch_restatement(torch, env, w, T)

    def fns(hip):
        def add(k):
            if hip:
                buf.pos = k % T
                buf.add(*step)
            else:
                e_add(k % T, *step)
        return {"add": add,
                "sample": (lambda k: buf.sample(MINIBATCH, normalize=False)) if hip else (lambda k: e_sample(MINIBATCH, T, False)),
                "sample_norm": (lambda k: buf.sample(MINIBATCH, normalize=True)) if hip else (lambda k: e_sample(MINIBATCH, T, True))}

    def stream_us(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for k in range(WARM):
            fn(k)
        torch.cuda.synchronize()
        ev0.record()
        for k in range(ITERS):
            fn(k)
        ev1.record()
        torch.cuda.synchronize()
        return 1e3 * ev0.elapsed_time(ev1) / ITERS

    if args.op == "stream":                                    # profiler off: every line, both spellings, alternating, three repetitions
        res = {op: {"hip": [], "torch": []} for op in OPS}
        for rep in range(3):
            for op in OPS:
                for impl in ("hip", "torch"):
                    res[op][impl].append(stream_us(fns(impl == "hip")[op]))
        print("RESULT " + json.dumps(res))
        return
    for op in args.op.split(","):                              # under the profiler: the rex_rbuf_* launches only
        stream_us(fns(True)[op])
    print("RESULT " + json.dumps({"calls": ITERS + WARM}))


def kernel_time_from_trace(trace_dir, name):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None, "no kernel_stats.csv under %s" % trace_dir
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            if name in row["Name"]:
                return {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                        "max_us": float(row["MaxNs"]) / 1e3}, None
    return None, "no %s in %s" % (name, files[0])


def child(cmd, timeout):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    res = None
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            res = json.loads(line[7:])
    return p.returncode, res, (p.stdout + p.stderr)[-2000:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="run", choices=["run", "payload"])
    ap.add_argument("--kind", default="hopper", choices=sorted(WORKLOADS))
    ap.add_argument("--op", default="stream")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_buffer_times.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "scratch", "replay_buffer_trace"))
    args = ap.parse_args()
    if args.mode == "payload":
        return payload(args)
    me = os.path.abspath(__file__)
    out = {"workloads": {k: {"batch": v[1], "T": v[2]} for k, v in WORKLOADS.items()}, "minibatch": MINIBATCH, "iterations": ITERS, "warm_up": WARM,
           "method": __doc__.split("\n\n")[1]}
    for kind in WORKLOADS:
        rec = {}
        rc, res, tail = child(["timeout", "-k", "10", "300", sys.executable, me, "payload", "--kind", kind, "--op", "stream"], 330)
        print("[probe] %s stream times: exit %d %s" % (kind, rc, res), flush=True)
        if rc != 0 or not res:                                 # a failed GPU process: record it and start nothing more
            out[kind] = {"error": "exit %d" % rc, "tail": tail}
            json.dump(out, open(args.out, "w"), indent=1)
            print(tail)
            return 1
        for op in OPS:
            hip, tor = sorted(res[op]["hip"])[1], sorted(res[op]["torch"])[1]
            rec[op] = {"stream_us_per_call": {"hip": hip, "torch": tor, "torch_to_hip": tor / hip, "runs": res[op]}}
        for ops in ("add,sample", "sample_norm"):
            d = os.path.join(args.trace_dir, "%s_%s" % (kind, ops.replace(",", "_")))
            cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me,
                   "payload", "--kind", kind, "--op", ops]
            rc, _, tail = child(cmd, 330)
            print("[probe] %s trace of %s: exit %d" % (kind, ops, rc), flush=True)
            if rc != 0:
                rec["trace_error"] = {"ops": ops, "error": "exit %d" % rc, "tail": tail}
                out[kind] = rec
                json.dump(out, open(args.out, "w"), indent=1)
                print(tail)
                return 1
            for op in ops.split(","):
                kt, why = kernel_time_from_trace(d, KERNELS[op])
                rec[op]["kernel_us"], rec[op]["kernel_missing"] = kt, why
        out[kind] = rec
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out, indent=1)[-6000:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
