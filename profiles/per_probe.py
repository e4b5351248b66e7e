#!/usr/bin/env python3
"""Measurements of the device-side prioritised replay (prioritised replay paragraph): writes profiles/per_times.json.

Workload: hopper 32 768 envs x T = 64 slots (N = 2 097 152 priorities, a tree of depth 4), minibatches of 4 096, priorities away from
uniform.  For each of add (the priority part of a step: rex_per_add), draw (rex_per_draw) and update (rex_per_update of 4 096 ids):
  (a) the stream time per call (HIP events around a loop of calls after a warm-up, profiler off, one child process) of the rex_per_*
      call and of the torch spelling a user writes today, in the same process -- priorities as a float32 tensor; add: a slice copy of
      the running maximum; draw: cumsum in fp64 over all N, stratified uniforms, searchsorted, the probabilities by indexing; update:
      index_put_ and the running maximum -- and their ratio;
  (b) the GPU time per call of every per_* kernel from ``rocprofv3 --kernel-trace --stats``, in a profiled child process of its own
      (nothing else traced).

    python3 profiles/per_probe.py                 # everything (needs a GPU and rocprofv3), writes the JSON
    python3 profiles/per_probe.py payload ...     # what a child process runs

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
ENV_ID, BATCH, SLOTS = "RandomHopper-v0", 32768, 64
OPS = ("add", "draw", "update")
KERNELS = ("per_fill_kernel", "per_clear_kernel", "per_scatter_kernel", "per_refresh_kernel", "per_top_kernel", "per_draw_kernel")
ITERS, WARM = 1000, 100
MINIBATCH = 4096


def setup():
    import ctypes
    import torch
    import random_envs_amd as rex
    env = rex.make(ENV_ID, batch=BATCH, seed=0)
    buf = rex.PrioritizedReplayBuffer(env, SLOTS)
    L, h, per = env._L, env._h, buf._per
    for t in range(SLOTS):                                     # the priority part alone: the rows play no part in what is measured
        assert L.rex_per_add(h, ctypes.byref(per), t, env._stream()) == 0
    g = torch.Generator().manual_seed(0)
    ids = [torch.randint(0, SLOTS * BATCH, (MINIBATCH,), generator=g).cuda() for _ in range(8)]
    vals = [(10.0 ** (torch.rand(MINIBATCH, generator=g) * 3 - 2)).cuda() for _ in range(8)]
    every = torch.randperm(SLOTS * BATCH, generator=g).cuda()
    spread = (10.0 ** (torch.rand(SLOTS * BATCH, generator=g) * 3 - 2)).cuda()
    for k in range(0, SLOTS * BATCH, 1 << 18):                 # priorities away from uniform
        i, v = every[k:k + (1 << 18)].contiguous(), spread[k:k + (1 << 18)].contiguous()
        assert L.rex_per_update(h, ctypes.byref(per), i.data_ptr(), v.data_ptr(), i.numel(), env._stream()) == 0
    torch.cuda.synchronize()
    return ctypes, torch, env, buf, ids, vals


def torch_spelling(torch, buf):
    """the same three steps out of torch calls: what a user writes today"""
    N, B, dev = buf.n_slots * buf.batch, buf.batch, buf.device
    prio = buf.priority.reshape(-1).clone()
    maxp = buf.max_priority.clone()
    strata = torch.arange(MINIBATCH, device=dev, dtype=torch.float64)

    def add(t):
        prio[t * B:(t + 1) * B].copy_(maxp.expand(B))

    def draw():
        c = torch.cumsum(prio.double(), 0)
        x = (strata + torch.rand(MINIBATCH, device=dev, dtype=torch.float64)) * (c[-1] / MINIBATCH)
        idx = torch.searchsorted(c, x).clamp_(max=N - 1)
        return idx, (prio[idx].double() / c[-1]).float()

    def update(idx, p):
        prio.index_put_((idx,), p)
        torch.maximum(maxp, p.max().reshape(1), out=maxp)

    return add, draw, update


def payload(args):
    ctypes, torch, env, buf, ids, vals = setup()
    L, h, per = env._L, env._h, buf._per
    e_add, e_draw, e_update = torch_spelling(torch, buf)
    idx_out = torch.empty(MINIBATCH, dtype=torch.int64, device=env.device)
    prob_out = torch.empty(MINIBATCH, dtype=torch.float32, device=env.device)

    def fns(hip):
        if hip:
            return {"add": lambda k: L.rex_per_add(h, ctypes.byref(per), k % SLOTS, env._stream()),
                    "draw": lambda k: L.rex_per_draw(h, ctypes.byref(per), MINIBATCH, 7, k, idx_out.data_ptr(), prob_out.data_ptr(), env._stream()),
                    "update": lambda k: L.rex_per_update(h, ctypes.byref(per), ids[k % 8].data_ptr(), vals[k % 8].data_ptr(), MINIBATCH, env._stream())}
        return {"add": lambda k: e_add(k % SLOTS), "draw": lambda k: e_draw(), "update": lambda k: e_update(ids[k % 8], vals[k % 8])}

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
    for op in OPS:                                             # under the profiler: the rex_per_* launches only
        stream_us(fns(True)[op])
    print("RESULT " + json.dumps({"calls": ITERS + WARM}))


def kernel_times_from_trace(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None, "no kernel_stats.csv under %s" % trace_dir
    out = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            for name in KERNELS:
                if name in row["Name"]:
                    out[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                                 "max_us": float(row["MaxNs"]) / 1e3}
    missing = [k for k in KERNELS if k not in out]
    return out, ("no %s in %s" % (missing, files[0]) if missing else None)


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
    ap.add_argument("--op", default="stream", choices=["stream", "trace"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_times.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "scratch", "per_trace"))
    args = ap.parse_args()
    if args.mode == "payload":
        return payload(args)
    me = os.path.abspath(__file__)
    out = {"workload": {"env": ENV_ID, "batch": BATCH, "T": SLOTS}, "minibatch": MINIBATCH, "iterations": ITERS, "warm_up": WARM,
           "method": __doc__.split("\n\n")[1]}
    rc, res, tail = child(["timeout", "-k", "10", "240", sys.executable, me, "payload", "--op", "stream"], 270)
    print("[probe] stream times: exit %d %s" % (rc, res), flush=True)
    if rc != 0 or not res:                                     # a failed GPU process: record it and start nothing more
        out["error"] = {"step": "stream", "exit": rc, "tail": tail}
        json.dump(out, open(args.out, "w"), indent=1)
        print(tail)
        return 1
    for op in OPS:
        hip, tor = sorted(res[op]["hip"])[1], sorted(res[op]["torch"])[1]
        out[op] = {"stream_us_per_call": {"hip": hip, "torch": tor, "torch_to_hip": tor / hip, "runs": res[op]}}
    json.dump(out, open(args.out, "w"), indent=1)
    cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.trace_dir, "--", sys.executable, me,
           "payload", "--op", "trace"]
    rc, _, tail = child(cmd, 270)
    print("[probe] trace: exit %d" % rc, flush=True)
    if rc != 0:
        out["error"] = {"step": "trace", "exit": rc, "tail": tail}
        json.dump(out, open(args.out, "w"), indent=1)
        print(tail)
        return 1
    out["kernel_us"], out["kernel_missing"] = kernel_times_from_trace(args.trace_dir)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out, indent=1)[-6000:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
