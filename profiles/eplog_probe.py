#!/usr/bin/env python3
"""Measurements of the episode ledger: writes profiles/eplog_times.json.

Workloads: hopper 32 768 envs and humanoid 4 096 envs, uniform DR of +-10 %, dr_training and auto-reset on (the training
configuration), settled for 300 steps.  Per workload:
  (a) GPU time per call of the two rex_eplog_step launches and of the step kernel of the SAME run, from a
      ``rocprofv3 --kernel-trace --stats`` child process of its own (nothing else traced) that runs step_soa + record().  The
      step kernel is matched by name and reported as its AverageNs (the 300 settling launches of the same kernel are in the
      trace as well, so its total is not divided by the loop's call count); the ledger kernels run in the loop only;
  (b) the same for the eager spelling of the ledger -- get_task() + accumulate + done.nonzero() + index_select -- whose nonzero()
      forces one host synchronisation per step (its result's shape is data-dependent): summed time, per loop iteration, of
      every kernel the loop launches at least once per iteration that is not one of the library's own (step, reset, derive,
      forward: those belong to the step and to the settling phase);
  (c) env-steps/s of step_soa alone, step_soa + record() and step_soa + the eager spelling in ONE process with the profiler off
      (bench.py's method: 16 pre-generated action tensors, a host clock around `steps` launches that ends in a device
      synchronise), alternating the three, several repetitions: median [min - max].

    python3 profiles/eplog_probe.py                 # everything (needs a GPU and rocprofv3), writes the JSON
    python3 profiles/eplog_probe.py payload ...     # what a child process runs

A measurement that could not be taken is recorded as null with the reason: nothing is estimated."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOADS = {"hopper": ("RandomHopper-v0", 32768), "humanoid": ("RandomHumanoid-v0", 4096)}
LEDGER_KERNELS = ("el_count_kernel", "el_append_kernel")
STEP_KERNELS = ("step_kernel",)                                # planar_step_kernel<...>, humanoid_pair_step_kernel, ...
OWN_KERNELS = ("step_kernel", "reset_kernel", "derive_kernel", "forward_kernel", "fill_rows_kernel", "el_sync_kernel")   # the library's, not the eager spelling's
TRACE_ITERS, TRACE_WARM = 300, 30


def setup(kind):
    import numpy as np
    import torch
    import random_envs_amd as rex
    env_id, batch = WORKLOADS[kind]
    env = rex.make(env_id, batch=batch, seed=0)
    nom = np.array(env.original_task)
    env.set_dr_distribution("uniform", np.stack([0.9 * nom, 1.1 * nom], 1).ravel().tolist())
    env.set_dr_training(True)
    env.reset()
    g = torch.Generator().manual_seed(0)
    amp = float(env.dims.act_high)
    acts = [((torch.rand(env.dims.act_dim, batch, generator=g) * 2 - 1) * amp).cuda().contiguous() for _ in range(16)]
    for k in range(300):                                       # settle: the batch reaches its steady mix of episode phases
        env.step_soa(acts[k % 16])
    log = rex.EpisodeLog(env, 1 << 23)                           # room for every episode of the throughput run: no record is dropped
    torch.cuda.synchronize()
    return torch, env, acts, log


class Eager:
    """what a user of step_soa writes today to pair finished episodes with their task"""

    def __init__(self, torch, env):
        self.t, self.env = torch, env
        self.ret = torch.zeros(env.batch, dtype=torch.float64, device=env.device)
        self.len = torch.zeros(env.batch, dtype=torch.int32, device=env.device)
        self.task = env.get_task()
        self.rows = 0

    def before(self):
        self.task = self.env.get_task()                         # the task the step is about to run under (task_dim copy launches)

    def after(self, reward, done):
        self.ret += reward
        self.len += 1
        idx = done.nonzero().squeeze(1)                         # data-dependent shape: the host waits for the device here
        if idx.numel():
            rec = (self.task.index_select(0, idx), self.ret.index_select(0, idx), self.len.index_select(0, idx))
            self.rows += rec[1].numel()
            self.ret.index_fill_(0, idx, 0.0); self.len.index_fill_(0, idx, 0)


def payload(args):
    torch, env, acts, log = setup(args.kind)
    B = env.batch
    eager = Eager(torch, env)

    def alone(k):
        env.step_soa(acts[k % 16])

    def with_record(k):
        env.step_soa(acts[k % 16])
        log.record(truncated=False)

    def with_eager(k):
        eager.before()
        _, reward, done = env.step_soa(acts[k % 16])
        eager.after(reward, done)

    if args.op == "throughput":
        fns = (("step_soa", alone), ("step_soa+record", with_record), ("step_soa+eager", with_eager))
        res = {name: [] for name, _ in fns}
        for rep in range(args.reps):
            for name, fn in fns:
                for k in range(50):
                    fn(k)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(args.steps):
                    fn(k)
                torch.cuda.synchronize()
                res[name].append(B * args.steps / (time.perf_counter() - t0))
        c = log.read()
        print("RESULT " + json.dumps({"runs": res, "ledger": c, "eager_rows": eager.rows}))
        return
    fn = with_record if args.impl == "hip" else with_eager
    for k in range(TRACE_WARM + TRACE_ITERS):
        fn(k)
    torch.cuda.synchronize()
    print("RESULT " + json.dumps({"calls": TRACE_WARM + TRACE_ITERS, "ledger": log.read(), "eager_rows": eager.rows}))


def kernels_from_trace(trace_dir, calls):
    """per-kernel rows of rocprofv3's kernel_stats.csv for the kernels launched at least once per call"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None, "no kernel_stats.csv under %s" % trace_dir
    rows = []
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            n = int(row["Calls"])
            if n >= calls:
                rows.append({"name": row["Name"][:96], "calls": n, "avg_us": float(row["AverageNs"]) / 1e3, "us_per_call": float(row["TotalDurationNs"]) / 1e3 / calls})
    return rows, None


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
    ap.add_argument("--op", default="trace", choices=["trace", "throughput"])
    ap.add_argument("--impl", default="hip", choices=["hip", "eager"])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eplog_times.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "scratch", "eplog_trace"))
    args = ap.parse_args()
    if args.mode == "payload":
        return payload(args)
    me = os.path.abspath(__file__)
    out = {"workloads": {k: {"env": v[0], "batch": v[1]} for k, v in WORKLOADS.items()}, "method": __doc__.split("\n\n")[1]}

    def save():
        json.dump(out, open(args.out, "w"), indent=1)

    for kind in ("hopper", "humanoid"):
        rec = out[kind] = {}
        for impl in ("hip", "eager"):
            d = os.path.join(args.trace_dir, "%s_%s" % (kind, impl))
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me, "payload", "--kind", kind,
                   "--op", "trace", "--impl", impl]
            rc, res, tail = child(cmd, 420)
            print("[probe] %s trace %s: exit %d %s" % (kind, impl, rc, res), flush=True)
            if rc != 0:                                        # a failed GPU process: record it and start nothing more
                rec["trace_" + impl] = {"error": "exit %d" % rc, "tail": tail}
                save(); print(tail)
                return 1
            calls = TRACE_WARM + TRACE_ITERS
            rows, why = kernels_from_trace(d, calls)
            line = {"kernels": rows, "trace_missing": why, "payload": res}
            if rows:
                named = lambda r, names: any(k in r["name"] for k in names)
                step = [r for r in rows if named(r, STEP_KERNELS)]
                line["step_kernel_us"] = sum(r["avg_us"] for r in step) if step else None       # AverageNs: the settling launches are in Calls too
                line["step_kernel_names"] = [r["name"] for r in step]
                if impl == "hip":
                    mine = [r for r in rows if named(r, LEDGER_KERNELS)]
                    line["ledger_us_per_call"] = sum(r["us_per_call"] for r in mine)
                    line["ledger_launches_per_call"] = sum(r["calls"] for r in mine) / calls
                else:
                    rest = [r for r in rows if not named(r, OWN_KERNELS)]
                    line["eager_us_per_call"] = sum(r["us_per_call"] for r in rest)
                    line["eager_launches_per_call"] = sum(r["calls"] for r in rest) / calls
                    line["host_synchronisations_per_step"] = 1
            rec["trace_" + impl] = line
            save()
        rc, res, tail = child([sys.executable, me, "payload", "--kind", kind, "--op", "throughput", "--steps", str(args.steps), "--reps", str(args.reps)], 420)
        print("[probe] %s throughput: exit %d" % (kind, rc), flush=True)
        if rc != 0:
            rec["throughput"] = {"error": "exit %d" % rc, "tail": tail}
            save(); print(tail)
            return 1
        tp = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for k, v in res["runs"].items()}
        base = tp["step_soa"]["median"]
        for k in tp:
            tp[k]["relative_to_step_soa"] = tp[k]["median"] / base
        rec["throughput_env_steps_per_s"] = tp
        rec["throughput_payload"] = {k: res[k] for k in ("ledger", "eager_rows")}
        save()
    print(json.dumps(out, indent=1)[-6000:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
