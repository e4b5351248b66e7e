#!/usr/bin/env python3
"""Measurements of the automatic-domain-randomisation layer: writes profiles/adr_times.json.

Workloads: hopper 32 768 envs and humanoid 4 096 envs, dr_training off and auto-reset on (the configuration the layer runs in),
settled for 300 steps; AutoDR over every task index, zero-width start, buffer_size 240, p_boundary 0.5.  Per workload:
  (a) GPU time per call of the three rex_adr_record launches and of the step kernel of the SAME run, from a
      ``rocprofv3 --kernel-trace --stats`` child process of its own (nothing else traced) that runs step_soa + record().  The
      step kernel is matched by name and reported as its AverageNs (the 300 settling launches of the same kernel are in the
      trace as well); the layer's kernels run in the loop only;
  (b) env-steps/s of step_soa alone, step_soa + record() and step_soa + an eager torch spelling of the same semantics --
      accumulate, done.nonzero(), index_add_ into the tallies, the box move on the host, torch.rand tasks, set_task -- in ONE
      process with the profiler off (bench.py's method: 16 pre-generated action tensors, a host clock around `steps` launches
      that ends in a device synchronise), alternating the three, several repetitions: median [min - max].

    python3 profiles/adr_probe.py                 # everything (needs a GPU and rocprofv3), writes the JSON
    python3 profiles/adr_probe.py payload ...     # what a child process runs

A measurement that could not be taken is recorded as null with the reason: nothing is estimated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eplog_probe import child, kernels_from_trace  # noqa: E402  (the same trace reader and child runner)

WORKLOADS = {"hopper": ("RandomHopper-v0", 32768), "humanoid": ("RandomHumanoid-v0", 4096)}
THRESHOLDS = {"hopper": (100.0, 300.0), "humanoid": (100.0, 300.0)}      # mean-return thresholds: the moves cost the same whichever way they go
ADR_KERNELS = ("adr_tally_kernel", "adr_fold_kernel", "adr_assign_kernel")
STEP_KERNELS = ("step_kernel",)
BUFFER, P_B = 240, 0.5
TRACE_ITERS, TRACE_WARM = 300, 30


def setup(kind):
    import numpy as np
    import torch
    import random_envs_amd as rex
    env_id, batch = WORKLOADS[kind]
    env = rex.make(env_id, batch=batch, seed=0)
    env.reset()
    g = torch.Generator().manual_seed(0)
    amp = float(env.dims.act_high)
    acts = [((torch.rand(env.dims.act_dim, batch, generator=g) * 2 - 1) * amp).cuda().contiguous() for _ in range(16)]
    for k in range(300):                                       # settle: the batch reaches its steady mix of episode phases
        env.step_soa(acts[k % 16])
    centre = np.asarray(env.original_task, np.float32)
    adr = rex.AutoDR(env, THRESHOLDS[kind][0], THRESHOLDS[kind][1], 0.05 * centre, p_boundary=P_B, buffer_size=BUFFER, seed=0)
    adr.assign()
    torch.cuda.synchronize()
    return torch, np, env, acts, adr


class Eager:
    """what a user of step_soa writes today for the same semantics: one host synchronisation per step (nonzero), tallies by
    index_add_, the box on the host, a full set_task"""

    def __init__(self, torch, np, env, kind):
        self.t, self.np, self.env = torch, np, env
        B, d, dev = env.batch, env.task_dim, env.device
        self.d, self.J = d, 2 * d
        self.ret = torch.zeros(B, dtype=torch.float64, device=dev)
        self.bnd = torch.full((B,), -1, dtype=torch.int64, device=dev)
        self.n = torch.zeros(self.J, dtype=torch.int64, device=dev)
        self.s = torch.zeros(self.J, dtype=torch.float64, device=dev)
        self.centre = np.asarray(env.original_task, np.float64)
        self.lim_lo, self.lim_hi = env.get_task_search_bounds()
        self.lo, self.hi = self.centre.copy(), self.centre.copy()
        self.delta = 0.05 * self.centre
        self.t_lo, self.t_hi = THRESHOLDS[kind]
        self.task = env.get_task().clone()
        self.moves = 0

    def after(self, reward, done):
        t, np_ = self.t, self.np
        self.ret += reward
        idx = done.nonzero().squeeze(1)                         # data-dependent shape: the host waits for the device here
        if not idx.numel():
            return
        b = self.bnd.index_select(0, idx)
        on = b >= 0
        self.n.index_add_(0, b[on], t.ones_like(b[on]))
        self.s.index_add_(0, b[on], self.ret.index_select(0, idx)[on])
        n, s = self.n.cpu().numpy(), self.s.cpu().numpy()
        for a in np_.flatnonzero(n >= BUFFER):
            k, mean = a >> 1, s[a] / n[a]
            if mean >= self.t_hi:
                self.hi[k], self.lo[k] = (min(self.lim_hi[k], self.hi[k] + self.delta[k]), self.lo[k]) if a & 1 else (self.hi[k], max(self.lim_lo[k], self.lo[k] - self.delta[k]))
            elif mean <= self.t_lo:
                self.hi[k], self.lo[k] = (max(self.centre[k], self.hi[k] - self.delta[k]), self.lo[k]) if a & 1 else (self.hi[k], min(self.centre[k], self.lo[k] + self.delta[k]))
            self.n[a] = 0; self.s[a] = 0.0
            self.moves += 1
        m, dev = idx.numel(), self.env.device
        lo, hi = t.as_tensor(self.lo, dtype=t.float32, device=dev), t.as_tensor(self.hi, dtype=t.float32, device=dev)
        xi = lo + (hi - lo) * t.rand(m, self.d, device=dev)
        pinned = t.rand(m, device=dev) < P_B
        a = t.randint(0, self.J, (m,), device=dev)
        k = a >> 1
        edge = t.where((a & 1).bool(), hi[k], lo[k])
        xi[pinned, k[pinned]] = edge[pinned]
        self.task[idx] = xi
        self.bnd[idx] = t.where(pinned, a, t.full_like(a, -1))
        self.ret.index_fill_(0, idx, 0.0)
        self.env.set_task(self.task)


def payload(args):
    torch, np, env, acts, adr = setup(args.kind)
    B = env.batch
    eager = Eager(torch, np, env, args.kind)

    def alone(k):
        env.step_soa(acts[k % 16])

    def with_record(k):
        env.step_soa(acts[k % 16])
        adr.record()

    def with_eager(k):
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
        st = adr.state()
        print("RESULT " + json.dumps({"runs": res, "evaluations": int(st["counters"].sum()), "eager_moves": eager.moves}))
        return
    for k in range(TRACE_WARM + TRACE_ITERS):
        with_record(k)
    torch.cuda.synchronize()
    print("RESULT " + json.dumps({"calls": TRACE_WARM + TRACE_ITERS, "evaluations": int(adr.state()["counters"].sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="run", choices=["run", "payload"])
    ap.add_argument("--kind", default="hopper", choices=sorted(WORKLOADS))
    ap.add_argument("--op", default="trace", choices=["trace", "throughput"])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adr_times.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "scratch", "adr_trace"))
    args = ap.parse_args()
    if args.mode == "payload":
        return payload(args)
    me = os.path.abspath(__file__)
    out = {"workloads": {k: {"env": v[0], "batch": v[1]} for k, v in WORKLOADS.items()}, "method": __doc__.split("\n\n")[1],
           "settings": {"buffer_size": BUFFER, "p_boundary": P_B, "thresholds": THRESHOLDS, "delta": "0.05 * nominal task"}}

    def save():
        json.dump(out, open(args.out, "w"), indent=1)

    for kind in ("hopper", "humanoid"):
        rec = out[kind] = {}
        d = os.path.join(args.trace_dir, kind)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me, "payload", "--kind", kind, "--op", "trace"]
        rc, res, tail = child(cmd, 300)
        print("[probe] %s trace: exit %d %s" % (kind, rc, res), flush=True)
        if rc != 0:                                            # a failed GPU process: record it and start nothing more
            rec["trace"] = {"error": "exit %d" % rc, "tail": tail}
            save(); print(tail)
            return 1
        calls = TRACE_WARM + TRACE_ITERS
        rows, why = kernels_from_trace(d, calls)
        line = {"kernels": rows, "trace_missing": why, "payload": res}
        if rows:
            named = lambda r, names: any(k in r["name"] for k in names)
            step = [r for r in rows if named(r, STEP_KERNELS)]
            line["step_kernel_us"] = sum(r["avg_us"] for r in step) if step else None
            mine = [r for r in rows if named(r, ADR_KERNELS)]
            line["record_us_by_kernel"] = {k: sum(r["us_per_call"] for r in mine if k in r["name"]) for k in ADR_KERNELS}
            line["record_us_per_call"] = sum(r["us_per_call"] for r in mine)
            line["record_launches_per_call"] = sum(r["calls"] for r in mine) / calls
        rec["trace"] = line
        save()
        rc, res, tail = child([sys.executable, me, "payload", "--kind", kind, "--op", "throughput", "--steps", str(args.steps), "--reps", str(args.reps)], 300)
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
        rec["throughput_payload"] = {k: res[k] for k in ("evaluations", "eager_moves")}
        save()
    print(json.dumps(out, indent=1)[-5000:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
