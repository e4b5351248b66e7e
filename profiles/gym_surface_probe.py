#!/usr/bin/env python3
"""Measurements of the gym surface ("Gym surface"): writes profiles/gym_surface_times.json.

Per configuration one child process runs three legs alternated A B C three times, each leg a 100-step warm-up and 2 000 steps under a
host clock that ends in a device synchronise, on settled envs of one seed with 16 device-resident pre-generated [B, act_dim] float32
actions (CartPole: int32 [B], the dtype both layouts take without a conversion):
  A  step() of the default mode (the transposing copy of the action, two .bool() kernels, transposed views out);
  B  step() of a row_major=True env (rex_step_rows on the caller's tensors);
  C  step_soa on pre-transposed [act_dim, B] actions (the path bench.py measures).
The humanoid adds A' = A followed by obs.contiguous(): the transposition A leaves to its consumer and B has already done.
A second set of children runs a few hundred steps of legs A and B under ``rocprofv3 --kernel-trace --stats`` (nothing else traced) and
counts the kernels per step() call by name.

    python3 profiles/gym_surface_probe.py                 # everything (needs a GPU; the launch counts need rocprofv3)
    python3 profiles/gym_surface_probe.py payload ...     # what a child runs

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
CONFIGS = {"hopper": ("RandomHopper-v0", 32768), "C3": ("RandomHalfCheetahNoisy-v0", 16384), "C5": ("RandomHumanoid-v0", 32768),
           "cartpole": ("RandomCartPole-v0", 32768)}           # C3, C5: the BASELINE configurations of bench.py --config
EXPECTED_B_LAUNCHES = {"hopper": 1, "C3": 1, "C5": 3, "cartpole": 2}
STEPS, WARM, REPS, SETTLE = 2000, 100, 3, 200


def setup(config, want):
    """settled envs of the legs in `want` (A and C share the default-mode env) and the pre-generated actions in both layouts"""
    import torch
    import random_envs_amd as rex
    eid, B = CONFIGS[config]
    envs = {}
    if "A" in want or "C" in want:
        envs["soa"] = rex.make(eid, batch=B, seed=0)
    if "B" in want:
        envs["rows"] = rex.make(eid, batch=B, seed=0, row_major=True)
    dims = next(iter(envs.values())).dims
    g = torch.Generator().manual_seed(0)
    if dims.discrete_action:
        rows = [torch.randint(0, 2, (B,), generator=g, dtype=torch.int32).cuda() for _ in range(16)]
        soa = rows
    else:
        rows = [((torch.rand(B, dims.act_dim, generator=g) * 2 - 1) * float(dims.act_high)).cuda().contiguous() for _ in range(16)]
        soa = [a.t().contiguous() for a in rows]
    for env in envs.values():
        env.reset()
        for k in range(SETTLE):
            env.step(rows[k % 16])
    torch.cuda.synchronize()
    legs = {}
    if "A" in want:
        legs["A"] = lambda k: envs["soa"].step(rows[k % 16])
        if config == "C5":
            legs["A_contiguous"] = lambda k: envs["soa"].step(rows[k % 16])[0].contiguous()
    if "B" in want:
        legs["B"] = lambda k: envs["rows"].step(rows[k % 16])
    if "C" in want:
        legs["C"] = lambda k: envs["soa"].step_soa(soa[k % 16])
    return torch, envs, legs


def payload(args):
    if args.leg:                                               # the profiled child: one leg, a few hundred calls, nothing else
        torch, envs, legs = setup(args.config, args.leg)
        torch.cuda.synchronize()
        for k in range(args.steps):
            legs[args.leg](k)
        torch.cuda.synchronize()
        print("RESULT " + json.dumps({"calls": args.steps, "settle_calls": SETTLE}))
        return
    torch, envs, legs = setup(args.config, "ABC")
    res = {name: [] for name in legs}
    for rep in range(REPS):
        for name, fn in legs.items():
            for k in range(WARM):
                fn(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                fn(k)
            torch.cuda.synchronize()
            res[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    for env in envs.values():
        c = env.counters()
        assert c["nonfinite"] == 0, c
    print("RESULT " + json.dumps(res))


def launches_from_trace(trace_dir, calls):
    """kernels per step() call from rocprofv3's kernel_stats.csv: the kernels launched at least once per call (settle + measured calls;
    set-up launches number far fewer), by name, in whole launches per call (`launches` keeps the total: the one reset() of the set-up and
    the rare fill kernel of a torch op add a handful to `calls` times the figure)"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None, "no kernel_stats.csv under %s" % trace_dir
    kernels = []
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            n = int(row["Calls"])
            if n >= calls:
                kernels.append({"name": row["Name"][:100], "per_call": n // calls, "launches": n, "avg_us": float(row["AverageNs"]) / 1e3,
                                "torch": "at::native" in row["Name"] or "at::cuda" in row["Name"]})
    return {"calls": calls, "kernels_per_call": sum(k["per_call"] for k in kernels), "torch_kernels_per_call": sum(k["per_call"] for k in kernels if k["torch"]),
            "kernels": kernels}, None


def child(cmd, timeout):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    res = None
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            res = json.loads(line[7:])
    return p.returncode, res, (p.stdout + p.stderr)[-2000:]


def summarise(runs):
    return {"mean": statistics.mean(runs), "spread": max(runs) - min(runs), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="run", choices=["run", "payload"])
    ap.add_argument("--config", default="hopper", choices=sorted(CONFIGS))
    ap.add_argument("--leg", default=None, choices=["A", "B"])
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--trace-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gym_surface_times.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "scratch", "gym_surface_trace"))
    args = ap.parse_args()
    if args.mode == "payload":
        return payload(args)
    me = os.path.abspath(__file__)
    out = {"unit": "ms per step() call", "steps": args.steps, "warmup": WARM, "alternations": REPS, "method": __doc__.split("\n\n")[1]}

    def fail(rec, key, rc, tail):                               # a failed GPU process: record it and start nothing more
        rec[key] = {"error": "exit %d" % rc, "tail": tail}
        json.dump(out, open(args.out, "w"), indent=1)
        print(tail)
        return 1

    for config in CONFIGS:
        eid, B = CONFIGS[config]
        rec = out[config] = {"env_id": eid, "batch": B}
        rc, res, tail = child([sys.executable, me, "payload", "--config", config, "--steps", str(args.steps)], 600)
        print("[probe] %s legs: exit %d %s" % (config, rc, res), flush=True)
        if rc != 0 or not res:
            return fail(rec, "legs", rc, tail)
        legs = rec["legs_ms_per_step"] = {k: summarise(v) for k, v in res.items()}
        a, b, c = legs["A"], legs["B"], legs["C"]
        rec["B_below_A_by_more_than_A_spread"] = b["mean"] < a["mean"] - a["spread"]
        rec["A_minus_B_ms"] = a["mean"] - b["mean"]
        rec["C_over_B"] = c["mean"] / b["mean"]                # B's throughput as a fraction of step_soa's
        rec["C_over_A"] = c["mean"] / a["mean"]
        if "A_contiguous" in legs:
            ac = legs["A_contiguous"]
            rec["B_not_slower_than_A_contiguous_beyond_spread"] = b["mean"] <= ac["mean"] + max(ac["spread"], b["spread"])
        json.dump(out, open(args.out, "w"), indent=1)
        rec["launches"] = {}
        for leg in ("A", "B"):
            d = os.path.join(args.trace_dir, "%s_%s" % (config, leg))
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me, "payload", "--config", config,
                   "--leg", leg, "--steps", str(args.trace_steps)]
            rc, res, tail = child(cmd, 420)
            print("[probe] %s leg %s trace: exit %d %s" % (config, leg, rc, res), flush=True)
            if rc != 0 or not res:
                return fail(rec["launches"], leg, rc, tail)
            kt, why = launches_from_trace(d, res["calls"] + res["settle_calls"])
            rec["launches"][leg] = kt if kt else {"missing": why}
        lb = rec["launches"]["B"]
        if "kernels_per_call" in lb:
            rec["launches"]["B_as_required"] = lb["kernels_per_call"] == EXPECTED_B_LAUNCHES[config] and lb["torch_kernels_per_call"] == 0
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
