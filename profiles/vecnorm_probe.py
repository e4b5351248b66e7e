#!/usr/bin/env python3
"""Measurements of the device-side normalisation: writes profiles/vecnorm_times.json.

For hopper and humanoid at 32 768 envs:
  (a) GPU time per step of the two rex_norm_step launches against the summed kernel time of the torch-eager spelling of the
      same update on the same buffers, both from ``rocprofv3 --kernel-trace --stats`` (one profiled child process per
      measurement, nothing else traced);
  (b) achieved bytes/s of the two launches against the algorithmic traffic (two reads and one write of the observation block,
      plus the reward / done / per-lane rows) and its share of the HBM peak;
  (c) env-steps/s of step_soa + normalise against step_soa alone (bench.py's method: a settled env, 16 pre-generated action
      tensors, a host clock around `steps` launches that ends in a device synchronise), alternating the two, several repetitions.

    python3 profiles/vecnorm_probe.py                 # everything (needs a GPU and rocprofv3), writes the JSON
    python3 profiles/vecnorm_probe.py payload ...     # what a profiled child runs

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
ENVS = {"hopper": "RandomHopper-v0", "humanoid": "RandomHumanoid-v0"}
BATCH = 32768
HBM_PEAK = 8.0e12          # bytes/s, MI355X
ITERS, WARM = 300, 30


def setup(kind, batch=BATCH):
    import torch
    import random_envs_amd as rex
    env = rex.make(ENVS[kind], batch=batch, seed=0)
    env.reset()
    g = torch.Generator().manual_seed(0)
    amp = float(env.dims.act_high)
    acts = [((torch.rand(env.dims.act_dim, batch, generator=g) * 2 - 1) * amp).cuda().contiguous() for _ in range(16)]
    return torch, rex, env, acts


class EagerNorm:
    """The update of rex_norm_step spelled in torch eager ops on the same SoA buffers: what a user of the plain env writes."""

    def __init__(self, torch, env, dtype):
        self.t, self.dt = torch, dtype
        D, B, dev = env.dims.obs_dim, env.batch, env.device
        z = lambda *s, **k: torch.zeros(*s, device=dev, **k)
        self.count = torch.full((D + 1,), 1e-4, device=dev, dtype=dtype); self.mean = z(D + 1, dtype=dtype); self.var = torch.ones(D + 1, device=dev, dtype=dtype)
        self.ret = z(B, dtype=dtype); self.ep_return = z(B, dtype=dtype); self.ep_len = z(B, dtype=torch.int32)
        self.ep_return_out = z(B, dtype=dtype); self.ep_len_out = z(B, dtype=torch.int32)
        self.agg = z(3, dtype=torch.float64)
        self.D = D

    def _merge(self, sl, x, dim):
        t = self.t
        bv, bm = t.var_mean(x, dim=dim, unbiased=False)
        bc = x.shape[dim]
        delta = bm - self.mean[sl]
        tot = self.count[sl] + bc
        m2 = self.var[sl] * self.count[sl] + bv * bc + delta * delta * self.count[sl] * bc / tot
        self.mean[sl] = self.mean[sl] + delta * bc / tot
        self.var[sl] = m2 / tot
        self.count[sl] = tot

    def step(self, obs, reward, done, term_obs):
        t, D = self.t, self.D
        d = done.bool()
        x = obs.to(self.dt)
        self._merge(slice(0, D), x, 1)
        r = reward.to(self.dt)
        self.ret = self.ret * 0.99 + r
        self._merge(slice(D, D + 1), self.ret.unsqueeze(0), 1)
        inv = t.rsqrt(self.var[:D] + 1e-8).unsqueeze(1)
        mean = self.mean[:D].unsqueeze(1)
        nobs = ((x - mean) * inv).clamp(-10.0, 10.0).float()
        nrew = (r * t.rsqrt(self.var[D] + 1e-8)).clamp(-10.0, 10.0).float()
        nterm = t.where(d, ((term_obs.to(self.dt) - mean) * inv).clamp(-10.0, 10.0).float(), term_obs)
        self.ret = t.where(d, t.zeros_like(self.ret), self.ret)
        self.ep_return = self.ep_return + r
        self.ep_len = self.ep_len + 1
        self.ep_return_out = t.where(d, self.ep_return, self.ep_return_out)
        self.ep_len_out = t.where(d, self.ep_len, self.ep_len_out)
        self.agg += t.stack([d.sum().double(), (self.ep_return * d).sum().double(), (self.ep_len * d).sum().double()])
        self.ep_return = t.where(d, t.zeros_like(self.ep_return), self.ep_return)
        self.ep_len = t.where(d, t.zeros_like(self.ep_len), self.ep_len)
        return nobs, nrew, nterm


def payload(args):
    """norm-only loops on buffers a short rollout left behind (for the profiler), or the throughput comparison"""
    torch, rex, env, acts = setup(args.kind)
    if args.impl == "throughput":
        w = rex.NormalizedVecRandomEnv(env)
        w.reset()
        for k in range(300):                                   # settle: the batch reaches its steady mix of episode phases
            w.step_soa(acts[k % 16])
        torch.cuda.synchronize()
        res = {"alone": [], "with_norm": []}
        for rep in range(args.reps):
            for name, fn in (("alone", env.step_soa), ("with_norm", w.step_soa)):
                for k in range(50):
                    fn(acts[k % 16])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(args.steps):
                    fn(acts[k % 16])
                torch.cuda.synchronize()
                res[name].append(env.batch * args.steps / (time.perf_counter() - t0))
        print("RESULT " + json.dumps(res))
        return
    for k in range(40):
        env.step(acts[k % 16].t())                             # step(): terminal observations are written too
    torch.cuda.synchronize()
    if args.impl == "hip":
        w = rex.NormalizedVecRandomEnv(env)
        fn = lambda: w._norm_step(True)
    else:
        e = EagerNorm(torch, env, torch.float64 if args.impl == "eager64" else torch.float32)
        fn = lambda: e.step(env._obs, env._reward, env._done, env._term_obs)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(ITERS):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    print("RESULT " + json.dumps({"stream_us_per_step": 1e3 * ev0.elapsed_time(ev1) / ITERS, "iters": ITERS + WARM}))


def kernel_time_from_trace(trace_dir, impl, iters):
    """us per step from rocprofv3's kernel_stats.csv: the two vn_* kernels (hip), or every kernel the loop launched (eager: the kernels
    called at least once per iteration; the set-up launches number far fewer)"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None, "no kernel_stats.csv under %s" % trace_dir
    total, kernels, launches = 0.0, [], 0
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            calls = int(row["Calls"])
            mine = ("vn_moments_kernel" in row["Name"] or "vn_normalise_kernel" in row["Name"]) if impl == "hip" else calls >= iters
            if mine:
                total += float(row["TotalDurationNs"]); launches += calls
                kernels.append({"name": row["Name"][:80], "calls": calls, "avg_us": float(row["AverageNs"]) / 1e3})
    if not kernels:
        return None, "no matching kernel in %s" % files[0]
    return {"gpu_us_per_step": total / iters / 1e3, "launches_per_step": launches / iters, "kernels": kernels}, None


def child(cmd, timeout):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    res = None
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            res = json.loads(line[7:])
    return p.returncode, res, (p.stdout + p.stderr)[-2000:]


def algorithmic_bytes(obs_dim, batch):
    """per step: the observation block read twice and written once; reward read twice and written once, done read by every row of the
    second launch is served by the cache and counted once per launch; ret, ep_return (fp64) and ep_len read and written"""
    return 3 * obs_dim * batch * 4 + 3 * batch * 4 + 2 * batch + batch * (2 * 8 + 2 * 8 + 2 * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="run", choices=["run", "payload"])
    ap.add_argument("--kind", default="hopper", choices=sorted(ENVS))
    ap.add_argument("--impl", default="hip", choices=["hip", "eager64", "eager32", "throughput"])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecnorm_times.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "scratch", "vecnorm_trace"))
    args = ap.parse_args()
    if args.mode == "payload":
        return payload(args)
    me = os.path.abspath(__file__)
    out = {"batch": BATCH, "iters": ITERS + WARM, "hbm_peak_bytes_per_s": HBM_PEAK, "method": __doc__.split("\n\n")[1]}
    for kind, obs_dim in (("hopper", 11), ("humanoid", 376)):
        rec = {}
        for impl in ("hip", "eager64", "eager32"):
            d = os.path.join(args.trace_dir, "%s_%s" % (kind, impl))
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me, "payload", "--kind", kind,
                   "--impl", impl]
            rc, res, tail = child(cmd, 420)
            print("[probe] %s %s: exit %d %s" % (kind, impl, rc, res), flush=True)
            if rc != 0:                                         # a failed GPU process: record it and start nothing more
                rec[impl] = {"error": "exit %d" % rc, "tail": tail}
                out[kind] = rec
                json.dump(out, open(args.out, "w"), indent=1)
                print(tail)
                return 1
            kt, why = kernel_time_from_trace(d, impl, ITERS + WARM)
            rec[impl] = {"trace": kt, "trace_missing": why, "stream_us_per_step_under_profiler": res and res["stream_us_per_step"]}
        rc, res, tail = child([sys.executable, me, "payload", "--kind", kind, "--impl", "throughput", "--steps", str(args.steps), "--reps", str(args.reps)], 420)
        print("[probe] %s throughput: exit %d" % (kind, rc), flush=True)
        if rc != 0:
            rec["throughput"] = {"error": "exit %d" % rc, "tail": tail}
            out[kind] = rec
            json.dump(out, open(args.out, "w"), indent=1)
            print(tail)
            return 1
        rec["throughput_env_steps_per_s"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for k, v in res.items()}
        hip = rec["hip"]["trace"]
        if hip:
            nbytes = algorithmic_bytes(obs_dim, BATCH)
            bps = nbytes / (hip["gpu_us_per_step"] * 1e-6)
            rec["traffic"] = {"algorithmic_bytes_per_step": nbytes, "achieved_bytes_per_s": bps, "fraction_of_hbm_peak": bps / HBM_PEAK}
            for e in ("eager64", "eager32"):
                if rec[e]["trace"]:
                    rec[e]["ratio_to_hip"] = rec[e]["trace"]["gpu_us_per_step"] / hip["gpu_us_per_step"]
        out[kind] = rec
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
