#!/usr/bin/env python3
"""Measurements of the device-side rollout buffer: writes profiles/rollout_times.json.

Workloads: hopper 32 768 envs x T = 128 and humanoid 4 096 envs x T = 32.  For each of add, GAE, statistics (with the
normalising rewrite) and one gather of 8 192 samples (random ids, and runs of 64 consecutive ids):
  (a) GPU time per call of the rex_rollout_* launches against the summed kernel time of the torch-eager spelling of the same
      operation on the same buffers, both from ``rocprofv3 --kernel-trace --stats`` (one profiled child process per line,
      nothing else traced), and the stream time per call of both (HIP events around the loop) in a process of its own with
      the profiler off;
  (b) algorithmic bytes / GPU time against the HBM peak;
  (c) env-steps/s of step_soa + add against step_soa alone (bench.py's method: a settled env, 16 pre-generated action tensors,
      a host clock around `steps` launches that ends in a device synchronise), alternating the two, several repetitions,
      with the profiler off.

    python3 profiles/rollout_probe.py                 # everything (needs a GPU and rocprofv3), writes the JSON
    python3 profiles/rollout_probe.py payload ...     # what a child process runs

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
WORKLOADS = {"hopper": ("RandomHopper-v0", 32768, 128), "humanoid": ("RandomHumanoid-v0", 4096, 32)}
OPS = ("add", "gae", "stats", "gather_random", "gather_tile64")
KERNELS = {"add": ("ro_add_kernel",), "gae": ("ro_gae_kernel",), "stats": ("ro_moments_kernel", "ro_finish_kernel"),
           "gather_random": ("ro_gather_kernel",), "gather_tile64": ("ro_gather_kernel",)}
ITERS = {"add": (300, 30), "gae": (20, 4), "stats": (100, 10), "gather_random": (200, 20), "gather_tile64": (200, 20)}   # measured, warm-up
MINIBATCH = 8192
HBM_PEAK = 8.0e12          # bytes/s, MI355X
GAMMA, LAM = 0.99, 0.95


def setup(kind):
    import torch
    import random_envs_amd as rex
    env_id, batch, T = WORKLOADS[kind]
    env = rex.make(env_id, batch=batch, seed=0)
    env.reset()
    g = torch.Generator().manual_seed(0)
    amp = float(env.dims.act_high)
    acts = [((torch.rand(env.dims.act_dim, batch, generator=g) * 2 - 1) * amp).cuda().contiguous() for _ in range(16)]
    buf = rex.RolloutBuffer(env, T, gamma=GAMMA, gae_lambda=LAM)
    for k in ("obs", "action", "reward", "value", "log_prob"):
        getattr(buf, k).normal_()
    buf.done.copy_(torch.rand(T, batch, device=env.device) < 0.01)
    buf.pos = T
    return torch, rex, env, acts, buf


def eager_ops(torch, env, buf):
    """every operation spelled in torch eager ops on the same SoA tensors: what a user of step_soa writes today"""
    T, B = buf.n_steps, buf.batch

    def add(t, obs, act, reward, done, value, logp, trunc, tv):
        buf.obs[t].copy_(obs); buf.action[t].copy_(act); buf.done[t].copy_(done); buf.value[t].copy_(value); buf.log_prob[t].copy_(logp)
        buf.reward[t].copy_(torch.where(trunc.bool(), reward + GAMMA * tv, reward))

    def gae(last):
        a = torch.zeros(B, device=env.device)
        for t in reversed(range(T)):
            nnt = 1.0 - buf.done[t].float()
            nv = last if t == T - 1 else buf.value[t + 1]
            delta = buf.reward[t] + GAMMA * nv * nnt - buf.value[t]
            a = delta + GAMMA * LAM * nnt * a
            buf.advantage[t].copy_(a)
        torch.add(buf.advantage, buf.value, out=buf.returns)

    def stats():
        buf.advantage.copy_((buf.advantage - buf.advantage.mean()) / (buf.advantage.std() + 1e-8))

    def gather(idx):
        t, b = idx // B, idx % B
        return (buf.obs[t, :, b], buf.action[t, :, b], buf.advantage.view(-1).index_select(0, idx), buf.returns.view(-1).index_select(0, idx),
                buf.value.view(-1).index_select(0, idx), buf.log_prob.view(-1).index_select(0, idx))

    return add, gae, stats, gather


def payload(args):
    torch, rex, env, acts, buf = setup(args.kind)
    T, B, dev = buf.n_steps, buf.batch, env.device
    value, logp, tv, last = (torch.randn(B, device=dev) for _ in range(4))
    trunc = (torch.rand(B, device=dev) < 0.002).to(torch.uint8)
    if args.op == "throughput":
        for k in range(300):                                   # settle: the batch reaches its steady mix of episode phases
            env.step_soa(acts[k % 16])
        torch.cuda.synchronize()

        def with_add(k):
            obs, reward, done = env.step_soa(acts[k % 16])
            buf.pos = k % T
            buf.add(obs, acts[k % 16], reward, done, value, logp)
        res = {"alone": [], "with_add": []}
        for rep in range(args.reps):
            for name, fn in (("alone", lambda k: env.step_soa(acts[k % 16])), ("with_add", with_add)):
                for k in range(50):
                    fn(k)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(args.steps):
                    fn(k)
                torch.cuda.synchronize()
                res[name].append(B * args.steps / (time.perf_counter() - t0))
        print("RESULT " + json.dumps(res))
        return
    env.step_soa(acts[0])
    e_add, e_gae, e_stats, e_gather = eager_ops(torch, env, buf)
    gen = torch.Generator(device=dev).manual_seed(1)
    ids = {"gather_random": buf.permutation(gen)[:MINIBATCH].contiguous(), "gather_tile64": buf.permutation(gen, tile=64)[:MINIBATCH].contiguous()}
    L, desc = buf._L, __import__("ctypes").byref(buf._desc)

    def fns(hip):
        def add(k):
            if hip:
                buf.pos = k % T
                buf.add(env._obs, acts[0], env._reward, env._done, value, logp, trunc, tv)
            else:
                e_add(k % T, env._obs, acts[0], env._reward, env._done, value, logp, trunc, tv)
        return {"add": add,
                "gae": (lambda k: L.rex_rollout_gae(buf._h, desc, last.data_ptr(), GAMMA, LAM, buf._stream())) if hip else (lambda k: e_gae(last)),
                "stats": (lambda k: L.rex_rollout_adv_stats(buf._h, desc, 1, buf._stream())) if hip else (lambda k: e_stats()),
                "gather_random": (lambda k: buf.gather(ids["gather_random"])) if hip else (lambda k: e_gather(ids["gather_random"])),
                "gather_tile64": (lambda k: buf.gather(ids["gather_tile64"])) if hip else (lambda k: e_gather(ids["gather_tile64"]))}

    def stream_us(fn, op):
        if op == "stats":
            buf.advantage.normal_()
        iters, warm = ITERS[op]
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for k in range(warm):
            fn(k)
        torch.cuda.synchronize()
        ev0.record()
        for k in range(iters):
            fn(k)
        ev1.record()
        torch.cuda.synchronize()
        return 1e3 * ev0.elapsed_time(ev1) / iters

    if args.op == "stream":                                    # profiler off: the stream time per call of every line, both spellings
        res = {op: {impl: stream_us(fns(impl == "hip")[op], op) for impl in ("hip", "eager")} for op in OPS}
        print("RESULT " + json.dumps(res))
        return
    us = stream_us(fns(args.impl == "hip")[args.op], args.op)
    print("RESULT " + json.dumps({"stream_us_per_call": us, "calls": sum(ITERS[args.op])}))


def kernel_time_from_trace(trace_dir, op, impl, calls):
    """us per call from rocprofv3's kernel_stats.csv: the ro_* kernels of the operation (hip), or every kernel the loop launched (eager:
    the kernels called at least once per call; the set-up launches number far fewer)"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None, "no kernel_stats.csv under %s" % trace_dir
    total, kernels, launches = 0.0, [], 0
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            n = int(row["Calls"])
            mine = any(k in row["Name"] for k in KERNELS[op]) if impl == "hip" else n >= calls
            if mine:
                total += float(row["TotalDurationNs"]); launches += n
                kernels.append({"name": row["Name"][:80], "calls": n, "avg_us": float(row["AverageNs"]) / 1e3})
    if not kernels:
        return None, "no matching kernel in %s" % files[0]
    return {"gpu_us_per_call": total / calls / 1e3, "launches_per_call": launches / calls, "kernels": kernels}, None


def child(cmd, timeout):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    res = None
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            res = json.loads(line[7:])
    return p.returncode, res, (p.stdout + p.stderr)[-2000:]


def algorithmic_bytes(op, obs_dim, act_dim, B, T):
    """what the operation has to move once: add reads and writes a step's rows; GAE reads reward, value (4 B) and done (1 B) and writes
    advantage and returns; the statistics read the advantages twice and write them once; a gather reads and writes n rows plus the ids"""
    step = (obs_dim + act_dim + 3) * 4 + 1
    return {"add": 2 * step * B, "gae": (3 * 4 + 1 + 4) * B * T, "stats": 3 * 4 * B * T,
            "gather_random": MINIBATCH * (2 * (obs_dim + act_dim + 4) * 4 + 8), "gather_tile64": MINIBATCH * (2 * (obs_dim + act_dim + 4) * 4 + 8)}[op]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="run", choices=["run", "payload"])
    ap.add_argument("--kind", default="hopper", choices=sorted(WORKLOADS))
    ap.add_argument("--op", default="add", choices=OPS + ("throughput", "stream"))
    ap.add_argument("--impl", default="hip", choices=["hip", "eager"])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_times.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "scratch", "rollout_trace"))
    args = ap.parse_args()
    if args.mode == "payload":
        return payload(args)
    me = os.path.abspath(__file__)
    out = {"workloads": {k: {"batch": v[1], "T": v[2]} for k, v in WORKLOADS.items()}, "minibatch": MINIBATCH, "hbm_peak_bytes_per_s": HBM_PEAK,
           "method": __doc__.split("\n\n")[1]}

    def fail(rec, kind, key, rc, tail):                        # a failed GPU process: record it and start nothing more
        rec[key] = {"error": "exit %d" % rc, "tail": tail}
        out[kind] = rec
        json.dump(out, open(args.out, "w"), indent=1)
        print(tail)
        return 1

    for kind, (obs_dim, act_dim) in (("hopper", (11, 3)), ("humanoid", (376, 17))):
        _, B, T = WORKLOADS[kind]
        rec = {}
        for op in OPS:
            line = {}
            for impl in ("hip", "eager"):
                d = os.path.join(args.trace_dir, "%s_%s_%s" % (kind, op, impl))
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me, "payload", "--kind", kind,
                       "--op", op, "--impl", impl]
                rc, res, tail = child(cmd, 420)
                print("[probe] %s %s %s: exit %d %s" % (kind, op, impl, rc, res), flush=True)
                if rc != 0:
                    rec[op] = line
                    return fail(rec, kind, "%s_%s" % (op, impl), rc, tail)
                kt, why = kernel_time_from_trace(d, op, impl, sum(ITERS[op]))
                line[impl] = {"trace": kt, "trace_missing": why, "stream_us_per_call_under_profiler": res and res["stream_us_per_call"]}
            if line["hip"]["trace"]:
                nbytes = algorithmic_bytes(op, obs_dim, act_dim, B, T)
                bps = nbytes / (line["hip"]["trace"]["gpu_us_per_call"] * 1e-6)
                line["traffic"] = {"algorithmic_bytes": nbytes, "achieved_bytes_per_s": bps, "fraction_of_hbm_peak": bps / HBM_PEAK}
                if line["eager"]["trace"]:
                    line["eager_to_hip_gpu_time"] = line["eager"]["trace"]["gpu_us_per_call"] / line["hip"]["trace"]["gpu_us_per_call"]
            rec[op] = line
            out[kind] = rec
            json.dump(out, open(args.out, "w"), indent=1)
        rc, res, tail = child([sys.executable, me, "payload", "--kind", kind, "--op", "stream"], 420)
        print("[probe] %s stream times: exit %d %s" % (kind, rc, res), flush=True)
        if rc != 0:
            return fail(rec, kind, "stream", rc, tail)
        rec["stream_us_per_call_profiler_off"] = res
        rc, res, tail = child([sys.executable, me, "payload", "--kind", kind, "--op", "throughput", "--steps", str(args.steps), "--reps", str(args.reps)], 420)
        print("[probe] %s throughput: exit %d" % (kind, rc), flush=True)
        if rc != 0:
            return fail(rec, kind, "throughput", rc, tail)
        rec["throughput_env_steps_per_s"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for k, v in res.items()}
        out[kind] = rec
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out, indent=1)[-6000:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
