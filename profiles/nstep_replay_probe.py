#!/usr/bin/env python3
"""Measurements of the n-step sample launch (n-step returns section): writes profiles/nstep_replay_times.json.

Workloads: those of replay_buffer_probe.py -- hopper 32 768 envs x T = 64 slots and humanoid 32 768 envs x T = 8 slots, minibatches of 4 096,
a full ring whose head is slot T - 1, no normalisation.  For sample_nstep at n_step 1, 5 and 32, for the plain sample (rb_sample_kernel, the
kernel of the parent commit, unchanged) and for a torch restatement of the n-step sample over the same [T][B] storage (an [n, n_step] index
matrix modulo the ring, three gathers over reward / done / timeout, the first end of every window, a masked power sum, the row gathers):
  (a) the stream time per call (HIP events around a loop of calls after a warm-up, profiler off, one child process per workload, the
      variants alternating, three repetitions, the median reported);
  (b) the GPU time per call of rb_nstep_kernel and rb_sample_kernel from ``rocprofv3 --kernel-trace --stats``, in profiled child processes
      of their own (one per n_step: the kernel's name is the same for all of them; nothing else traced).

    python3 profiles/nstep_replay_probe.py                 # everything (needs a GPU and rocprofv3), writes the JSON
    python3 profiles/nstep_replay_probe.py payload ...     # what a child process runs

A measurement that could not be taken is recorded as null with the reason: nothing is estimated.  A failed child process ends the run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from replay_buffer_probe import ITERS, MINIBATCH, WARM, WORKLOADS, child, kernel_time_from_trace, setup  # noqa: E402

N_STEPS = (1, 5, 32)
GAMMA = 0.99
HBM_MISS_US = 0.37                                    # about 900 cycles, the hardware guide's figure for an HBM miss, at 2.4 GHz
VARIANTS = ["sample"] + ["nstep_%d" % k for k in N_STEPS] + ["torch_nstep_%d" % k for k in N_STEPS]


def torch_nstep(torch, buf):
    """the n-step sample out of torch calls over the buffer's own storage: what a user of ReplayBuffer writes today"""
    T, B, D, A, dev = buf.n_slots, buf.batch, buf.obs_dim, buf.act_dim, buf.device
    obs, nxt, act = buf.obs.view(T * B, D), buf.next_obs.view(T * B, D), buf.action.view(T * B, A)
    rew, done, tout = buf.reward.view(-1), buf.done.view(-1), buf.timeout.view(-1)

    def sample(n, n_step, gamma):
        head = (buf.pos - 1) % T
        k = torch.arange(n_step, device=dev)
        gpow = torch.full((n_step + 1,), gamma, dtype=torch.float64, device=dev).cumprod(0) / gamma      # gamma^0 .. gamma^n_step
        idx = torch.randint(0, T * B, (n,), device=dev)
        t0, b = idx // B, idx % B
        t = (t0[:, None] + k[None, :]) % T
        s = t * B + b[:, None]
        r, d, to = rew[s], done[s], tout[s]
        end = (d != 0) | (to != 0) | (t == head)
        end[:, -1] = True
        last = (end.cumsum(1) == 0).sum(1)                                                                # the first end of every window
        ret = (r.double() * gpow[None, :n_step] * (k[None, :] <= last[:, None])).sum(1).float()
        s_last = s.gather(1, last[:, None]).squeeze(1)
        dn = (d.gather(1, last[:, None]).squeeze(1) != 0) & (to.gather(1, last[:, None]).squeeze(1) == 0)
        return obs[idx], nxt[s_last], act[idx], ret, dn.float(), gpow[last + 1].float(), (last + 1).int(), idx

    return sample


def payload(args):
    torch, env, w, acts, buf, step = setup(args.kind)
    e_nstep = torch_nstep(torch, buf)
    fns = {"sample": lambda: buf.sample(MINIBATCH, normalize=False)}
    for k in N_STEPS:
        fns["nstep_%d" % k] = (lambda k: lambda: buf.sample_nstep(MINIBATCH, k, GAMMA, normalize=False))(k)
        fns["torch_nstep_%d" % k] = (lambda k: lambda: e_nstep(MINIBATCH, k, GAMMA))(k)

    def stream_us(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(ITERS):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return 1e3 * ev0.elapsed_time(ev1) / ITERS

    if args.op == "stream":                                    # profiler off: every variant, alternating, three repetitions
        res = {v: [] for v in VARIANTS}
        for rep in range(3):
            for v in VARIANTS:
                res[v].append(stream_us(fns[v]))
        steps = {str(k): float(buf.sample_nstep(MINIBATCH, k, GAMMA, normalize=False)["steps"].float().mean()) for k in N_STEPS}
        print("RESULT " + json.dumps({"runs": res, "mean_steps": steps}))
        return
    for v in args.op.split(","):                               # under the profiler: the launches of the package only
        stream_us(fns[v])
    print("RESULT " + json.dumps({"calls": ITERS + WARM}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="run", choices=["run", "payload"])
    ap.add_argument("--kind", default="hopper", choices=sorted(WORKLOADS))
    ap.add_argument("--op", default="stream")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nstep_replay_times.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "scratch", "nstep_replay_trace"))
    args = ap.parse_args()
    if args.mode == "payload":
        return payload(args)
    me = os.path.abspath(__file__)
    out = {"workloads": {k: {"batch": v[1], "T": v[2]} for k, v in WORKLOADS.items()}, "minibatch": MINIBATCH, "iterations": ITERS, "warm_up": WARM,
           "gamma": GAMMA, "method": __doc__.split("\n\n")[1]}

    def stop(kind, rec, tail):
        out[kind] = rec
        json.dump(out, open(args.out, "w"), indent=1)
        print(tail)
        return 1

    for kind in WORKLOADS:
        rc, res, tail = child(["timeout", "-k", "10", "300", sys.executable, me, "payload", "--kind", kind, "--op", "stream"], 330)
        print("[probe] %s stream times: exit %d %s" % (kind, rc, res), flush=True)
        if rc != 0 or not res:                                 # a failed GPU process: record it and start nothing more
            return stop(kind, {"error": "exit %d" % rc, "tail": tail}, tail)
        rec = {v: {"stream_us_per_call": sorted(res["runs"][v])[1], "runs": res["runs"][v]} for v in VARIANTS}
        rec["mean_steps_per_window"] = res["mean_steps"]
        for k in N_STEPS:                                      # one profiled process per n_step; the plain sample rides with the first
            ops = "nstep_%d" % k + (",sample" if k == N_STEPS[0] else "")
            d = os.path.join(args.trace_dir, "%s_%d" % (kind, k))
            cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me,
                   "payload", "--kind", kind, "--op", ops]
            rc, _, tail = child(cmd, 330)
            print("[probe] %s trace of %s: exit %d" % (kind, ops, rc), flush=True)
            if rc != 0:
                rec["trace_error"] = {"ops": ops, "error": "exit %d" % rc, "tail": tail}
                return stop(kind, rec, tail)
            for op in ops.split(","):
                kt, why = kernel_time_from_trace(d, "rb_sample_kernel" if op == "sample" else "rb_nstep_kernel")
                rec[op]["kernel_us"], rec[op]["kernel_missing"] = kt, why
        k1, k32 = rec["nstep_1"]["kernel_us"], rec["nstep_32"]["kernel_us"]
        if k1 and k32:
            rec["window_cost"] = {"kernel_us_32_minus_1": k32["avg_us"] - k1["avg_us"], "serial_walk_estimate_us": 31 * HBM_MISS_US,
                                  "note": "31 dependent HBM misses of about 0.37 us each is what a serial walk of a 32-step window would add"}
        else:
            rec["window_cost"] = None
        out[kind] = rec
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out, indent=1)[-6000:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
