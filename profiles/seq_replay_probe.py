#!/usr/bin/env python3
"""Measurements of the sequence-window launch (sequence windows section): writes profiles/seq_replay_times.json.

Workloads: hopper 4 096 envs x T = 256 slots and humanoid 4 096 envs x T = 64 slots, minibatches of 256 windows of L = 8, 32 and 64 steps, a
full ring whose head is slot T - 1, no normalisation.  The stored tensors are written directly: normal observations, actions and rewards, a
done on 1 % of the transitions and a time limit beside a third of those, so the windows end in all three ways.  For sample_seq
(rb_seq_kernel) and for a torch restatement that builds the same seven tensors from ReplayBuffer.views() (an [n, L] index matrix modulo the
ring, one advanced-index gather per stored field, the first end of every window from a cumulative sum, where() for the zero padding, an
index_put for the row to bootstrap from) -- what a user writes at the parent commit, checked EQUAL to the launch's outputs on the
launch's ids before anything is timed:
  (a) the stream time per call (HIP events around a loop of calls after a warm-up, profiler off, one child process per workload, the
      variants alternating, three repetitions, the median reported), the ratio torch / launch, and the algorithmic bytes (rows and flags
      read, outputs written, from the window lengths of one draw) over the launch's time;
  (b) the GPU time per call of rb_seq_kernel from ``rocprofv3 --kernel-trace``, one profiled child process per workload running the three
      lengths one after the other (the kernel's name is the same for all of them: its dispatches are split by their order), and the
      algorithmic bytes over it.

    python3 profiles/seq_replay_probe.py                 # everything (needs a GPU and rocprofv3), writes the JSON
    python3 profiles/seq_replay_probe.py payload ...     # what a child process runs

A measurement that could not be taken is recorded as null with the reason: nothing is estimated.  A failed child process ends the run."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from replay_buffer_probe import child  # noqa: E402

WORKLOADS = {"hopper": ("RandomHopper-v0", 4096, 256), "humanoid": ("RandomHumanoid-v0", 4096, 64)}
SEQ_LENS = (8, 32, 64)
MINIBATCH = 256
ITERS, WARM = 1000, 100
P_DONE = 0.01
FIELDS = ("obs", "action", "reward", "done", "mask", "length", "index")
VARIANTS = ["seq_%d" % L for L in SEQ_LENS] + ["torch_seq_%d" % L for L in SEQ_LENS]


def setup(kind):
    import torch
    import random_envs_amd as rex
    env_id, batch, T = WORKLOADS[kind]
    env = rex.make(env_id, batch=batch, seed=0)
    env.reset()
    buf = rex.ReplayBuffer(env, T, seed=3)
    g = torch.Generator(device=env.device).manual_seed(0)
    for k in ("obs", "next_obs", "action", "reward"):
        getattr(buf, k).normal_(generator=g)
    done = torch.rand(T, batch, generator=g, device=env.device) < P_DONE
    buf.done.copy_(done)
    buf.timeout.copy_(done & (torch.rand(T, batch, generator=g, device=env.device) < 1.0 / 3.0))
    buf.pos, buf.full = 0, True                                # a full ring, the head is slot T - 1
    torch.cuda.synchronize()
    return torch, env, buf


def torch_seq(torch, buf):
    """the sequence sample out of torch calls over ReplayBuffer.views(): what a user of ReplayBuffer writes without the launch"""
    T, B, D, A, dev = buf.n_slots, buf.batch, buf.obs_dim, buf.act_dim, buf.device
    v = buf.views()
    obs, nxt, act = v["obs"].view(T * B, D), v["next_obs"].view(T * B, D), v["action"].view(T * B, A)
    rew, done, tout = v["reward"].view(-1), v["done"].view(-1), v["timeout"].view(-1)

    def sample(n, L, idx=None):
        head = (buf.pos - 1) % T
        if idx is None:
            idx = torch.randint(0, T * B, (n,), device=dev)
        k = torch.arange(L, device=dev)
        t0, b = idx // B, idx % B
        t = (t0[:, None] + k[None, :]) % T
        s = t * B + b[:, None]
        d, to = done[s], tout[s]
        end = (d != 0) | (to != 0) | (t == head)
        end[:, -1] = True
        m = (end.cumsum(1) == 0).sum(1) + 1                                                              # the first end of every window
        mask = k[None, :] < m[:, None]
        o = torch.zeros(n, L + 1, D, dtype=torch.float32, device=dev)
        o[:, :L] = torch.where(mask[:, :, None], obs[s], 0.0)
        o[torch.arange(n, device=dev), m] = nxt[s.gather(1, (m - 1)[:, None]).squeeze(1)]
        a = torch.where(mask[:, :, None], act[s], torch.zeros((), dtype=act.dtype, device=dev))
        r = torch.where(mask, rew[s], 0.0)
        dn = torch.where(mask, ((d != 0) & (to == 0)).float(), 0.0)
        return dict(obs=o, action=a, reward=r, done=dn, mask=mask.float(), length=m.int(), index=idx)

    return sample


def algorithmic_bytes(length, L, D, A):
    """what one call has to move, from the window lengths of a draw: rows and flags read (m obs rows, one next_obs row, m action rows, the
    reward and the two flag bytes of m steps, the id is drawn) and the seven outputs written"""
    n, steps = len(length), int(sum(length))
    read = 4 * D * (steps + n) + 4 * A * steps + 6 * steps
    written = n * (4 * D * (L + 1) + 4 * A * L + 3 * 4 * L + 4 + 8)
    return read + written


def payload(args):
    torch, env, buf = setup(args.kind)
    e_seq = torch_seq(torch, buf)
    fns, mean_bytes, mean_steps = {}, {}, {}
    for L in SEQ_LENS:                                         # equal on the launch's own ids before anything is timed
        out = buf.sample_seq(MINIBATCH, L, normalize=False)
        ref = e_seq(MINIBATCH, L, out["index"])
        for k in FIELDS:
            if out[k].dtype != ref[k].dtype or out[k].shape != ref[k].shape or not torch.equal(out[k].contiguous().view(torch.uint8), ref[k].contiguous().view(torch.uint8)):
                print("the torch restatement and the launch disagree on %s at L = %d" % (k, L))
                return 1
        length = out["length"].cpu().tolist()
        mean_bytes[str(L)] = algorithmic_bytes(length, L, buf.obs_dim, buf.act_dim)
        mean_steps[str(L)] = sum(length) / len(length)
        fns["seq_%d" % L] = (lambda L: lambda: buf.sample_seq(MINIBATCH, L, normalize=False))(L)
        fns["torch_seq_%d" % L] = (lambda L: lambda: e_seq(MINIBATCH, L))(L)

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
        print("RESULT " + json.dumps({"runs": res, "bytes": mean_bytes, "mean_steps": mean_steps}))
        return 0
    for L in SEQ_LENS:                                         # under the profiler: the launches of the package only, one length after the other
        stream_us(fns["seq_%d" % L])
    print("RESULT " + json.dumps({"calls_per_length": ITERS + WARM}))
    return 0


def kernel_times_from_trace(trace_dir, name, groups, per_group, skip):
    """average duration (us) of the dispatches of kernel ``name`` in each of ``groups`` consecutive runs of ``per_group`` dispatches, the first
    ``skip`` of a run left out.  The payload's equality check dispatches the kernel once per length ahead of them."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None, "no kernel_trace.csv under %s" % trace_dir
    with open(files[0]) as f:
        rows = list(csv.DictReader(f))
    if not rows:
        return None, "%s is empty" % files[0]
    col = {c.lower(): c for c in rows[0]}
    try:
        kn, t0, t1 = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    except KeyError:
        return None, "columns of %s: %s" % (files[0], sorted(col))
    d = sorted((int(r[t0]), int(r[t1])) for r in rows if name in r[kn])
    d = d[groups:]                                             # the equality check's dispatches
    if len(d) != groups * per_group:
        return None, "%d dispatches of %s, expected %d" % (len(d), name, groups * per_group)
    out = []
    for g in range(groups):
        run = d[g * per_group + skip:(g + 1) * per_group]
        out.append({"calls": len(run), "avg_us": sum(b - a for a, b in run) / len(run) / 1e3, "min_us": min(b - a for a, b in run) / 1e3,
                    "max_us": max(b - a for a, b in run) / 1e3})
    return out, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="run", choices=["run", "payload"])
    ap.add_argument("--kind", default="hopper", choices=sorted(WORKLOADS))
    ap.add_argument("--op", default="stream")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_replay_times.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "scratch", "seq_replay_trace"))
    args = ap.parse_args()
    if args.mode == "payload":
        return payload(args)
    me = os.path.abspath(__file__)
    out = {"workloads": {k: {"batch": v[1], "T": v[2]} for k, v in WORKLOADS.items()}, "minibatch": MINIBATCH, "seq_lens": list(SEQ_LENS),
           "iterations": ITERS, "warm_up": WARM, "p_done": P_DONE, "method": __doc__.split("\n\n")[1]}

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
        rec = {}
        for L in SEQ_LENS:
            hip, tor = sorted(res["runs"]["seq_%d" % L])[1], sorted(res["runs"]["torch_seq_%d" % L])[1]
            rec["L_%d" % L] = {"stream_us_per_call": {"launch": hip, "torch": tor, "torch_to_launch": tor / hip,
                                                      "runs": {"launch": res["runs"]["seq_%d" % L], "torch": res["runs"]["torch_seq_%d" % L]}},
                               "mean_steps_per_window": res["mean_steps"][str(L)], "algorithmic_bytes": res["bytes"][str(L)],
                               "GB_per_s_over_stream_time": res["bytes"][str(L)] / hip / 1e3}
        d = os.path.join(args.trace_dir, kind)
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, me, "payload",
               "--kind", kind, "--op", "trace"]
        rc, _, tail = child(cmd, 330)
        print("[probe] %s trace: exit %d" % (kind, rc), flush=True)
        if rc != 0:
            rec["trace_error"] = {"error": "exit %d" % rc, "tail": tail}
            return stop(kind, rec, tail)
        kt, why = kernel_times_from_trace(d, "rb_seq_kernel", len(SEQ_LENS), ITERS + WARM, WARM)
        for i, L in enumerate(SEQ_LENS):
            r = rec["L_%d" % L]
            r["kernel_us"], r["kernel_missing"] = (kt[i] if kt else None), why
            r["GB_per_s_over_kernel_time"] = r["algorithmic_bytes"] / kt[i]["avg_us"] / 1e3 if kt else None
        out[kind] = rec
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out, indent=1)[-6000:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
