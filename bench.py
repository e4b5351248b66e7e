#!/usr/bin/env python3
"""bench.py -- env-steps/sec of the batched RandomHopper-v0 hot path on N MI355X (one process per GPU).

Contract: `python bench.py --gpus N --steps K --warmup W`.  For N > 1 the driver launches it under
torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE from the env); started WITHOUT a launcher and with
--gpus N > 1 it starts the N ranks itself (child processes, before anything touches the GPU in the parent) and
relays rank 0's line.  A "step" is one `env.step()` of the whole per-GPU batch: the step kernel (hopper: 4 RK4
mj_steps = 16 forward-dynamics solves per env) with the auto-reset (rocRAND init noise + xi resample) fused in.
Actions, state and xi are resident in HBM before the timed region starts.  The env batch is sharded by index
(weak scaling: 32768 envs per GPU); the ONLY collective is the all-reduce of the step counter (plus the
max-over-ranks of the elapsed time required by the contract).

`--config C1|C2|C3|C4|C5` selects the other BASELINE.json configurations with SURVEY.md section 8(d)'s inputs
(per-GPU shard of the config, its env id, its DR distribution); without it the north-star point (hopper,
32768 envs per GPU, uniform xi nominal +-10 %) runs.  `metric` is BASELINE.json's string on the north-star line only;
every other line names its own quantity (env id, batch, GPUs) there.

Rank 0 prints ONE JSON line with the contract fields plus
  "roofline":     HBM roofline of the dominant kernel, from HIP-event durations of launches of the timed region,
  "cpu_baseline": (--full only) the fp64 oracle (a CPU port of the same step, oracle/) timed on this host's cores on a
                  bounded sample of the SAME workload: the GPU leg's settled states, xi and action sequence, auto-reset
                  included (N=1, rank 0 only).

A plain run sets up, settles, warms up, times --steps steps and prints the line.  `--full` adds what takes time of its
own: the CPU baseline, and (short timed regions) 128 more launches of the same workload, every one bracketed by HIP
events, after the timed region so the roofline's kernel average does not rest on a handful of samples.
`--dump-outputs DIR` writes what the last timed step returned (obs, reward, done) to DIR/<name>.npy (dump_outputs).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENV_ID = "RandomHopper-v0"
BATCH_PER_GPU = 32768
# algorithmic bytes per env-step = read (qpos,qvel,action,xi) + write (qpos,qvel,obs,reward,done)
BYTES_PER_KIND = {"hopper": 173, "walker2d": 293, "halfcheetah": 273, "cartpole": 73, "humanoid": 2073}
# the names rocprofv3 / profiles/hbm_traffic.json show for the launched instantiation: <spec, PAIR = two lanes per env, ROLLED>
PLANAR_SPEC = {"hopper": "HopperSpec", "walker2d": "Walker2dSpec", "halfcheetah": "HalfCheetahSpec"}


def kernel_of(kind, shape):
    """Name of the step kernel a handle launches, from the launch shape rex_create picked for it (VecRandomEnv.launch_shape(): planar chains two
    lanes per env up to 32 envs x SIMDs and one lane per env past that, the hopper past 64 envs x SIMDs on the 256-register kernel with the
    rolled general solver)."""
    if kind == "cartpole":
        return "cartpole_step_kernel"
    if kind == "humanoid":
        return "humanoid_pair_step_kernel" if shape["hum_pair"] else "humanoid_step_kernel"
    return "planar_step_kernel<rex::%s, %s, %s>" % (PLANAR_SPEC[kind], "true" if shape["pair"] else "false", "true" if shape["rolled"] else "false")


METRIC = "env-steps/sec at batch 32768, RandomHopper-v0, 1/2/4/8 MI355X; % HBM roofline"   # BASELINE.json


def metric_of(env_id, batch_per_gpu, global_batch, world, scaling, replay=False):
    """The `metric` string of a line: BASELINE.json's on the line that measures it (RandomHopper-v0 at 32 768 envs -- per GPU under weak
    scaling, in total under strong scaling: SURVEY.md 8(d)), the line's own quantity everywhere else."""
    headline = env_id == ENV_ID and not replay and (batch_per_gpu if scaling == "weak" else global_batch) == BATCH_PER_GPU
    if headline:
        return METRIC
    what = "replayed env-steps/sec" if replay else "env-steps/sec"
    return "%s at batch %d%s, %s, %d MI355X; %% HBM roofline" % (what, global_batch if scaling == "strong" else batch_per_gpu,
                                                                  " in total" if scaling == "strong" and world > 1 else (" per GPU" if world > 1 else ""),
                                                                  env_id, world)
HBM_PEAK_GBS = 8000.0             # MI355X_MICROARCH.md: 8.0 TB/s spec

# BASELINE.json configs[1..4] with SURVEY.md section 8(d)'s synthetic inputs; `batch` is the per-GPU shard
CONFIGS = {
    "C1": dict(env="RandomCartPole-v0", batch=1, dr="none",
               note="batch 1, actions ~ U{0,1}, reset on done, no DR (test_random_policy.py:12-32): plumbing -- one env is one lane of one wave, "
                    "the line is the launch latency of a step"),
    "C2": dict(env="RandomHopper-v0", batch=4096, dr="readme",
               note="uniform xi, distr [0.9,1.1,1.9,2.1,2.9,3.1,3.9,4.1] (README.md:58)"),
    "C3": dict(env="RandomHalfCheetahNoisy-v0", batch=16384, dr="cheetah",
               note="uniform xi: nominal masses +-20 %, friction U(0.3,0.5); obs noise of the Noisy id"),
    "C4": dict(env="RandomWalker2d-v0", batch=8192, dr="truncnorm",
               note="truncnorm xi: mean nominal, std 10 % of mean, lower bounds random_walker2d.py:80-96 (32768 over 4 GPUs)"),
    "C5": dict(env="RandomHumanoid-v0", batch=32768, dr="search_bounds",
               note="uniform xi over the search bounds random_humanoid.py:72-105 (262144 over 8 GPUs)"),
}


def apply_dr(env, mode):
    """The DR distribution of a configuration; returns a description for the JSON line."""
    import numpy as np
    nom = np.asarray(env.original_task, dtype=np.float64)
    if mode == "none":
        return "no DR (nominal xi)"
    if mode == "readme":
        env.set_dr_distribution("uniform", [0.9, 1.1, 1.9, 2.1, 2.9, 3.1, 3.9, 4.1])
        return "uniform xi [0.9,1.1]x[1.9,2.1]x[2.9,3.1]x[3.9,4.1]"
    if mode == "cheetah":
        lo, hi = 0.8 * nom, 1.2 * nom
        lo[7], hi[7] = 0.3, 0.5
        env.set_dr_distribution("uniform", np.stack([lo, hi], 1).ravel().tolist())
        return "uniform xi: masses nominal +-20 %, friction U(0.3,0.5)"
    if mode == "truncnorm":
        env.set_dr_distribution("truncnorm", np.stack([nom, 0.1 * nom], 1).ravel().tolist())
        return "truncnorm xi: mean nominal, std 10 % of mean"
    if mode == "search_bounds":
        lo, hi = env.get_task_search_bounds()
        env.set_dr_distribution("uniform", np.stack([np.asarray(lo), np.asarray(hi)], 1).ravel().tolist())
        return "uniform xi over the search bounds"
    env.set_dr_distribution("uniform", np.stack([0.9 * nom, 1.1 * nom], 1).ravel().tolist())
    return "uniform DR over the %d-dim xi (nominal +-10%%)" % env.task_dim


def reset_states(kind, n, rng):
    """reset_model() states of the reference (random_hopper.py:112-120, random_half_cheetah.py:123-131,
    random_walker2d.py:144-153, random_humanoid.py:219-234): what a finished lane restarts from."""
    import numpy as np
    from oracle_bindings import DIMS
    d = DIMS[kind]
    if kind == "humanoid":
        q = np.tile(np.array([0, 0, 1.4, 1, 0, 0, 0] + [0] * 17, dtype=float), (n, 1)) + rng.uniform(-.01, .01, (n, 24))
        v = rng.uniform(-.01, .01, (n, 23))
    elif kind == "halfcheetah":
        q = rng.uniform(-.1, .1, (n, 9)); v = 0.1 * rng.randn(n, 9)
    else:
        q = rng.uniform(-.005, .005, (n, d["nq"])); q[:, 1] += 1.25
        v = rng.uniform(-.005, .005, (n, d["nv"]))
    return q, v


def cpu_baseline(env_id, kind, q, v, xi, acts, steps, seed=0, min_seconds=12.0, max_envs=None):
    """oracle ("port") timed on the host cores on the GPU leg's own workload: its settled states (q, v), its xi and its
    action sequence for `steps` env-steps, finished lanes restarting from reset_model() states like the GPU's fused
    auto-reset.  Bounded: a prefix of the batch (`max_envs`) and repeats of the same rollout until >= min_seconds."""
    import numpy as np
    from oracle_bindings import oracle_rollout, oracle_rollout_autoreset
    cores = len(os.sched_getaffinity(0))
    rng = np.random.RandomState(seed)
    n = q.shape[0] if max_envs is None else min(q.shape[0], max_envs)
    q, v, xi, acts = q[:n], v[:n], xi[:n], acts[:steps, :n]
    qr, vr = reset_states(kind, n, rng)
    oracle_rollout(kind, q[:64], v[:64], acts[:2, :64], xi[:64], nthreads=cores)   # warm the library
    reps, dt, resets = 0, 0.0, 0
    t0 = time.perf_counter()
    while dt < min_seconds and reps < 64:
        out = oracle_rollout_autoreset(kind, q, v, acts, xi, qr, vr, nthreads=cores)   # MuJoCo's own solver tolerance 1e-8
        reps += 1; dt = time.perf_counter() - t0; resets = int(out["resets"].sum())
    # the reference's own usage shape: ONE env stepped by ONE core; ~2 s
    t1, r1 = 0.0, 0
    t0 = time.perf_counter()
    while t1 < 2.0 and r1 < 100000:
        oracle_rollout_autoreset(kind, q[:1], v[:1], acts[:, :1], xi[:1], qr[:1], vr[:1], nthreads=1)
        r1 += 1; t1 = time.perf_counter() - t0
    return dict(value=n * steps * reps / dt, unit="env-steps/s", cores=cores, kind="port", one_env_one_core=steps * r1 / t1,
                sample="%s: the first %d envs of the GPU leg's settled batch (its states, xi and actions) x %d env-steps, "
                       "auto-reset from reset_model() states (%d resets per pass), %d passes, fp64, %d threads, %.1f s"
                       % (env_id, n, steps, resets, reps, cores, dt))


def cpu_baseline_cartpole(env_id, q, v, xi, acts, min_seconds=3.0):
    """C1's CPU leg: the fp64 port of RandomCartPoleEnv.step (oracle/cartpole.c, pinned bit-exact to the reference by tests/golden/cartpole_*.json)
    stepping the GPU leg's own settled states one batched call per env-step -- at batch 1 that is the reference's usage shape, one env on one core
    (test_random_policy.py:25-32), ctypes call overhead included; finished envs restart from U(-0.05, 0.05)^4 (random_cartpole.py:226-229)."""
    import numpy as np
    from oracle_bindings import oracle_cartpole_step
    n = q.shape[0]
    rng = np.random.RandomState(0)
    st = np.stack([q[:, 0], v[:, 0], q[:, 1], v[:, 1]], 1)   # (x, x_dot, theta, theta_dot)
    steps, dt, resets = 0, 0.0, 0
    t0 = time.perf_counter()
    while dt < min_seconds:
        for k in range(256):
            st, _, done = oracle_cartpole_step(st, acts[k % len(acts)], xi)
            if done.any():
                st[done] = rng.uniform(-0.05, 0.05, (int(done.sum()), 4)); resets += int(done.sum())
        steps += 256; dt = time.perf_counter() - t0
    return dict(value=n * steps / dt, unit="env-steps/s", cores=1, kind="port", one_env_one_core=(steps / dt) if n == 1 else None,
                sample="%s: the GPU leg's %d settled env(s) x %d env-steps through oracle/cartpole.c (one ctypes call per batched step), "
                       "%d resets, fp64, 1 thread, %.1f s" % (env_id, n, steps, resets, dt))


DUMP_CAP_BYTES = 64 * 10 ** 6


def dump_outputs(dirname, arrays, cap=DUMP_CAP_BYTES, seed=0):
    """--dump-outputs: the arrays the last timed step returned (SoA, the env axis last, as step_soa / replay_soa return them) as
    DIR/<name>.npy in float32 (done as 0 / 1).  Past `cap` bytes in all, the same seeded sample of envs is kept from every array
    and its indices go to env_index.npy (float64).  Returns the names written."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: np.ascontiguousarray(np.asarray(a), dtype=np.float32) for k, a in arrays.items()}
    n = next(iter(arrays.values())).shape[-1]
    per_env = sum(a.nbytes for a in arrays.values()) // max(n, 1)
    budget = cap - 4096 * (len(arrays) + 1)          # room for the .npy headers
    if per_env * n > budget:
        idx = np.sort(np.random.RandomState(seed).choice(n, budget // (per_env + 8), replace=False))
        arrays = {k: np.ascontiguousarray(a[..., idx]) for k, a in arrays.items()}
        arrays["env_index"] = idx.astype(np.float64)
    for k, a in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), a)
    return sorted(arrays)


def source_digest():
    """sha256 over the kernel sources: ties a committed PMC traffic figure to the code it was measured on."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "random-envs_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp")):
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(key, batch, kernel):
    """HBM bytes per launch of the dominant kernel from the separate rocprofv3 --pmc passes (profiles/collect_cfg.sh + summarise_cfg.py write
    profiles/hbm_traffic.json together with the digest of the sources, the per-GPU batch and the kernel they profiled).  Returns (bytes or
    None, stale): a figure is reported only for the sources, batch and kernel instantiation it was measured on."""
    tp = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    if not os.path.exists(tp):
        return None, False
    try:
        rec = json.load(open(tp))
    except Exception:
        return None, False
    rec = next((r for r in (rec.get(key), rec.get("%s@%d" % (key, batch)))
                if isinstance(r, dict) and "bytes_per_launch" in r and r.get("batch", batch) == batch and r.get("kernel", kernel) == kernel), None)
    if rec is None:
        return None, False         # nothing measured at this batch / launch shape
    if rec.get("source_digest") != source_digest():
        return None, True          # kernels changed since the PMC run: do not report a stale figure
    return rec["bytes_per_launch"], False


def self_launch(n):
    """`bench.py --gpus N` without a launcher: start N ranks as child processes (nothing in this parent has touched the GPU
    or imported torch), hand each its RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*, relay their output, exit with the worst code."""
    import socket
    import tempfile
    rc = 1
    for attempt in range(3):   # the rendezvous port is picked by bind(0) and released before rank 0 listens on it: retry if somebody took it
        s = socket.socket(); s.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        base = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                    HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        out0 = tempfile.TemporaryFile()   # rank 0's stdout goes to a file: nothing to drain, so the parent is free to supervise
        err0 = tempfile.TemporaryFile()
        procs = []
        for r in range(n):
            env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=out0 if r == 0 else subprocess.DEVNULL, stderr=err0 if r == 0 else None))
        # supervise: the first rank that exits non-zero ends the run at once (its siblings would otherwise sit in the rendezvous or in a
        # collective until torch's 10- to 30-minute timeout, holding the GPUs)
        rc, live = 0, list(procs)
        while live and rc == 0:
            time.sleep(0.2)
            for p in list(live):
                if p.poll() is not None:
                    live.remove(p)
                    rc = rc or p.returncode
        if rc != 0:
            for p in live:
                p.terminate()
            for p in live:
                try:
                    p.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    p.kill(); p.wait()
        err0.seek(0); err = err0.read().decode(errors="replace")
        if rc != 0 and attempt < 2 and ("EADDRINUSE" in err or "Address already in use" in err):
            continue
        sys.stderr.write(err)
        out0.seek(0); sys.stdout.write(out0.read().decode()); sys.stdout.flush()
        break
    sys.exit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--batch", type=int, default=None, help="envs per GPU (weak) / global batch (strong); default 32768 or the --config's shard")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: --batch envs on every GPU; strong: --batch envs in total, split by index (SURVEY 8d north-star point)")
    ap.add_argument("--env", default=None)
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="BASELINE.json configs[1..4] with SURVEY 8(d)'s inputs")
    ap.add_argument("--replay", action="store_true",
                    help="second workload (SURVEY 8 f2): ONE logged transition replayed under a fresh candidate xi per env and step "
                         "(one rex_replay launch per call, nothing of the env touched)")
    ap.add_argument("--counter-every", type=int, default=256, help="steps between asynchronous all-reduces of the step counter")
    ap.add_argument("--settle", type=int, default=300,
                    help="untimed steps before the warm-up: right after reset every env is in the same phase of its first episode "
                         "(in the air, no contact rows -- cheaper than the steady state where episodes end and restart all the time)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true", help="diagnostic: skip the per-launch HIP events")
    ap.add_argument("--time-every", type=int, default=8,
                    help="bracket every n-th launch of the timed region with HIP events (the two event packets cost ~8 us of stream "
                         "time per bracketed launch, 9 %% of a hopper step: timing every launch would lower `value` by that much)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N>1 (nccl = RCCL; gloo only to rehearse the launch path on one GPU)")
    ap.add_argument("--same-device", action="store_true", help="rehearsal: every rank uses GPU 0")
    ap.add_argument("--cpu-sample-steps", type=int, default=8)
    ap.add_argument("--pin-shape", action="store_true",
                    help="strong scaling: every shard runs the launch shape the GLOBAL batch gets on one GPU (sharding.pin_global_shape), so the "
                         "sharded run reproduces the single-GPU trajectories bit for bit; default: each shard runs the fastest shape for its own size")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the CPU baseline and, after a short timed region, 128 "
                         "launches with every one bracketed by HIP events for the roofline's kernel average")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (obs, reward, done; rank 0's shard) to DIR/<name>.npy, float32, "
                         "at most 64 MB in all (a seeded sample of envs past that)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)          # never returns

    cfg = CONFIGS.get(args.config, {})
    env_id = args.env or cfg.get("env", ENV_ID)
    batch = args.batch if args.batch is not None else cfg.get("batch", BATCH_PER_GPU)

    import torch
    import __graft_entry__ as graft
    from random_envs_amd import sharding
    from random_envs_amd.specs import IDS
    rank, local_rank, world = sharding.dist_env()
    if args.same_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if rank == 0 and not os.environ.get("REX_LIB"):   # REX_LIB: a tuning build chosen by hand (profiles/ab_bench.sh)
        graft.build()
    dev = torch.device("cuda", local_rank)
    cdev = dev if args.backend == "nccl" else torch.device("cpu")   # where the collectives' tensors live
    sharding.init(args.backend, dev)   # "nccl" = RCCL over xGMI; no-op at N=1
    sharding.barrier()
    world = sharding.world_size()      # the ranks the process group actually has
    import random_envs_amd as rex

    if args.scaling == "strong":
        env_offset, B = sharding.shard_strong(batch, rank, world)   # fixed global batch split by index
    else:
        env_offset, B = sharding.shard(batch, rank)                 # fixed per-GPU batch
    kind = IDS[env_id][0]
    env = rex.make(env_id, batch=B, device=local_rank, seed=0, env_offset=env_offset, autoreset=not args.replay)
    if args.pin_shape and args.scaling == "strong":
        sharding.pin_global_shape(env, batch)
    dr_note = apply_dr(env, cfg.get("dr"))
    env.set_dr_training(cfg.get("dr") != "none")
    env.reset()
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)
    nact = 16
    amp = float(env.dims.act_high)   # U(-1,1) (hopper/walker/cheetah) or U(-0.4,0.4) (humanoid, humanoid.xml:6)
    if kind == "cartpole":           # Discrete(2): action_space.sample() of test_random_policy.py:26
        actions = [torch.randint(0, 2, (B,), generator=g, dtype=torch.int32).cuda(local_rank).contiguous() for _ in range(nact)]
    else:
        actions = [((torch.rand(env.dims.act_dim, B, generator=g) * 2 - 1) * amp).cuda(local_rank).contiguous() for _ in range(nact)]
    if args.replay:
        # the logged transition: the state reached after a few random steps of env 0, replicated; candidates: fresh xi draws
        for k in range(8):
            env.step_soa(actions[k % nact])
        q, v = env.get_state()
        q0 = q[:1].clone().expand(B, -1).contiguous(); v0 = v[:1].clone().expand(B, -1).contiguous()
        cands = env.sample_tasks(nact).contiguous()        # [nact, B, task_dim] on the device
        q0z = q0.clone(); q0z[:, 0] = 0                     # get_full_mjstate: root x zeroed
        if kind == "humanoid":
            q0z[:, 1] = 0
        q_soa, v_soa = q0z.t().contiguous(), v0.t().contiguous()
        cands_soa = cands.transpose(1, 2).contiguous()      # [nact, task_dim, B]

        def one_step(k):                                    # ONE launch: caller's SoA (state, xi, action) in, (obs', r, done) out
            return env.replay_soa(q_soa, v_soa, cands_soa[k % nact], actions[0])
    else:
        def one_step(k):
            return env.step_soa(actions[k % nact])

    def sync():
        sharding.barrier()
        torch.cuda.synchronize()

    # every one-time cost goes BEFORE the timed region: the HIP-event pool is created here and the warm-up launches
    # are already timing-enabled (the first timed hipEventRecord on a stream pays a one-off profiling set-up)
    for k in range(0 if args.replay else args.settle):
        one_step(k)
    torch.cuda.synchronize()
    t_setup0 = time.perf_counter()
    every = 0 if args.no_kernel_timing else max(1, min(args.time_every, max(args.steps // 4, 1)))
    env.enable_timing(every)
    one_step(0)
    torch.cuda.synchronize()
    timing_setup_ms = 1e3 * (time.perf_counter() - t_setup0)
    for k in range(args.warmup):
        one_step(k)
    sync()
    env.read_timing()                                        # drop the warm-up samples
    want_cpu = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not args.replay
    if want_cpu:                                             # the CPU leg starts from exactly these states
        qs, vs = env.get_state(); xs = env.get_task()
        settled = [z.clone() for z in (qs, vs, xs)]
    counter = sharding.StepCounter(cdev, every=args.counter_every)
    sync()
    t0 = time.perf_counter()
    for k in range(args.steps):
        last = one_step(k)
        counter.add(B)                                       # async all-reduce every --counter-every steps (N > 1)
    sync()
    elapsed = time.perf_counter() - t0
    kernel_ms = env.read_timing()
    if args.dump_outputs and rank == 0:                      # before anything below steps the env again
        dump_outputs(args.dump_outputs, {name: z.cpu().numpy() for name, z in zip(("obs", "reward", "done"), last)})
    # a short timed region leaves few bracketed launches (the driver's command: 20 steps -> 4): with --full, continue the SAME
    # workload outside the timed region with every launch bracketed, so the kernel average does not rest on a handful of samples
    n_extra = 0
    if args.full and every and len(kernel_ms) < 64:
        import numpy as np
        env.enable_timing(1)
        n_extra = 128
        for k in range(n_extra):
            one_step(args.steps + k)
        torch.cuda.synchronize()
        kernel_ms_ext = np.concatenate([kernel_ms, env.read_timing()])
    else:
        kernel_ms_ext = kernel_ms
    env.enable_timing(False)

    # the only collectives of the path: SUM of the step counter (asynchronous, above), MAX of the elapsed time
    total_steps = counter.total()
    elapsed = sharding.reduce_max(elapsed, cdev)
    counters = env.counters()
    shape = env.launch_shape()

    if rank == 0:
        value = total_steps / elapsed
        n_k = len(kernel_ms)
        kavg_region = float(kernel_ms.mean()) if n_k else float("nan")
        kavg_ms = float(kernel_ms_ext.mean()) if len(kernel_ms_ext) else float("nan")
        ksum_ms = kavg_region * args.steps if n_k else float("nan")
        bytes_step = BYTES_PER_KIND[kind] + (4 * env.task_dim if args.replay else 0)   # replay also reads the candidate xi rows
        achieved = bytes_step * B / (kavg_ms * 1e-3) / 1e9 if kavg_ms == kavg_ms else None
        wall_ms = 1e3 * elapsed / args.steps
        achieved_wall = bytes_step * B / (wall_ms * 1e-3) / 1e9
        traffic, stale = pmc_traffic(args.config or env_id, B, kernel_of(kind, shape)) if not args.replay else (None, False)
        out = {
            "metric": metric_of(env_id, B, batch if args.scaling == "strong" else B * world, world, args.scaling, args.replay),
            "value": value, "unit": "env-steps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": wall_ms,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s%s%s, batch %d per GPU, %s, %s actions, %s"
                                   % (("%s: " % args.config) if args.config else "", env_id,
                                      " [replay: 1 logged transition x B candidate xi]" if args.replay else "", B, dr_note,
                                      "U{0,1}" if kind == "cartpole" else "U(-%.1f,%.1f)" % (amp, amp),
                                      "one fused rex_replay launch per call" if args.replay else
                                      ("auto-reset" if cfg.get("dr") == "none" else "auto-reset + xi resample")),
                       "global_batch": total_steps // max(args.steps, 1),
                       "parallelism": "index-sharded envs x%d (%s scaling), no data-path collective; step counter all-reduced "
                                      "asynchronously every %d steps" % (world, args.scaling, args.counter_every)},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": (achieved / HBM_PEAK_GBS) if achieved else None, "traffic": traffic,
                         "kernel": kernel_of(kind, shape), "launch_shape": shape, "kernel_avg_ms": kavg_ms, "kernel_launches_timed": len(kernel_ms_ext),
                         "kernel_launches_timed_in_region": n_k, "kernel_avg_ms_in_region": kavg_region if n_k else None,
                         "algorithmic_bytes_per_launch": bytes_step * B, "bytes_per_env_step": bytes_step,
                         # the same fraction on the WALL clock of the timed region (what `value` is computed from)
                         "achieved_wall": achieved_wall, "frac_wall": achieved_wall / HBM_PEAK_GBS,
                         "note": "VALU-issue/latency-bound by construction (hopper: 16 forward-dynamics solves per 173 B); HBM fraction "
                                 "reported because the metric asks for it"},
            # wall time of the timed region minus the summed kernel time: launch + host overhead per run
            "host_gap_ms": (1e3 * elapsed - ksum_ms) if n_k else None,
            "timing_setup_ms": timing_setup_ms,
            "counter_reductions": counter.reductions,
            "solver_capped_waves": counters["solver_capped"], "nonfinite_lanes": counters["nonfinite"],
            "overflow_lanes": counters["overflow"],
        }
        if args.config:
            out["config"]["baseline_config"] = "%s: %s" % (args.config, cfg["note"])
        if stale:
            out["roofline"]["traffic_note"] = "profiles/hbm_traffic.json was measured on other kernel sources (digest mismatch): re-run profiles/collect.sh"
        if want_cpu:
            import numpy as np
            qs, vs, xs = [z.cpu().double().numpy() for z in settled]
            n_cpu_steps = max(1, min(args.cpu_sample_steps, args.steps))
            if kind == "cartpole":
                out["cpu_baseline"] = cpu_baseline_cartpole(env_id, qs, vs, xs, [a.cpu().numpy() for a in actions])
            else:
                acts = np.stack([actions[k % nact].t().cpu().double().numpy() for k in range(n_cpu_steps)])
                out["cpu_baseline"] = cpu_baseline(env_id, kind, qs, vs, xs, acts, n_cpu_steps,
                                                   max_envs=4096 if kind == "humanoid" else None)
        print(json.dumps(out), flush=True)
    env.close()
    sharding.shutdown()


if __name__ == "__main__":
    main()
