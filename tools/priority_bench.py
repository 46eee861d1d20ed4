#!/usr/bin/env python3
"""tools/priority_bench.py - what the prioritized sampler (include/agx_priority.h) costs, at N = 1024, kind base at 12 x 12 (small
frames, full-size bookkeeping), fs = 2, a full history of T = 64 and T = 1024 env-steps per env, every row's priority set from
random values, forward = 1, for B = 256 / 4096 / 32768 samples:

  (a) prioritized.sample(B)              weights + chunk scan + env scan + draw, four launches over T * N rows;
  (b) uniform.sample(B)                  the uniform draw of include/agx_replay.h, two small dependent launches: the yardstick;
  (c) what a caller writes today         a [T, N] float32 priority tensor of its own: torch.cumsum over it in float64, B uniform
                                         numbers times the total, torch.searchsorted (it cannot test acceptance at all, and its
                                         sums are rounded);
  (d) prioritized.update(B)              one launch.

Each sits between a begin and an end event of its own on the stream; each figure is the median (with min and p90) over --iters
repetitions after --warmup.  rows_per_us is T * N over (a)'s median, bytes_per_row what the four launches move per row by
construction (12 table + 1 age read, 8 prefix written).  Writes profiles/priority_bench.json.

    python tools/priority_bench.py [--iters 200] [--warmup 20] [--capacities 64 1024] [--out profiles/priority_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "active-gym_amd"))


def _stats(us):
    us = np.asarray(us)
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "p90_us": float(np.percentile(us, 90))}


def timed(fn, iters, warmup):
    """Median / min / p90 in microseconds of fn() between two events of its own."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return _stats([a.elapsed_time(b) * 1e3 for a, b in ev])


def one_capacity(N, T, batches, iters, warmup):
    from active_gym import FrameHistory, ObsPipeline, PrioritizedSampler, ReplaySampler
    dev = torch.device("cuda:0")
    fs = 2
    pipe = ObsPipeline(N, "base", obs_size=(12, 12), frame_stack=fs, device=dev)
    hist = FrameHistory(pipe, T)
    g = torch.Generator(device=dev).manual_seed(0)
    cmd = torch.full((N,), 2, dtype=torch.uint8, device=dev)
    for _ in range(T + fs):                       # fill the history: every index beyond the oldest fs - 1 retained ones is valid
        pipe.ingest_gray(torch.randint(0, 256, (N, 2, 12, 12), dtype=torch.uint8, device=dev, generator=g), cmd)
        pipe.observe_full()
        hist.push(cmd)
    per = PrioritizedSampler(hist, back=0, forward=1, seed=0)
    uni = ReplaySampler(hist, back=0, forward=1, seed=0)
    last = hist.last_index()
    env_all = torch.arange(N, dtype=torch.int32, device=dev).repeat(T)
    idx_all = (last.repeat(T) - torch.arange(T, device=dev).repeat_interleave(N)).contiguous()
    per.update(env_all, idx_all, (torch.rand((T * N,), device=dev, generator=g) * 4 + 1e-3).contiguous())
    own = torch.rand((T, N), device=dev, generator=g) * 4 + 1e-3          # (c): the caller's own priority tensor
    res = {"capacity": T, "rows": T * N, "table_bytes": per.bytes(), "history_bytes": hist.nbytes, "batches": {}}
    for B in batches:
        env = torch.empty((B,), dtype=torch.int32, device=dev)
        idx = torch.empty((B,), dtype=torch.int64, device=dev)
        ok = torch.empty((B,), dtype=torch.uint8, device=dev)
        wt = torch.empty((B,), dtype=torch.int64, device=dev)
        prio = (torch.rand((B,), device=dev, generator=g) * 4 + 1e-3).contiguous()

        def prioritized():
            per.sample(B, env, idx, ok, wt)

        def uniform():
            uni.sample(B, env, idx, ok)

        def caller():
            c = torch.cumsum(own.reshape(-1).to(torch.float64), 0)
            at = torch.searchsorted(c, torch.rand((B,), device=dev, dtype=torch.float64) * c[-1]).clamp(max=T * N - 1)
            env.copy_(at % N)
            idx.copy_(at // N)

        def update():
            per.update(env, idx, prio)

        prioritized()
        torch.cuda.synchronize()
        assert bool(ok.all()) and int(per.accepted()) >= (T - fs) * N, "the benchmark's history must be full and drawable"
        r = {"accepted": int(per.accepted()), "total": int(per.total()),
             "prioritized": timed(prioritized, iters, warmup), "uniform": timed(uniform, iters, warmup),
             "caller_cumsum_searchsorted": timed(caller, iters, warmup)}
        prioritized()                             # update() times the sampler's own samples
        r["update"] = timed(update, iters, warmup)
        r["prioritized_over_uniform"] = r["prioritized"]["median_us"] / r["uniform"]["median_us"]
        r["prioritized_over_caller"] = r["prioritized"]["median_us"] / r["caller_cumsum_searchsorted"]["median_us"]
        r["rows_per_us"] = T * N / r["prioritized"]["median_us"]
        res["batches"][str(B)] = r
    pipe.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--capacities", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096, 32768])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "priority_bench.json"))
    a = ap.parse_args()
    from active_gym import _native as nat
    res = {"envs": a.envs, "forward": 1, "back": 0, "bytes_per_row": {"read": 13, "written": 8}, "build": nat.build_info(), "iters": a.iters,
           "capacities": [one_capacity(a.envs, T, a.batches, a.iters, a.warmup) for T in a.capacities]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
