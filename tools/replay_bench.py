#!/usr/bin/env python3
"""tools/replay_bench.py - what the replay sampler (include/agx_replay.h) costs, at N = 1024, 84 x 84 / 30 x 30, fs = 4, a full
history, forward = 1, for B = 256 / 4096 / 32768 samples:

  (a) sampler.sample(B)                  the scan and the draw, two launches;
  (b) history.observe of the same B      what the samples are drawn for, in the same process;
  (c) the draw a caller makes today      last_index().cpu(), a NumPy draw of B (env, index) pairs inside the retained range
                                         (it cannot see age: it does no acceptance test at all), and the upload of both arrays.

(a) and (b) sit between a begin and an end event of their own on the stream; (c) crosses the host, so it is timed with the host
clock between two device synchronisations - and so is (a) once more ("sample_host"), so that (a) / (c) compares like with like.
Each figure is the median (with min and p90) over --iters repetitions after --warmup.  The yardsticks are ratios inside one
run: sample_over_observe (events) and sample_over_host_draw (host clock).  Writes profiles/replay_bench.json.

    python tools/replay_bench.py [--iters 200] [--warmup 20] [--capacity 64] [--out profiles/replay_bench.json]
"""
import argparse
import json
import os
import sys
import time

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


def timed_host(fn, iters, warmup):
    """Median / min / p90 in microseconds of fn() followed by a device synchronisation, on the host clock."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return _stats(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096, 32768])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "replay_bench.json"))
    a = ap.parse_args()
    from active_gym import FrameHistory, ObsPipeline, ReplaySampler
    from active_gym import _native as nat
    dev = torch.device("cuda:0")
    N, fs, T = a.envs, 4, a.capacity
    pipe = ObsPipeline(N, "fixed", obs_size=(84, 84), frame_stack=fs, fov_size=(30, 30), resize_to_full=True, device=dev)
    hist = FrameHistory(pipe, T)
    g = torch.Generator(device=dev).manual_seed(0)
    cmd = torch.full((N,), 2, dtype=torch.uint8, device=dev)
    for _ in range(T + fs):                       # fill the history: every index beyond the oldest fs - 1 retained ones is valid
        pipe.ingest_gray(torch.randint(0, 256, (N, 2, 84, 84), dtype=torch.uint8, device=dev, generator=g), cmd)
        pipe.fovea(torch.rand((N, 2), device=dev, generator=g) * 54)
        hist.push(cmd)
    smp = ReplaySampler(hist, back=0, forward=1, seed=0)
    rng = np.random.default_rng(0)
    res = {"envs": N, "capacity": T, "forward": 1, "back": 0, "attempts": smp.attempts, "build": nat.build_info(), "iters": a.iters,
           "batches": {}}
    for B in a.batches:
        env = torch.empty((B,), dtype=torch.int32, device=dev)
        idx = torch.empty((B,), dtype=torch.int64, device=dev)
        ok = torch.empty((B,), dtype=torch.uint8, device=dev)
        out = torch.empty((B,) + hist.obs_row_shape(), dtype=torch.float32, device=dev)
        loc = torch.empty((B, 2), dtype=torch.int32, device=dev)
        val = torch.empty((B,), dtype=torch.uint8, device=dev)

        def sample():
            smp.sample(B, env, idx, ok)

        def observe():
            hist.observe(env, idx, out=out, loc_out=loc, valid_out=val)

        def host_draw():
            last = hist.last_index().cpu().numpy()
            e = rng.integers(0, N, B).astype(np.int32)
            lo = np.maximum(last[e] + 1 - T, 0)
            k = (lo + rng.integers(0, 1 << 62, B) % np.maximum(last[e] - lo, 1)).astype(np.int64)
            env.copy_(torch.from_numpy(e))
            idx.copy_(torch.from_numpy(k))

        sample()
        observe()
        torch.cuda.synchronize()
        accepted = int(ok.sum())
        assert accepted >= 0.99 * B and bool(val.bool().eq(ok.bool()).all()), "the benchmark's samples must be accepted and valid"
        r = {"accepted": accepted, "total": int(smp.total()),
             "sample": timed(sample, a.iters, a.warmup), "observe": None, "sample_host": timed_host(sample, a.iters, a.warmup),
             "host_draw": timed_host(host_draw, a.iters, a.warmup)}
        sample()                                  # observe() times the sampler's own samples, not the host draw's
        r["observe"] = timed(observe, a.iters, a.warmup)
        r["sample_over_observe"] = r["sample"]["median_us"] / r["observe"]["median_us"]
        r["sample_over_host_draw"] = r["sample_host"]["median_us"] / r["host_draw"]["median_us"]
        res["batches"][str(B)] = r
    pipe.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
