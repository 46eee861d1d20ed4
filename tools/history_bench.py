#!/usr/bin/env python3
"""tools/history_bench.py - what the frame history (include/agx_history.h) costs, at N = 1024, 84 x 84 / 30 x 30, fs = 4, resize:

  * the step (ingest + agx_fovea_fixed) with and without agx_history_push behind it;
  * agx_history_observe at B = 1024 uniformly random valid samples;
  * agx_fovea_fixed in the same process, measured the same way.

Every launch (or launch sequence) sits between a begin and an end event of its own on the stream; the figure is the median
over --iters repetitions after --warmup.  The two yardsticks are ratios inside one run: observe / fovea (same store stream,
reads 3 % of its bytes) and step with push / step without.  Writes profiles/history_bench.json.

    python tools/history_bench.py [--iters 200] [--warmup 20] [--capacity 64] [--out profiles/history_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "active-gym_amd"))


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
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "p90_us": float(np.percentile(us, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "history_bench.json"))
    a = ap.parse_args()
    from active_gym import FrameHistory, ObsPipeline
    from active_gym import _native as nat
    dev = torch.device("cuda:0")
    N, fs, T = a.envs, 4, a.capacity
    pipe = ObsPipeline(N, "fixed", obs_size=(84, 84), frame_stack=fs, fov_size=(30, 30), resize_to_full=True, device=dev)
    hist = FrameHistory(pipe, T)
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.randint(0, 256, (N, 2, 210, 160, 3), dtype=torch.uint8, device=dev, generator=g)
    cmd = torch.full((N,), 2, dtype=torch.uint8, device=dev)
    act = torch.rand((N, 2), device=dev, generator=g) * 54
    obs = torch.empty(pipe.obs_shape, dtype=torch.float32, device=dev)
    loc = torch.empty((N, 2), dtype=torch.int32, device=dev)
    index = torch.empty((N,), dtype=torch.int64, device=dev)

    def step():
        pipe.ingest(frames, cmd)
        pipe.fovea(act, out=obs, loc_out=loc)

    def step_push():
        step()
        hist.push(cmd, out=index)

    for _ in range(T + fs):                       # fill the history: every retained index is valid afterwards
        step_push()
    count = int(hist.last_index()[0]) + 1
    B = 1024
    env = torch.randint(0, N, (B,), dtype=torch.int32, device=dev, generator=g)
    idx = torch.randint(count - T + fs - 1, count, (B,), dtype=torch.int64, device=dev, generator=g)
    out = torch.empty((B,) + hist.obs_row_shape(), dtype=torch.float32, device=dev)
    oloc = torch.empty((B, 2), dtype=torch.int32, device=dev)
    oval = torch.empty((B,), dtype=torch.uint8, device=dev)
    hist.observe(env, idx, out=out, loc_out=oloc, valid_out=oval)
    assert bool(oval.all()), "the benchmark's samples must all be valid"
    res = {"envs": N, "samples": B, "capacity": T, "history_bytes": hist.nbytes, "build": nat.build_info(), "iters": a.iters}
    res["fovea_fixed"] = timed(lambda: pipe.fovea(act, out=obs, loc_out=loc), a.iters, a.warmup)
    res["observe"] = timed(lambda: hist.observe(env, idx, out=out, loc_out=oloc, valid_out=oval), a.iters, a.warmup)
    res["observe_full"] = timed(lambda: hist.observe(env, idx, what="full", out=out, loc_out=oloc, valid_out=oval), a.iters, a.warmup)
    res["push"] = timed(lambda: hist.push(cmd, out=index), a.iters, a.warmup)
    res["step"] = timed(step, a.iters, a.warmup)
    res["step_push"] = timed(step_push, a.iters, a.warmup)
    res["observe_over_fovea"] = res["observe"]["median_us"] / res["fovea_fixed"]["median_us"]
    res["step_push_over_step"] = res["step_push"]["median_us"] / res["step"]["median_us"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
