#!/usr/bin/env python3
"""tools/glimpse_bench.py - what the glimpse memory (include/agx_glimpse.h) costs, at N = B = 1024, 84 x 84 / 30 x 30, fs = 4,
P = 3, in mask-out and in resize mode:

  * agx_history_observe_memory (one launch);
  * the composition it replaces, in the same process: P calls of agx_history_observe into P batches plus P - 1
    torch.maximum passes;
  * one agx_history_observe.

Every launch (or launch sequence) sits between a begin and an end event of its own on the stream; the figure is the median
over --iters repetitions after --warmup.  The yardsticks are ratios inside one run: memory / composition and
memory / observe.  Writes profiles/glimpse_bench.json.

    python tools/glimpse_bench.py [--iters 200] [--warmup 20] [--capacity 64] [--out profiles/glimpse_bench.json]
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


def one_mode(mode, a, dev):
    from active_gym import FrameHistory, GlimpseMemory, ObsPipeline
    N, fs, T, P, B = a.envs, 4, a.capacity, a.glimpses, a.envs
    pipe = ObsPipeline(N, "fixed", obs_size=(84, 84), frame_stack=fs, fov_size=(30, 30), resize_to_full=mode == "resize",
                       mask_out=mode == "mask", device=dev)
    hist = FrameHistory(pipe, T)
    mem = GlimpseMemory(hist, P)
    g = torch.Generator(device=dev).manual_seed(0)
    cmd = torch.full((N,), 2, dtype=torch.uint8, device=dev)
    for _ in range(T + fs):                       # fill the history: every retained index is valid afterwards
        pipe.ingest_gray(torch.randint(0, 256, (N, 2, 84, 84), dtype=torch.uint8, device=dev, generator=g), cmd)
        pipe.fovea(torch.rand((N, 2), device=dev, generator=g) * 54)
        hist.push(cmd)
    count = int(hist.last_index()[0]) + 1
    env = torch.randint(0, N, (B,), dtype=torch.int32, device=dev, generator=g)
    idx = torch.randint(count - T + fs - 1 + P - 1, count, (B,), dtype=torch.int64, device=dev, generator=g)
    older = [idx - i for i in range(P)]
    out = torch.empty((B,) + hist.obs_row_shape(), dtype=torch.float32, device=dev)
    parts = [torch.empty_like(out) for _ in range(P)]
    comp = torch.empty_like(out)
    mloc = torch.empty((B, P, 2), dtype=torch.int32, device=dev)
    oloc = torch.empty((B, 2), dtype=torch.int32, device=dev)
    taken = torch.empty((B,), dtype=torch.uint8, device=dev)
    oval = torch.empty((B,), dtype=torch.uint8, device=dev)

    def memory():
        mem.observe(env, idx, out=out, loc_out=mloc, taken_out=taken)

    def composition():
        for i in range(P):
            hist.observe(env, older[i], out=parts[i], loc_out=oloc, valid_out=oval)
        torch.maximum(parts[0], parts[1], out=comp)
        for i in range(2, P):
            torch.maximum(comp, parts[i], out=comp)

    def observe():
        hist.observe(env, idx, out=parts[0], loc_out=oloc, valid_out=oval)

    memory()
    composition()
    assert bool((taken == P).all()), "the benchmark's samples must take every glimpse"
    assert torch.equal(out.view(torch.int32), comp.view(torch.int32)), "the memory differs from the composition"
    res = {"memory": timed(memory, a.iters, a.warmup), "composition": timed(composition, a.iters, a.warmup),
           "observe": timed(observe, a.iters, a.warmup)}
    res["memory_over_composition"] = res["memory"]["median_us"] / res["composition"]["median_us"]
    res["memory_over_observe"] = res["memory"]["median_us"] / res["observe"]["median_us"]
    pipe.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--glimpses", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "glimpse_bench.json"))
    a = ap.parse_args()
    from active_gym import _native as nat
    dev = torch.device("cuda:0")
    res = {"envs": a.envs, "samples": a.envs, "capacity": a.capacity, "glimpses": a.glimpses, "build": nat.build_info(), "iters": a.iters}
    for mode in ("mask", "resize"):
        res[mode] = one_mode(mode, a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
