#!/usr/bin/env python3
"""tools/shift_bench.py - what the random-shift augmentation (include/agx_augment.h) costs, at N = B = 1024, 84 x 84 / 30 x 30,
fs = 4, pad = 4, valid samples, for resize / mask / raw / full in float32 and bfloat16:

  (a) agx_history_observe (its code is the parent commit's: the yardstick);
  (b) agx_history_observe_shifted with the shifts already on the device;
  (c) what a caller writes without it, in the same process: (a) followed by the torch gather of the batch - one
      advanced-indexing read `plain[b, p, iy, ix]` into a new tensor, with the index tensors built per call;
  (d) agx_shift_draw.

Every launch (or launch sequence) sits between a begin and an end event of its own on the stream; the figures are the median /
min / p90 over --iters repetitions after --warmup.  The yardsticks are ratios inside one run: (b) / (a), with (a)'s own spread
p90 - median next to it, and (b) / (c).  Writes profiles/shift_bench.json.

    python tools/shift_bench.py [--iters 200] [--warmup 20] [--capacity 64] [--out profiles/shift_bench.json]
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


def one_mode(mode, dtype, a, dev):
    from active_gym import FrameHistory, ObsPipeline, RandomShift
    N, fs, T, B, pad = a.envs, 4, a.capacity, a.envs, a.pad
    what = "full" if mode == "full" else "fovea"
    pipe = ObsPipeline(N, "fixed", obs_size=(84, 84), frame_stack=fs, fov_size=(30, 30), resize_to_full=mode in ("resize", "full"),
                       mask_out=mode == "mask", device=dev, obs_dtype=dtype)
    hist = FrameHistory(pipe, T)
    aug = RandomShift(hist, pad=pad, seed=1)
    g = torch.Generator(device=dev).manual_seed(0)
    cmd = torch.full((N,), 2, dtype=torch.uint8, device=dev)
    for _ in range(T + fs):                       # fill the history: every retained index is valid afterwards
        pipe.ingest_gray(torch.randint(0, 256, (N, 2, 84, 84), dtype=torch.uint8, device=dev, generator=g), cmd)
        pipe.fovea(torch.rand((N, 2), device=dev, generator=g) * 54)
        hist.push(cmd)
    count = int(hist.last_index()[0]) + 1
    env = torch.randint(0, N, (B,), dtype=torch.int32, device=dev, generator=g)
    idx = torch.randint(count - T + fs - 1, count, (B,), dtype=torch.int64, device=dev, generator=g)
    shift = aug.draw(B)
    plain = torch.empty((B,) + hist.obs_row_shape(what), dtype=dtype, device=dev)
    shifted = torch.empty_like(plain)
    loc = torch.empty((B, 2), dtype=torch.int32, device=dev)
    val = torch.empty((B,), dtype=torch.uint8, device=dev)
    h, w = plain.shape[-2:]
    bi = torch.arange(B, device=dev)[:, None, None, None]
    pi = torch.arange(fs, device=dev)[None, :, None, None]
    ar_h, ar_w = torch.arange(h, device=dev)[None, :], torch.arange(w, device=dev)[None, :]

    def observe():
        hist.observe(env, idx, what=what, out=plain, loc_out=loc, valid_out=val)

    def observe_shifted():
        aug.observe(env, idx, what=what, shift=shift, out=shifted, loc_out=loc, valid_out=val)

    def observe_then_gather():
        hist.observe(env, idx, what=what, out=plain, loc_out=loc, valid_out=val)
        d = shift.to(torch.int64)                 # the index tensors are built per call: the shifts are new every time
        iy = (ar_h + d[:, :1] - pad).clamp_(0, h - 1)
        ix = (ar_w + d[:, 1:] - pad).clamp_(0, w - 1)
        return plain[bi, pi, iy[:, None, :, None], ix[:, None, None, :]]        # one advanced-indexing gather, nothing behind it

    def draw():
        aug.draw(B, out=shift_out)

    shift_out = torch.empty_like(shift)
    observe_shifted()
    gathered = observe_then_gather()
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert bool(val.all()), "the benchmark's samples must be valid"
    assert torch.equal(shifted.view(bits), gathered.view(bits)), "the shifted observe differs from observe + gather"
    res = {"observe": timed(observe, a.iters, a.warmup), "shifted": timed(observe_shifted, a.iters, a.warmup),
           "observe_then_gather": timed(observe_then_gather, a.iters, a.warmup), "draw": timed(draw, a.iters, a.warmup)}
    res["observe_spread_us"] = res["observe"]["p90_us"] - res["observe"]["median_us"]
    res["shifted_minus_observe_us"] = res["shifted"]["median_us"] - res["observe"]["median_us"]
    res["shifted_over_observe"] = res["shifted"]["median_us"] / res["observe"]["median_us"]
    res["shifted_over_gather"] = res["shifted"]["median_us"] / res["observe_then_gather"]["median_us"]
    pipe.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--pad", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shift_bench.json"))
    a = ap.parse_args()
    from active_gym import _native as nat
    dev = torch.device("cuda:0")
    res = {"envs": a.envs, "samples": a.envs, "capacity": a.capacity, "pad": a.pad, "build": nat.build_info(), "iters": a.iters}
    for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
        res[name] = {mode: one_mode(mode, dtype, a, dev) for mode in ("resize", "mask", "raw", "full")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
