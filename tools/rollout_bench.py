#!/usr/bin/env python3
"""tools/rollout_bench.py - what an on-policy rollout (include/agx_rollout.h) costs, at N = 1024 envs, L = 128, a history of
T = 256 filled by scripted steps with resets (autoresets with TERMINATED and TRUNCATED, resets nothing announced, a few rows
never recorded), 84 x 84 / 30 x 30, fs = 4, a 12-byte payload:

  (g) agx_rollout_gather, all six outputs;
  (a) agx_rollout_gae on the gathered arrays;
  (t) the yardstick for (a): the usual torch loop over t = L - 1 .. 0 on the same device arrays, with its masks (BOOT,
      TERMINATED, the chain breaks, the live slots) computed once outside the timed region.

In the same process (a) is checked against (t): the loop rounds in the same order, so the two are compared bit for bit and the
largest difference is recorded.  Every launch sequence sits between a begin and an end event of its own on the stream; the
figures are the median / min / p90 over --iters repetitions after --warmup.  Writes profiles/rollout_bench.json.

    python tools/rollout_bench.py [--iters 200] [--warmup 20] [--out profiles/rollout_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "active-gym_amd"))
CLEAR, SKIP = 0x04, 0x08


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


def fill(pipe, hist, log, steps, g, dev):
    """Scripted steps: per env and step an autoreset with TERMINATED (1 %) or TRUNCATED (0.5 %), a reset nothing announced
    (0.5 %), a row never recorded (0.2 %), else a plain recorded step."""
    N = pipe.num_envs
    two = torch.full((N,), 2, dtype=torch.uint8, device=dev)
    for step in range(steps):
        u = torch.rand((N,), device=dev, generator=g)
        term, trunc, silent, unrec = u < 0.01, (u >= 0.01) & (u < 0.015), (u >= 0.015) & (u < 0.02), (u >= 0.02) & (u < 0.022)
        if step == 0:
            term, trunc, unrec, silent = (torch.zeros_like(term),) * 3 + (torch.ones_like(term),)
        cmd = two | (silent.to(torch.uint8) * CLEAR)
        pipe.ingest_gray(torch.randint(0, 256, (N, 2, 84, 84), dtype=torch.uint8, device=dev, generator=g), cmd)
        pipe.fovea(torch.rand((N, 2), device=dev, generator=g) * 54)
        index = hist.push(cmd)
        index = torch.where(silent | unrec, torch.full_like(index, -1), index)
        log.record(index, torch.randn((N,), device=dev, generator=g), term.to(torch.uint8) + trunc.to(torch.uint8) * 2,
                   torch.randint(0, 256, (N, 12), dtype=torch.uint8, device=dev, generator=g))
        auto = term | trunc
        if bool(auto.any()):
            cmd = torch.where(auto, two | CLEAR, two | SKIP)
            pipe.ingest_gray(torch.randint(0, 256, (N, 2, 84, 84), dtype=torch.uint8, device=dev, generator=g), cmd)
            pipe.fovea(torch.rand((N, 2), device=dev, generator=g) * 54)
            hist.push(cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_bench.json"))
    a = ap.parse_args()
    from active_gym import FrameHistory, ObsPipeline, Rollout, StepLog
    from active_gym import _native as nat
    from active_gym.rollout import BOOT, TERMINATED
    dev = torch.device("cuda:0")
    N, L, T, gamma, lam = a.envs, a.length, a.capacity, 0.99, 0.95
    pipe = ObsPipeline(N, "fixed", obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), resize_to_full=True, device=dev)
    hist = FrameHistory(pipe, T)
    log = StepLog(hist, 12)
    roll = Rollout(log)
    g = torch.Generator(device=dev).manual_seed(0)
    fill(pipe, hist, log, T + 40, g, dev)
    batch = roll.gather(L)
    value = torch.randn((L, N), device=dev, generator=g)
    boot = torch.randn((L, N), device=dev, generator=g)
    adv, ret = roll.gae(batch, value, boot, gamma, lam)

    ptr = [ctypes.c_void_p(batch[k].data_ptr()) for k in ("len", "obs_index", "next_index", "reward", "ends", "payload")]

    def gather():                                 # the entry point alone: Rollout.gather adds the live mask, two torch launches
        nat.check(roll._lib.agx_rollout_gather(log._s, L, *ptr, pipe._stream()), pipe._ctx)

    def gae():
        roll.gae(batch, value, boot, gamma, lam, adv_out=adv, ret_out=ret)

    ends, reward, live = batch["ends"], batch["reward"], batch["live"]
    is_boot, is_term = (ends & BOOT) != 0, (ends & TERMINATED) != 0
    go = ((ends & 7) == 0).to(torch.float32)
    go[L - 1] = 0
    gl = float(np.float32(gamma) * np.float32(lam))
    zero = torch.zeros((N,), device=dev)
    t_adv = torch.empty((L, N), device=dev)

    def torch_loop():
        last = zero
        for t in range(L - 1, -1, -1):
            nv = torch.where(is_boot[t], boot[t], torch.where(is_term[t], zero, value[t + 1] if t < L - 1 else zero))
            delta = reward[t] + gamma * nv - value[t]
            last = torch.where(live[t], delta + gl * go[t] * last, zero)
            t_adv[t] = last
        return t_adv, torch.where(live, t_adv + value, zero)

    w_adv, w_ret = torch_loop()
    same = bool(torch.equal(adv.view(torch.int32), w_adv.view(torch.int32)) and torch.equal(ret.view(torch.int32), w_ret.view(torch.int32)))
    diff = float(torch.maximum((adv - w_adv).abs().max(), (ret - w_ret).abs().max()))
    assert torch.allclose(adv, w_adv, rtol=1e-4, atol=1e-4) and torch.allclose(ret, w_ret, rtol=1e-4, atol=1e-4), diff
    length = batch["len"].cpu().numpy()
    e = ends[live].cpu().numpy()
    res = {"envs": N, "L": L, "capacity": T, "payload_bytes": 12, "build": nat.build_info(), "iters": a.iters, "gamma": gamma, "lambda": lam,
           "len": {"min": int(length.min()), "median": float(np.median(length)), "max": int(length.max()), "full": int((length == L).sum())},
           "live_slots": int(live.sum()), "slots": L * N,
           "ends": {"terminated": int((e & 1 != 0).sum()), "truncated": int((e & 2 != 0).sum()), "cut": int((e & 4 != 0).sum()), "boot": int((e & 8 != 0).sum())},
           "gae_equals_torch_loop_bit_for_bit": same, "gae_max_abs_difference": diff,
           "rollout_gather": timed(gather, a.iters, a.warmup), "rollout_gae": timed(gae, a.iters, a.warmup),
           "torch_loop_gae": timed(torch_loop, a.iters, 2)}
    res["gae_over_torch_loop"] = res["rollout_gae"]["median_us"] / res["torch_loop_gae"]["median_us"]
    pipe.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
