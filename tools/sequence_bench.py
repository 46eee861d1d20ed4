#!/usr/bin/env python3
"""tools/sequence_bench.py - what sequence replay (include/agx_sequence.h) costs, at N = 1024, 84 x 84 / 30 x 30, fs = 4, resize
mode, a full history of T = 128 with a few resets, in float32 and bfloat16, for B = 64 / L = 64 and B = 16 / L = 256:

  (a) what a caller writes without it (its code is the parent commit's: the yardstick): the prefix mask from a known length in
      torch, torch.zeros of the whole [B * L, fs, h, w] batch and history.observe on the flattened, masked indices;
  (o) history.observe alone on the same indices, into a buffer that is already there;
  (b) agx_sequence_observe at planes = fs;
  (c) agx_sequence_observe at planes = 1;
  (d) agx_sequence_gather against its composition: agx_replay_inspect + the torch prefix mask + StepLog.gather on the flattened
      list; (l) agx_sequence_lengths alone.

In the same process (b) is checked against (a) and (d) against its composition, bit for bit.  Every launch sequence sits between
a begin and an end event of its own on the stream; the figures are the median / min / p90 over --iters repetitions after
--warmup.  Writes profiles/sequence_bench.json.

    python tools/sequence_bench.py [--iters 200] [--warmup 20] [--out profiles/sequence_bench.json]
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


def one_type(dtype, a, dev):
    from active_gym import FrameHistory, ObsPipeline, SequenceReplay, StepLog, replay
    N, fs, T, nstep, gamma = a.envs, 4, a.capacity, 5, 0.99
    pipe = ObsPipeline(N, "fixed", obs_size=(84, 84), frame_stack=fs, fov_size=(30, 30), resize_to_full=True, device=dev, obs_dtype=dtype)
    hist = FrameHistory(pipe, T)
    log = StepLog(hist, 12)
    seq = SequenceReplay(log)
    g = torch.Generator(device=dev).manual_seed(0)
    for _ in range(T + fs):                       # fill the history; about one env-step in 50 starts a new episode
        cmd = torch.full((N,), 2, dtype=torch.uint8, device=dev) | ((torch.rand((N,), device=dev, generator=g) < 0.02).to(torch.uint8) * 4)
        pipe.ingest_gray(torch.randint(0, 256, (N, 2, 84, 84), dtype=torch.uint8, device=dev, generator=g), cmd)
        pipe.fovea(torch.rand((N, 2), device=dev, generator=g) * 54)
        index = hist.push(cmd)
        log.record(index, torch.randn((N,), device=dev, generator=g), (torch.rand((N,), device=dev, generator=g) < 0.02).to(torch.uint8),
                   torch.randint(0, 256, (N, 12), dtype=torch.uint8, device=dev, generator=g))
    count = int(hist.last_index()[0]) + 1
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    out = {}
    for B, L in ((64, 64), (16, 256)):
        env = torch.randint(0, N, (B,), dtype=torch.int32, device=dev, generator=g)
        idx = torch.randint(count - T + fs - 1, count, (B,), dtype=torch.int64, device=dev, generator=g)
        length = seq.lengths(env, idx, L)
        steps = torch.arange(L, device=dev)
        row = hist.obs_row_shape("fovea")
        buf = torch.empty((B * L,) + row, dtype=dtype, device=dev)
        loc = torch.empty((B * L, 2), dtype=torch.int32, device=dev)
        val = torch.empty((B * L,), dtype=torch.uint8, device=dev)
        full = torch.empty((B, L) + row, dtype=dtype, device=dev)
        one = torch.empty((B, L, 1) + row[1:], dtype=dtype, device=dev)
        sloc = torch.empty((B, L, 2), dtype=torch.int32, device=dev)
        slive = torch.empty((B, L), dtype=torch.uint8, device=dev)

        def flatten(length):
            live = steps[None, :] < length[:, None]
            fe = torch.where(live, env[:, None], -1).reshape(-1).to(torch.int32)
            fi = torch.where(live, idx[:, None] + steps[None, :], -1).reshape(-1)
            return fe, fi, live

        fe0, fi0, live0 = flatten(length)

        def today():
            fe, fi, live = flatten(length)
            batch = torch.zeros((B * L,) + row, dtype=dtype, device=dev)
            hist.observe(fe, fi, out=batch, loc_out=loc, valid_out=val)
            return batch, live

        def observe_alone():
            hist.observe(fe0, fi0, out=buf, loc_out=loc, valid_out=val)

        def seq_full():
            seq.observe(env, idx, length, L, out=full, loc_out=sloc, live_out=slive)

        def seq_one():
            seq.observe(env, idx, length, L, planes=1, out=one, loc_out=sloc, live_out=slive)

        def seq_lengths():
            seq.lengths(env, idx, L, out=length)

        def seq_gather():
            return seq.gather(env, idx, L, nstep, gamma)

        def composed():
            ahead = replay.inspect(hist, env, idx)[1]
            n = torch.where(ahead < 0, 0, 1 + ahead.clamp(max=L - 1)).to(torch.int32)
            fe, fi, _ = flatten(n)
            rows = log.gather(fe, fi, nstep, gamma)
            rows["length"] = n
            return rows

        batch, live = today()
        seq_full()
        seq_one()
        assert torch.equal(full.view(bits).reshape(batch.shape), batch.view(bits)), "agx_sequence_observe differs from zeros + observe"
        assert torch.equal(one.view(bits).reshape(B * L, *row[1:]), batch.view(bits)[:, fs - 1]), "planes = 1 is not the newest frame"
        assert torch.equal(slive.bool(), live)
        got, want = seq_gather(), composed()
        for key, t in want.items():
            gt = got[key].reshape(t.shape)
            assert torch.equal(gt.view(torch.int32) if t.dtype == torch.float32 else gt, t.view(torch.int32) if t.dtype == torch.float32 else t), key
        del batch
        res = {"live_steps": int(live.sum()), "rows": B * L, "batch_bytes": int(full.numel() * full.element_size()),
               "today": timed(today, a.iters, a.warmup), "observe_alone": timed(observe_alone, a.iters, a.warmup),
               "sequence_observe": timed(seq_full, a.iters, a.warmup), "sequence_observe_planes1": timed(seq_one, a.iters, a.warmup),
               "sequence_lengths": timed(seq_lengths, a.iters, a.warmup), "sequence_gather": timed(seq_gather, a.iters, a.warmup),
               "inspect_gather_mask": timed(composed, a.iters, a.warmup)}
        med = {k: v["median_us"] for k, v in res.items() if isinstance(v, dict)}
        res["observe_spread_us"] = res["observe_alone"]["p90_us"] - med["observe_alone"]
        res["sequence_minus_observe_us"] = med["sequence_observe"] - med["observe_alone"]
        res["sequence_over_today"] = med["sequence_observe"] / med["today"]
        res["planes1_over_sequence"] = med["sequence_observe_planes1"] / med["sequence_observe"]
        res["byte_ratio"] = 1.0 / fs
        res["gather_over_composition"] = med["sequence_gather"] / med["inspect_gather_mask"]
        out[f"B{B}_L{L}"] = res
        del buf, full, one
    pipe.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=128)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sequence_bench.json"))
    a = ap.parse_args()
    from active_gym import _native as nat
    dev = torch.device("cuda:0")
    res = {"envs": a.envs, "capacity": a.capacity, "build": nat.build_info(), "iters": a.iters}
    for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
        res[name] = one_type(dtype, a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
