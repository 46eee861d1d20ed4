#!/usr/bin/env python3
"""tools/chunks_bench.py - what the minibatches of a recurrent-PPO epoch on a rollout (include/agx_chunks.h) cost, at N = 1024
envs, L = 128, chunks of C = 16 steps, minibatches of 256 chunks (4096 steps), four f32 streams (adv, ret, value, logp) and a
12-byte payload, on a history filled as tools/rollout_bench.py fills its own:

  (e) one epoch on the device, through the Python binding: Chunker.select and the N * ceil(L / C) / 256 = 32 Chunker.take;
  (E) the yardstick, today's path on the same arrays in the same process: the Rollout arrays viewed as [G][C][N], a nonzero over
      the chunk-live flags (the host waits for the count), torch.randperm, the start flags built in torch, and per minibatch one
      advanced-indexing read per array - obs_index, next_index, ends, start, live, the payload and the four streams.

(E) runs ceil(total / 256) minibatches - its count is data - (e) always 32, the chunks past the list invalid.  Every epoch sits
between a begin and an end event of its own on the stream, and so do select and one take alone; the figures are the median / min /
p90 over --iters repetitions after --warmup ((E): --torch-iters).  In the same process the two paths are checked to agree as sets
of (env, chunk, step, slot, start) rows.  Writes profiles/chunks_bench.json.

    python tools/chunks_bench.py [--iters 200] [--torch-iters 20] [--warmup 20] [--out profiles/chunks_bench.json]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "active-gym_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from rollout_bench import fill, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "chunks_bench.json"))
    a = ap.parse_args()
    from active_gym import FrameHistory, ObsPipeline, Rollout, StepLog
    from active_gym import _native as nat
    dev = torch.device("cuda:0")
    N, L, C, T, size = a.envs, a.length, a.chunk, a.capacity, a.size
    G = -(-L // C)
    pipe = ObsPipeline(N, "fixed", obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), resize_to_full=True, device=dev)
    hist = FrameHistory(pipe, T)
    log = StepLog(hist, 12)
    roll = Rollout(log)
    ch = roll.chunker(0)
    g = torch.Generator(device=dev).manual_seed(0)
    fill(pipe, hist, log, T + 40, g, dev)
    batch = roll.gather(L)
    names = ("adv", "ret", "value", "logp")
    streams = {k: torch.randn((L, N), device=dev, generator=g) for k in names}
    firsts = list(range(0, N * G, size))

    # (e) the device epoch, into the same output dicts every time
    ch.select(batch, C)
    outs = [ch.take(batch, first, size, C, streams=streams) for first in firsts]

    def epoch():
        ch.select(batch, C)
        for first, out in zip(firsts, outs):
            ch.take(batch, first, size, C, streams=streams, out=out)

    def select():
        ch.select(batch, C)

    def take():
        ch.take(batch, 0, size, C, streams=streams, out=outs[0])

    # (E) today's path
    pad = G * C - L

    def chunked(x):
        """[L, N, ...] -> [G, C, N, ...], zero-padded behind L."""
        if pad:
            x = torch.cat([x, x.new_zeros((pad,) + tuple(x.shape[1:]))])
        return x.view((G, C) + tuple(x.shape[1:]))

    def torch_epoch(keep=None):
        live, ends = batch["live"], batch["ends"]
        broke = torch.zeros_like(live)
        broke[1:] = ((ends[:-1] & 7) != 0) & live[:-1]            # an episode ended behind the live step before
        live_c = chunked(live)
        seen = live_c.to(torch.int32).cumsum(1)
        start = (live_c & (seen == 1)).to(torch.uint8) + chunked(live & broke).to(torch.uint8) * 2
        at = live_c.any(1).nonzero()                              # (the host waits for the count)
        gg, nn = at[:, 0], at[:, 1]
        order = torch.randperm(at.shape[0], device=dev)
        views = [chunked(batch[k]) for k in ("obs_index", "next_index", "ends", "payload")] + [start, live_c] + [chunked(s) for s in streams.values()]
        got = None
        for first in range(0, at.shape[0], size):
            rows = order[first:first + size]
            g_, n_ = gg[rows], nn[rows]
            got = [n_.to(torch.int32), g_.to(torch.int32)] + [v[g_, :, n_] for v in views]        # each [rows, C, ...]
            if keep is not None:
                keep.append(got)
        return got

    def keys(n, g_, l, slot, start):
        return (((n.long() * G + g_.long()) * C + l.long()) * (L * N + 1) + (slot.long() + 1)) * 4 + start.long()

    # the check: the valid chunks of one device epoch and one torch epoch are the same (env, chunk, step, slot, start) rows
    epoch()
    torch.cuda.synchronize()
    steps = torch.arange(C, device=dev)[:, None].expand(C, size)
    mine = []
    for o in outs:
        v = o["valid"].bool()
        mine.append(keys(o["env"][:, v], o["chunk"][None, v].expand(C, -1), steps[:, v], o["slot"][:, v], o["start"][:, v]).reshape(-1))
    mine = torch.cat(mine).sort().values
    kept = []
    torch_epoch(kept)
    theirs = []
    for n_, g_, obs_index, next_index, ends, payload, start, live, *_ in kept:
        l = torch.arange(C, device=dev)[None, :].expand(n_.shape[0], C)
        t = g_[:, None].long() * C + l
        slot = torch.where(live, t * N + n_[:, None].long(), torch.full_like(t, -1))
        theirs.append(keys(n_[:, None].expand(-1, C), g_[:, None].expand(-1, C), l, slot, start).reshape(-1))
    theirs = torch.cat(theirs).sort().values
    agree = bool(torch.equal(mine, theirs))
    total = int(ch.total().item())
    live_slots = int(batch["live"].sum().item())
    masked = int(sum(int(o["mask"].sum().item()) for o in outs))
    assert agree and masked == live_slots and total == sum(k[0].shape[0] for k in kept)

    res = {"envs": N, "L": L, "C": C, "capacity": T, "payload_bytes": 12, "size": size, "steps_per_minibatch": size * C, "f32_streams": len(names),
           "build": nat.build_info(), "iters": a.iters, "torch_iters": a.torch_iters, "chunks": total, "chunks_at_most": N * G, "live_slots": live_slots,
           "minibatches_device": len(firsts), "minibatches_torch": -(-total // size), "paths_agree_as_sets_of_chunk_step_rows": agree,
           "epoch_select_and_takes": timed(epoch, a.iters, a.warmup), "select_alone": timed(select, a.iters, a.warmup),
           "take_alone": timed(take, a.iters, a.warmup), "torch_epoch_view_nonzero_randperm_indexing": timed(torch_epoch, a.torch_iters, a.warmup)}
    res["epoch_over_torch_epoch"] = res["epoch_select_and_takes"]["median_us"] / res["torch_epoch_view_nonzero_randperm_indexing"]["median_us"]
    torch.cuda.synchronize()
    pipe.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
