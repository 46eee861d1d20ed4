#!/usr/bin/env python3
"""tools/minibatch_bench.py - what the minibatches of a PPO epoch on a rollout (include/agx_minibatch.h) cost, at N = 1024 envs,
L = 128, minibatches of 4096 rows, four f32 streams (adv, ret, value, logp) and a 12-byte payload, on a history filled as
tools/rollout_bench.py fills its own:

  (e) one epoch on the device: agx_minibatch_select and the 32 agx_minibatch_take of L * N / 4096 minibatches;
  (b) the BOOT list: select + take (4 * N rows: the scripted fill truncates often; no shuffle) + scatter of per-row values into boot_value;
  (E) the yardstick for (e), today's path on the same arrays: Rollout.flat (a nonzero, with its wait), torch.randperm, and per
      minibatch one advanced-indexing read per array - env, obs_index, next_index, the payload and the four streams;
  (B) the yardstick for (b): Rollout.boot_rows (a nonzero, with its wait) and the advanced-indexing scatter.

(E) runs ceil(live / 4096) minibatches - its count is data - (e) always L * N / 4096, the rows past the live slots invalid.
Every launch sequence sits between a begin and an end event of its own on the stream, and so do select, one take and the
scatter alone; the figures are the median / min / p90 over --iters repetitions after --warmup.  In the same process the valid
rows of (e) are checked to be (E)'s live slots, each once.  Writes profiles/minibatch_bench.json.

    python tools/minibatch_bench.py [--iters 200] [--warmup 20] [--out profiles/minibatch_bench.json]
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
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "minibatch_bench.json"))
    a = ap.parse_args()
    from active_gym import FrameHistory, ObsPipeline, Rollout, StepLog
    from active_gym import _native as nat
    dev = torch.device("cuda:0")
    N, L, T, size = a.envs, a.length, a.capacity, a.size
    pipe = ObsPipeline(N, "fixed", obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), resize_to_full=True, device=dev)
    hist = FrameHistory(pipe, T)
    log = StepLog(hist, 12)
    roll = Rollout(log)
    mb = roll.minibatcher(0)
    g = torch.Generator(device=dev).manual_seed(0)
    fill(pipe, hist, log, T + 40, g, dev)
    batch = roll.gather(L)
    names = ("adv", "ret", "value", "logp")
    streams = {k: torch.randn((L, N), device=dev, generator=g) for k in names}
    cells = L * N
    firsts = list(range(0, cells, size))

    # (e) the device epoch, into the same 32 output dicts every time
    mb.select(batch)
    outs = [mb.take(batch, first, size, streams=streams) for first in firsts]

    def epoch():
        mb.select(batch)
        for first, out in zip(firsts, outs):
            mb.take(batch, first, size, streams=streams, out=out)

    def select():
        mb.select(batch)

    def take():
        mb.take(batch, 0, size, streams=streams, out=outs[0])

    # (b) the BOOT list
    boot_value = torch.zeros((L, N), device=dev)
    cap = 4 * N
    mb.select(batch, "boot")
    boot_rows = mb.take(batch, 0, cap, which="boot", permute=False)
    critic = torch.randn((cap,), device=dev, generator=g)

    def boot():
        mb.select(batch, "boot")
        mb.take(batch, 0, cap, which="boot", permute=False, out=boot_rows)
        mb.scatter(boot_rows, critic, boot_value)

    def scatter():
        mb.scatter(boot_rows, critic, boot_value)

    # (E), (B) today's path
    payload = batch["payload"]

    def torch_epoch():
        at = batch["live"].nonzero()                          # (Rollout.flat's nonzero: the host waits for the count)
        t, n = at[:, 0], at[:, 1]
        order = torch.randperm(at.shape[0], device=dev)
        got = None
        for first in range(0, at.shape[0], size):
            rows = order[first:first + size]
            tt, nn = t[rows], n[rows]
            got = [nn.to(torch.int32), batch["obs_index"][tt, nn], batch["next_index"][tt, nn], payload[tt, nn]] + [s[tt, nn] for s in streams.values()]
        return got

    def torch_boot():
        at, env, index = roll.boot_rows(batch)
        boot_value[at[:, 0], at[:, 1]] = critic[:at.shape[0]]
        return env, index

    # the check: the valid rows of one device epoch are the live slots, each once, and carry their arrays
    epoch()
    torch.cuda.synchronize()
    slot = torch.cat([o["slot"] for o in outs])
    valid = torch.cat([o["valid"] for o in outs]).bool()
    live = batch["live"].reshape(-1).nonzero()[:, 0]
    covered = bool(torch.equal(slot[valid].long().sort().values, live))
    same = all(bool(torch.equal(torch.cat([o[k] for o in outs]).view(torch.int32), streams[k].reshape(-1)[slot.long()].view(torch.int32))) for k in names)
    same = same and bool(torch.equal(torch.cat([o["obs_index"] for o in outs]), batch["obs_index"].reshape(-1)[slot.long()]))
    assert covered and same and bool((slot >= 0).all())
    n_boot = int(mb.total("boot").item())
    assert n_boot == int(((batch["ends"] & 8) != 0).sum()) <= cap

    res = {"envs": N, "L": L, "capacity": T, "payload_bytes": 12, "size": size, "f32_streams": len(names), "build": nat.build_info(), "iters": a.iters,
           "slots": cells, "live_slots": int(live.numel()), "boot_slots": n_boot, "boot_capacity": cap, "minibatches_device": len(firsts),
           "minibatches_torch": -(-int(live.numel()) // size), "epoch_covers_every_live_slot_once": covered, "rows_equal_indexed_reads": same,
           "epoch_select_and_takes": timed(epoch, a.iters, a.warmup), "select_alone": timed(select, a.iters, a.warmup),
           "take_alone": timed(take, a.iters, a.warmup), "boot_select_take_scatter": timed(boot, a.iters, a.warmup),
           "scatter_alone": timed(scatter, a.iters, a.warmup), "torch_epoch_flat_randperm_indexing": timed(torch_epoch, a.iters, a.warmup),
           "torch_boot_rows_and_scatter": timed(torch_boot, a.iters, a.warmup)}
    res["epoch_over_torch_epoch"] = res["epoch_select_and_takes"]["median_us"] / res["torch_epoch_flat_randperm_indexing"]["median_us"]
    res["boot_over_torch_boot"] = res["boot_select_take_scatter"]["median_us"] / res["torch_boot_rows_and_scatter"]["median_us"]
    torch.cuda.synchronize()
    pipe.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
