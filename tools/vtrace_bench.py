#!/usr/bin/env python3
"""tools/vtrace_bench.py - what V-trace over a gathered rollout (include/agx_vtrace.h) costs, at N = 1024 envs, L = 128, on the
scripted history of tools/rollout_bench.py (T = 256, autoresets with TERMINATED and TRUNCATED, resets nothing announced, a few
rows never recorded, 84 x 84 / 30 x 30, fs = 4, a 12-byte payload):

  (v) agx_vtrace_returns on the gathered arrays, rho = exp(0.3 z): about half of the ratios are cut at the levels 1 / 1 / 1;
  (a) agx_rollout_gae on the same arrays in the same process: the yardstick - V-trace moves 25 bytes per slot where GAE moves 21;
  (t) the usual torch loop over t = L - 1 .. 0 for V-trace on the same device arrays, its masks (BOOT, TERMINATED, the chain
      breaks, the live slots) computed once outside the timed region, the clipped ratios inside it.

In the same process (v) is checked against (t): the loop rounds in the same order, so the two are compared bit for bit.  Every
launch sits between a begin and an end event of its own on the stream; the figures are the median / min / p90 over --iters
repetitions after --warmup.  Writes profiles/vtrace_bench.json.

    python tools/vtrace_bench.py [--iters 200] [--warmup 20] [--out profiles/vtrace_bench.json]

The set depth of k_slot_fold<VtraceFold> is a compile-time constant (AGX_VTRACE_AHEAD, 8; GAE's is AGX_GAE_AHEAD, 16).  To measure another one, build a library of its own
and select it through AGX_LIB; --set-depth only labels the result:

    python -c "import sys; sys.path.insert(0, 'active-gym_amd'); import build; \\
               build.build(extra=('-DAGX_VTRACE_AHEAD=16',), out=build.OUT_DIR + '/libagx_vtrace16.so')"
    AGX_LIB=active-gym_amd/lib/libagx_vtrace16.so python tools/vtrace_bench.py --set-depth 16 --out profiles/vtrace_bench_depth16.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "active-gym_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rollout_bench import fill, timed  # noqa: E402  (the same scripted history and the same timing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--set-depth", type=int, default=8, help="label: the AGX_VTRACE_AHEAD the loaded library was built with")
    ap.add_argument("--busy", type=int, default=40, help="torch loops run before anything is timed (about 0.4 s of launches)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vtrace_bench.json"))
    a = ap.parse_args()
    from active_gym import FrameHistory, ObsPipeline, Rollout, StepLog, VTrace
    from active_gym import _native as nat
    from active_gym.rollout import BOOT, TERMINATED
    dev = torch.device("cuda:0")
    N, L, T, gamma, lam, bars = a.envs, a.length, a.capacity, 0.99, 1.0, (1.0, 1.0, 1.0)
    pipe = ObsPipeline(N, "fixed", obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), resize_to_full=True, device=dev)
    hist = FrameHistory(pipe, T)
    log = StepLog(hist, 12)
    roll, vt = Rollout(log), VTrace(log)
    g = torch.Generator(device=dev).manual_seed(0)
    fill(pipe, hist, log, T + 40, g, dev)
    batch = roll.gather(L)
    value = torch.randn((L, N), device=dev, generator=g)
    boot = torch.randn((L, N), device=dev, generator=g)
    rho = torch.exp(0.3 * torch.randn((L, N), device=dev, generator=g))
    vs, pg = vt.returns(batch, value, boot, rho, gamma, lam, *bars)
    adv, ret = roll.gae(batch, value, boot, gamma, lam)

    def vtrace():
        vt.returns(batch, value, boot, rho, gamma, lam, *bars, vs_out=vs, pg_adv_out=pg)

    def gae():
        roll.gae(batch, value, boot, gamma, lam, adv_out=adv, ret_out=ret)

    def vtrace_no_boot():                         # k_slot_fold<VtraceFold, false>: one stream fewer, 21 bytes per slot (the values are not used)
        vt.returns(batch, value, None, rho, gamma, lam, *bars, vs_out=vs, pg_adv_out=pg)

    def gae_no_boot():                            # k_slot_fold<GaeFold, false>: 17 bytes per slot
        roll.gae(batch, value, None, gamma, lam, adv_out=adv, ret_out=ret)

    ends, reward, live = batch["ends"], batch["reward"], batch["live"]
    is_boot, is_term = (ends & BOOT) != 0, (ends & TERMINATED) != 0
    go = (ends & 7) == 0
    go[L - 1] = False
    zero = torch.zeros((N,), device=dev)
    t_A, t_pg = torch.empty((L, N), device=dev), torch.empty((L, N), device=dev)
    bar = [torch.full((), b, device=dev) for b in bars]

    def torch_loop():
        rho_c, rho_pg = torch.where(rho < bar[0], rho, bar[0]), torch.where(rho < bar[2], rho, bar[2])
        gcc = gamma * (lam * torch.where(rho < bar[1], rho, bar[1]))
        last = zero
        for t in range(L - 1, -1, -1):
            nv = torch.where(is_boot[t], boot[t], torch.where(is_term[t], zero, value[t + 1] if t < L - 1 else zero))
            carry = torch.where(go[t], last, zero)
            td = reward[t] + gamma * nv - value[t]
            last = torch.where(live[t], rho_c[t] * td + gcc[t] * carry, zero)
            t_A[t] = last
            t_pg[t] = rho_pg[t] * (reward[t] + gamma * (nv + carry) - value[t])
        return torch.where(live, t_A + value, zero), torch.where(live, t_pg, zero)

    for _ in range(a.busy):                       # an idle device: without this the first timed block of a process read 31 - 33 us
        torch_loop()                              # (median) where the same launches read 21 us a block later
    w_vs, w_pg = torch_loop()
    same =bool(torch.equal(vs.view(torch.int32), w_vs.view(torch.int32)) and torch.equal(pg.view(torch.int32), w_pg.view(torch.int32)))
    diff = float(torch.maximum((vs - w_vs).abs().max(), (pg - w_pg).abs().max()))
    assert torch.allclose(vs, w_vs, rtol=1e-4, atol=1e-4) and torch.allclose(pg, w_pg, rtol=1e-4, atol=1e-4), diff
    length = batch["len"].cpu().numpy()
    e = ends[live].cpu().numpy()
    res = {"envs": N, "L": L, "capacity": T, "build": nat.build_info(), "library": os.path.basename(os.environ.get("AGX_LIB", nat.LIB_PATH)),
           "set_depth": a.set_depth, "iters": a.iters, "gamma": gamma, "lambda": lam, "levels": list(bars),
           "rho": {"min": float(rho.min()), "median": float(rho.median()), "max": float(rho.max()), "above_1": float((rho > 1).float().mean())},
           "len": {"min": int(length.min()), "median": float(np.median(length)), "max": int(length.max()), "full": int((length == L).sum())},
           "live_slots": int(live.sum()), "slots": L * N,
           "ends": {"terminated": int((e & 1 != 0).sum()), "truncated": int((e & 2 != 0).sum()), "cut": int((e & 4 != 0).sum()), "boot": int((e & 8 != 0).sum())},
           "vtrace_equals_torch_loop_bit_for_bit": same, "vtrace_max_abs_difference": diff,
           "vtrace_returns": timed(vtrace, a.iters, a.warmup), "rollout_gae": timed(gae, a.iters, a.warmup),
           "vtrace_returns_again": timed(vtrace, a.iters, a.warmup),
           "vtrace_returns_no_boot": timed(vtrace_no_boot, a.iters, a.warmup), "rollout_gae_no_boot": timed(gae_no_boot, a.iters, a.warmup),
           "torch_loop_vtrace": timed(torch_loop, a.iters, 2)}
    y = res["rollout_gae"]
    res["bytes_per_slot"] = {"vtrace": 25, "gae": 21}
    res["expected_median_us"] = y["median_us"] * 25 / 21 + (y["p90_us"] - y["median_us"])
    res["vtrace_over_gae"] = res["vtrace_returns"]["median_us"] / y["median_us"]
    res["vtrace_over_torch_loop"] = res["vtrace_returns"]["median_us"] / res["torch_loop_vtrace"]["median_us"]
    pipe.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
