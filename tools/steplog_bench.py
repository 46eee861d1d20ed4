#!/usr/bin/env python3
"""tools/steplog_bench.py - what the step log (include/agx_steplog.h) costs, at N = 1024, 84 x 84 / 30 x 30, fs = 4, a full
history of T = 64 with every row recorded, for B = 256 / 4096 / 32768 sampled rows and nstep = 1 / 5:

  (a) agx_steplog_gather of B samples     one launch into outputs that exist ("gather"); and StepLog.gather, which also allocates
                                          and zero-fills its six outputs ("gather_py": the like-for-like of (b));
  (b) the composition a caller writes     replay.inspect for `ahead`, then torch advanced indexing over the caller's own [T, N]
      today                               reward / flags tensors with an nstep-long masked loop, in the same process; its
                                          steps / next_index / ret / discount are checked EQUAL to (a)'s (ret, discount as bits);
  (c) history.observe of the same B       what the rows are gathered for;
  (d) AtariVecEnv.step end to end         N = 1024 gray screens, native loop, history_len = 64, with and without step_log: two envs
                                          in one process, timed in alternating windows of >= 0.35 s on the host clock, each window
                                          closed by a device synchronisation.

(a) - (c) sit between a begin and an end event of their own on the stream; each figure is the median (with min and p90) over
--iters repetitions after --warmup.  The yardsticks are ratios inside one run: gather_over_composition, gather_over_observe and
step_log_over_step.  Writes profiles/steplog_bench.json.

    python tools/steplog_bench.py [--iters 200] [--warmup 20] [--capacity 64] [--no-e2e] [--out profiles/steplog_bench.json]
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


def compose(hist, env, idx, reward, flags, nstep, gamma, T):
    """The n-step rows as a caller builds them from replay.inspect and its own [T, N] tensors: every product and every sum is an
    op of its own, so the float32 results carry the same roundings as the library's fold."""
    from active_gym.replay import inspect
    _, ahead = inspect(hist, env, idx)
    e = env.clamp(min=0).long()
    alive = ahead >= 0
    G = torch.zeros(env.shape, dtype=torch.float32, device=env.device)
    disc = torch.ones_like(G)
    m = torch.zeros_like(ahead)
    last = torch.zeros(env.shape, dtype=torch.uint8, device=env.device)
    for i in range(1, nstep + 1):
        alive = alive & (ahead >= i)
        row = (idx + i).clamp(min=0) % T
        r, f = reward[row, e], flags[row, e]
        G = torch.where(alive, G + disc * r, G)
        disc = torch.where(alive, disc * gamma, disc)
        m = torch.where(alive, torch.full_like(m, i), m)
        last = torch.where(alive, f, last)
        alive = alive & ((f & 3) == 0)
    discount = torch.where(((last & 1) != 0) | (m == 0), torch.zeros_like(disc), disc)
    return G, discount, m, torch.where(m > 0, idx + m, torch.full_like(idx, -1))


def bench_e2e(N, T, window_s=0.35, repeats=3):
    from active_gym import AtariEnvArgs, AtariVecEnv
    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    envs = {}
    for name, on in (("step", False), ("step_log", True)):
        args = AtariEnvArgs(frame_format="gray", game="breakout", seed=1, obs_size=(84, 84), fov_size=(30, 30), fov_init_loc=(0, 0),
                            sensory_action_mode="absolute", resize_to_full=True, frame_source="native", device="cuda:0", num_workers=workers,
                            h2d_chunk_envs=0, scripted_lives=3, scripted_p_life=6, scripted_p_over=1, history_len=T, step_log=on)
        envs[name] = AtariVecEnv(args, N, kind="fixed")
        envs[name].reset()
    act = {"motor_action": np.zeros(N, np.int64), "sensory_action": torch.full((N, 2), 20.0, dtype=torch.float32, device="cuda:0")}
    steps = {}
    for name, env in envs.items():
        for _ in range(8):
            env.step(act)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(8):
            env.step(act)
        torch.cuda.synchronize()
        steps[name] = max(16, int(window_s / max((time.perf_counter() - t0) / 8, 1e-4)) + 1)
    times = {name: [] for name in envs}
    for _ in range(repeats):
        for name, env in envs.items():           # alternating: both see the same minutes of a shared host
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps[name]):
                env.step(act)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps[name] * 1e3)
    out = {"envs": N, "workers": workers, "history_len": T, "loop": "native" if envs["step"]._loop is not None else "python",
           "steps_per_window": steps, "repeats": repeats}
    for name, env in envs.items():
        out[name] = {"ms_per_step_median": float(np.median(times[name])), "ms_per_step_min": float(min(times[name])), "ms_per_step_all": times[name]}
        env.close()
    out["step_log_over_step"] = out["step_log"]["ms_per_step_median"] / out["step"]["ms_per_step_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096, 32768])
    ap.add_argument("--nsteps", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "steplog_bench.json"))
    a = ap.parse_args()
    from active_gym import FrameHistory, ObsPipeline, ReplaySampler, StepLog
    from active_gym import _native as nat
    from active_gym import steplog as sl
    import ctypes
    P, lib = ctypes.c_void_p, sl.lib()
    dev = torch.device("cuda:0")
    N, fs, T = a.envs, 4, a.capacity
    pipe = ObsPipeline(N, "fixed", obs_size=(84, 84), frame_stack=fs, fov_size=(30, 30), resize_to_full=True, device=dev)
    hist = FrameHistory(pipe, T)
    log = StepLog(hist, 4)
    g = torch.Generator(device=dev).manual_seed(0)
    cmd = torch.full((N,), 2, dtype=torch.uint8, device=dev)
    my_reward = torch.zeros((T, N), dtype=torch.float32, device=dev)          # the caller's own columns, for (b)
    my_flags = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    cols = torch.arange(N, device=dev)
    for _ in range(T + fs):                       # fill the history and the log: every retained row is recorded
        pipe.ingest_gray(torch.randint(0, 256, (N, 2, 84, 84), dtype=torch.uint8, device=dev, generator=g), cmd)
        pipe.fovea(torch.rand((N, 2), device=dev, generator=g) * 54)
        index = hist.push(cmd)
        rew = torch.randn((N,), device=dev, generator=g) * 3
        flg = (torch.rand((N,), device=dev, generator=g) < 0.05).to(torch.uint8)          # TERMINATED
        log.record(index, rew, flg, torch.randint(0, 256, (N, 4), dtype=torch.uint8, device=dev, generator=g))
        my_reward[index % T, cols], my_flags[index % T, cols] = rew, flg
    smp = ReplaySampler(hist, back=0, forward=1, seed=0)
    res = {"envs": N, "capacity": T, "payload_bytes": 4, "gamma": a.gamma, "build": nat.build_info(), "iters": a.iters, "log_bytes": log.bytes(),
           "batches": {}}
    for B in a.batches:
        env, idx, ok = smp.sample(B)
        out = torch.empty((B,) + hist.obs_row_shape(), dtype=torch.float32, device=dev)
        loc = torch.empty((B, 2), dtype=torch.int32, device=dev)
        val = torch.empty((B,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert int(ok.sum()) >= 0.99 * B, "the benchmark's samples must be accepted"

        def observe():
            hist.observe(env, idx, out=out, loc_out=loc, valid_out=val)

        r = {"accepted": int(ok.sum()), "observe": timed(observe, a.iters, a.warmup)}
        for nstep in a.nsteps:
            def gather_py():
                return log.gather(env, idx, nstep, a.gamma)

            def gather():                         # the entry point alone, into outputs that exist: one launch
                lib.agx_steplog_gather(log._s, *ptr[:2], B, nstep, a.gamma, *ptr[2:], pipe._stream())

            def composition():
                return compose(hist, env, idx, my_reward, my_flags, nstep, a.gamma, T)

            got, (G, discount, m, nxt) = gather_py(), composition()
            ptr = [P(t.data_ptr()) for t in (env, idx, got["ret"], got["discount"], got["steps"], got["next_index"], got["flags"], got["payload"])]
            torch.cuda.synchronize()
            assert torch.equal(got["steps"], m) and torch.equal(got["next_index"], nxt), "the composition's steps differ from gather's"
            assert torch.equal(got["ret"].view(torch.int32), G.view(torch.int32)), "the composition's returns differ from gather's"
            assert torch.equal(got["discount"].view(torch.int32), discount.view(torch.int32)), "the composition's discounts differ from gather's"
            q = {"steps_mean": float(m.float().mean()), "gather": timed(gather, a.iters, a.warmup), "gather_py": timed(gather_py, a.iters, a.warmup),
                 "composition": timed(composition, a.iters, a.warmup)}
            q["gather_over_composition"] = q["gather"]["median_us"] / q["composition"]["median_us"]
            q["gather_py_over_composition"] = q["gather_py"]["median_us"] / q["composition"]["median_us"]
            q["gather_over_observe"] = q["gather"]["median_us"] / r["observe"]["median_us"]
            r[f"nstep_{nstep}"] = q
        res["batches"][str(B)] = r
    pipe.close()
    if not a.no_e2e:
        res["e2e"] = bench_e2e(N, T)
        res["step_log_over_step"] = res["e2e"]["step_log_over_step"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
