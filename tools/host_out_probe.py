"""Host (NumPy) outputs at N = 1024, fixed kind, headline geometry (84 x 84, fov 30 x 30, resize_to_full), one process, one GPU.

Default run: ms per AtariVecEnv.step of the unchunked path (args.host_obs_chunks = 0) and of the chunked host-output step with
C = 2, 4, 8 (agx_loop_step_host), INTERLEAVED in rounds so that drift hits all of them alike, for gray and RGB screens; the same
run's bare pinned H2D / D2H rates and emulator time, and the floor they give: max(H2D time, D2H time) + emulator time.  Medians
over >= 200 steps per variant after warm-up; the spread reported is that of the per-round medians.  Writes JSON (--out).

    python tools/host_out_probe.py --out profiles/host_chunks.json

--outputs-cost: the older table (profiles/r04_host_outputs.txt): fresh pageable arrays / pooled pinned / pinned pair / device outputs.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "active-gym_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from active_gym import AtariEnvArgs, AtariVecEnv  # noqa: E402
from active_gym import _native as nat  # noqa: E402

N = 1024
ACT = {"motor_action": np.zeros(N, np.int64), "sensory_action": np.full((N, 2), 20.0, np.float32)}


def make(fmt, device=None, **over):
    kw = dict(frame_format=fmt, game="breakout", seed=1, obs_size=(84, 84), fov_size=(30, 30), fov_init_loc=(0, 0),
              sensory_action_mode="absolute", resize_to_full=True, frame_source="native", device=device,
              scripted_lives=3, scripted_p_life=6, scripted_p_over=1)
    kw.update(over)
    env = AtariVecEnv(AtariEnvArgs(**kw), N, kind="fixed")
    env.reset()
    return env


def copy_rate(nbytes, h2d, reps=12):
    """GB/s of one pinned <-> device copy of nbytes (median; the first copies map the fresh pinned buffer: not timed)."""
    h = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    d = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    ts = []
    for k in range(reps + 3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        (d if h2d else h).copy_(h if h2d else d, non_blocking=True)
        torch.cuda.synchronize()
        if k >= 3:
            ts.append(time.perf_counter() - t)
    return nbytes / statistics.median(ts) / 1e9


def chunks_probe(out, rounds, per_round, warm):
    result = {"build": nat.build_info(), "device": torch.cuda.get_device_name(0), "N": N, "kind": "fixed",
              "geometry": "obs 84x84, fov 30x30, resize_to_full, frame_stack 4, float32", "steps_per_variant": rounds * per_round,
              "formats": {}}
    d2h_bytes = N * 4 * 84 * 84 * 4
    for fmt in ("gray", "rgb"):
        envs = {c: make(fmt, host_obs_chunks=c) for c in (0, 2, 4, 8)}
        for c, e in envs.items():
            assert e.host_obs_chunks == c
            for _ in range(warm):
                e.step(ACT)
        per = {c: [] for c in envs}            # per-round medians (ms)
        every = {c: [] for c in envs}
        for _ in range(rounds):
            for c, e in envs.items():
                ts = []
                for _ in range(per_round):
                    t = time.perf_counter()
                    e.step(ACT)
                    ts.append((time.perf_counter() - t) * 1e3)
                per[c].append(statistics.median(ts))
                every[c] += ts
        # the emulators alone (the unchunked env's runner writes its own pinned staging), and this format's H2D bytes
        e0 = envs[0]
        h2d_bytes = int(e0._staging.h_frames.numel()) + N
        motor = np.zeros(N, np.int64)
        ts = []
        for _ in range(60):
            t = time.perf_counter()
            e0.runner.step(motor)
            ts.append((time.perf_counter() - t) * 1e3)
        emu_ms = statistics.median(ts[10:])
        for e in envs.values():
            e.close()
        h2d_rate, d2h_rate = copy_rate(h2d_bytes, True), copy_rate(d2h_bytes, False)
        floor_ms = max(h2d_bytes / h2d_rate, d2h_bytes / d2h_rate) / 1e6 + emu_ms
        rec = {"h2d_bytes": h2d_bytes, "d2h_bytes": d2h_bytes, "h2d_GBps": round(h2d_rate, 2), "d2h_GBps": round(d2h_rate, 2),
               "emulator_ms": round(emu_ms, 3), "floor_ms": round(floor_ms, 3), "hoped_for_ms": {"gray": 2.6, "rgb": 3.3}[fmt],
               "ms_per_step": {}}
        for c in envs:
            rec["ms_per_step"][f"C={c}"] = {"median": round(statistics.median(every[c]), 3), "round_medians_min": round(min(per[c]), 3),
                                           "round_medians_max": round(max(per[c]), 3)}
        base = rec["ms_per_step"]["C=0"]
        rec["spread_ms"] = round(max(v["round_medians_max"] - v["round_medians_min"] for v in rec["ms_per_step"].values()), 3)
        best = min((c for c in envs if c), key=lambda c: rec["ms_per_step"][f"C={c}"]["median"])
        rec["best"] = {"C": best, "median_ms": rec["ms_per_step"][f"C={best}"]["median"],
                       "gain_over_C0_ms": round(base["median"] - rec["ms_per_step"][f"C={best}"]["median"], 3),
                       "above_floor_ms": round(rec["ms_per_step"][f"C={best}"]["median"] - floor_ms, 3),
                       "above_hoped_for_ms": round(rec["ms_per_step"][f"C={best}"]["median"] - rec["hoped_for_ms"], 3)}
        result["formats"][fmt] = rec
        print(fmt, json.dumps(rec), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return result


def outputs_cost():
    for dev, copy, nbuf in ((None, True, 0), (None, True, 4), (None, False, 0), ("cuda:0", False, 0)):
        env = make("gray", device=dev, copy_obs=copy, host_obs_buffers=nbuf)
        K = 30 if (dev is None and copy and not nbuf) else 200
        for _ in range(20):
            env.step(ACT)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(K):
            o = env.step(ACT)[0]
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / K
        print(f"device={dev} copy_obs={copy} host_obs_buffers={nbuf}: {dt*1e3:.2f} ms/step, {N/dt/1e6:.3f} M env steps/s, obs {type(o).__name__}", flush=True)
        env.close()
    x = torch.empty((N, 4, 84, 84), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(5):
        x.cpu()
    print(f".cpu() (pageable): {(time.perf_counter()-t)/5*1e3:.2f} ms")
    print(f"pinned D2H: {copy_rate(x.numel() * 4, False):.1f} GB/s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--outputs-cost", action="store_true")
    a = ap.parse_args()
    if a.outputs_cost:
        outputs_cost()
    else:
        chunks_probe(a.out, a.rounds, a.per_round, a.warmup)
