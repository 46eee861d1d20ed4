#!/usr/bin/env python3
"""tools/obs_dtype_bench.py [--n 1024] [--steps 300] [--out profiles/obs16] [--no-rocprof] - the 16-bit observation outputs
(obs_dtype bfloat16 / float16) against float32 at N envs on the headline geometry (84x84, fov 30x30, frame_stack 4).

Per kernel and element type: the fovea kernel's own begin / end (agx_profile_next events, every 4th step of an ingest + fovea
loop; median) for K2 in resize, mask and raw modes, K3 (peripheral 20x20) with antialias 0 and 1 and K4 (flexible, resize);
k_full (the base kind's observation; back-to-back launches between stream events, per launch); and the whole agx_step_fixed
step (K1 + K2 resize, back to back between stream events, per step).  Each line carries the algorithmic bytes and their
fraction of 8 TB/s.  Then the same loops once more under `rocprofv3 --kernel-trace --stats` (a child process) for the
profiler's per-kernel durations.  Writes <out>_bench.json (one JSON object per line) and <out>_kernel_stats.csv."""
import argparse, glob, json, os, shutil, statistics, subprocess, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "active-gym_amd"), REPO]
import torch
import bench
from active_gym import ObsPipeline

DTYPES = ("float32", "bfloat16", "float16")
CASES = [("fixed", "resize", 1), ("fixed", "mask", 1), ("fixed", "raw", 1), ("peripheral", "resize", 0), ("peripheral", "resize", 1),
         ("flexible", "resize", 1)]


def pipeline(kind, mode, aa, n, dt, dev):
    kw = dict(num_envs=n, kind=kind, obs_size=(84, 84), frame_stack=4, device=dev, obs_dtype=dt)
    if kind != "base":
        kw.update(fov_size=(30, 30), fov_init_loc=(0, 0), sensory_action_mode="absolute", antialias=bool(aa),
                  resize_to_full=mode == "resize", mask_out=mode == "mask")
    if kind == "peripheral":
        kw["peripheral_res"] = (20, 20)
    return ObsPipeline(**kw)


def fovea_kernel_us(pipe, inp, steps, types=None):
    frames, cmds, acts = inp
    n = pipe.num_envs
    obs = torch.empty(pipe.obs_shape, dtype=pipe.obs_dtype, device=pipe.device)
    loc = torch.empty((n, 2), dtype=torch.int32, device=pipe.device)
    res = torch.empty((n, 2), dtype=torch.int32, device=pipe.device)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps // 4 + 1)]
    for a, b in ev:                    # a recorded event has a handle
        a.record()
        b.record()
    armed = []
    for k in range(steps + 50):
        i = k % len(frames)
        pipe.ingest(frames[i], cmds[i])
        if k >= 50 and k % 4 == 0:
            e = ev[len(armed)]
            pipe.profile_next("fovea", e[0], e[1])
            armed.append(e)
        if pipe.kind == "flexible":
            pipe.fovea(acts[i], action_type=types[i], out=obs, loc_out=loc, res_out=res)
        else:
            pipe.fovea(acts[i], out=obs, loc_out=loc)
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in armed)


def back_to_back_us(fn, steps):
    for k in range(50):
        fn(k)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(steps):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def run(args):
    dev = torch.device("cuda:0")
    n = args.n
    inp = bench.synth_inputs(torch, dev, n, 4, 1234)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    types = [torch.randint(0, 2, (n,), dtype=torch.int32, device=dev, generator=g) for _ in range(4)]
    facts = [torch.where(types[i][:, None] == 1, torch.randint(10, 61, (n, 2), device=dev, generator=g).float(), inp[2][i]).contiguous()
             for i in range(4)]
    rows = []

    def emit(row):
        row["gbps_frac"] = round(row["bytes"] / (row["us"] * 1e-6) / 8e12, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)

    for kind, mode, aa in CASES:
        for dt in DTYPES:
            p = pipeline(kind, mode, aa, n, dt, dev)
            us = fovea_kernel_us(p, (inp[0], inp[1], facts if kind == "flexible" else inp[2]), args.steps, types)
            emit(dict(kernel={"fixed": "K2", "peripheral": "K3", "flexible": "K4"}[kind], kind=kind, mode=mode, antialias=aa, dtype=dt,
                      n=n, us=round(us, 2), bytes=p.algorithmic_bytes("fovea")))
            p.close()
    for dt in DTYPES:
        p = pipeline("base", None, 1, n, dt, dev)
        p.ingest(inp[0][0], inp[1][0])
        out = torch.empty(p.full_shape, dtype=p.obs_dtype, device=dev)
        us = back_to_back_us(lambda k: p.observe_full(out), args.steps)
        emit(dict(kernel="k_full", kind="base", mode=None, antialias=None, dtype=dt, n=n, us=round(us, 2), bytes=p.algorithmic_bytes("full")))
        p.close()
    for dt in DTYPES:
        p = pipeline("fixed", "resize", 1, n, dt, dev)
        out = torch.empty(p.obs_shape, dtype=p.obs_dtype, device=dev)
        loc = torch.empty((n, 2), dtype=torch.int32, device=dev)
        us = back_to_back_us(lambda k: p.step_fixed(inp[0][k % 4], inp[1][k % 4], inp[2][k % 4], out=out, loc_out=loc), args.steps)
        emit(dict(kernel="agx_step_fixed", kind="fixed", mode="resize", antialias=1, dtype=dt, n=n, us=round(us, 2),
                  bytes=p.algorithmic_bytes("ingest") + p.algorithmic_bytes("fovea"), env_steps_per_s=round(n / (us * 1e-6))))
        p.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "obs16"))
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--inner", action="store_true", help="(the rocprofv3 child: run the loops, write nothing)")
    args = ap.parse_args()
    if args.inner:
        run(args)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    t0 = time.time()
    rows = run(args)
    by = {(r["kernel"], r["mode"], r["antialias"], r["dtype"]): r["us"] for r in rows}
    print("\n| kernel | mode | aa | f32 us | bf16 us (x f32) | f16 us (x f32) |\n|---|---|---|---|---|---|")
    for key in dict.fromkeys((r["kernel"], r["mode"], r["antialias"]) for r in rows):
        f = by[key + ("float32",)]
        print(f"| {key[0]} | {key[1]} | {key[2]} | {f:.2f} | " + " | ".join(f"{by[key + (d,)]:.2f} ({by[key + (d,)] / f:.2f})"
                                                                       for d in ("bfloat16", "float16")) + " |")
    with open(args.out + "_bench.json", "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    print(f"wrote {args.out}_bench.json ({time.time() - t0:.0f} s)")
    if args.no_rocprof or not shutil.which("rocprofv3"):
        return
    d = tempfile.mkdtemp(prefix="obs16_rocprof_")
    cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--inner", "--n", str(args.n), "--steps", str(min(args.steps, 100))]
    rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
    stats = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if rc != 0 or not stats:
        print(f"rocprofv3 pass failed (exit {rc})")
        sys.exit(1)
    shutil.copy(stats[0], args.out + "_kernel_stats.csv")
    shutil.rmtree(d, ignore_errors=True)
    print(f"wrote {args.out}_kernel_stats.csv")


if __name__ == "__main__":
    main()
