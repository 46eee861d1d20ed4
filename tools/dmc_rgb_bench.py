#!/usr/bin/env python3
"""tools/dmc_rgb_bench.py [--n 1024] [--steps 300] [--out profiles/dmc_rgb] - colour (AGX_FRAME_RGB) DMC observations against
gray ones in the same run, at N envs on the DMC default geometry (84x84, fov 30x30, frame_stack 3, peripheral 20x20).

For each wrapper kind and each of gray / colour: the DMC ingest (agx_ingest_rgb: cv15 luma for gray, AGX_GRAY_NONE planar for
colour) and the kind's observation kernel (fovea K2 / K3 / K4, or k_full for the base kind), each as its own begin / end
(agx_profile_next events, every 4th step of an ingest + observe loop; median), and the whole step (ingest + observe back to back
between stream events, per step).  Every kernel line carries the algorithmic bytes (agx_algorithmic_bytes) and their fraction
of the 8 TB/s HBM peak.  Writes <out>_bench.json (one JSON object per line) and prints a table."""
import argparse, json, os, statistics, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "active-gym_amd"), REPO]
import torch
from active_gym import ObsPipeline, _native as nat

PEAK = 8e12
CASES = [("base", None, 1), ("fixed", "resize", 1), ("fixed", "mask", 1), ("fixed", "raw", 1), ("flexible", "resize", 1),
         ("flexible", "mask", 1), ("peripheral", "resize", 1), ("peripheral", "resize", 0)]


def pipeline(kind, mode, aa, n, ch, dev):
    kw = dict(num_envs=n, kind=kind, obs_size=(84, 84), frame_stack=3, device=dev, channels=ch)
    if kind != "base":
        kw.update(fov_size=(30, 30), fov_init_loc=(0, 0), sensory_action_mode="absolute", antialias=bool(aa),
                  resize_to_full=mode == "resize", mask_out=mode == "mask")
    if kind == "peripheral":
        kw["peripheral_res"] = (20, 20)
    return ObsPipeline(**kw)


def inputs(n, dev, pool=4):
    g = torch.Generator(device="cpu")
    g.manual_seed(0)
    frames = [torch.randint(0, 256, (n, 84, 84, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(pool)]
    cmds = [torch.ones((n,), dtype=torch.uint8).to(dev) for _ in range(pool)]
    acts = [(torch.rand((n, 2), generator=g) * 60).to(dev) for _ in range(pool)]
    types = [torch.zeros((n,), dtype=torch.int32).to(dev) for _ in range(pool)]
    return frames, cmds, acts, types


def run(pipe, inp, steps):
    frames, cmds, acts, types = inp
    n, mode = pipe.num_envs, nat.GRAY_NONE if pipe.channels == 3 else nat.GRAY_CV15
    out = torch.empty(pipe.obs_shape if pipe.kind != "base" else pipe.full_shape, dtype=torch.float32, device=pipe.device)
    loc = torch.empty((n, 2), dtype=torch.int32, device=pipe.device)
    res = torch.empty((n, 2), dtype=torch.int32, device=pipe.device)

    def observe(i):
        if pipe.kind == "base":
            pipe.observe_full(out)
        elif pipe.kind == "flexible":
            pipe.fovea(acts[i], action_type=types[i], out=out, loc_out=loc, res_out=res)
        else:
            pipe.fovea(acts[i], out=out, loc_out=loc)

    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps // 4 + 1)]
          for k in ("ingest", "fovea")}
    for lst in ev.values():
        for a, b in lst:
            a.record()
            b.record()
    armed = {"ingest": [], "fovea": []}
    for k in range(steps + 50):
        i = k % len(frames)
        if k >= 50 and k % 4 == 0:
            e = ev["ingest"][len(armed["ingest"])]
            pipe.profile_next("ingest", e[0], e[1])
            armed["ingest"].append(e)
            if pipe.kind != "base":
                e = ev["fovea"][len(armed["fovea"])]
                pipe.profile_next("fovea", e[0], e[1])
                armed["fovea"].append(e)
        pipe.ingest_rgb(frames[i], cmds[i], mode)
        observe(i)
    torch.cuda.synchronize()
    r = {"ingest_us": statistics.median(a.elapsed_time(b) * 1e3 for a, b in armed["ingest"])}
    if pipe.kind != "base":
        r["obs_us"] = statistics.median(a.elapsed_time(b) * 1e3 for a, b in armed["fovea"])
    else:        # k_full: back-to-back launches between stream events
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(20):
            observe(0)
        a.record()
        for _ in range(steps):
            observe(0)
        b.record()
        torch.cuda.synchronize()
        r["obs_us"] = a.elapsed_time(b) * 1e3 / steps
    # the whole step: ingest + observe back to back
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(steps):
        i = k % len(frames)
        pipe.ingest_rgb(frames[i], cmds[i], mode)
        observe(i)
    b.record()
    torch.cuda.synchronize()
    r["step_us"] = a.elapsed_time(b) * 1e3 / steps
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dmc_rgb"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    inp = inputs(a.n, dev)
    lines = []
    print(f"N={a.n} obs 84x84 fov 30x30 fs 3 (peripheral 20x20); {nat.build_info()}")
    print("| kind | mode | aa | frames | ingest us | ingest GB/s frac | observe us | observe bytes | frac of 8 TB/s | step us |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for kind, mode, aa in CASES:
        for ch in (1, 3):
            pipe = pipeline(kind, mode, aa, a.n, ch, dev)
            r = run(pipe, inp, a.steps)
            ib = pipe.algorithmic_bytes("ingest_rgb")
            ob = pipe.algorithmic_bytes("full" if kind == "base" else "fovea")
            r.update(kind=kind, mode=mode, antialias=aa, channels=ch, n=a.n, ingest_bytes=ib, obs_bytes=ob,
                     ingest_frac=ib / (r["ingest_us"] * 1e-6) / PEAK, obs_frac=ob / (r["obs_us"] * 1e-6) / PEAK,
                     build=nat.build_info())
            lines.append(r)
            print(f"| {kind} | {mode or '-'} | {aa} | {'colour' if ch == 3 else 'gray'} | {r['ingest_us']:.1f} | {r['ingest_frac']:.2f} | "
                  f"{r['obs_us']:.1f} | {ob / 1e6:.1f} MB | {r['obs_frac']:.2f} | {r['step_us']:.1f} |", flush=True)
            pipe.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out + "_bench.json", "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
