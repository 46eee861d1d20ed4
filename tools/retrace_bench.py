#!/usr/bin/env python3
"""tools/retrace_bench.py - what the Retrace-family Q-return over a sequence-replay batch (include/agx_retrace.h, K16) costs, at
B = 64, L = 64 (the sequence benchmark's shape) and B = 1024, L = 128 (the rollout benchmark's), in both layouts, on synthetic
arrays as tests/retrace_model.py draws them (lengths 0 .. L, rows missing in the middle of live runs, c uniform in [0, 1]):

  (k) Retrace.targets on the arrays, through the Python binding, outputs reused;
  (t) the torch loop over l = L - 1 .. 0 on the same device arrays in the same process - the path a user has today and the
      yardstick; its masks (has, which step bootstraps from boot) are computed once outside the timed region.

In the same process (k) is checked against (t): the loop rounds in the same order, so the two are compared bit for bit.  Every
call sits between a begin and an end event of its own on the stream; the figures are the median / min / p90 over --iters
repetitions after --warmup.  Writes profiles/retrace_bench.json.

    python tools/retrace_bench.py [--iters 200] [--warmup 20] [--out profiles/retrace_bench.json]

The batch-major form that ships is the strided one.  --tiled also times the LDS-tiled form it was measured against
(csrc/experiments/agx_retrace_tiled.h): the experiments build with AGX_RETRACE_TILED=1, in a child process of its own that ends
before this one opens the GPU:

    python active-gym_amd/build.py --experiments
    python tools/retrace_bench.py --tiled
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "active-gym_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((64, 64), (1024, 128))


def arrays(B, L, time_major, dev):
    g = torch.Generator(device=dev).manual_seed(1000 * B + L)
    length = torch.randint(0, L + 1, (B,), device=dev, generator=g, dtype=torch.int32)
    length[::4] = L
    shape = (L, B) if time_major else (B, L)
    at = torch.arange(L, device=dev)
    inside = (at[:, None] < length[None, :]) if time_major else (at[None, :] < length[:, None])
    steps = (inside & (torch.rand(shape, device=dev, generator=g) > 0.05)).to(torch.int32)
    f = lambda: torch.randn(shape, device=dev, generator=g)
    batch = dict(length=length, steps=steps, ret=f(), discount=torch.full(shape, 0.99, device=dev))
    return batch, f(), f(), torch.rand(shape, device=dev, generator=g), torch.randn((B,), device=dev, generator=g)


def measure(a, dev):
    from rollout_bench import timed
    from active_gym import FrameHistory, ObsPipeline, Retrace, StepLog
    from active_gym import _native as nat
    pipe = ObsPipeline(1, "base", obs_size=(12, 12), frame_stack=1, device=dev)
    rt = Retrace(StepLog(FrameHistory(pipe, 1), 4))
    res = {"build": nat.build_info(), "library": os.path.basename(os.environ.get("AGX_LIB", nat.LIB_PATH)), "iters": a.iters, "shapes": {}}
    for B, L in SHAPES:
        for time_major in (False, True):
            batch, q, v, c, boot = arrays(B, L, time_major, dev)
            out = rt.targets(batch, q, v, c, boot, time_major=time_major)

            def kernel():
                rt.targets(batch, q, v, c, boot, out=out, time_major=time_major)

            step = (lambda x, l: x[l]) if time_major else (lambda x, l: x[:, l])
            length, steps, reward, discount = batch["length"], batch["steps"], batch["ret"], batch["discount"]
            has = [(l < length) & (step(steps, l) == 1) for l in range(L)]
            from_v = [(l + 1 < length) for l in range(L)]
            zero = torch.zeros((B,), device=dev)
            t_T, t_td = torch.empty_like(q), torch.empty_like(q)

            def torch_loop():
                carry = zero
                for l in range(L - 1, -1, -1):
                    vnext = torch.where(from_v[l], step(v, l + 1), boot) if l + 1 < L else boot
                    T = step(reward, l) + step(discount, l) * (vnext + carry)
                    td = T - step(q, l)
                    step(t_T, l).copy_(torch.where(has[l], T, zero))
                    step(t_td, l).copy_(torch.where(has[l], td, zero))
                    carry = torch.where(has[l], step(c, l) * td, zero)
                return t_T, t_td

            for _ in range(a.busy):               # an idle device reads slower in its first timed block (tools/vtrace_bench.py)
                kernel()
            w_T, w_td = torch_loop()
            same = bool(torch.equal(out["target"].view(torch.int32), w_T.view(torch.int32)) and torch.equal(out["td"].view(torch.int32), w_td.view(torch.int32)))
            assert torch.allclose(out["target"], w_T, rtol=1e-4, atol=1e-4) and torch.allclose(out["td"], w_td, rtol=1e-4, atol=1e-4)
            r = {"kernel": timed(kernel, a.iters, a.warmup), "kernel_again": timed(kernel, a.iters, a.warmup),
                 "equals_torch_loop_bit_for_bit": same, "valid_steps": int(out["valid"].sum()), "steps": B * L}
            if not a.child:
                r["torch_loop"] = timed(torch_loop, max(a.iters // 10, 5), 2)
                r["kernel_over_torch_loop"] = r["kernel"]["median_us"] / r["torch_loop"]["median_us"]
            res["shapes"][f"B{B}_L{L}_{'time' if time_major else 'batch'}_major"] = r
    pipe.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--busy", type=int, default=200, help="calls made before anything is timed")
    ap.add_argument("--tiled", action="store_true", help="also time the LDS-tiled batch-major form of the experiments build (lib/libagx_exp.so)")
    ap.add_argument("--child", action="store_true", help="(internal) time the kernel only and print the result")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "retrace_bench.json"))
    a = ap.parse_args()
    tiled = None
    if a.tiled:                                   # a process of its own, before this one opens the GPU: one library per process
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "tiled.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--warmup", str(a.warmup), "--busy", str(a.busy),
                            "--out", path], check=True, env=dict(os.environ, AGX_LIB=os.path.join(REPO, "active-gym_amd", "lib", "libagx_exp.so"), AGX_RETRACE_TILED="1"),
                           stdout=subprocess.DEVNULL, timeout=600)
            tiled = json.load(open(path))
    res = measure(a, torch.device("cuda:0"))
    res["through"] = "the Python binding (Retrace.targets with out=): argument checks and one ctypes call per launch are inside every figure"
    for B, L in SHAPES:
        bm, tm = res["shapes"][f"B{B}_L{L}_batch_major"], res["shapes"][f"B{B}_L{L}_time_major"]
        bm["batch_over_time_major"] = bm["kernel"]["median_us"] / tm["kernel"]["median_us"]
        if tiled:
            d = tiled["shapes"][f"B{B}_L{L}_batch_major"]
            bm["lds_tiled_form"] = {"library": tiled["library"] + " with AGX_RETRACE_TILED=1", "kernel": d["kernel"], "kernel_again": d["kernel_again"],
                                    "equals_torch_loop_bit_for_bit": d["equals_torch_loop_bit_for_bit"]}
            bm["tiled_over_strided"] = d["kernel"]["median_us"] / bm["kernel"]["median_us"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
