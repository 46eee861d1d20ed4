#!/usr/bin/env python
"""One CRC-32 line per (case, call) of the active_gym Python bindings on one GPU: run it once per package directory against the
same libagx.so and compare the outputs line for line (profiles/binding_refactor.md).

    python tools/package_crc.py --package active-gym_amd > new.txt
    python tools/package_crc.py --package /somewhere/parent/active-gym_amd > parent.txt      # AGX_LIB / AGXR_LIB: the same libraries

A CRC covers everything the call returned - tensors by their bytes, dicts in dictionary order, lists element by element; rows a
call leaves as allocated (invalid samples, ok = 0) are masked out first.  A call that raises prints the exception's type and text.
Only names that both packages have are used."""
import argparse
import os
import sys
import zlib

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--package", required=True, help="directory that holds the active_gym package: goes first on sys.path")
ap.add_argument("--only", default="", help="run only the sections named here (comma separated: pipe, hist, refuse, env)")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.package))
sys.path.append(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))      # lcg_ale.py

import torch  # noqa: E402

import active_gym  # noqa: E402
from active_gym import _native as nat  # noqa: E402
from active_gym import AtariEnvArgs, AtariVecEnv, FrameHistory, GlimpseMemory, ObsPipeline, ReplaySampler, StepLog  # noqa: E402

from lcg_ale import LcgALE  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(active_gym.__file__))) == os.path.abspath(a.package), active_gym.__file__
DEV = torch.device("cuda", 0)
LINES = 0


def crc(x, c=0):
    if isinstance(x, torch.Tensor):
        t = x.detach().contiguous().cpu()
        t = t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t
        c = zlib.crc32(repr((str(x.dtype), tuple(x.shape), x.device.type)).encode(), c)
        return zlib.crc32(t.numpy().tobytes(), c)
    if isinstance(x, np.ndarray):
        c = zlib.crc32(repr((str(x.dtype), x.shape)).encode(), c)
        if x.dtype == object:
            for v in x.ravel():
                c = crc(v, c)
            return c
        return zlib.crc32(np.ascontiguousarray(x).tobytes(), c)
    if isinstance(x, dict):
        for k, v in x.items():
            c = crc(v, zlib.crc32(str(k).encode(), c))
        return c
    if isinstance(x, (list, tuple)):
        c = zlib.crc32(b"[%d" % len(x), c)
        for v in x:
            c = crc(v, c)
        return c
    return zlib.crc32(repr(x).encode(), c)


def call(name, fn, post=None):
    """Print the line of one call; returns what it returned (None when it raised)."""
    global LINES
    LINES += 1
    try:
        r = fn()
        print(f"{name} {crc(post(r) if post else r):08x}")
        return r
    except Exception as e:  # noqa: BLE001
        print(f"{name} {type(e).__name__}: {e}")
        return None


def rnd_u8(g, shape):
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(DEV)


def rows(mask, *ts):
    """Every tensor restricted to the rows where mask is true (the others are left as allocated), and the mask."""
    m = mask.bool()
    return [m] + [None if t is None else t[m] for t in ts]


def batch_post(hist):
    """For a transition batch: obs / fov_loc rows where ok is true only, and of a glimpse memory's fov_loc [B, P, 2] only the
    glimpses that were taken (an episode younger than P has fewer; the others are left as allocated)."""
    def post(r):
        m, out = r["ok"].bool(), {}
        for k, v in r.items():
            if k in ("fov_loc", "next_fov_loc") and v.dim() == 3:
                taken = GlimpseMemory(hist, v.shape[1]).observe(r["env"], r["index" if k == "fov_loc" else "next_index"])[2].long()
                keep = torch.arange(v.shape[1], device=DEV)[None, :] < taken[:, None]
                v = torch.where(keep[..., None], v, torch.zeros_like(v))
            out[k] = v[m] if k in ("obs", "next_obs", "fov_loc", "next_fov_loc") else v
        return out
    return post


def bad_variants(t):
    """A wrong shape, a wrong dtype, a CPU tensor and a non-contiguous tensor of t's shape."""
    other = torch.float64 if t.dtype != torch.float64 else torch.float32
    strided = torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype, device=t.device)[..., 0]
    return {"shape": torch.zeros((t.shape[0] + 1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device), "dtype": t.to(other),
            "cpu": t.cpu(), "strided": strided}


def refusals(name, fn, kw):
    """fn(**kw) with each tensor argument replaced by each bad variant, one at a time."""
    for key, val in kw.items():
        if isinstance(val, torch.Tensor):
            for what, bad in bad_variants(val).items():
                call(f"{name}.refuse.{key}.{what}", lambda: fn(**{**kw, key: bad}), post=lambda r: "accepted")


GEOMS = {"g84": dict(obs_size=(84, 84), fov_size=(30, 30), frame_stack=4), "g40": dict(obs_size=(40, 40), fov_size=(12, 12), frame_stack=2)}
MODES = {"base": dict(kind="base"), "fixed_resize": dict(kind="fixed", resize_to_full=True), "fixed_mask": dict(kind="fixed", mask_out=True),
         "fixed_raw": dict(kind="fixed"), "flexible_mask": dict(kind="flexible", mask_out=True), "flexible_raw": dict(kind="flexible"),
         "peripheral": dict(kind="peripheral", peripheral_res=(14, 14)), "fixed_relative": dict(kind="fixed", resize_to_full=True,
                                                                                             sensory_action_mode="relative", sensory_action_space=(-8, 8))}
N = 5
ACT_DTYPES = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "i64": torch.int64, "f16": torch.float16}


def make_pipe(geom, mode, obs_dtype="float32", channels=1):
    kw = dict(GEOMS[geom], **MODES[mode])
    if kw["kind"] == "base":
        kw.pop("fov_size")
    return ObsPipeline(N, fov_init_loc=(1, 2), device=DEV, obs_dtype=obs_dtype, channels=channels, **kw)


def actions(g, pipe, n=N):
    hi = max(pipe.obs_size[0] - pipe.fov_size[0], 1)
    base = torch.randint(0, hi + 1, (n, 2), generator=g)
    return {name: base.to(dt).to(DEV) for name, dt in ACT_DTYPES.items()}


# ---------------------------------------------------------------------------------------------------------------- ObsPipeline
def section_pipe():
    for geom in GEOMS:
        for mode in MODES:
            for od in ("float32", "bfloat16"):
                tag = f"pipe.{geom}.{mode}.{od}"
                g = torch.Generator().manual_seed(11)
                pipe = make_pipe(geom, mode, od)
                oh, ow = pipe.obs_size
                cmd = torch.full((N,), 2, dtype=torch.uint8, device=DEV)
                clear = torch.full((N,), 2 | nat.CMD_CLEAR, dtype=torch.uint8, device=DEV)
                R = len(pipe.source_rows())
                call(f"{tag}.source_rows", pipe.source_rows)
                ingests = {"ingest": (pipe.ingest, (N, 2, nat.RAW_H, nat.RAW_W, 3)), "ingest_gray_raw": (pipe.ingest_gray_raw, (N, 2, nat.RAW_H, nat.RAW_W)),
                           "ingest_compact": (pipe.ingest_compact, (N, 2, R, nat.RAW_W, 3)),
                           "ingest_gray_raw_compact": (pipe.ingest_gray_raw_compact, (N, 2, R, nat.RAW_W)),
                           "ingest_gray": (pipe.ingest_gray, (N, 2, oh, ow)), "ingest_rgb": (pipe.ingest_rgb, (N, oh, ow, 3))}
                for k, (name, (fn, shape)) in enumerate(ingests.items()):
                    fr = rnd_u8(g, shape)
                    call(f"{tag}.{name}", lambda: (fn(fr, clear if k == 0 else cmd), pipe.stack_u8())[1])
                call(f"{tag}.observe_full.alloc", pipe.observe_full)
                call(f"{tag}.observe_full.passed", lambda: pipe.observe_full(torch.zeros(pipe.full_shape, dtype=pipe.obs_dtype, device=DEV)))
                call(f"{tag}.fov_state", pipe.fov_state)
                if pipe.kind == "base":
                    call(f"{tag}.fovea", pipe.fovea)
                    call(f"{tag}.step_fixed", lambda: pipe.step_fixed(rnd_u8(g, (N, 2, nat.RAW_H, nat.RAW_W, 3)), cmd))
                    call(f"{tag}.fovea_packed", pipe.fovea_packed)
                    pipe.close()
                    continue
                acts = actions(g, pipe)
                flex = pipe.kind == "flexible"
                atype = torch.tensor([0, 1, 0, 1, 1], dtype=torch.int32, device=DEV) if flex else None
                mask = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=DEV)

                def outs():
                    o = dict(out=torch.zeros(pipe.obs_shape, dtype=pipe.obs_dtype, device=DEV), loc_out=torch.zeros((N, 2), dtype=torch.int32, device=DEV))
                    if flex:
                        o["res_out"] = torch.zeros((N, 2), dtype=torch.int32, device=DEV)
                    return o
                tkw = dict(action_type=atype) if flex else {}
                call(f"{tag}.fovea.none.alloc", lambda: pipe.fovea(None, **tkw))
                call(f"{tag}.fovea.none.passed", lambda: pipe.fovea(None, **tkw, **outs()))
                for an, act in acts.items():
                    call(f"{tag}.fovea.{an}.alloc", lambda: pipe.fovea(act, **tkw))
                    call(f"{tag}.fovea.{an}.passed", lambda: pipe.fovea(act, **tkw, **outs()))
                call(f"{tag}.fovea.mask", lambda: pipe.fovea(acts["f32"], mask=mask, **tkw, **outs()))
                call(f"{tag}.fovea_reset.mask", lambda: (pipe.fovea_reset(mask), pipe.fov_state())[1])
                loc, res = pipe.fov_state()
                call(f"{tag}.set_fov_state", lambda: (pipe.set_fov_state(loc.flip(0).contiguous(), res), pipe.fov_state())[1])
                call(f"{tag}.set_stack_u8", lambda: (pipe.set_stack_u8(rnd_u8(g, pipe.full_shape)), pipe.stack_u8(), pipe.fovea(None, **tkw))[1:])
                frames = rnd_u8(g, (N, 2, nat.RAW_H, nat.RAW_W, 3))
                for an in (None, "f32", "i64", "f16"):
                    act = None if an is None else acts[an]
                    call(f"{tag}.step_fixed.{an}.alloc", lambda: pipe.step_fixed(frames, cmd, act))
                    call(f"{tag}.step_fixed.{an}.passed", lambda: pipe.step_fixed(frames, cmd, act, **{k: v for k, v in outs().items() if k != "res_out"}))

                def pouts():
                    cap = N * pipe.frame_stack * oh * ow
                    return dict(packed=torch.zeros((cap,), dtype=torch.float32, device=DEV), offsets=torch.zeros((N + 1,), dtype=torch.int64, device=DEV),
                                loc_out=torch.zeros((N, 2), dtype=torch.int32, device=DEV), res_out=torch.zeros((N, 2), dtype=torch.int32, device=DEV))

                def used(r):
                    return (r[0][:int(r[1][-1])],) + tuple(r[1:])
                screens = {"rgb": frames, "gray": rnd_u8(g, (N, 2, nat.RAW_H, nat.RAW_W)), "rgb_compact": rnd_u8(g, (N, 2, R, nat.RAW_W, 3)),
                           "gray_compact": rnd_u8(g, (N, 2, R, nat.RAW_W)), "rows7": rnd_u8(g, (N, 2, 7, nat.RAW_W)), "dim3": rnd_u8(g, (N, 2, nat.RAW_H))}
                for an in (None, "f32", "f64", "i32", "i64", "f16"):
                    act = None if an is None else acts[an]
                    call(f"{tag}.fovea_packed.{an}.alloc", lambda: pipe.fovea_packed(act, atype), used)
                    call(f"{tag}.fovea_packed.{an}.passed", lambda: pipe.fovea_packed(act, atype, **pouts()), used)
                for sn, scr in screens.items():
                    call(f"{tag}.step_flexible_packed.{sn}.alloc", lambda: pipe.step_flexible_packed(scr, cmd, acts["f32"], atype), used)
                    call(f"{tag}.step_flexible_packed.{sn}.passed", lambda: pipe.step_flexible_packed(scr, cmd, acts["i64"], atype, **pouts()), used)
                call(f"{tag}.step_flexible_packed.f16", lambda: pipe.step_flexible_packed(frames, cmd, acts["f16"], atype), used)
                call(f"{tag}.fovea_packed.packed2d", lambda: pipe.fovea_packed(None, atype, packed=torch.zeros((4, 4), dtype=torch.float32, device=DEV)), used)
                pipe.close()
    # colour frames
    for geom in GEOMS:
        g = torch.Generator().manual_seed(12)
        pipe = make_pipe(geom, "fixed_resize", channels=3)
        cmd = torch.full((N,), 1 | nat.CMD_CLEAR, dtype=torch.uint8, device=DEV)
        call(f"pipe.{geom}.rgb.ingest_rgb", lambda: (pipe.ingest_rgb(rnd_u8(g, (N,) + pipe.obs_size + (3,)), cmd), pipe.stack_u8())[1])
        call(f"pipe.{geom}.rgb.ingest", lambda: pipe.ingest(rnd_u8(g, (N, 2, nat.RAW_H, nat.RAW_W, 3)), cmd))
        call(f"pipe.{geom}.rgb.observe_full", pipe.observe_full)
        call(f"pipe.{geom}.rgb.fovea", lambda: pipe.fovea(actions(g, pipe)["f32"]))
        pipe.close()


# ------------------------------------------------------------------------------------- history, glimpse, replay, step log
def fill(pipe, hist, g, steps, logs=()):
    """steps ingests + foveas + pushes with CLEARs sprinkled in; every log records a reward / flag / payload row per push."""
    oh, ow = pipe.obs_size
    for t in range(steps):
        c = torch.full((N,), 2, dtype=torch.uint8)
        if t == 0:
            c |= nat.CMD_CLEAR
        elif t % 5 == 4:
            c[t % N] |= nat.CMD_CLEAR
        if t % 7 == 3:
            c[(t + 2) % N] = nat.CMD_SKIP
        c = c.to(DEV)
        pipe.ingest_gray(rnd_u8(g, (N, 2, oh, ow)), c)
        if pipe.kind == "base":
            pipe.observe_full()
        else:
            pipe.fovea(actions(g, pipe)["i32"])
        index = hist.push(c)
        for log in logs:
            reward = torch.randint(-3, 4, (N,), generator=g).float().to(DEV)
            flags = ((c & nat.CMD_CLEAR) == 0).to(torch.uint8) * (torch.randint(0, 6, (N,), generator=g) == 0).to(torch.uint8).to(DEV)
            payload = rnd_u8(g, (N, log.payload_bytes)) if log.payload_bytes else None
            log.record(index, reward, flags, payload)


def section_hist(refuse=False):
    for geom in GEOMS:
        for mode in ("base", "fixed_resize", "fixed_mask", "fixed_raw", "flexible_mask"):
            for od in ("float32", "bfloat16"):
                tag = f"hist.{geom}.{mode}.{od}"
                g = torch.Generator().manual_seed(21)
                pipe = make_pipe(geom, mode, od)
                hist = call(f"{tag}.create", lambda: FrameHistory(pipe, 12), post=lambda h: (h.capacity, h.nbytes))
                if hist is None:
                    pipe.close()
                    continue
                fixed = pipe.kind == "fixed"
                logs = [StepLog(hist, 0), StepLog(hist, 12)]
                call(f"{tag}.last_index.empty", hist.last_index)
                fill(pipe, hist, g, 9, logs)
                cmd = torch.full((N,), 2, dtype=torch.uint8, device=DEV)
                call(f"{tag}.push.alloc", lambda: hist.push(cmd))
                call(f"{tag}.push.passed", lambda: hist.push(cmd, torch.zeros((N,), dtype=torch.int64, device=DEV)))
                call(f"{tag}.last_index.alloc", hist.last_index)
                call(f"{tag}.last_index.passed", lambda: hist.last_index(torch.zeros((N,), dtype=torch.int64, device=DEV)))
                B = 12
                env = torch.randint(0, N, (B,), generator=g, dtype=torch.int32).to(DEV)
                index = torch.randint(-1, 13, (B,), generator=g, dtype=torch.int64).to(DEV)
                acts = actions(g, pipe, B) if pipe.kind != "base" else {k: torch.zeros((B, 2), dtype=dt, device=DEV) for k, dt in ACT_DTYPES.items()}

                def obs_post(r):
                    return rows(r[2], r[0], r[1] if fixed else None)
                for what in ("fovea", "full", "other"):
                    for an in (None,) + tuple(ACT_DTYPES):
                        act = None if an is None else acts[an]
                        shape = (B,) + (hist.obs_row_shape(what) if what != "other" else (1,))
                        call(f"{tag}.observe.{what}.{an}.alloc", lambda: hist.observe(env, index, act, what), obs_post)
                        call(f"{tag}.observe.{what}.{an}.passed", lambda: hist.observe(
                            env, index, act, what, out=torch.zeros(shape, dtype=pipe.obs_dtype, device=DEV),
                            loc_out=torch.zeros((B, 2), dtype=torch.int32, device=DEV), valid_out=torch.zeros((B,), dtype=torch.uint8, device=DEV)))
                for P in (1, 3, 9):
                    mem = call(f"{tag}.glimpse{P}.create", lambda: GlimpseMemory(hist, P), post=lambda m: m.glimpses)
                    if mem is None:
                        continue

                    def mem_post(r):
                        taken = r[2].long()
                        keep = torch.arange(r[1].shape[1], device=DEV)[None, :] < taken[:, None]
                        return r[0][taken > 0], torch.where(keep[..., None], r[1], torch.zeros_like(r[1])), r[2]
                    call(f"{tag}.glimpse{P}.observe.alloc", lambda: mem.observe(env, index), mem_post)
                    call(f"{tag}.glimpse{P}.observe.passed", lambda: mem.observe(
                        env, index, out=torch.zeros((B,) + hist.obs_row_shape(), dtype=pipe.obs_dtype, device=DEV),
                        loc_out=torch.zeros((B, P, 2), dtype=torch.int32, device=DEV), taken_out=torch.zeros((B,), dtype=torch.uint8, device=DEV)))
                    if refuse:
                        refusals(f"{tag}.glimpse{P}.observe", mem.observe, dict(
                            env=env, index=index, out=torch.zeros((B,) + hist.obs_row_shape(), dtype=pipe.obs_dtype, device=DEV),
                            loc_out=torch.zeros((B, P, 2), dtype=torch.int32, device=DEV), taken_out=torch.zeros((B,), dtype=torch.uint8, device=DEV)))
                smp = call(f"{tag}.sampler.create", lambda: ReplaySampler(hist, back=2, forward=1, seed=5), post=lambda s: (s.back, s.forward, s.attempts))
                call(f"{tag}.sampler.badargs", lambda: ReplaySampler(hist, back=99))
                call(f"{tag}.sample.alloc", lambda: smp.sample(16) + (smp.total(),))
                call(f"{tag}.sample.passed", lambda: smp.sample(16, torch.zeros((16,), dtype=torch.int32, device=DEV),
                                                                 torch.zeros((16,), dtype=torch.int64, device=DEV), torch.zeros((16,), dtype=torch.uint8, device=DEV)))
                call(f"{tag}.sample.negative", lambda: smp.sample(-1))
                call(f"{tag}.inspect", lambda: smp.inspect(env, index))

                post = batch_post(hist)
                for gl in (None, 3, 4):
                    call(f"{tag}.transitions.{gl}", lambda: smp.transitions(16, glimpses=gl), post)
                smp0 = ReplaySampler(hist, back=0, forward=0, seed=6)
                call(f"{tag}.transitions.forward0", lambda: smp0.transitions(4))
                for li, log in enumerate(logs):
                    call(f"{tag}.log{li}.bytes", log.bytes)
                    for nstep in (1, 5, 0, 65):
                        call(f"{tag}.log{li}.gather.n{nstep}", lambda: log.gather(env, index, nstep, 0.9))
                    for gl in (None, 3):
                        call(f"{tag}.log{li}.batch.{gl}", lambda: log.batch(smp, 16, nstep=3, gamma=0.9, glimpses=gl), post)
                        if gl is not None and fixed and pipe.out_mode != nat.OUT_RAW:
                            own = GlimpseMemory(hist, gl)
                            call(f"{tag}.log{li}.batch.{gl}.memory", lambda: log.batch(smp, 16, nstep=3, gamma=0.9, glimpses=gl, memory=own), post)
                            call(f"{tag}.log{li}.batch.{gl}.memory4", lambda: log.batch(smp, 16, glimpses=gl, memory=GlimpseMemory(hist, 4)))
                            call(f"{tag}.log{li}.batch.memory_without_glimpses", lambda: log.batch(smp, 16, memory=own))
                    call(f"{tag}.log{li}.batch.back", lambda: log.batch(smp0, 16, glimpses=3))
                    call(f"{tag}.log{li}.record.no_payload", lambda: log.record(hist.last_index(), torch.zeros((N,), device=DEV), torch.zeros((N,), dtype=torch.uint8, device=DEV)))
                call(f"{tag}.steplog.badwidth", lambda: StepLog(hist, 6))
                if refuse:
                    i64, z8 = torch.zeros((N,), dtype=torch.int64, device=DEV), torch.zeros((N,), dtype=torch.uint8, device=DEV)
                    refusals(f"{tag}.push", hist.push, dict(cmd=cmd, out=i64))
                    refusals(f"{tag}.last_index", hist.last_index, dict(out=i64))
                    refusals(f"{tag}.observe", hist.observe, dict(
                        env=env, index=index, action=acts["f32"], out=torch.zeros((B,) + hist.obs_row_shape(), dtype=pipe.obs_dtype, device=DEV),
                        loc_out=torch.zeros((B, 2), dtype=torch.int32, device=DEV), valid_out=torch.zeros((B,), dtype=torch.uint8, device=DEV)))
                    refusals(f"{tag}.sample", lambda **kw: smp.sample(16, **kw), dict(
                        env_out=torch.zeros((16,), dtype=torch.int32, device=DEV), index_out=torch.zeros((16,), dtype=torch.int64, device=DEV),
                        ok_out=torch.zeros((16,), dtype=torch.uint8, device=DEV)))
                    refusals(f"{tag}.inspect", smp.inspect, dict(env=env, index=index))
                    refusals(f"{tag}.gather", logs[1].gather, dict(env=env, index=index))
                    refusals(f"{tag}.record", logs[1].record, dict(index=i64, reward=torch.zeros((N,), device=DEV), flags=z8,
                                                                   payload=torch.zeros((N, 12), dtype=torch.uint8, device=DEV)))
                    call(f"{tag}.observe.env2d", lambda: hist.observe(env.reshape(2, 6), index))
                    call(f"{tag}.observe.envlist", lambda: hist.observe([0, 1], index))
                call(f"{tag}.clear", lambda: (hist.clear(), hist.last_index(), logs[1].gather(env, index, 2, 0.9), hist.observe(env, index)[2])[1:])
                hist.close()
                call(f"{tag}.closed.sample", lambda: smp.sample(4))
                call(f"{tag}.closed.gather", lambda: logs[0].gather(env, index))
                pipe.close()


def section_refuse():
    """Every tensor argument of every public ObsPipeline method, each bad in four ways; the history's are in section_hist."""
    for mode in ("fixed_resize", "flexible_raw", "peripheral", "base"):
        tag = f"pipe.g84.{mode}"
        g = torch.Generator().manual_seed(31)
        pipe = make_pipe("g84", mode)
        oh, ow = pipe.obs_size
        R = len(pipe.source_rows())
        cmd = torch.full((N,), 2, dtype=torch.uint8, device=DEV)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)  # noqa: E731
        for name, shape in (("ingest", (N, 2, nat.RAW_H, nat.RAW_W, 3)), ("ingest_gray_raw", (N, 2, nat.RAW_H, nat.RAW_W)), ("ingest_compact", (N, 2, R, nat.RAW_W, 3)),
                            ("ingest_gray_raw_compact", (N, 2, R, nat.RAW_W)), ("ingest_gray", (N, 2, oh, ow)), ("ingest_rgb", (N, oh, ow, 3))):
            fn = getattr(pipe, name)
            refusals(f"{tag}.{name}", lambda frames, cmd, fn=fn: fn(frames, cmd), dict(frames=z(shape, torch.uint8), cmd=cmd))
        refusals(f"{tag}.observe_full", pipe.observe_full, dict(out=z(pipe.full_shape, pipe.obs_dtype)))
        refusals(f"{tag}.set_stack_u8", pipe.set_stack_u8, dict(stack=z(pipe.full_shape, torch.uint8)))
        refusals(f"{tag}.fovea_reset", pipe.fovea_reset, dict(mask=z((N,), torch.uint8)))
        refusals(f"{tag}.set_fov_state", pipe.set_fov_state, dict(loc=z((N, 2), torch.int32), res=z((N, 2), torch.int32)))
        fkw = dict(action=z((N, 2), torch.float32), mask=z((N,), torch.uint8), out=z(pipe.obs_shape, pipe.obs_dtype), loc_out=z((N, 2), torch.int32))
        pkw = dict(action=z((N, 2), torch.float32), action_type=z((N,), torch.int32), packed=z((N * pipe.frame_stack * oh * ow,), torch.float32),
                   offsets=z((N + 1,), torch.int64), loc_out=z((N, 2), torch.int32), res_out=z((N, 2), torch.int32))
        if pipe.kind == "flexible":
            fkw.update(action_type=z((N,), torch.int32), res_out=z((N, 2), torch.int32))
        refusals(f"{tag}.fovea", pipe.fovea, fkw)
        refusals(f"{tag}.step_fixed", pipe.step_fixed, dict(frames=z((N, 2, nat.RAW_H, nat.RAW_W, 3), torch.uint8), cmd=cmd, action=fkw["action"],
                                                            out=fkw["out"], loc_out=fkw["loc_out"]))
        refusals(f"{tag}.fovea_packed", pipe.fovea_packed, pkw)
        refusals(f"{tag}.step_flexible_packed", pipe.step_flexible_packed, dict(screens=z((N, 2, nat.RAW_H, nat.RAW_W), torch.uint8), cmd=cmd, **pkw))
        call(f"{tag}.fovea.action_f16", lambda: pipe.fovea(z((N, 2), torch.float16)))
        call(f"{tag}.fovea.action_numpy", lambda: pipe.fovea(np.zeros((N, 2), np.float32)))
        pipe.close()
    for what, kw in (("kind", dict(kind="circular")), ("channels", dict(channels=2)), ("obs_dtype", dict(obs_dtype="uint8")), ("fov", dict(kind="fixed", fov_size=(90, 90))),
                     ("mode", dict(kind="fixed", fov_size=(30, 30), sensory_action_mode="polar")), ("device", dict(device="cpu"))):
        call(f"pipe.create.{what}", lambda: ObsPipeline(N, **{"kind": "base", **kw}))


# ---------------------------------------------------------------------------------------------------------------- env level
def make_env(kind, variant, rekind=False):
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", num_workers=2, scripted_actions=4, scripted_lives=2, scripted_p_life=150,
              scripted_p_over=80, history_len=8, step_log=True)
    lcg = lambda a, i: LcgALE(a.seed + i, 4, 2, 150, 80)  # noqa: E731  (the Python runner on tests/lcg_ale.py)
    kw.update({"lcg_py_dev": dict(device="cuda:0", frame_source=lcg), "lcg_host_pool": dict(device=None, frame_source=lcg),
               "py_dev": dict(device="cuda:0", native_loop=False), "nat_dev": dict(device="cuda:0"), "host_pool": dict(device=None),
               "host_chunks2": dict(device=None, host_obs_chunks=2)}[variant])
    env = AtariVecEnv(AtariEnvArgs(**kw), N, kind="base" if rekind else kind, noop_fn=lambda: 2)
    if rekind:
        env.rekind(kind)
    if variant.endswith("host_pool"):
        env._host.min_elems = 0
    return env


def section_env():
    fewest = None
    for kind, variant, rekind in [(k, v, False) for v in ("py_dev", "nat_dev", "host_pool", "host_chunks2", "lcg_py_dev", "lcg_host_pool") for k in ("base", "fixed")] + \
                                 [("fixed", "py_dev", True), ("fixed", "nat_dev", True)]:
        tag = f"env.{'rekind.' if rekind else ''}{kind}.{variant}"
        rng = np.random.RandomState(7)
        env = make_env(kind, variant, rekind)
        print(f"# {tag}: loop {'native' if env._loop is not None else 'python'}, host_obs_chunks {env.host_obs_chunks}, payload {env.steplog.payload_bytes}")
        ends = 0

        post = batch_post(env.history)
        call(f"{tag}.reset", env.reset)
        for t in range(30):
            motor = rng.randint(0, 4, N)
            sens = rng.randint(0, 55, (N, 2))
            sens = sens.astype((np.int64, np.float32, np.float64, np.int32)[t % 4])
            action = motor if kind == "base" else {"motor_action": motor, "sensory_action": sens}
            r = call(f"{tag}.step{t}", lambda: env.step(action))
            ends += int(np.asarray(r[2].cpu() if isinstance(r[2], torch.Tensor) else r[2]).sum())
            call(f"{tag}.step{t}.glimpse_memory", lambda: env.glimpse_memory(3))
            call(f"{tag}.step{t}.replay_batch", lambda: env.replay_batch(4, nstep=3, glimpses=3 if kind == "fixed" else None), post)
            if t == 14:
                call(f"{tag}.reset_envs", lambda: env.reset_envs([0, 3]))
                call(f"{tag}.replay_batch.glimpses_on_{kind}", lambda: env.replay_batch(4, nstep=3, glimpses=3), post)
                call(f"{tag}.replay_sampler", lambda: env.replay_sampler(back=1, forward=2).sample(8))
                call(f"{tag}.replay_sampler.cached", lambda: env.replay_sampler(back=1, forward=2) is env.replay_sampler(back=1, forward=2))
        call(f"{tag}.history_len", lambda: (env.history_len, env.step_log, env.history.capacity, env.steplog.payload_bytes))
        env.close()
        print(f"# {tag}: {ends} episode ends")
        if ends < 10:
            raise SystemExit(f"{tag}: only {ends} episode ends")
        fewest = ends if fewest is None else min(fewest, ends)
    print(f"# env cases: fewest episode ends {fewest}")


print(f"# {nat.build_info()}")
only = set(filter(None, a.only.split(",")))
if not only or "pipe" in only:
    section_pipe()
if not only or "hist" in only:
    section_hist(refuse=not only or "refuse" in only)
if not only or "refuse" in only:
    section_refuse()
if not only or "env" in only:
    section_env()
print(f"# {LINES} calls")
