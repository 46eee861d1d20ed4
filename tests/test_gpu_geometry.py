"""GPU: every fovea kernel form against the oracle, each form reached the way a user reaches it - by geometry.

agx_create picks a kernel form from the geometry alone.  tests/golden/geometry_cases.json lists geometries and the form each
selects (pinned on the CPU by tests/test_geometry_plan_cpu.py, which also says which forms the table must reach); here
every case runs through libagx and is compared with oracle.oracle fed ``float32(u8) / 255`` widened to float64.  No knob
(AGX_FOVEA_GENERIC, AGX_*_V2) is set anywhere.

Bars: fov_loc / fov_res, raw crops, masks and the pasted fovea window bit-exact; resampled values within FLOAT_TOL of the
float64 oracle (the project's bar, tests/test_gpu_parity.py).  The RNG seed of a test is derived from its id, so one case
can be re-run alone: ``pytest tests/test_gpu_geometry.py -k o40x160_f12x50_p20x40_aa1-flex_resize``."""
import json
import os
import re
import zlib

import numpy as np
import pytest
import torch

from golden_util import unit64
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FLOAT_TOL = 1e-5               # tests/test_gpu_parity.py
SENTINEL = -12345.0            # exactly representable in bf16 and f16
TAIL = 4096                    # guard elements behind every output
DEV = torch.device("cuda:0")
CMD_SKIP = 8

CASES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_cases.json")))
MODES = {"fixed_resize": ("fixed", "resize"), "fixed_raw": ("fixed", "raw"), "fixed_mask": ("fixed", "mask"),
         "flex_resize": ("flexible", "resize"), "flex_raw": ("flexible", "raw"), "flex_mask": ("flexible", "mask"),
         "peripheral": ("peripheral", "resize")}


def _case_name(c):
    return "o{}x{}_f{}x{}_p{}x{}_aa{}".format(*c["obs"], *c["fov"], *c["per"], c["aa"])


def _label(v):
    """A plan label as part of a test id: the form and what selects it, without the LDS bytes."""
    v = re.sub(r" lds=\d+", "", v)
    return re.sub(r"[^A-Za-z0-9.+]+", ".", v.replace("<", "_").replace(">", "")).strip(".")


def _params(which):
    out = []
    for c in CASES:
        for key, label in c["plan"].items():
            if which == "refused" and not label.startswith("refused"):
                continue
            if which != "refused" and label.startswith("refused"):
                continue
            if which == "big" and key not in c["big"]:
                continue
            if which == "extras" and not c["extras"]:
                continue
            out.append(pytest.param(c, key, id=f"{_case_name(c)}-{key}-{_label(label)}"))
    return out


def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def _guarded(shape, dtype=torch.float32):
    """An output tensor of `shape` whose storage continues with TAIL sentinel elements; everything starts as SENTINEL."""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def _tail_ok(buf, n):
    tail = buf[n:]
    return torch.equal(tail, torch.full_like(tail, SENTINEL))


def _kw(case, key, mode):
    kind, out = MODES[key]
    oh, ow = case["obs"]
    fh, fw = case["fov"]
    kw = dict(obs_size=(oh, ow), fov_size=(fh, fw), fov_init_loc=(min(2, oh - fh), min(3, ow - fw)),
              sensory_action_mode=mode, sensory_action_space=(-7.0, 9.0) if mode == "relative" else None,
              antialias=bool(case["aa"]))
    if kind == "peripheral":
        kw["peripheral_res"] = tuple(case["per"])
    okw = dict(kw, resize_to_full=out == "resize", mask_out=out == "mask")
    pkw = dict(okw, kind=kind, frame_stack=case["fs"], device=DEV)
    return kind, out, okw, pkw


def _oracle(kind, okw):
    return {"fixed": O.FixedFovealOracle, "flexible": O.FlexibleFovealOracle, "peripheral": O.PeripheralOracle}[kind](**okw)


def _pipe(N, pkw, **extra):
    """A case the table says builds must build: a refusal by agx_create fails the test."""
    from active_gym import ObsPipeline
    return ObsPipeline(num_envs=N, **pkw, **extra)


def _loc_actions(rng, N, oh, ow, mode, step):
    """Float location actions: out of range on both sides, exact .5 ties, f32 or f64."""
    if mode == "absolute":
        a = rng.uniform(-6.0, max(oh, ow) + 6.0, (N, 2))
    else:
        a = rng.uniform(-12.0, 12.0, (N, 2))
    a[::3] = np.floor(a[::3]) + 0.5
    edge = [(-3.5, max(oh, ow) + 4.5), (max(oh, ow) + 2.5, -1.5), (0.5, 1.5), (2.5, 3.5)][step % 4]
    if mode == "relative":
        edge = [(-11.5, 11.5), (10.5, -8.5), (0.5, 1.5), (-2.5, 3.5)][step % 4]
    a[(step * 5) % N] = edge
    return a.astype(np.float32 if step % 2 else np.float64)


def _special_res(oh, ow, fh, fw):
    """Resolutions 1, fov, fov + 1, obs on each axis independently: rows squeeze (rh > fov_h) while columns do not, and the
    reverse (the reference tests rows only, fov_env.py:286)."""
    hs, ws = sorted({1, fh, fh + 1, oh}), sorted({1, fw, fw + 1, ow})
    return [(h, w) for h in hs for w in ws]


def _flex_actions(rng, N, oh, ow, fh, fw, mode, step, sample):
    """(action f64 [N,2], types i32 [N]): resolution actions walk the special list (env by env, step by step), the other
    envs draw random resolutions or float location actions."""
    types = rng.integers(0, 2, N).astype(np.int32)
    if step == 0:
        types[:] = 1
    a = _loc_actions(rng, N, oh, ow, mode, step).astype(np.float64)
    res = np.stack([rng.integers(1, oh + 1, N), rng.integers(1, ow + 1, N)], 1).astype(np.float64)
    spec = _special_res(oh, ow, fh, fw)
    ids = np.arange(N) if sample is None else np.asarray(sample)
    for j, i in enumerate(ids):
        if j % 2 == 0 or step == 0:
            res[i] = spec[(step * len(ids) + j) % len(spec)]
    a = np.where(types[:, None] == 1, res, a)
    return a, types


def _check_obs(kind, out, got, want, orc, fov, what):
    """One env's observation against the oracle's: bit-exact where nothing is resampled, FLOAT_TOL where it is."""
    want32 = want.astype(np.float32)
    if kind == "fixed":
        assert got.shape == want.shape, (what, got.shape, want.shape)
        if out == "resize":
            err = float(np.abs(got - want).max())
            assert err <= FLOAT_TOL, (what, err)
        else:
            assert np.array_equal(got, want32), what
        return
    r, c = int(orc.fov_loc[0]), int(orc.fov_loc[1])
    if kind == "peripheral":
        assert got.shape == want.shape, (what, got.shape, want.shape)
        err = float(np.abs(got - want).max())
        assert err <= FLOAT_TOL, (what, err)
        assert np.array_equal(got[..., r:r + fov[0], c:c + fov[1]], want32[..., r:r + fov[0], c:c + fov[1]]), (what, "window")
        return
    rh, rw = int(orc.fov_res[0]), int(orc.fov_res[1])
    squeezed = rh > fov[0]
    if out == "raw":
        assert not got[..., rh:, :].any() and not got[..., :, rw:].any(), (what, "padding outside fov_res is not zero")
        got = got[..., :rh, :rw]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if out == "mask":
        outside = np.ones(got.shape[-2:], bool)
        outside[r:r + rh, c:c + rw] = False
        assert not got[..., outside].any(), (what, "mask-out is not zero outside the window")
    if out != "resize" and not squeezed:
        assert np.array_equal(got, want32), (what, "unsqueezed crop is not bit-exact")
    else:
        err = float(np.abs(got - want).max()) if got.size else 0.0
        assert err <= FLOAT_TOL, (what, err, (rh, rw))


def _run(case, key, N, mode, seed, steps=4, sample=None, channels=1, packed_steps=0):
    """`steps` calls of one kind-mode of a case against per-env oracles: a random u8 ring every step, step 2 a masked call
    into a sentinel-filled output, a fovea_reset of a subset before step 3; then `packed_steps` calls of the packed ragged
    form on the same pipeline.  `sample`: the envs to check (all when None)."""
    kind, out, okw, pkw = _kw(case, key, mode)
    (oh, ow), (fh, fw), fs = case["obs"], case["fov"], case["fs"]
    rng = np.random.default_rng(seed)
    p = _pipe(N, pkw, channels=channels)
    ids = list(range(N)) if sample is None else list(sample)
    orcs = {i: _oracle(kind, okw) for i in ids}
    planes = (fs, 3) if channels == 3 else (fs,)

    def frames(st, i):
        return unit64(st[i]).reshape(-1, oh, ow)            # colour: every channel is a plane of its own

    def step_oracle(i, st, a, types):
        if kind == "flexible":
            return orcs[i].step(frames(st, i), a[i], np.array((types[i],)))
        return orcs[i].step(frames(st, i), a[i])

    loc_prev = None
    for step in range(steps):
        st = rng.integers(0, 256, (N,) + planes + (oh, ow), dtype=np.uint8)
        p.set_stack_u8(_t(st))
        extra, types = {}, None
        if kind == "flexible":
            a, types = _flex_actions(rng, N, oh, ow, fh, fw, mode, step, sample)
            extra = dict(action_type=_t(types))
        else:
            a = _loc_actions(rng, N, oh, ow, mode, step)
        mask = None
        if step == 2:
            mask = (rng.random(N) < 0.5).astype(np.uint8)
            mask[ids[0]] = 0
            if len(ids) > 1:
                mask[ids[1]] = 1
            extra["loc_out"] = loc_prev.clone()
        if step == 3:
            rs = (rng.random(N) < 0.4).astype(np.uint8)
            rs[ids[-1]] = 1
            p.fovea_reset(_t(rs))
            for i in ids:
                if rs[i]:
                    orcs[i].init_loc()
                    if kind == "flexible":
                        orcs[i].init_res()
        buf, o = _guarded(p.obs_shape)
        r = p.fovea(_t(a), mask=None if mask is None else _t(mask), out=o, **extra)
        torch.cuda.synchronize()
        assert _tail_ok(buf, o.numel()), f"step {step}: the launch wrote behind its output"
        obs, loc = o.cpu().numpy(), r[1].cpu().numpy()
        loc_prev = r[1]
        st_loc, st_res = (x.cpu().numpy() for x in p.fov_state())
        for i in ids:
            what = (_case_name(case), key, f"N={N}", mode, f"step {step}", f"env {i}")
            if mask is not None and not mask[i]:
                assert (obs[i] == SENTINEL).all(), (what, "a masked-out env was written")
            else:
                want = step_oracle(i, st, a, types)
                _check_obs(kind, out, obs[i].reshape((-1,) + obs[i].shape[-2:]), want, orcs[i], (fh, fw), what)
            assert np.array_equal(loc[i], orcs[i].fov_loc), (what, loc[i], orcs[i].fov_loc)
            assert np.array_equal(st_loc[i], orcs[i].fov_loc), (what, "state", st_loc[i], orcs[i].fov_loc)
            if kind == "flexible":
                if mask is None or mask[i]:
                    assert np.array_equal(r[2].cpu().numpy()[i], orcs[i].fov_res), (what, orcs[i].fov_res)
                assert np.array_equal(st_res[i], orcs[i].fov_res), (what, "state", st_res[i], orcs[i].fov_res)
    for step in range(steps, steps + packed_steps):
        st = rng.integers(0, 256, (N, fs, oh, ow), dtype=np.uint8)
        p.set_stack_u8(_t(st))
        a, types = _flex_actions(rng, N, oh, ow, fh, fw, mode, step, sample)
        cap = N * fs * oh * ow
        buf, flat = _guarded((cap,))
        if oh == ow and step % 2 == 1:
            # the whole step as one call, every env's command = SKIP: the ring set above stands
            scr = rng.integers(0, 256, (N, 2, 210, 160, 3), dtype=np.uint8)
            _, off, loc, res = p.step_flexible_packed(_t(scr), _t(np.full(N, CMD_SKIP, np.uint8)), _t(a), action_type=_t(types), packed=flat)
        else:
            _, off, loc, res = p.fovea_packed(_t(a), action_type=_t(types), packed=flat)
        torch.cuda.synchronize()
        assert _tail_ok(buf, cap), f"packed step {step}: the launch wrote behind its buffer"
        flat_n, off, loc, res = flat.cpu().numpy(), off.cpu().numpy(), loc.cpu().numpy(), res.cpu().numpy()
        sizes = np.zeros(N, np.int64)
        for i in ids:
            what = (_case_name(case), key, f"N={N}", mode, f"packed step {step}", f"env {i}")
            want = step_oracle(i, st, a, types)
            assert np.array_equal(loc[i], orcs[i].fov_loc) and np.array_equal(res[i], orcs[i].fov_res), what
            rh, rw = int(orcs[i].fov_res[0]), int(orcs[i].fov_res[1])
            sizes[i] = fs * rh * rw
            got = flat_n[off[i]:off[i + 1]].reshape(fs, rh, rw)
            if rh > fh:
                err = float(np.abs(got - want).max())
                assert err <= FLOAT_TOL, (what, err, (rh, rw))
            else:
                assert np.array_equal(got, want.astype(np.float32)), (what, "unsqueezed packed crop is not bit-exact")
        assert off[0] == 0 and np.array_equal(np.diff(off), sizes), (_case_name(case), key, "offsets are not the running sum of fs*rh*rw")
        assert (flat_n[off[N]:] == SENTINEL).all(), (_case_name(case), key, "written behind the last crop")
    p.close()


def _seed(request, *more):
    return zlib.crc32("/".join([request.node.name, *map(str, more)]).encode())


@pytest.mark.parametrize("case,key", _params("all"))
def test_form_vs_oracle(request, case, key):
    """N = 1 relative and N = 7 absolute (N = 1 absolute and N = 7 relative for the odd-numbered kind-modes), 4 steps each;
    flexible raw cases go on with the packed ragged form."""
    flip = zlib.crc32(request.node.name.encode()) & 1
    packed = 2 if key == "flex_raw" else 0
    for N, mode in ((1, "relative"), (7, "absolute")) if flip else ((1, "absolute"), (7, "relative")):
        _run(case, key, N, mode, _seed(request, N), packed_steps=packed)


@pytest.mark.parametrize("case,key", _params("big"))
def test_form_vs_oracle_full_size(request, case, key):
    """N = 1024 at a geometry that is not the headline one: first, last and 30 envs drawn by the case seed are checked."""
    N = 1024
    rng = np.random.default_rng(_seed(request, "sample"))
    sample = [0] + sorted(rng.choice(np.arange(1, N - 1), 30, replace=False).tolist()) + [N - 1]
    _run(case, key, N, "absolute", _seed(request, N), sample=sample)


@pytest.mark.parametrize("case,key", _params("extras"))
def test_form_colour_vs_oracle(request, case, key):
    """A colour context (channels = 3) against the oracle run on every channel."""
    _run(case, key, 3, "absolute", _seed(request, "rgb"), channels=3)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case,key", _params("extras"))
def test_form_16_bit_is_the_f32_output_cast_once(request, case, key, dtype):
    kind, out, okw, pkw = _kw(case, key, "absolute")
    (oh, ow), (fh, fw), fs = case["obs"], case["fov"], case["fs"]
    N = 5
    rng = np.random.default_rng(_seed(request))
    p32, p16 = _pipe(N, pkw), _pipe(N, pkw, obs_dtype=dtype)
    for step in range(3):
        st = _t(rng.integers(0, 256, (N, fs, oh, ow), dtype=np.uint8))
        p32.set_stack_u8(st)
        p16.set_stack_u8(st)
        extra = {}
        if kind == "flexible":
            a, types = _flex_actions(rng, N, oh, ow, fh, fw, "absolute", step, None)
            extra = dict(action_type=_t(types))
        else:
            a = _loc_actions(rng, N, oh, ow, "absolute", step)
        b32, o32 = _guarded(p32.obs_shape)
        b16, o16 = _guarded(p16.obs_shape, dtype)
        r32 = p32.fovea(_t(a), out=o32, **extra)
        r16 = p16.fovea(_t(a), out=o16, **extra)
        torch.cuda.synchronize()
        for x, y in zip(r32[1:], r16[1:]):
            assert torch.equal(x, y)
        assert torch.equal(_bits(o16), _bits(o32.to(dtype))), (_case_name(case), key, step)
        assert _tail_ok(b16, o16.numel()) and _tail_ok(b32, o32.numel())
    p32.close()
    p16.close()


@pytest.mark.parametrize("case,key", _params("refused"))
def test_geometry_over_the_lds_limit_is_refused_with_the_lds_message(case, key):
    from active_gym._native import AgxError
    kind, out, okw, pkw = _kw(case, key, "absolute")
    need = re.search(r"lds=(\d+)", case["plan"][key]).group(1)
    with pytest.raises(AgxError) as e:
        _pipe(1, pkw)
    assert f"geometry needs {need} B of LDS per workgroup" in str(e.value), str(e.value)
