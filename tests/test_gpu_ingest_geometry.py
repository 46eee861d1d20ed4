"""GPU: every K1 ingest form against the oracle, each form reached the way a user reaches it - by obs_size.

agx_create picks the K1 form (band12 or the general band kernel, rows per band, affine or tabled source rows) from obs_size
alone.  tests/golden/ingest_cases.json lists sizes and the form each of the four screen layouts selects there (pinned on
the CPU by tests/test_ingest_plan_cpu.py, which also says what the table must reach); here every case runs through libagx in
every layout and is compared with oracle.oracle: ALE luminance -> OpenCV fixed-point resize -> max of the sampled frames ->
frame-stack ring.  K1 is integer work: every comparison is byte for byte, no tolerance anywhere.  No knob is set, except in
the test that forces the general kernel where band12 applies.

The RNG seed of a test is derived from its id, so one case can be re-run alone:
``pytest tests/test_gpu_ingest_geometry.py -k o212_fs4_n5-rgb-compact``."""
import functools
import json
import os
import re
import zlib

import numpy as np
import pytest
import torch

from golden_util import tie_pixels
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CMD_CLEAR, CMD_SKIP = 4, 8
RAW_H, RAW_W = 210, 160
LAYOUTS = ("rgb", "gray", "rgb-compact", "gray-compact")

CASES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest_cases.json")))
BY_SIZE = {c["obs"]: c for c in CASES}
_ties = functools.lru_cache(None)(tie_pixels)


def _case_name(c):
    return "o{}_fs{}_n{}".format(c["obs"], c["fs"], c["n"])


def _label(v):
    return re.sub(r"[^A-Za-z0-9]+", ".", v).strip(".")


def _id(c, layout):
    return f"{_case_name(c)}-{layout}-{_label(c['plan'][layout])}"


def _seed(request, *more):
    return zlib.crc32("/".join([request.node.name, *map(str, more)]).encode())


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pipe(n, obs, fs, **kw):
    from active_gym import ObsPipeline
    return ObsPipeline(num_envs=n, obs_size=(obs, obs), frame_stack=fs, device=DEV, **{"kind": "base", **kw})


def _screens(rng, n, gray):
    """Whole screens u8 [n, 2, 210, 160(, 3)]: random, RGB ones sprinkled with exact .5 luminance ties; rows of 0 and of 255;
    the last source row and the last source column the complement of their neighbours, so that a tap clamped one short
    (or one too far) changes the result."""
    ties = _ties()
    assert len(ties) > 50
    fr = rng.integers(0, 256, (n, 2, RAW_H, RAW_W) + (() if gray else (3,)), dtype=np.uint8)
    if not gray:
        mask = rng.random((n, 2, RAW_H, RAW_W)) < 0.02
        fr[mask] = ties[rng.integers(0, len(ties), int(mask.sum()))]
    fr[0, 0, :20] = 255
    fr[0, 1, :20] = 0
    fr[n - 1, 0, 100:109] = 0
    fr[n - 1, 1, 100:109] = 255
    fr[:, :, RAW_H - 1] = 255 - fr[:, :, RAW_H - 2]
    fr[:, :, :, RAW_W - 1] = 255 - fr[:, :, :, RAW_W - 2]
    return fr


def _commands(rng, n, fs, step):
    """(nvalid, clear, skip) u8 [n]: random NVALID 0 / 1 / 2, CLEAR (with nvalid 1, as a reset issues it) and SKIP.  Step 0
    skips nothing.  Env 0 is neither cleared nor skipped while its ring fills, and gets CLEAR on the step after it has
    wrapped (step fs); env 1 is skipped on steps 1 and 2."""
    nvalid = rng.integers(0, 3, n).astype(np.uint8)
    clear = (rng.random(n) < 0.2).astype(np.uint8)
    skip = (rng.random(n) < 0.2).astype(np.uint8)
    if step == 0:
        skip[:] = 0
    clear[0] = 1 if step == fs else 0
    skip[0] = 0
    if n > 1 and step in (1, 2):
        skip[1] = 1
    nvalid[clear == 1] = 1
    return nvalid, clear, skip


def _ingest(p, layout, whole, rows, cmd):
    """One ingest of `whole` screens through the entry point of `layout` (compact: only the rows the resize reads)."""
    scr = _t(whole[:, :, rows] if "compact" in layout else whole)
    {"rgb": p.ingest, "gray": p.ingest_gray_raw, "rgb-compact": p.ingest_compact, "gray-compact": p.ingest_gray_raw_compact}[layout](scr, cmd)
    return scr


def _check_rows(p, obs):
    rows = p.source_rows()
    ty = O.cv_tables_y(RAW_H, obs)
    assert np.array_equal(rows, np.unique(np.concatenate([ty[0], ty[1]]))), "agx_source_rows vs the oracle's cv2 row table"
    return rows


def _params():
    return [pytest.param(c, lay, id=_id(c, lay)) for c in CASES for lay in LAYOUTS]


@pytest.mark.parametrize("case,layout", _params())
def test_ingest_form_vs_oracle(request, case, layout):
    """fs + 3 steps (the ring wraps) of one layout of one case against a RingOracle fed the same whole screens: RGB layouts
    against luminance + resize (O.get_state_u8), gray layouts against the resize of the same gray screens
    (O.cv_resize_linear_u8); the compact layouts against the oracle too, which reads the whole screens."""
    obs, fs, n = case["obs"], case["fs"], case["n"]
    gray = layout.startswith("gray")
    rng = np.random.default_rng(_seed(request))
    p = _pipe(n, obs, fs)
    rows = _check_rows(p, obs)
    ring = O.RingOracle(n, fs, (obs, obs))
    wrapped_clear = double_skip = False
    prev_skip = np.zeros(n, np.uint8)
    for step in range(fs + 3):
        whole = _screens(rng, n, gray)
        nvalid, clear, skip = _commands(rng, n, fs, step)
        wrapped_clear |= step == fs and bool(clear[0]) and not skip[0]
        double_skip |= bool((skip & prev_skip).any())
        prev_skip = skip
        _ingest(p, layout, whole, rows, _t((nvalid | clear * CMD_CLEAR | skip * CMD_SKIP).astype(np.uint8)))
        ring.ingest(whole, nvalid, clear=clear, skip=skip, gray=gray)
        got, want = p.stack_u8().cpu().numpy(), ring.stack_u8()
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{request.node.name} step {step}: {len(bad)} bytes differ, first at (env, slot, row, col) "
                                 f"{bad[0].tolist()}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}; "
                                 f"cmd {(nvalid | clear * CMD_CLEAR | skip * CMD_SKIP).tolist()}")
    assert wrapped_clear and (double_skip or n == 1)
    assert ring.stack_u8().any()
    full = p.observe_full().cpu().numpy()
    assert full.dtype == np.float32 and np.array_equal(full, O.u8_to_unit(ring.stack_u8()))
    p.close()


# ---------------------------------------------------------------- one-call steps at K1 forms off the headline one
# (size, fov): a tiny size with tabled source rows, a size with affine rows and fewer than 12 rows per band, an up-scaling
# size with more than 256 columns (x-table tail loop, 3-row bands).  All three are sizes of the case table.
STEP_GEOMS = [(20, 8), (100, 30), (264, 20)]
# agx_create refuses a flexible context whose generic-kernel LDS plan (two f32 frames) exceeds the 160 KiB limit: obs > 143.
# agx_step_flexible_packed therefore cannot reach an up-scaling K1 form; 140 (7-row bands) is the largest table size it reaches.
PACKED_GEOMS = [(20, 8), (100, 30), (140, 30)]


def _rgb_label(obs):
    return _label(BY_SIZE[obs]["plan"]["rgb"])


@pytest.mark.parametrize("obs,fov", [pytest.param(o, f, id=f"o{o}_f{f}-{_rgb_label(o)}") for o, f in STEP_GEOMS])
def test_step_fixed_equals_ingest_then_fovea(request, obs, fov):
    """agx_step_fixed (whole RGB screens) == agx_ingest then agx_fovea_fixed, bit for bit, and its ring == the oracle's."""
    n, fs = 5, 3
    rng = np.random.default_rng(_seed(request))
    kw = dict(kind="fixed", fov_size=(fov, fov), fov_init_loc=(1, 2), resize_to_full=True, sensory_action_mode="relative",
              sensory_action_space=(-9.0, 9.0))
    a, b = _pipe(n, obs, fs, **kw), _pipe(n, obs, fs, **kw)
    ring = O.RingOracle(n, fs, (obs, obs))
    for step in range(fs + 3):
        whole = _screens(rng, n, False)
        nvalid, clear, skip = _commands(rng, n, fs, step)
        cmd = _t((nvalid | clear * CMD_CLEAR | skip * CMD_SKIP).astype(np.uint8))
        act = _t(rng.uniform(-11, 11, (n, 2)))
        scr = _t(whole)
        oa, la = a.step_fixed(scr, cmd, act)
        b.ingest(scr, cmd)
        ob, lb = b.fovea(act)
        ring.ingest(whole, nvalid, clear=clear, skip=skip)
        assert torch.equal(la, lb), step
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), f"step {step}: agx_step_fixed != ingest + fovea"
        assert torch.equal(a.stack_u8(), b.stack_u8()), step
        assert np.array_equal(a.stack_u8().cpu().numpy(), ring.stack_u8()), step
    a.close()
    b.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("obs,fov", [pytest.param(o, f, id=f"o{o}_f{f}-{_rgb_label(o)}") for o, f in PACKED_GEOMS])
def test_step_flexible_packed_equals_ingest_then_packed_fovea(request, obs, fov, layout):
    """agx_step_flexible_packed == agx_ingest* then agx_fovea_flexible_packed, bit for bit, in every screen layout: the
    three-launch form the call takes wherever the band12 plan does not apply.  The ring is held against the oracle as well."""
    n, fs = 5, 3
    gray = layout.startswith("gray")
    rng = np.random.default_rng(_seed(request))
    kw = dict(kind="flexible", fov_size=(fov, fov), fov_init_loc=(1, 2), resize_to_full=False, mask_out=False,
              sensory_action_mode="absolute", antialias=True)
    a, b = _pipe(n, obs, fs, **kw), _pipe(n, obs, fs, **kw)
    rows = _check_rows(a, obs)
    ring = O.RingOracle(n, fs, (obs, obs))
    cap = n * fs * obs * obs
    for step in range(fs + 3):
        whole = _screens(rng, n, gray)
        nvalid, clear, skip = _commands(rng, n, fs, step)
        cmd = _t((nvalid | clear * CMD_CLEAR | skip * CMD_SKIP).astype(np.uint8))
        types = rng.integers(0, 2, n).astype(np.int32)
        res = np.stack([rng.integers(1, obs + 1, n), rng.integers(1, obs + 1, n)], 1).astype(np.float64)
        act = _t(np.where(types[:, None] == 1, res, rng.uniform(-5.0, obs + 5.0, (n, 2))))
        scr = _ingest(a, layout, whole, rows, cmd)
        pa, offa, la, ra = a.fovea_packed(act, action_type=_t(types), packed=torch.zeros(cap, dtype=torch.float32, device=DEV))
        pb, offb, lb, rb = b.step_flexible_packed(scr, cmd, act, action_type=_t(types), packed=torch.zeros(cap, dtype=torch.float32, device=DEV))
        ring.ingest(whole, nvalid, clear=clear, skip=skip, gray=gray)
        assert torch.equal(offa, offb) and torch.equal(la, lb) and torch.equal(ra, rb), step
        assert int(offa[-1]) == int((fs * ra[:, 0].long() * ra[:, 1].long()).sum())
        assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), f"step {step}: the one call != ingest + packed fovea"
        assert torch.equal(a.stack_u8(), b.stack_u8()), step
        assert np.array_equal(b.stack_u8().cpu().numpy(), ring.stack_u8()), step
    a.close()
    b.close()


def test_flexible_context_is_refused_where_k1_up_scales():
    """Why PACKED_GEOMS stops at 140: no flexible context exists at an up-scaling obs_size (>= 212)."""
    from active_gym._native import AgxError
    with pytest.raises(AgxError, match="of LDS per workgroup"):
        _pipe(1, 264, 3, kind="flexible", fov_size=(20, 20), fov_init_loc=(0, 0), resize_to_full=False, sensory_action_mode="absolute")


# ---------------------------------------------------------------- the general kernel where band12 applies
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("obs", [60, 72])
def test_forced_general_kernel_equals_band12(request, obs, layout, monkeypatch):
    """AGX_INGEST_NO_FULL=1 at the band12 sizes tests/test_gpu_parity.py does not force: same ring as the default run."""
    assert BY_SIZE[obs]["plan"][layout].startswith("band12 ")
    n, fs = 7, 3
    gray = layout.startswith("gray")
    monkeypatch.delenv("AGX_INGEST_NO_FULL", raising=False)
    d = _pipe(n, obs, fs)
    monkeypatch.setenv("AGX_INGEST_NO_FULL", "1")
    g = _pipe(n, obs, fs)
    rows = _check_rows(d, obs)
    rng = np.random.default_rng(_seed(request))
    for step in range(fs + 3):
        whole = _screens(rng, n, gray)
        nvalid, clear, skip = _commands(rng, n, fs, step)
        cmd = _t((nvalid | clear * CMD_CLEAR | skip * CMD_SKIP).astype(np.uint8))
        _ingest(d, layout, whole, rows, cmd)
        _ingest(g, layout, whole, rows, cmd)
        assert torch.equal(d.stack_u8(), g.stack_u8()), step
    assert d.stack_u8().any()
    d.close()
    g.close()
