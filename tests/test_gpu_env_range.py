"""GPU: launches over a range of envs (agx_env_range, include/agx_hostout.h).  A context that walks a partition of [0, N) in
ascending order, one call of an entry point per range, must leave bit for bit what a whole-batch context leaves: the ring
(agx_get_stack_u8), the fov state and the observations.  The whole-batch context is the reference: same library, same
inputs, so every comparison is exact equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INGESTS = ("rgb", "gray_raw", "rgb_compact", "gray_raw_compact", "small")
# every kind x out mode x antialias
CONFIGS = ([("base", "full", True)]
           + [("fixed", m, True) for m in ("raw", "resize", "mask")]
           + [("flexible", m, aa) for m in ("raw", "resize", "mask") for aa in (False, True)]
           + [("peripheral", "resize", aa) for aa in (False, True)])
# Every kind x out mode x antialias x dtype cell walks a partition with MORE than one range (3 or 8); each config runs at N = 1024
# in one of its two dtypes and at N = 37 in the other; absolute and relative actions both occur at N = 1024 in every fovea kind; the
# five ingest forms cycle through the 24 cells.  A few one-range walks (agx_env_range(0, N) set explicitly) come on top.
CASES = []
for _d, _dt in enumerate(("float32", "float16")):
    for _c, _cfg in enumerate(CONFIGS):
        CASES.append(_cfg + (_dt, INGESTS[(_c + 12 * _d) % 5], 1024 if (_c + _d) % 2 == 0 else 37, (3, 8)[(_c // 2 + _c + _d) % 2],
                             ((_c >> 1) + _d) % 2 == 1))
CASES += [("base", "full", True, "float16", "gray_raw", 37, 1, False), ("fixed", "raw", True, "float16", "rgb", 37, 1, True),
          ("flexible", "resize", True, "float32", "small", 1024, 1, False)]
# the table is what the comment says it is
for _cfg in CONFIGS:
    for _dt in ("float32", "float16"):
        assert any(c[:4] == _cfg + (_dt,) and c[6] > 1 for c in CASES), (_cfg, _dt)
    assert any(c[:3] == _cfg and c[5] == 1024 and c[6] > 1 for c in CASES) and any(c[:3] == _cfg and c[5] == 37 for c in CASES), _cfg
for _kind in ("fixed", "flexible", "peripheral"):
    for _rel in (False, True):
        assert any(c[0] == _kind and c[5] == 1024 and c[6] > 1 and c[7] == _rel for c in CASES), (_kind, _rel)
assert {c[4] for c in CASES if c[6] > 1} == set(INGESTS) and {c[6] for c in CASES} == {1, 3, 8}


def _pipe(kind, mode, aa, dtype, N, relative, **over):
    from active_gym import ObsPipeline
    kw = dict(num_envs=N, kind=kind, obs_size=(84, 84), frame_stack=4, device=torch.device(DEV), obs_dtype=dtype)
    if kind != "base":
        kw.update(fov_size=(30, 30), fov_init_loc=(3, 5), sensory_action_mode="relative" if relative else "absolute",
                  sensory_action_space=(-9, 9) if relative else None, resize_to_full=mode == "resize", mask_out=mode == "mask",
                  antialias=aa)
        if kind == "peripheral":
            kw["peripheral_res"] = (20, 20)
    kw.update(over)
    return ObsPipeline(**kw)


def _cuts(rng, N, parts):
    """`parts` ranges of unequal sizes covering [0, N), ascending."""
    while True:
        c = [0] + sorted(rng.choice(np.arange(1, N), parts - 1, replace=False).tolist()) + [N] if parts > 1 else [0, N]
        sizes = np.diff(c)
        if parts < 3 or len(set(sizes.tolist())) > 1:
            return [(int(c[k]), int(sizes[k])) for k in range(parts)]


def _screens(rng, pipe, form, N):
    rows = pipe.source_rows()
    if form == "small":
        return torch.from_numpy(rng.integers(0, 256, (N, 2, 84, 84), dtype=np.uint8)).to(DEV)
    gray = form.startswith("gray")
    full = rng.integers(0, 256, (N, 2, 210, 160) + (() if gray else (3,)), dtype=np.uint8)
    if form.endswith("compact"):
        full = np.ascontiguousarray(full[:, :, rows])
    return torch.from_numpy(full).to(DEV)


def _ingest(pipe, form, screens, cmd):
    {"rgb": pipe.ingest, "gray_raw": pipe.ingest_gray_raw, "rgb_compact": pipe.ingest_compact,
     "gray_raw_compact": pipe.ingest_gray_raw_compact, "small": pipe.ingest_gray}[form](screens, cmd)


def _cmd(rng, N, step):
    from active_gym import _native as nat
    cmd = rng.integers(0, 3, N).astype(np.uint8)                  # nvalid 0 | 1 | 2
    if step > 0:
        cmd[rng.random(N) < 0.2] |= nat.CMD_CLEAR
        cmd[rng.random(N) < 0.2] |= nat.CMD_SKIP
    return torch.from_numpy(cmd).to(DEV)


def _observe(pipe, kind, out, loc, res, action=None, types=None, mask=None):
    if kind == "base":
        pipe.observe_full(out)
    elif kind == "flexible":
        pipe.fovea(action, action_type=types, mask=mask, out=out, loc_out=loc, res_out=res)
    else:
        pipe.fovea(action, mask=mask, out=out, loc_out=loc)


def _same_state(a, b, kind, tag):
    assert torch.equal(a.stack_u8(), b.stack_u8()), f"{tag}: ring differs"
    if kind != "base":
        (la, ra), (lb, rb) = a.fov_state(), b.fov_state()
        assert torch.equal(la, lb), f"{tag}: fov_loc differs"
        assert torch.equal(ra, rb), f"{tag}: fov_res differs"


@pytest.mark.parametrize("kind,mode,aa,dtype,form,N,parts,relative", CASES)
def test_partition_walk_equals_whole_batch(kind, mode, aa, dtype, form, N, parts, relative):
    import zlib
    rng = np.random.default_rng(zlib.crc32(repr((kind, mode, aa, dtype)).encode()))
    whole = _pipe(kind, mode, aa, dtype, N, relative)
    ranged = _pipe(kind, mode, aa, dtype, N, relative)
    shape = whole.obs_shape if kind != "base" else whole.full_shape
    tdt = whole.obs_dtype
    outs = [torch.full(shape, -7.0, dtype=tdt, device=DEV) for _ in range(2)]
    locs = [torch.full((N, 2), -99, dtype=torch.int32, device=DEV) for _ in range(2)]
    ress = [torch.full((N, 2), -99, dtype=torch.int32, device=DEV) for _ in range(2)]
    for step in range(3):
        screens, cmd = _screens(rng, whole, form, N), _cmd(rng, N, step)
        action = types = None
        if kind != "base":
            a = rng.integers(-9, 10, (N, 2)) if relative else rng.uniform(-8, 70, (N, 2))
            action = torch.from_numpy(a.astype((np.int64, np.float32, np.float64)[step])).to(DEV)
            if kind == "flexible":
                types = torch.from_numpy(rng.integers(0, 2, N).astype(np.int32)).to(DEV)
                if not relative:                                      # a resolution action: a window size
                    action = torch.where(types[:, None] == 1, torch.from_numpy(rng.integers(4, 80, (N, 2))).to(DEV).to(action.dtype), action)
        cuts = _cuts(rng, N, parts)
        _ingest(whole, form, screens, cmd)
        for lo, n in cuts:                      # one entry point per walk, as the contract states it
            ranged.env_range(lo, n)
            _ingest(ranged, form, screens, cmd)
        ranged.env_range()
        _same_state(whole, ranged, kind, f"step {step} after ingest")
        _observe(whole, kind, outs[0], locs[0], ress[0], action, types)
        for lo, n in cuts:
            ranged.env_range(lo, n)
            _observe(ranged, kind, outs[1], locs[1], ress[1], action, types)
        ranged.env_range()
        assert torch.equal(outs[0], outs[1]), f"step {step}: observations differ"
        if kind != "base":
            assert torch.equal(locs[0], locs[1]) and (kind != "flexible" or torch.equal(ress[0], ress[1])), f"step {step}: fov rows differ"
        _same_state(whole, ranged, kind, f"step {step}")
    if kind != "base":
        # the autoreset tail's calls: fov state reset of a masked subset, masked re-observation without an action
        mask = torch.from_numpy((rng.random(N) < 0.4).astype(np.uint8)).to(DEV)
        cuts = _cuts(rng, N, parts)
        whole.fovea_reset(mask)
        for lo, n in cuts:
            ranged.env_range(lo, n)
            ranged.fovea_reset(mask)
        ranged.env_range()
        _same_state(whole, ranged, kind, "masked fovea_reset")
        _observe(whole, kind, outs[0], locs[0], ress[0], mask=mask)
        for lo, n in cuts:
            ranged.env_range(lo, n)
            _observe(ranged, kind, outs[1], locs[1], ress[1], mask=mask)
        ranged.env_range()
        assert torch.equal(outs[0], outs[1]) and torch.equal(locs[0], locs[1]), "masked re-observation differs"
        _same_state(whole, ranged, kind, "masked re-observation")
    whole.close()
    ranged.close()


@pytest.mark.parametrize("kind,mode", [("fixed", "resize"), ("flexible", "mask"), ("peripheral", "resize"), ("base", "full")])
def test_single_range_call_leaves_everything_else_untouched(kind, mode):
    """One ranged ingest + one ranged observation on a context with two steps of history: canary-filled output rows, the ring and
    the fov state of every env outside [lo, lo + n) are what they were; the envs inside changed."""
    N, lo, n = 37, 9, 13
    rng = np.random.default_rng(3)
    pipe = _pipe(kind, mode, True, "float32", N, False)
    shape = pipe.obs_shape if kind != "base" else pipe.full_shape
    out = torch.empty(shape, dtype=torch.float32, device=DEV)
    loc = torch.empty((N, 2), dtype=torch.int32, device=DEV)
    res = torch.empty((N, 2), dtype=torch.int32, device=DEV)
    two = torch.full((N,), 2, dtype=torch.uint8, device=DEV)
    for _ in range(2):
        pipe.ingest(_screens(rng, pipe, "rgb", N), two)
        act = torch.from_numpy(rng.uniform(0, 50, (N, 2)).astype(np.float32)).to(DEV)
        _observe(pipe, kind, out, loc, res, act, torch.zeros(N, dtype=torch.int32, device=DEV) if kind == "flexible" else None)
    ring0 = pipe.stack_u8().clone()
    state0 = [t.clone() for t in pipe.fov_state()] if kind != "base" else None
    out.fill_(-7.0)
    loc.fill_(-99)
    res.fill_(-99)
    pipe.env_range(lo, n)
    pipe.ingest(_screens(rng, pipe, "rgb", N), two)
    act = torch.from_numpy(rng.uniform(0, 50, (N, 2)).astype(np.float32) + 1.0).to(DEV)
    _observe(pipe, kind, out, loc, res, act, torch.zeros(N, dtype=torch.int32, device=DEV) if kind == "flexible" else None)
    pipe.env_range()
    outside = torch.ones(N, dtype=torch.bool, device=DEV)
    outside[lo:lo + n] = False
    assert bool((out[outside] == -7.0).all()), "an observation row outside the range was written"
    assert not bool((out[~outside] == -7.0).any()), "an observation row inside the range was not written"
    ring1 = pipe.stack_u8()
    assert torch.equal(ring1[outside], ring0[outside]), "the ring of an env outside the range changed"
    assert all(not torch.equal(ring1[i], ring0[i]) for i in range(lo, lo + n)), "the ring of an env inside the range did not change"
    if kind != "base":
        assert bool((loc[outside] == -99).all()) and not bool((loc[~outside] == -99).any())
        if kind == "flexible":
            assert bool((res[outside] == -99).all()) and not bool((res[~outside] == -99).any())
        l1, r1 = pipe.fov_state()
        assert torch.equal(l1[outside], state0[0][outside]) and torch.equal(r1[outside], state0[1][outside])
        assert torch.equal(l1[~outside], loc[~outside])
    pipe.close()


def test_refusals_and_argument_checks():
    from active_gym import _native as nat
    N = 16
    fixed = _pipe("fixed", "resize", True, "float32", N, False)
    for lo, n in ((-1, 4), (0, 0), (0, N + 1), (N, 1), (5, N - 4)):
        with pytest.raises(nat.AgxError) as e:
            fixed.env_range(lo, n)
        assert e.value.code == nat.E_INVALID, (lo, n)
    frames = torch.zeros((N, 2, 210, 160, 3), dtype=torch.uint8, device=DEV)
    cmd = torch.full((N,), 2, dtype=torch.uint8, device=DEV)
    fixed.env_range(4, 8)
    with pytest.raises(nat.AgxError) as e:
        fixed.step_fixed(frames, cmd)
    assert e.value.code == nat.E_STATE
    with pytest.raises(nat.AgxError) as e:
        fixed.ingest_rgb(torch.zeros((N, 84, 84, 3), dtype=torch.uint8, device=DEV), cmd)
    assert e.value.code == nat.E_STATE
    fixed.env_range()
    fixed.step_fixed(frames, cmd)                                     # the whole batch again: accepted
    fixed.close()
    flex = _pipe("flexible", "raw", True, "float32", N, False)
    flex.env_range(0, N - 1)
    for call in (lambda: flex.fovea_packed(), lambda: flex.step_flexible_packed(frames, cmd)):
        with pytest.raises(nat.AgxError) as e:
            call()
        assert e.value.code == nat.E_STATE
    flex.env_range(0, N)
    flex.step_flexible_packed(frames, cmd)
    flex.close()
    colour = _pipe("fixed", "resize", True, "float32", N, False, channels=3)
    with pytest.raises(nat.AgxError) as e:
        colour.env_range(2, 3)
    assert e.value.code == nat.E_STATE
    colour.env_range(0, N)                                            # the whole batch is what a colour context acts on anyway
    colour.close()
    torch.cuda.synchronize()


def test_whole_range_restored_equals_a_fresh_context():
    """After ranged calls and agx_env_range(0, N), a whole-batch step gives what a context that never saw a range gives."""
    N = 37
    rng = np.random.default_rng(8)
    used = _pipe("flexible", "resize", True, "float32", N, False)
    fresh = _pipe("flexible", "resize", True, "float32", N, False)
    two = torch.full((N,), 2, dtype=torch.uint8, device=DEV)
    types = torch.from_numpy(rng.integers(0, 2, N).astype(np.int32)).to(DEV)
    for step in range(3):
        screens = _screens(rng, used, "gray_raw", N)
        act = torch.from_numpy(rng.uniform(4, 60, (N, 2)).astype(np.float32)).to(DEV)
        fresh.ingest_gray_raw(screens, two)
        want = fresh.fovea(act, action_type=types)
        if step < 2:                         # two steps as ranges (descending order: any order leaves every env's state current)
            for lo, n in ((20, 17), (0, 20)):
                used.env_range(lo, n)
                used.ingest_gray_raw(screens, two)
            got = [torch.empty_like(t) for t in want]
            for lo, n in ((20, 17), (0, 20)):
                used.env_range(lo, n)
                used.fovea(act, action_type=types, out=got[0], loc_out=got[1], res_out=got[2])
            used.env_range(0, N)
        else:
            used.ingest_gray_raw(screens, two)
            got = used.fovea(act, action_type=types)
        for g, w in zip(got, want):
            assert torch.equal(g, w), step
    _same_state(used, fresh, "flexible", "restored")
    used.close()
    fresh.close()
