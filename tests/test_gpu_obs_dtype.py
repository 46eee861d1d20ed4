"""GPU: 16-bit observation outputs (obs_dtype bfloat16 / float16, AGX_OBS_* in the C ABI).  The contract: every 16-bit
observation is the float32 observation of the same inputs rounded to nearest-even once - ``out16 == out32.to(dtype)`` bit
for bit - whatever the kernel form, and a 16-bit launch writes nothing outside its rows."""
import random

import numpy as np
import pytest
import torch

from active_gym import _native as nat

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = -12345.0            # exactly representable in bf16 and f16
TAIL = 4096                    # guard elements behind every output


def _guarded(shape, dtype):
    """An output tensor of `shape` whose storage continues with TAIL sentinel elements; everything starts as SENTINEL."""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _same(out16, out32):
    """out16 == out32 rounded to out16's dtype, bit for bit (NaN-free data: integer compare of the bit patterns)."""
    want = out32.to(out16.dtype)
    if not torch.equal(_bits(out16), _bits(want)):
        d = (_bits(out16) != _bits(want)).nonzero()
        raise AssertionError(f"{d.shape[0]} elements differ, first at {d[0].tolist()}: "
                             f"{out16[tuple(d[0])].item()} vs {want[tuple(d[0])].item()} (f32 {out32[tuple(d[0])].item()})")


def _kw(kind, mode, aa, geom, fs, rel):
    obs, fov, per = geom
    kw = dict(kind=kind, obs_size=obs, frame_stack=fs, device=DEV)
    if kind != "base":
        kw.update(fov_size=fov, fov_init_loc=(1, 2), antialias=bool(aa),
                  sensory_action_mode="relative" if rel else "absolute",
                  sensory_action_space=(-9.0, 9.0) if rel else None,
                  resize_to_full=mode == "resize", mask_out=mode == "mask")
    if kind == "peripheral":
        kw["peripheral_res"] = per
    return kw


HEADLINE = ((84, 84), (30, 30), (20, 20))
SMALL = ((64, 64), (21, 19), (13, 11))          # odd raw crop (21 x 19): 16-bit rows of odd length


def _run_pair(N, kw, dtype, steps=5, seed=0):
    """Two pipelines of the same config, float32 and `dtype`, fed identical inputs: CLEAR / SKIP / nvalid 0, 1, 2 commands,
    absolute or relative (and for the flexible kind resolution) actions, masked calls.  Every step compares the outputs and
    checks the guard tail and the masked-out rows."""
    from active_gym import ObsPipeline
    p32 = ObsPipeline(num_envs=N, obs_dtype=torch.float32, **kw)
    p16 = ObsPipeline(num_envs=N, obs_dtype=dtype, **kw)
    assert p16.obs_dtype is dtype and p32.obs_dtype is torch.float32
    kind = kw["kind"]
    shape = p32.full_shape if kind == "base" else p32.obs_shape
    rng = np.random.default_rng(seed)
    obs_h, obs_w = kw["obs_size"]
    for step in range(steps):
        frames = torch.from_numpy(rng.integers(0, 256, (N, 2, nat.RAW_H, nat.RAW_W, 3), dtype=np.uint8)).to(DEV)
        cmd = rng.integers(0, 3, N).astype(np.uint8)                              # nvalid 0 / 1 / 2
        if step == 0:
            cmd[:] = 2 | nat.CMD_CLEAR
        else:
            cmd[rng.random(N) < 0.15] |= nat.CMD_CLEAR
            cmd[rng.random(N) < 0.15] |= nat.CMD_SKIP
        cmd = torch.from_numpy(cmd).to(DEV)
        p32.ingest(frames, cmd)
        p16.ingest(frames, cmd)
        b32, o32 = _guarded(shape, torch.float32)
        b16, o16 = _guarded(shape, dtype)
        mask = None
        if kind == "base":
            p32.observe_full(o32)
            p16.observe_full(o16)
        else:
            act = torch.from_numpy(rng.uniform(-12, obs_h + 12, (N, 2)).astype(np.float32)).to(DEV)
            if step % 2 == 1:
                m = (rng.random(N) < 0.6).astype(np.uint8)
                m[0] = 0
                mask = torch.from_numpy(m).to(DEV)
            extra = {}
            if kind == "flexible":
                types = torch.from_numpy(rng.integers(0, 2, N).astype(np.int32)).to(DEV)
                act = torch.where(types[:, None] == 1, torch.from_numpy(rng.integers(4, obs_h - 3, (N, 2)).astype(np.float32)).to(DEV), act)
                extra = dict(action_type=types)
            if kind == "flexible":
                extra.update(res_out=torch.zeros((N, 2), dtype=torch.int32, device=DEV))
            r32 = p32.fovea(act.contiguous(), mask=mask, out=o32, loc_out=torch.zeros((N, 2), dtype=torch.int32, device=DEV), **extra)
            if kind == "flexible":
                extra.update(res_out=torch.zeros((N, 2), dtype=torch.int32, device=DEV))
            r16 = p16.fovea(act.contiguous(), mask=mask, out=o16, loc_out=torch.zeros((N, 2), dtype=torch.int32, device=DEV), **extra)
            for a, b in zip(r32[1:], r16[1:]):
                assert torch.equal(a, b)
        torch.cuda.synchronize()
        _same(o16, o32)
        tail = b16[o16.numel():]
        assert torch.equal(tail, torch.full_like(tail, SENTINEL)), f"step {step}: a 16-bit launch wrote past its output"
        if mask is not None:
            off = (mask == 0).nonzero().flatten()
            assert torch.equal(o16[off], torch.full_like(o16[off], SENTINEL)), "masked-out envs must keep their rows"
    torch.cuda.synchronize()
    assert torch.equal(p32.stack_u8(), p16.stack_u8())
    p32.close()
    p16.close()


CASES = [("base", None, 1)] + [("fixed", m, 1) for m in ("raw", "resize", "mask")] + \
        [("flexible", m, aa) for m in ("raw", "resize", "mask") for aa in (0, 1)] + [("peripheral", "resize", aa) for aa in (0, 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("kind,mode,aa", CASES)
def test_every_kind_and_mode_equals_f32_cast(kind, mode, aa, dtype):
    _run_pair(5, _kw(kind, mode, aa, HEADLINE, 4, rel=False), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("kind,mode,aa", CASES)
@pytest.mark.parametrize("fs", [1, 3])
def test_other_geometry_relative_actions(kind, mode, aa, dtype, fs):
    _run_pair(5, _kw(kind, mode, aa, SMALL, fs, rel=True), dtype, seed=fs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("kind,mode,aa", [c for c in CASES if c[0] in ("flexible", "peripheral")])
def test_generic_fallback_kernels(kind, mode, aa, dtype, monkeypatch):
    monkeypatch.setenv("AGX_FOVEA_GENERIC", "1")          # read once per context, in agx_create
    _run_pair(3, _kw(kind, mode, aa, HEADLINE, 4, rel=False), dtype, steps=3)
    _run_pair(1, _kw(kind, mode, aa, SMALL, 3, rel=True), dtype, steps=3)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("kind,mode,aa", [("base", None, 1), ("fixed", "resize", 1), ("fixed", "raw", 1), ("flexible", "resize", 1),
                                          ("peripheral", "resize", 1)])
def test_batch_sizes(kind, mode, aa, dtype):
    _run_pair(1, _kw(kind, mode, aa, HEADLINE, 4, rel=False), dtype, steps=3)
    _run_pair(1024, _kw(kind, mode, aa, HEADLINE, 4, rel=False), dtype, steps=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("mode", ["resize", "raw", "mask"])
def test_step_fixed_equals_the_two_calls(dtype, mode):
    from active_gym import ObsPipeline
    N = 37
    kw = _kw("fixed", mode, 1, HEADLINE, 4, rel=False)
    a = ObsPipeline(num_envs=N, obs_dtype=dtype, **kw)
    b = ObsPipeline(num_envs=N, obs_dtype=dtype, **kw)
    c = ObsPipeline(num_envs=N, obs_dtype=torch.float32, **kw)
    rng = np.random.default_rng(5)
    for step in range(4):
        frames = torch.from_numpy(rng.integers(0, 256, (N, 2, nat.RAW_H, nat.RAW_W, 3), dtype=np.uint8)).to(DEV)
        cmd = torch.from_numpy(np.full(N, 2 | (nat.CMD_CLEAR if step == 0 else 0), np.uint8)).to(DEV)
        act = torch.from_numpy(rng.uniform(-5, 60, (N, 2)).astype(np.float32)).to(DEV)
        oa, la = a.step_fixed(frames, cmd, act)
        b.ingest(frames, cmd)
        ob, lb = b.fovea(act)
        oc, lc = c.step_fixed(frames, cmd, act)
        torch.cuda.synchronize()
        assert oa.dtype is dtype and torch.equal(_bits(oa), _bits(ob)) and torch.equal(la, lb) and torch.equal(la, lc)
        _same(oa, oc)


def test_algorithmic_bytes_count_the_element_size():
    from active_gym import ObsPipeline
    N, fs, px, win = 8, 4, 84 * 84, 30 * 30
    kw = _kw("fixed", "resize", 1, HEADLINE, fs, rel=False)
    for dt, e in ((torch.float32, 4), (torch.bfloat16, 2), (torch.float16, 2)):
        p = ObsPipeline(num_envs=N, obs_dtype=dt, **kw)
        assert p.algorithmic_bytes("fovea") == N * fs * (win + px * e)
        assert p.algorithmic_bytes("full") == N * fs * px * (1 + e)
        p.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_graph_replay_of_a_16bit_step(dtype):
    from active_gym import ObsPipeline
    n = 33
    kw = _kw("fixed", "resize", 1, HEADLINE, 4, rel=False)
    rng = np.random.default_rng(2)
    frames = [torch.from_numpy(rng.integers(0, 256, (n, 2, nat.RAW_H, nat.RAW_W, 3), dtype=np.uint8)).to(DEV) for _ in range(4)]
    cmds = [torch.from_numpy(np.full(n, 2 | (nat.CMD_CLEAR if i == 0 else 0), np.uint8)).to(DEV) for i in range(4)]
    acts = [torch.from_numpy(rng.uniform(-5, 60, (n, 2)).astype(np.float32)).to(DEV) for _ in range(4)]

    def make():
        p = ObsPipeline(num_envs=n, obs_dtype=dtype, **kw)
        obs = torch.empty(p.obs_shape, dtype=dtype, device=DEV)
        loc = torch.empty((n, 2), dtype=torch.int32, device=DEV)
        return p, (lambda i: p.step_fixed(frames[i], cmds[i], acts[i], out=obs, loc_out=loc)), obs, loc

    pa, sa, oa, la = make()
    pb, sb, ob, lb = make()
    for i in (0, 1, 2, 3, 0, 1, 2, 3):
        sb(i)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in (0, 1):
            sa(i)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        for i in (2, 3, 0, 1):
            sa(i)
    graph.replay()
    for i in (2, 3):                    # launch by launch after the replay, on the stream the replay ran on
        sa(i)
    torch.cuda.synchronize()
    assert torch.equal(pa.stack_u8(), pb.stack_u8()) and torch.equal(la, lb)
    assert torch.equal(_bits(oa), _bits(ob))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_packed_ragged_crops_are_f32_only(dtype):
    from active_gym import ObsPipeline
    N = 4
    p = ObsPipeline(num_envs=N, obs_dtype=dtype, **_kw("flexible", "raw", 1, HEADLINE, 4, rel=False))
    with pytest.raises(nat.AgxError) as e:
        p.fovea_packed()
    assert e.value.code == nat.E_STATE
    screens = torch.zeros((N, 2, nat.RAW_H, nat.RAW_W, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(nat.AgxError) as e:
        p.step_flexible_packed(screens, torch.full((N,), 2, dtype=torch.uint8, device=DEV))
    assert e.value.code == nat.E_STATE
    p.close()


def test_out_tensors_are_checked_at_the_pipeline_dtype():
    from active_gym import ObsPipeline
    p = ObsPipeline(num_envs=2, obs_dtype="bfloat16", **_kw("fixed", "resize", 1, HEADLINE, 4, rel=False))
    with pytest.raises(TypeError):
        p.fovea(out=torch.empty(p.obs_shape, dtype=torch.float32, device=DEV))
    assert p.fovea()[0].dtype is torch.bfloat16
    p.close()


# ---------------------------------------------------------------- envs
def _env_kw(**kw):
    base = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2),
                sensory_action_mode="absolute", resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2,
                scripted_actions=4, scripted_lives=1, scripted_p_life=0, scripted_p_over=150)
    base.update(kw)
    return base


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("kind,extra", [("fixed", {}), ("fixed", dict(native_loop=False)), ("base", {}),
                                        ("flexible", dict(resize_to_full=False, mask_out=True)),
                                        ("fixed", dict(resize_to_full=False, fov_size=(5, 7), frame_stack=3))])   # odd 16-bit rows
def test_vec_env_with_autoreset_equals_f32_env(dtype, kind, extra):
    from active_gym import AtariEnvArgs, AtariVecEnv
    N = 24
    kw = _env_kw(**extra)
    a = AtariVecEnv(AtariEnvArgs(obs_dtype=dtype, **kw), N, kind=kind, noop_fn=lambda: 2)
    b = AtariVecEnv(AtariEnvArgs(**kw), N, kind=kind, noop_fn=lambda: 2)
    tdt = getattr(torch, dtype)
    assert a.obs_dtype is tdt and b.obs_dtype is torch.float32
    assert (a._loop is None) == (b._loop is None) == (extra.get("native_loop", True) is False)
    oa, ob = a.reset()[0], b.reset()[0]
    assert oa.dtype is tdt
    _same(oa, ob)
    assert a.single_observation_space.dtype == (np.float16 if dtype == "float16" else np.float32)
    rng = np.random.default_rng(0)
    seen = 0
    for step in range(14):
        if kind == "base":
            act = rng.integers(0, 4, N)
        else:
            act = {"motor_action": rng.integers(0, 4, N), "sensory_action": rng.uniform(-5, 60, (N, 2)).astype(np.float32)}
            if kind == "flexible":
                act["sensory_action_type"] = rng.integers(0, 2, N)
        ra, rb = a.step(act), b.step(act)
        _same(ra[0], rb[0])
        assert np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
        for i in np.nonzero(ra[2])[0]:
            fa, fb = ra[4]["final_observation"][i], rb[4]["final_observation"][i]
            assert fa.dtype is tdt
            _same(fa, fb)
            seen += 1
    assert seen >= 5
    a.close()
    b.close()


def test_host_float16_outputs_equal_np_float16_of_f32():
    from active_gym import AtariEnvArgs, AtariVecEnv
    N = 16                                   # above the host pool's threshold: pinned float16 buffers
    kw = _env_kw(device=None)
    a = AtariVecEnv(AtariEnvArgs(obs_dtype="float16", **kw), N, kind="fixed", noop_fn=lambda: 2)
    b = AtariVecEnv(AtariEnvArgs(**kw), N, kind="fixed", noop_fn=lambda: 2)
    oa, ob = a.reset()[0], b.reset()[0]
    assert isinstance(oa, np.ndarray) and oa.dtype == np.float16
    assert np.array_equal(oa.view(np.uint16), ob.astype(np.float16).view(np.uint16))
    assert a.observation_space.dtype == np.float16
    rng = np.random.default_rng(1)
    for _ in range(6):
        act = {"motor_action": rng.integers(0, 4, N), "sensory_action": rng.uniform(-5, 60, (N, 2)).astype(np.float32)}
        ra, rb = a.step(act), b.step(act)
        assert ra[0].dtype == np.float16
        assert np.array_equal(ra[0].view(np.uint16), rb[0].astype(np.float16).view(np.uint16))
    a.close()
    b.close()


def test_single_env_fixed_fovea_float16():
    from active_gym import AtariEnvArgs, AtariFixedFovealEnv
    kw = dict(game="g", seed=5, obs_size=(84, 84), fov_size=(30, 30), fov_init_loc=(0, 0), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", scripted_actions=4)
    a = AtariFixedFovealEnv(AtariEnvArgs(obs_dtype="float16", **kw))
    b = AtariFixedFovealEnv(AtariEnvArgs(**kw))
    assert a.observation_space.dtype == np.float16 and b.observation_space.dtype == np.float32
    random.seed(4)                      # the reset no-ops come from the reference's process-global stream: the same draws for both
    oa = a.reset()[0]
    random.seed(4)
    ob = b.reset()[0]
    assert oa.dtype == np.float16 and np.array_equal(oa.view(np.uint16), ob.astype(np.float16).view(np.uint16))
    rng = np.random.default_rng(3)
    for _ in range(5):
        act = {"motor_action": int(rng.integers(0, 4)), "sensory_action": rng.uniform(0, 54, 2).astype(np.float32)}
        ra, rb = a.step(act), b.step(act)
        assert np.array_equal(ra[0].view(np.uint16), rb[0].astype(np.float16).view(np.uint16))
    a.close()
    b.close()


def test_dmc_vec_env_bfloat16():
    from fake_dmc import ScriptedDMC

    from active_gym import DMCEnvArgs
    from active_gym.dmc_env import DMCVecEnv
    N = 5

    def args(**kw):
        return DMCEnvArgs(domain_name="scripted", task_name="t", seed=4, obs_size=(12, 16), device="cuda:0",
                          frame_source=lambda a, i: ScriptedDMC(a.seed + i, episode_len=7), **kw)
    a = DMCVecEnv(args(obs_dtype="bfloat16"), N, kind="base")
    b = DMCVecEnv(args(), N, kind="base")
    assert a.obs_dtype is torch.bfloat16
    _same(a.reset()[0], b.reset()[0])
    rng = np.random.default_rng(0)
    for _ in range(10):
        act = rng.uniform(-1, 1, (N, a.single_action_space.shape[0])).astype(np.float32)
        ra, rb = a.step(act), b.step(act)
        _same(ra[0], rb[0])
        for i in np.nonzero(ra[2])[0]:
            _same(ra[4]["final_observation"][i], rb[4]["final_observation"][i])
    a.close()
    b.close()
