"""GPU: colour DMC pixel observations (AGX_FRAME_RGB, agx_ingest_rgb with AGX_GRAY_NONE, DMCVecEnv / DMC*Env with grey=False).

The colour path is the gray path applied to 3 planes per frame ("colour DMC observations"), so its
strongest check is an identity: channel c of every colour output equals, bit for bit, the output of a gray context with the
same configuration and the same actions that is fed channel c of the renders (agx_ingest_gray, nvalid 1).  The gray path
itself is pinned against the reference by tests/test_gpu_parity.py and tests/test_gpu_dmc.py."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from fake_dmc import ScriptedDMC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bits(t):
    t = t.detach().cpu()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy()
    return t.numpy().view(np.uint32)


def _cmds(rng, n, step):
    """step 0: full reset of every env; later steps: appends with some SKIP / CLEAR / nvalid-0 envs."""
    from active_gym import _native as nat
    if step == 0:
        return np.full(n, nat.CMD_CLEAR | 1, np.uint8)
    cmd = np.ones(n, np.uint8)
    u = rng.random(n)
    cmd[u < 0.15] = nat.CMD_SKIP | 1
    cmd[(u >= 0.15) & (u < 0.25)] = nat.CMD_CLEAR | 1
    cmd[(u >= 0.25) & (u < 0.35)] = 0                      # nvalid 0: a zero frame is appended
    return cmd


# ---------------------------------------------------------------------------------------------------------- 1. ingest
@pytest.mark.parametrize("n,obs,fs", [(1, (84, 84), 3), (5, (84, 84), 1), (5, (12, 16), 4), (1024, (84, 84), 3), (5, (36, 48), 3),
                                      (5, (10, 12), 3)])      # 120 px: not a multiple of 16, the dword form of the planar ingest
def test_colour_ingest_stack_and_full(n, obs, fs):
    """observe_full / stack_u8 of a colour pipeline = the renders transposed to CHW, /255, stack-ordered (oldest first)."""
    from active_gym import ObsPipeline, _native as nat
    pipe = ObsPipeline(num_envs=n, kind="base", obs_size=obs, frame_stack=fs, device=DEV, channels=3)
    assert pipe.full_shape == (n, fs, 3) + obs
    rng = np.random.default_rng(n * 7 + fs)
    ring = np.zeros((n, fs, 3) + obs, np.uint8)
    for step in range(6):
        frames = rng.integers(0, 256, (n,) + obs + (3,), dtype=np.uint8)
        cmd = _cmds(rng, n, step)
        pipe.ingest_rgb(torch.from_numpy(frames).to(DEV), torch.from_numpy(cmd).to(DEV), nat.GRAY_NONE)
        chw = frames.transpose(0, 3, 1, 2)
        for i in range(n):
            if cmd[i] & nat.CMD_SKIP:
                continue
            if cmd[i] & nat.CMD_CLEAR:
                ring[i] = 0
            new = chw[i] if (cmd[i] & 3) else np.zeros((3,) + obs, np.uint8)
            ring[i] = np.concatenate([ring[i, 1:], new[None]], 0)
        assert np.array_equal(pipe.stack_u8().cpu().numpy(), ring), step
    full = pipe.observe_full().cpu().numpy()
    assert full.shape == (n, fs, 3) + obs
    assert np.array_equal(full.view(np.uint32), (ring.astype(np.float32) / np.float32(255)).view(np.uint32))
    # set_stack_u8 round trip in the same layout
    other = rng.integers(0, 256, ring.shape, dtype=np.uint8)
    pipe.set_stack_u8(torch.from_numpy(other).to(DEV))
    assert np.array_equal(pipe.stack_u8().cpu().numpy(), other)
    px = obs[0] * obs[1]
    assert pipe.algorithmic_bytes("ingest_rgb") == n * px * 6
    assert pipe.algorithmic_bytes("full") == n * fs * 3 * px * 5
    pipe.close()


# ---------------------------------------------------------------------------------------------------------- 2. identity
def _cfg(kind, mode, aa, amode, geom):
    obs, fov, per = {"headline": ((84, 84), (30, 30), (20, 20)), "runtime": ((36, 48), (10, 14), (9, 12)),
                     "odd": ((10, 12), (4, 6), (5, 5))}[geom]      # odd: h * w % 16 != 0 (dword planar ingest)
    kw = dict(kind=kind, obs_size=obs, fov_size=fov, fov_init_loc=(2, 3), sensory_action_mode=amode, antialias=bool(aa),
              resize_to_full=mode == "resize", mask_out=mode == "mask")
    if amode == "relative":
        kw["sensory_action_space"] = (-7, 9)
    if kind == "peripheral":
        kw["peripheral_res"] = per
    return kw


def _actions(rng, kind, amode, n, obs):
    if amode == "relative":
        a = rng.uniform(-10, 12, (n, 2))
    else:
        a = rng.uniform(-4, max(obs) + 3, (n, 2))
    t = None
    if kind == "flexible":
        t = rng.integers(0, 2, n).astype(np.int32)
        res = np.stack([rng.integers(1, obs[0] + 1, n), rng.integers(1, obs[1] + 1, n)], 1)
        a = np.where(t[:, None] == 1, res, a)
    return torch.from_numpy(a.astype(np.float32)).to(DEV), (torch.from_numpy(t).to(DEV) if t is not None else None)


def _run_identity(kind, mode, aa, amode, geom, n, fs=3, steps=5, obs_dtype=torch.float32):
    from active_gym import ObsPipeline, _native as nat
    kw = _cfg(kind, mode, aa, amode, geom)
    col = ObsPipeline(num_envs=n, frame_stack=fs, device=DEV, channels=3, obs_dtype=obs_dtype, **kw)
    grays = [ObsPipeline(num_envs=n, frame_stack=fs, device=DEV, obs_dtype=obs_dtype, **kw) for _ in range(3)]
    obs = col.obs_size
    assert col.obs_shape[:3] == (n, fs, 3) and col.obs_shape[1:2] + col.obs_shape[3:] == grays[0].obs_shape[1:2] + grays[0].obs_shape[2:]
    rng = np.random.default_rng(zlib.crc32(repr((kind, mode, aa, amode, geom, n)).encode()))
    for step in range(steps):
        frames = rng.integers(0, 256, (n,) + obs + (3,), dtype=np.uint8)
        cmd = torch.from_numpy(_cmds(rng, n, step)).to(DEV)
        col.ingest_rgb(torch.from_numpy(frames).to(DEV), cmd, nat.GRAY_NONE)
        for c, g in enumerate(grays):
            small = np.zeros((n, 2) + obs, np.uint8)
            small[:, 0] = frames[..., c]
            small[:, 1] = 255 - frames[..., c]                   # never read (nvalid <= 1)
            g.ingest_gray(torch.from_numpy(small).to(DEV), cmd)
        if step == 3:                                            # re-initialise the fovea of a subset
            m = torch.from_numpy((rng.random(n) < 0.5).astype(np.uint8)).to(DEV)
            for p in [col] + grays:
                p.fovea_reset(m)
        mask = None
        if step == 2:
            mask = torch.from_numpy((rng.random(n) < 0.6).astype(np.uint8)).to(DEV)
        act, typ = _actions(rng, kind, amode, n, obs)
        if step == 1:
            act, typ = None, None                                # observe at the current location
        oc = torch.zeros(col.obs_shape, dtype=obs_dtype, device=DEV)
        outs = [torch.zeros(g.obs_shape, dtype=obs_dtype, device=DEV) for g in grays]
        rc = col.fovea(act, action_type=typ, mask=mask, out=oc)
        rg = [g.fovea(act, action_type=typ, mask=mask, out=o) for g, o in zip(grays, outs)]
        torch.cuda.synchronize()
        sel = mask.bool() if mask is not None else torch.ones(n, dtype=torch.bool, device=DEV)   # rows the call wrote
        for c in range(3):
            assert np.array_equal(_bits(oc[:, :, c]), _bits(outs[c])), (step, c)
            for a, b in zip(rc[1:], rg[c][1:]):
                assert torch.equal(a[sel], b[sel]), (step, c)
            for a, b in zip(col.fov_state(), grays[c].fov_state()):
                assert torch.equal(a, b), (step, c)
    for c in range(3):
        assert torch.equal(col.stack_u8()[:, :, c], grays[c].stack_u8())
        assert np.array_equal(_bits(col.observe_full()[:, :, c]), _bits(grays[c].observe_full()))
    for p in [col] + grays:
        p.close()


_CASES = ([("fixed", m, 1, a) for m in ("raw", "resize", "mask") for a in ("absolute", "relative")]
          + [("flexible", m, aa, a) for m in ("raw", "resize", "mask") for aa in (0, 1) for a in ("absolute", "relative")]
          + [("peripheral", "resize", aa, a) for aa in (0, 1) for a in ("absolute", "relative")])


@pytest.mark.parametrize("geom", ["headline", "runtime"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("kind,mode,aa,amode", _CASES)
def test_colour_channel_equals_gray_path(kind, mode, aa, amode, geom, n):
    _run_identity(kind, mode, aa, amode, geom, n)


@pytest.mark.parametrize("kind,mode", [("fixed", "resize"), ("fixed", "raw"), ("flexible", "mask"), ("flexible", "resize"),
                                       ("peripheral", "resize")])
def test_colour_channel_equals_gray_path_n1024(kind, mode):
    _run_identity(kind, mode, 1, "absolute", "headline", 1024, steps=3)


@pytest.mark.parametrize("kind,mode,aa", [("fixed", "resize", 1), ("fixed", "raw", 1), ("flexible", "mask", 0), ("peripheral", "resize", 1)])
def test_colour_channel_equals_gray_path_odd_pixel_count(kind, mode, aa):
    _run_identity(kind, mode, aa, "absolute", "odd", 5)


def test_colour_fallback_kernels_equal_gray_path(monkeypatch):
    """the generic / pass-by-pass fallback kernels (selected by the testing knobs, and by geometries outside the tuned plans)"""
    for knob in ("AGX_FOVEA_GENERIC", "AGX_FLEX_V2", "AGX_PER_V2"):
        monkeypatch.setenv(knob, "1")
        _run_identity("flexible", "resize", 1, "absolute", "runtime", 5, steps=3)
        _run_identity("peripheral", "resize", 0, "relative", "runtime", 5, steps=3)
        monkeypatch.delenv(knob)


# ---------------------------------------------------------------------------------------------------------- 3. 16-bit
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind,mode", [("base", None), ("fixed", "resize"), ("fixed", "raw"), ("flexible", "mask"),
                                       ("peripheral", "resize")])
def test_colour_16bit_equals_colour_f32_cast(kind, mode, dtype):
    from active_gym import ObsPipeline, _native as nat
    n, fs = 5, 3
    kw = dict(kind=kind, obs_size=(84, 84), frame_stack=fs, device=DEV, channels=3)
    if kind != "base":
        kw.update(_cfg(kind, mode, 1, "absolute", "headline"))
    p32 = ObsPipeline(num_envs=n, **kw)
    p16 = ObsPipeline(num_envs=n, obs_dtype=dtype, **kw)
    rng = np.random.default_rng(3)
    for step in range(3):
        frames = torch.from_numpy(rng.integers(0, 256, (n, 84, 84, 3), dtype=np.uint8)).to(DEV)
        cmd = torch.from_numpy(_cmds(rng, n, step)).to(DEV)
        for p in (p32, p16):
            p.ingest_rgb(frames, cmd, nat.GRAY_NONE)
        if kind == "base":
            a, b = p32.observe_full(), p16.observe_full()
        else:
            act, typ = _actions(rng, kind, "absolute", n, (84, 84))
            a, b = p32.fovea(act, action_type=typ)[0], p16.fovea(act, action_type=typ)[0]
        assert b.dtype == dtype and b.shape == a.shape
        assert np.array_equal(_bits(b), _bits(a.to(dtype)))


# ---------------------------------------------------------------------------------------------------------- 4. refusals
def test_colour_context_refuses_gray_and_atari_entry_points():
    from active_gym import ObsPipeline, _native as nat
    n = 3
    col = ObsPipeline(num_envs=n, kind="flexible", obs_size=(84, 84), frame_stack=2, fov_size=(30, 30), device=DEV, channels=3)
    gray = ObsPipeline(num_envs=n, kind="fixed", obs_size=(84, 84), frame_stack=2, fov_size=(30, 30), device=DEV)
    fixed = ObsPipeline(num_envs=n, kind="fixed", obs_size=(84, 84), frame_stack=2, fov_size=(30, 30), device=DEV, channels=3)
    cmd = torch.ones(n, dtype=torch.uint8, device=DEV)
    rgb = torch.zeros((n, 210, 160, 3), dtype=torch.uint8, device=DEV).reshape(n, 1, 210, 160, 3).expand(n, 2, 210, 160, 3).contiguous()
    gscr = torch.zeros((n, 2, 210, 160), dtype=torch.uint8, device=DEV)
    rows = len(col.source_rows())
    calls = {
        "ingest": lambda: col.ingest(rgb, cmd),
        "ingest_gray_raw": lambda: col.ingest_gray_raw(gscr, cmd),
        "ingest_compact": lambda: col.ingest_compact(rgb[:, :, :rows].contiguous(), cmd),
        "ingest_gray_raw_compact": lambda: col.ingest_gray_raw_compact(gscr[:, :, :rows].contiguous(), cmd),
        "ingest_gray": lambda: col.ingest_gray(torch.zeros((n, 2, 84, 84), dtype=torch.uint8, device=DEV), cmd),
        "step_fixed": lambda: fixed.step_fixed(rgb, cmd),
        "fovea_packed": lambda: col.fovea_packed(),
        "step_flexible_packed": lambda: col.step_flexible_packed(rgb, cmd),
        "ingest_rgb cv15 on colour": lambda: col.ingest_rgb(torch.zeros((n, 84, 84, 3), dtype=torch.uint8, device=DEV), cmd, nat.GRAY_CV15),
        "ingest_rgb cv14 on colour": lambda: col.ingest_rgb(torch.zeros((n, 84, 84, 3), dtype=torch.uint8, device=DEV), cmd, nat.GRAY_CV14),
        "ingest_rgb none on gray": lambda: gray.ingest_rgb(torch.zeros((n, 84, 84, 3), dtype=torch.uint8, device=DEV), cmd, nat.GRAY_NONE),
    }
    for name, fn in calls.items():
        with pytest.raises(nat.AgxError) as e:
            fn()
        assert e.value.code == nat.E_STATE, name
    for k in (nat.K_INGEST, nat.K_INGEST_GRAY_RAW):
        assert nat.lib().agx_algorithmic_bytes(col._ctx, k) == nat.E_STATE
    # the native (Atari) step loop
    from active_gym import native_loop as nl
    lib = nl._lib()
    src, cfg, h = nl.AgxHostSource(), nl.AgxLoopConfig(), C.c_void_p()
    cfg.struct_size = C.sizeof(nl.AgxLoopConfig)
    assert lib.agx_loop_create(col._ctx, C.byref(src), C.byref(cfg), C.byref(h)) == nat.E_STATE
    assert not h.value
    # the colour context still works after the refusals
    col.ingest_rgb(torch.full((n, 84, 84, 3), 7, dtype=torch.uint8, device=DEV), cmd)
    assert int(col.stack_u8()[:, -1].max()) == 7
    for p in (col, gray, fixed):
        p.close()


def test_unknown_gray_mode_is_invalid_on_both_context_kinds():
    from active_gym import ObsPipeline, _native as nat
    n = 2
    cmd = torch.ones(n, dtype=torch.uint8, device=DEV)
    rgb = torch.zeros((n, 84, 84, 3), dtype=torch.uint8, device=DEV)
    for ch in (1, 3):
        p = ObsPipeline(num_envs=n, kind="base", obs_size=(84, 84), frame_stack=2, device=DEV, channels=ch)
        for mode in (7, -1):
            with pytest.raises(nat.AgxError) as e:
                p.ingest_rgb(rgb, cmd, mode)
            assert e.value.code == nat.E_INVALID, (ch, mode)
        p.close()


def _dmc_args(seed=0, **kw):
    from active_gym import DMCEnvArgs
    base = dict(domain_name="scripted", task_name="t", seed=seed, obs_size=(84, 84), grey=False,
                frame_source=lambda a, i: ScriptedDMC(a.seed + i, episode_len=getattr(a, "episode_len", 23)))
    base.update(kw)
    return DMCEnvArgs(**base)


def test_colour_requests_refused_up_front():
    import active_gym
    from active_gym import AtariEnvArgs, AtariVecEnv, DMCVecEnv
    with pytest.raises(ValueError):
        DMCVecEnv(_dmc_args(fov_size=(30, 30), fov_init_loc=(0, 0), sensory_action_mode="absolute", resize_to_full=False,
                            ragged_obs="packed"), 2, kind="flexible")
    with pytest.raises(ValueError):
        AtariVecEnv(AtariEnvArgs(game="breakout", seed=0, obs_size=(84, 84), grey=False, frame_source="synthetic"), 2, kind="base")
    with pytest.raises(NotImplementedError):
        DMCVecEnv(_dmc_args(from_pixels=False), 2, kind="base")
    assert active_gym is not None


# ---------------------------------------------------------------------------------------------------------- 5./6. envs
class _Oracle:
    """N ScriptedDMC envs stepped as DMCHostRunner steps them, with the colour frame stack kept in NumPy."""

    def __init__(self, args, n, fs):
        self.envs = [ScriptedDMC(args.seed + i, episode_len=args.episode_len) for i in range(n)]
        self.ar, self.fs, self.obs = int(args.action_repeat), fs, tuple(args.obs_size)
        self.stack = np.zeros((n, fs, 3) + self.obs, np.float32)

    def _push(self, i, clear):
        img = self.envs[i].physics.render(self.obs[0], self.obs[1], 0).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
        if clear:
            self.stack[i] = 0
        self.stack[i] = np.concatenate([self.stack[i, 1:], img[None]], 0)

    def reset(self):
        for i, e in enumerate(self.envs):
            e.reset()
            self._push(i, True)
        return self.stack.copy()

    def step(self, true_actions):
        done = np.zeros(len(self.envs), bool)
        final = {}
        for i, e in enumerate(self.envs):
            for _ in range(self.ar):
                ts = e.step(true_actions[i])
                if ts.last():
                    break
            self._push(i, False)
            if ts.last():
                done[i] = True
                final[i] = self.stack[i].copy()
                e.reset()
                self._push(i, True)
        return self.stack.copy(), done, final


@pytest.mark.parametrize("out", ["device", "device_bf16", "host", "host_pinned", "device_copy"])
def test_vec_env_colour_autoreset_against_oracle(out):
    from active_gym import DMCVecEnv
    n, fs = 6, 3
    kw = dict(episode_len=9, frame_stack=fs, action_repeat=2)
    if out.startswith("device"):
        kw["device"] = "cuda:0"
    if out == "device_bf16":
        kw["obs_dtype"] = "bfloat16"
    if out == "host_pinned":
        kw["copy_obs"] = False
    if out == "device_copy":
        kw["copy_obs"] = True
    args = _dmc_args(seed=4, **kw)
    env = DMCVecEnv(args, n, kind="base")
    assert env.single_observation_space.shape == (fs, 3, 84, 84)
    assert env.observation_space.shape == (n, fs, 3, 84, 84)
    orc = _Oracle(args, n, fs)
    cast = (lambda a: torch.from_numpy(a).to(torch.bfloat16).float().numpy()) if out == "device_bf16" else (lambda a: a)

    def host(o):
        return (o.float().cpu().numpy() if isinstance(o, torch.Tensor) else np.asarray(o, np.float32))

    obs, _ = env.reset()
    assert np.array_equal(host(obs), cast(orc.reset()))
    rng = np.random.default_rng(1)
    ends = 0
    for _ in range(12):
        a = rng.uniform(-1, 1, (n, env.runner.action_dim)).astype(np.float32)
        obs, r, d, t, info = env.step(a)
        want, done, final = orc.step(env.runner.convert_action(a))
        assert np.array_equal(d, done)
        assert np.array_equal(host(obs), cast(want))
        if done.any():
            ends += 1
            for i in np.nonzero(done)[0]:
                assert np.array_equal(host(info["final_observation"][i]), cast(final[i]))
    assert ends >= 2
    env.close()


@pytest.mark.parametrize("kind", ["base", "fixed", "flexible", "peripheral"])
def test_single_env_colour_wrappers(kind):
    """DMC*Env(grey=False): (fs, 3, ...) observations whose channels equal those of an N = 1 gray ObsPipeline fed the same
    channel of the same renders; the observation spaces follow the channel axis; record=True keeps (fs, 3, H, W) float64."""
    import active_gym
    from active_gym import ObsPipeline, _native as nat
    fs = 3
    kw = dict(frame_stack=fs, fov_size=(30, 30), fov_init_loc=(0, 0), sensory_action_mode="absolute", resize_to_full=True,
              peripheral_res=(20, 20), record=True, episode_len=7)
    ctor = {"base": active_gym.DMCBaseEnv, "fixed": active_gym.DMCFixedFovealEnv, "flexible": active_gym.DMCFlexibleFovealEnv,
            "peripheral": active_gym.DMCFixedFovealPeripheralEnv}[kind]
    env = ctor(_dmc_args(seed=2, **kw))
    assert env.observation_space.shape == (fs, 3, 84, 84)
    assert env.unwrapped.observation_space.shape == (fs, 3, 84, 84) and env.unwrapped.grey is False
    pk = dict(kind=kind, obs_size=(84, 84), frame_stack=fs, device=DEV)
    if kind != "base":
        pk.update(fov_size=(30, 30), fov_init_loc=(0, 0), sensory_action_mode="absolute", resize_to_full=True)
    if kind == "peripheral":
        pk["peripheral_res"] = (20, 20)
    grays = [ObsPipeline(num_envs=1, **pk) for _ in range(3)]
    shadow = ScriptedDMC(2, episode_len=7)
    true = env.unwrapped._core.runner.convert_action

    def feed(clear):
        img = shadow.physics.render(84, 84, 0)
        for c, g in enumerate(grays):
            small = np.zeros((1, 2, 84, 84), np.uint8)
            small[0, 0] = img[..., c]
            g.ingest_gray(torch.from_numpy(small).to(DEV), torch.tensor([(nat.CMD_CLEAR if clear else 0) | 1], dtype=torch.uint8, device=DEV))

    def check(o, act=None, typ=None):
        assert o.shape == (fs, 3, 84, 84) and o.dtype == np.float32
        for c, g in enumerate(grays):
            want = g.observe_full()[0] if kind == "base" else g.fovea(act, action_type=typ)[0][0]
            assert np.array_equal(o[:, c].view(np.uint32), want.cpu().numpy().view(np.uint32)), c

    o, _ = env.reset()
    shadow.reset()
    feed(True)
    if kind != "base":
        for g in grays:
            g.fovea_reset()
    check(o)
    rng = np.random.default_rng(0)
    for step in range(9):
        m = rng.uniform(-1, 1, env.unwrapped._core.runner.action_dim).astype(np.float32)
        if kind == "base":
            a, act, typ = m, None, None
        else:
            loc = rng.integers(0, 55, 2)
            a = {"motor_action": m, "sensory_action": loc}
            act = torch.from_numpy(loc.astype(np.float32)[None]).to(DEV)
            typ = None
            if kind == "flexible":
                a["sensory_action_type"] = 0
                typ = torch.zeros(1, dtype=torch.int32, device=DEV)
        o, r, d, t, info = env.step(a)
        for _ in range(env.unwrapped.action_repeat):
            ts = shadow.step(true(m[None])[0])
            if ts.last():
                break
        feed(False)
        check(o, act, typ)
        if d:
            rec = env
            while not isinstance(rec, active_gym.RecordWrapper):
                rec = rec.env
            states = rec.record_buffer["state"]
            assert all(s.shape == (fs, 3, 84, 84) and s.dtype == np.float64 for s in states)
            o, _ = env.reset()
            shadow.reset()
            feed(True)
            if kind != "base":
                for g in grays:
                    g.fovea_reset()
            check(o)
    env.close()
    for g in grays:
        g.close()


# ---------------------------------------------------------------------------------------------------------- 7. capture
@pytest.mark.parametrize("kind", ["fixed", "flexible", "peripheral"])
def test_colour_captured_steps_replay_like_eager_steps(kind):
    """a captured colour step sequence (an even number of steps: the context flips its double buffers on the host) replays
    bit-identically to the same steps launched one by one"""
    from active_gym import ObsPipeline
    n = 17
    kw = dict(num_envs=n, kind=kind, obs_size=(84, 84), frame_stack=3, fov_size=(30, 30), fov_init_loc=(3, 7),
              sensory_action_mode="absolute", resize_to_full=True, device=DEV, channels=3)
    if kind == "peripheral":
        kw["peripheral_res"] = (20, 20)
    rng = np.random.default_rng(9)
    frames = [torch.from_numpy(rng.integers(0, 256, (n, 84, 84, 3), dtype=np.uint8)).to(DEV) for _ in range(4)]
    cmds = [torch.from_numpy(_cmds(rng, n, 1 + i)).to(DEV) for i in range(4)]
    acts = [_actions(rng, kind, "absolute", n, (84, 84)) for _ in range(4)]

    def make():
        p = ObsPipeline(**kw)
        obs = torch.empty(p.obs_shape, dtype=torch.float32, device=DEV)
        loc = torch.empty((n, 2), dtype=torch.int32, device=DEV)
        res = torch.empty((n, 2), dtype=torch.int32, device=DEV)

        def step(i):
            p.ingest_rgb(frames[i], cmds[i])
            if kind == "flexible":
                p.fovea(acts[i][0], action_type=acts[i][1], out=obs, loc_out=loc, res_out=res)
            else:
                p.fovea(acts[i][0], out=obs, loc_out=loc)
        return p, step, obs, loc, res

    pa, sa, oa, la, ra = make()
    pb, sb, ob, lb, rb = make()
    for i in (0, 1):
        sb(i)
    for _ in range(3):
        for i in (2, 3, 0, 1):
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
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pa.stack_u8(), pb.stack_u8())
    assert torch.equal(la, lb)
    if kind == "flexible":
        assert torch.equal(ra, rb)
    assert np.array_equal(_bits(oa), _bits(ob))
    del graph
    for p in (pa, pb):
        p.close()


# ---------------------------------------------------------------------------------------------------------- 5. goldens
import glob
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RGB_GOLDENS = sorted(glob.glob(os.path.join(GOLD, "colour_dmc_*.npz")))


def _golden_args(g, **extra):
    kind = str(g["kind"])
    kw = dict(obs_size=tuple(int(v) for v in g["obs_size"]), frame_stack=int(g["frame_stack"]),
              action_repeat=int(g["action_repeat"]), episode_len=int(g["episode_len"]), record=True)
    if kind != "base":
        kw.update(fov_size=tuple(int(v) for v in g["fov_size"]), fov_init_loc=tuple(float(v) for v in g["fov_init_loc"]),
                  sensory_action_mode=str(g["mode"]), sensory_action_space=tuple(float(v) for v in g["sensory_action_space"]),
                  resize_to_full=bool(g["resize_to_full"]), mask_out=bool(g["mask_out"]), antialias=bool(g["antialias"]),
                  peripheral_res=tuple(int(v) for v in g["peripheral_res"]))
    kw.update(extra)
    return _dmc_args(seed=int(g["seed"]), **kw)


def _golden_out(g):
    if "out_u8" in g.files:
        return g["out_u8"].astype(np.float32) / np.float32(255)
    return g["out"]


def _golden_action(g, kind, t):
    m = g["motor"][t]
    if kind == "base":
        return m
    typ = int(g["sens_type"][t])
    a = {"motor_action": m, "sensory_action": g["sens"][t].astype(np.int64) if typ else g["sens"][t]}
    if kind == "flexible":
        a["sensory_action_type"] = np.array((typ,))
    return a


def _close(got, want, exact, what):
    got = np.asarray(got, np.float32)
    assert got.shape == want.shape, what
    if exact:
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), what
    else:
        assert np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)), initial=0.0) <= 1e-5, what


@pytest.mark.parametrize("path", RGB_GOLDENS, ids=lambda p: os.path.basename(p)[11:-4])
def test_single_env_replays_colour_golden(path):
    """DMC*Env(grey=False) == the reference's colour run (tests/golden/make_golden_dmc_rgb.py), step for step: observations
    (crops / pastes exact, resampled <= 1e-5), fov_loc, the observation space and the record buffer's states."""
    import active_gym
    g = np.load(path, allow_pickle=False)
    kind, exact = str(g["kind"]), bool(g["exact"])
    ctor = {"base": active_gym.DMCBaseEnv, "fixed": active_gym.DMCFixedFovealEnv, "flexible": active_gym.DMCFlexibleFovealEnv,
            "peripheral": active_gym.DMCFixedFovealPeripheralEnv}[kind]
    env = ctor(_golden_args(g))
    ref_shape = tuple(int(v) for v in g["obs_space_shape"])
    if kind == "base":
        assert tuple(env.observation_space.shape) == ref_shape              # the reference's DMCEnv declares (fs, 3, H, W)
    else:
        # its fovea wrappers declare (fs,) + size whatever the channels (fov_env.py:132-142): the channel axis is inserted here
        assert tuple(env.observation_space.shape) == ref_shape[:1] + (3,) + ref_shape[1:]
    out = _golden_out(g)
    o, info = env.reset()
    _close(o, out[0], exact, 0)
    k, t = 1, 0
    while k < len(out):
        o, r, d, tr, info = env.step(_golden_action(g, kind, t))
        t += 1
        assert d == bool(g["dones"][k]), k
        _close(o, out[k], exact, k)
        if kind != "base":
            assert np.array_equal(np.asarray(info["fov_loc"]), g["fov_loc"][k]), k
        k += 1
        if d:
            o, info = env.reset()
            _close(o, out[k], exact, k)
            k += 1
    rec = env
    while not isinstance(rec, active_gym.RecordWrapper):
        rec = rec.env
    states = np.stack(rec.record_buffer["state"])
    assert states.dtype == np.float64
    want = (g["record_states_u8"].astype(np.float32) / np.float32(255)).astype(np.float64)
    assert np.array_equal(states, want)
    env.close()


@pytest.mark.parametrize("out_kind", ["device", "host"])
@pytest.mark.parametrize("path", RGB_GOLDENS, ids=lambda p: os.path.basename(p)[11:-4])
def test_vec_env_replays_colour_golden(path, out_kind):
    """DMCVecEnv(grey=False), N = 1 with autoreset: the step that ends an episode hands the reference's terminal observation
    out as final_observation and returns the reference's reset observation."""
    from active_gym import DMCVecEnv
    g = np.load(path, allow_pickle=False)
    kind, exact = str(g["kind"]), bool(g["exact"])
    extra = {"record": False}
    if out_kind == "device":
        extra["device"] = "cuda:0"
    env = DMCVecEnv(_golden_args(g, **extra), 1, kind=kind)
    out = _golden_out(g)

    def host(x):
        return x.float().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)

    o, _ = env.reset()
    _close(host(o)[0], out[0], exact, 0)
    k, t = 1, 0
    while k < len(out):
        a = _golden_action(g, kind, t)
        if kind == "base":
            va = a[None]
        else:
            va = {key: np.asarray(v)[None] if key != "sensory_action_type" else np.asarray(v) for key, v in a.items()}
        o, r, d, tr, info = env.step(va)
        t += 1
        assert bool(d[0]) == bool(g["dones"][k]), k
        if d[0]:
            _close(host(info["final_observation"][0]), out[k], exact, k)
            _close(host(o)[0], out[k + 1], exact, k + 1)
            k += 2
        else:
            _close(host(o)[0], out[k], exact, k)
            k += 1
    env.close()
