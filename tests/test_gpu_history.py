"""GPU: the frame history (include/agx_history.h) through ObsPipeline + FrameHistory.  Every case keeps a copy of each step's
returned observation and fov_loc, and after the run asks the history for every (env, index) ever issued - and for some that
never were: a retained sample is bit for bit what the step returned, validity and indices are the model's
(tests/history_model.py), and rows of invalid samples keep the sentinel the output was pre-filled with."""
import numpy as np
import pytest
import torch

from history_model import CLEAR, SKIP, HistoryModel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -3.0                 # exact in float32, bfloat16 and float16; no observation value is negative
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pipe(N, kind="fixed", obs=(84, 84), fov=(30, 30), fs=4, mode="resize", action_mode="absolute", dtype=torch.float32):
    from active_gym import ObsPipeline
    kw = dict(num_envs=N, kind=kind, obs_size=obs, frame_stack=fs, device=DEV, obs_dtype=dtype)
    if kind != "base":
        kw.update(fov_size=fov, fov_init_loc=(min(2, obs[0] - fov[0]), min(3, obs[1] - fov[1])), sensory_action_mode=action_mode,
                  sensory_action_space=(-7.0, 9.0) if action_mode == "relative" else None,
                  resize_to_full=mode == "resize", mask_out=mode == "mask")
    return ObsPipeline(**kw)


def commands(seed, N, steps, p_clear=0.15, p_skip=0.15):
    """The command bytes of a run, u8 [steps][N]: nvalid 1 | 2, about p_clear CLEAR, about p_skip SKIP (pure NumPy: the seed of a
    case is chosen on the model alone)."""
    rng = np.random.default_rng(seed)
    cmd = rng.integers(1, 3, (steps, N)).astype(np.uint8)
    cmd |= (rng.random((steps, N)) < p_clear).astype(np.uint8) * CLEAR
    cmd |= (rng.random((steps, N)) < p_skip).astype(np.uint8) * SKIP
    return cmd


def _run(pipe, hist, cmds, seed, full=False):
    """Drive ingest + observation + push over the command bytes.  Returns (model, rec): rec[(n, index)] = (obs row, fov_loc row or
    None, full row or None), device clones of what the step returned."""
    from active_gym.history import FrameHistory  # noqa: F401
    N, fs = pipe.num_envs, pipe.frame_stack
    oh, ow = pipe.obs_size
    rng = np.random.default_rng(seed + 1000)
    model = HistoryModel(N, fs, hist.capacity)
    rec = {}
    for cmd in cmds:
        small = rng.integers(0, 256, (N, 2, oh, ow), dtype=np.uint8)
        pipe.ingest_gray(_t(small), _t(cmd))
        loc = None
        if pipe.kind == "base":
            obs = pipe.observe_full()
        else:
            act = rng.uniform(-9, max(oh, ow) + 5, (N, 2)).astype(np.float32)
            obs, loc = pipe.fovea(_t(act))
        fl = pipe.observe_full() if full and pipe.kind != "base" else (obs if full else None)
        idx = hist.push(_t(cmd)).cpu().numpy()
        assert np.array_equal(idx, model.push(cmd)), "indices differ from the model"
        for n in range(N):
            if idx[n] >= 0:
                rec[(n, int(idx[n]))] = (obs[n].clone(), None if loc is None else loc[n].clone(), None if fl is None else fl[n].clone())
    return model, rec


def _samples(model, extra=True):
    """Every (n, k) ever issued plus, per env, one index below 0 and one that was never issued."""
    out = []
    for n in range(model.N):
        lo, hi = (-1, int(model.count[n]) + 1) if extra else (0, int(model.count[n]))
        out += [(n, k) for k in range(lo, hi)]
    return out


def _check(pipe, hist, model, rec, samples, what="fovea"):
    """observe(samples) into sentinel-filled outputs; returns the number of valid samples."""
    B = len(samples)
    env = _t(np.array([s[0] for s in samples], np.int32))
    idx = _t(np.array([s[1] for s in samples], np.int64))
    out = torch.full((B,) + hist.obs_row_shape(what), SENTINEL, dtype=pipe.obs_dtype, device=DEV)
    loc = torch.full((B, 2), -77, dtype=torch.int32, device=DEV)
    obs, loc, valid = hist.observe(env, idx, what=what, out=out, loc_out=loc)
    valid = valid.cpu().numpy()
    want_valid = np.array([model.valid(n, k) for n, k in samples])
    assert np.array_equal(valid.astype(bool), want_valid), "validity differs from the model"
    bits = BITS[pipe.obs_dtype]
    sent = torch.full(hist.obs_row_shape(what), SENTINEL, dtype=pipe.obs_dtype, device=DEV).view(bits)
    for b, (n, k) in enumerate(samples):
        if valid[b]:
            o, l, f = rec[(n, k)]
            want = f if what == "full" else o
            assert torch.equal(obs[b].view(bits), want.view(bits)), f"sample {(n, k)}: observation bits differ"
            if l is not None:
                assert torch.equal(loc[b], l), f"sample {(n, k)}: fov_loc differs"
        else:
            assert torch.equal(obs[b].view(bits), sent), f"invalid sample {(n, k)}: row was written"
            assert loc[b].tolist() == [-77, -77]
    return int(valid.sum())


def _kinds(model, rec, samples):
    """(valid, zero-frame, evicted, skipped-or-never) counts of the issued samples."""
    issued = [s for s in samples if s in rec]
    valid = [s for s in issued if model.valid(*s)]
    zero = [s for s in valid if None in model.rows(*s)]
    evicted = [s for s in issued if not model.valid(*s)]
    return len(issued), len(valid), len(zero), len(evicted)


MAIN_SEED = 3


def test_main_seed_covers_every_kind_of_sample():
    """The seed of the main case, on the model alone: at least a third of the issued samples are still valid, and zero-frame,
    evicted and skipped samples all occur."""
    cmds = commands(MAIN_SEED, 5, 13)
    m = HistoryModel(5, 4, 8)
    issued = []
    for cmd in cmds:
        idx = m.push(cmd)
        issued += [(n, int(k)) for n, k in enumerate(idx) if k >= 0]
    valid = [s for s in issued if m.valid(*s)]
    assert 3 * len(valid) >= len(issued)
    assert any(None in m.rows(*s) for s in valid) and len(valid) < len(issued) and (cmds & SKIP).any() and (cmds & CLEAR).any()
    assert int(m.count.max()) > 8            # wrap-around


@pytest.mark.parametrize("action_mode", ["absolute", "relative"])
@pytest.mark.parametrize("mode", ["resize", "raw", "mask"])
def test_main_case(mode, action_mode):
    """N = 5, fs = 4, 84 / 30 (the compile-time geometry), T = 8, 13 steps: wrap-around, CLEAR at ages below fs, SKIP."""
    from active_gym import FrameHistory
    pipe = _pipe(5, mode=mode, action_mode=action_mode)
    hist = FrameHistory(pipe, 8)
    cmds = commands(MAIN_SEED, 5, 13)
    model, rec = _run(pipe, hist, cmds, MAIN_SEED)
    samples = _samples(model)
    issued, valid, zero, evicted = _kinds(model, rec, samples)
    assert 3 * valid >= issued and zero >= 1 and evicted >= 1 and (cmds & SKIP).any()
    assert _check(pipe, hist, model, rec, samples) == valid
    assert hist.nbytes >= 8 * 5 * (84 * 84 + 9 + 0) and np.array_equal(hist.last_index().cpu().numpy(), model.count - 1)
    pipe.close()


@pytest.mark.parametrize("obs, fov, fs, mode", [
    ((100, 100), (30, 20), 3, "resize"), ((100, 100), (30, 20), 1, "mask"), ((40, 160), (12, 50), 3, "raw"),
    ((8, 264), (4, 100), 3, "resize"),       # wider than a workgroup: the striding H pass
    ((10, 12), (3, 5), 1, "resize"),         # a frame that is no multiple of 16 bytes: the dword push
    ((10, 12), (3, 5), 3, "raw"),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_generic_geometry(obs, fov, fs, mode):
    """The run-time geometry form, fs = 1 and fs = 3."""
    from active_gym import FrameHistory
    pipe = _pipe(4, obs=obs, fov=fov, fs=fs, mode=mode, action_mode="relative")
    hist = FrameHistory(pipe, 5)
    model, rec = _run(pipe, hist, commands(11, 4, 9), 11)
    samples = _samples(model)
    issued, valid, _, evicted = _kinds(model, rec, samples)
    assert valid >= 8 and evicted >= 1
    assert _check(pipe, hist, model, rec, samples) == valid
    pipe.close()


@pytest.mark.parametrize("kind, obs, fov, mode, dtype", [
    ("fixed", (8, 264), (4, 100), "resize", torch.float32),        # ow > 256: the striding phase C
    ("fixed", (40, 160), (24, 50), "resize", torch.float32),       # 960 window dwords > 3 x 256: window_tail runs
    ("fixed", (40, 160), (24, 50), "mask", torch.float32),
    ("fixed", (10, 12), (3, 5), "raw", torch.float32),             # oh * ow / 4 far below one pass
    ("base", (10, 12), (3, 5), "full", torch.float32),
    ("fixed", (84, 84), (30, 30), "resize", torch.float32),        # the compile-time geometry
    ("fixed", (84, 84), (30, 30), "resize", torch.bfloat16),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))
def test_three_readers_write_the_same_plane(kind, obs, fov, mode, dtype):
    """FrameHistory.observe, RandomShift(pad=0).observe and SequenceReplay.observe(L = 1, planes = fs) of every sample of the model,
    valid or not: bit-equal observation, fov_loc and valid / live byte on the valid rows.  Invalid rows keep the sentinel on the
    observe side and are zeros, fov_loc (0, 0), on the sequence side."""
    from active_gym import FrameHistory, RandomShift, SequenceReplay, StepLog
    from test_gpu_augment import _tensors
    fs, what = 3, "full" if mode == "full" else "fovea"
    pipe = _pipe(4, kind=kind, obs=obs, fov=fov, fs=fs, mode=mode, action_mode="relative", dtype=dtype)
    hist = FrameHistory(pipe, 5)
    model, rec = _run(pipe, hist, commands(11, 4, 9), 11)
    samples = _samples(model)
    issued, nvalid, _, evicted = _kinds(model, rec, samples)
    assert nvalid >= 8 and evicted >= 1
    env, idx = _tensors(samples)
    B, bits = len(samples), BITS[dtype]
    shape = (B,) + hist.obs_row_shape(what)
    aug, seq = RandomShift(hist, pad=0), SequenceReplay(StepLog(hist, 0))
    reads = []
    for read, kw in ((hist.observe, {}), (aug.observe, {"shift": torch.zeros((B, 2), dtype=torch.int32, device=DEV)})):
        out = torch.full(shape, SENTINEL, dtype=dtype, device=DEV)
        loc = torch.full((B, 2), -77, dtype=torch.int32, device=DEV)
        reads.append(read(env, idx, what=what, out=out, loc_out=loc, **kw))
    (obs_h, loc_h, valid_h), (obs_a, loc_a, valid_a) = reads
    out = torch.full((B, 1) + shape[1:], SENTINEL, dtype=dtype, device=DEV)
    loc = torch.full((B, 1, 2), -77, dtype=torch.int32, device=DEV)
    obs_s, loc_s, live = seq.observe(env, idx, seq.lengths(env, idx, 1), 1, what=what, planes=fs, out=out, loc_out=loc)
    obs_s, loc_s, live = obs_s[:, 0], loc_s[:, 0], live[:, 0]
    v = valid_h.bool()
    assert np.array_equal(v.cpu().numpy(), np.array([model.valid(n, k) for n, k in samples])) and int(v.sum()) == nvalid
    assert torch.equal(valid_a, valid_h) and torch.equal(live, valid_h), "the valid / live bytes differ"
    # the observe side, whole: equal on the valid rows, the sentinel on both elsewhere
    assert torch.equal(obs_a.view(bits), obs_h.view(bits)) and torch.equal(loc_a, loc_h)
    assert torch.equal(obs_h[~v].view(bits), torch.full_like(obs_h[~v], SENTINEL).view(bits)) and bool((loc_h[~v] == -77).all())
    assert torch.equal(obs_s[v].view(bits), obs_h[v].view(bits)), "sequence observe differs from observe on a valid row"
    assert not bool(obs_s[~v].view(bits).any()), "a dead step is not all-zero bytes"
    if kind == "fixed":
        assert torch.equal(loc_s[v], loc_h[v]) and not bool(loc_s[~v].any())
    for b in torch.nonzero(v).flatten().tolist():              # ... and all three are what the step wrote
        o, l, f = rec[samples[b]]
        assert torch.equal(obs_h[b].view(bits), (o if f is None else f).view(bits)), samples[b]
    pipe.close()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("mode", ["resize", "raw", "mask"])
def test_16_bit_outputs(mode, dtype):
    """bf16 / f16 contexts: bit-equal to that context's own step outputs, fovea and full."""
    from active_gym import FrameHistory
    pipe = _pipe(3, mode=mode, dtype=dtype)
    hist = FrameHistory(pipe, 6)
    model, rec = _run(pipe, hist, commands(5, 3, 8), 5, full=True)
    samples = _samples(model)
    assert _check(pipe, hist, model, rec, samples) >= 6
    assert _check(pipe, hist, model, rec, samples, what="full") >= 6
    pipe.close()


@pytest.mark.parametrize("kind, obs", [("base", (84, 84)), ("fixed", (84, 84)), ("base", (10, 12))])
def test_full_equals_observe_full(kind, obs):
    from active_gym import FrameHistory
    pipe = _pipe(4, kind=kind, obs=obs, fov=(30, 30) if obs == (84, 84) else (3, 5), fs=3)
    hist = FrameHistory(pipe, 5)
    model, rec = _run(pipe, hist, commands(8, 4, 9), 8, full=True)
    samples = _samples(model)
    assert _check(pipe, hist, model, rec, samples, what="full") >= 6
    pipe.close()


@pytest.mark.parametrize("action_mode", ["absolute", "relative"])
def test_counterfactual_action(action_mode):
    """observe(action=a): a scratch fixed, absolute-mode context loaded with the sample's own stack (set_stack_u8 of the
    AGX_HIST_FULL numerators) and asked for fovea(a) gives the same bits and the same fov_loc - all four action dtypes,
    out-of-range values and exact .5 included."""
    from active_gym import FrameHistory
    pipe = _pipe(5, action_mode=action_mode)
    hist = FrameHistory(pipe, 8)
    model, rec = _run(pipe, hist, commands(MAIN_SEED, 5, 13), MAIN_SEED)
    samples = [s for s in _samples(model, extra=False) if model.valid(*s)]
    B = len(samples)
    assert B >= 10
    env, idx = _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))
    full, _, v = hist.observe(env, idx, what="full")
    assert bool(v.all())
    stack = torch.round(full * 255.0).to(torch.uint8)
    scratch = _pipe(B, action_mode="absolute")
    rng = np.random.default_rng(4)
    base = rng.uniform(-12, 70, (B, 2))
    base[:6] = [[0.5, 1.5], [2.5, 53.5], [54.5, 54.0], [-0.5, 60.0], [1e9, -1e9], [53.5, 0.49999]]
    for dt in (np.float32, np.float64, np.int32, np.int64):
        a = _t(np.rint(base).astype(dt) if np.issubdtype(dt, np.integer) else base.astype(dt))
        got, gloc, v = hist.observe(env, idx, action=a)
        assert bool(v.all())
        scratch.set_stack_u8(stack)
        want, wloc = scratch.fovea(a)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), dt
        assert torch.equal(gloc, wloc), dt
    scratch.close()
    pipe.close()


def test_sample_shapes_and_clear():
    """B = 1; B = 37 with repeats in shuffled order; B = 0; after clear() everything is invalid and indices restart at 0."""
    from active_gym import FrameHistory
    pipe = _pipe(5)
    hist = FrameHistory(pipe, 8)
    cmds = commands(MAIN_SEED, 5, 13)
    model, rec = _run(pipe, hist, cmds, MAIN_SEED)
    every = _samples(model)
    good = [s for s in every if model.valid(*s)]
    assert _check(pipe, hist, model, rec, good[3:4]) == 1
    rng = np.random.default_rng(2)
    pick = [every[i] for i in rng.integers(0, len(every), 37)]
    assert len(set(pick)) < 37
    assert _check(pipe, hist, model, rec, pick) == sum(model.valid(*s) for s in pick) >= 5
    o, l, v = hist.observe(torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV))
    assert tuple(o.shape) == (0, 4, 84, 84) and tuple(v.shape) == (0,)
    hist.clear()
    model.clear()
    assert _check(pipe, hist, model, rec, every) == 0
    plain = np.full(5, 2, np.uint8)
    small = _t(np.random.default_rng(9).integers(0, 256, (5, 2, 84, 84), dtype=np.uint8))
    rec2 = {}
    for step in range(5):
        cmd = plain | (CLEAR if step == 3 else 0)
        pipe.ingest_gray(small, _t(cmd))
        obs, loc = pipe.fovea()
        idx = hist.push(_t(cmd)).cpu().numpy()
        assert np.array_equal(idx, model.push(cmd)) and (idx == step).all()
        for n in range(5):
            rec2[(n, step)] = (obs[n].clone(), loc[n].clone(), None)
    # the frames before the clear are gone: indices 0 .. 2 would reach behind it and stay invalid; 3 (CLEAR) and 4 are exact
    assert _check(pipe, hist, model, rec2, _samples(model)) == 5 * 2
    pipe.close()


def test_one_env_capacity_equals_frame_stack():
    """Low occupancy: N = 1, T = fs - one workgroup per stack position, every row of the history in use."""
    from active_gym import FrameHistory
    pipe = _pipe(1)
    hist = FrameHistory(pipe, 4)
    model, rec = _run(pipe, hist, commands(1, 1, 9, p_clear=0.3, p_skip=0.1), 1)
    samples = _samples(model)
    assert _check(pipe, hist, model, rec, samples) >= 1
    pipe.close()


def test_full_size():
    """N = 1024, T = 4, 6 steps, all retained samples in one observe."""
    from active_gym import FrameHistory
    N = 1024
    pipe = _pipe(N)
    hist = FrameHistory(pipe, 4)
    cmds = commands(6, N, 6)
    model = HistoryModel(N, 4, 4)
    rng = np.random.default_rng(6)
    kept = []
    for cmd in cmds:
        small = torch.randint(0, 256, (N, 2, 84, 84), dtype=torch.uint8, device=DEV)
        pipe.ingest_gray(small, _t(cmd))
        obs, loc = pipe.fovea(_t(rng.uniform(-9, 90, (N, 2)).astype(np.float32)))
        idx = hist.push(_t(cmd))
        assert np.array_equal(idx.cpu().numpy(), model.push(cmd))
        kept.append((obs.clone(), loc.clone(), idx.cpu().numpy()))
    where = {(n, int(k)): (s, n) for s, (_, _, idx) in enumerate(kept) for n, k in enumerate(idx) if k >= 0}
    samples = [s for s in _samples(model, extra=False) if model.valid(*s)]
    assert len(samples) >= N
    env, idx = _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))
    obs, loc, valid = hist.observe(env, idx)
    assert bool(valid.all())
    step = _t(np.array([where[s][0] for s in samples], np.int64))
    for s, (o, l, _) in enumerate(kept):
        sel = torch.nonzero(step == s).flatten()
        if len(sel):
            assert torch.equal(obs[sel].view(torch.int32), o[env[sel].long()].view(torch.int32)), s
            assert torch.equal(loc[sel], l[env[sel].long()]), s
    pipe.close()


def test_refusals():
    from active_gym import FrameHistory, ObsPipeline
    from active_gym import _native as nat
    per = ObsPipeline(2, "peripheral", fov_size=(30, 30), peripheral_res=(20, 20), device=DEV)
    flex = ObsPipeline(2, "flexible", fov_size=(30, 30), device=DEV)
    rgb = ObsPipeline(2, "base", channels=3, device=DEV)
    for pipe in (per, flex, rgb):
        with pytest.raises(nat.AgxError, match="not supported") as e:
            FrameHistory(pipe, 8)
        assert e.value.code == nat.E_STATE
        pipe.close()
    pipe = _pipe(4)
    with pytest.raises(nat.AgxError, match="below frame_stack") as e:
        FrameHistory(pipe, 3)
    assert e.value.code == nat.E_INVALID
    pipe.env_range(1, 2)
    with pytest.raises(nat.AgxError, match="env range") as e:
        FrameHistory(pipe, 8)
    assert e.value.code == nat.E_STATE
    pipe.env_range()
    hist = FrameHistory(pipe, 8)
    cmd = torch.full((4,), 2, dtype=torch.uint8, device=DEV)
    pipe.env_range(1, 2)
    with pytest.raises(nat.AgxError, match="env range") as e:
        hist.push(cmd)
    assert e.value.code == nat.E_STATE
    pipe.env_range()
    pipe.close()
    base = _pipe(2, kind="base")
    hist = FrameHistory(base, 4)
    z32, z64 = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(nat.AgxError, match="AGX_HIST_FULL only") as e:
        hist.observe(z32, z64, what="fovea", out=torch.empty((1, 4, 84, 84), device=DEV))
    assert e.value.code == nat.E_STATE
    with pytest.raises(TypeError):
        hist.observe(z64, z64, what="full")          # env must be int32
    with pytest.raises(ValueError):
        hist.observe(z32.cpu(), z64, what="full")    # ... on the pipeline's device
    base.close()


def _vec_env(native_loop, history_len):
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=150, native_loop=native_loop)
    if history_len is not None:
        kw["history_len"] = history_len
    return AtariVecEnv(AtariEnvArgs(**kw), 6, kind="fixed", noop_fn=lambda: 2)


def test_vec_env_history():
    """AtariVecEnv(history_len=16): every retained info["history_index"] re-creates the observation step returned, index - 1 of a
    done env its final_observation; the native loop and the Python loop agree; history_len = 0 leaves info without the key."""
    N, STEPS = 6, 40
    runs = []
    for native in (True, False):
        env = _vec_env(native, 16)
        assert (env._loop is not None) == native and env.history is not None and env.history.capacity == 16
        obs, info = env.reset()
        assert info["history_index"].dtype == torch.int64 and info["history_index"].device.type == "cuda"
        rec = [(obs.clone(), info["history_index"].clone())]
        finals = []
        rng = np.random.default_rng(0)
        dones = 0
        for step in range(STEPS):
            act = {"motor_action": rng.integers(0, 4, N), "sensory_action": rng.uniform(-5, 90, (N, 2)).astype(np.float32)}
            obs, _, done, _, info = env.step(act)
            hi = info["history_index"].clone()
            rec.append((obs.clone(), hi))
            for i in np.nonzero(done)[0]:
                finals.append((int(i), int(hi[i]) - 1, info["final_observation"][i].clone()))
                assert int(info["final_info"][i]["history_index"]) == int(hi[i]) - 1
                dones += 1
        assert dones >= 5                        # several autoresets
        # every index ever returned, in one observe
        env_i = torch.arange(N, dtype=torch.int32, device=DEV).repeat(len(rec))
        idx = torch.cat([r[1] for r in rec])
        got, _, valid = env.history.observe(env_i, idx)
        want = torch.cat([r[0] for r in rec])
        valid = valid.bool()
        assert bool(valid[-N:].all()) and int(valid.sum()) >= 8 * N
        assert torch.equal(got[valid].view(torch.int32), want[valid].view(torch.int32))
        checked = 0
        for i, k, fo in finals:
            o, _, v = env.history.observe(torch.tensor([i], dtype=torch.int32, device=DEV), torch.tensor([k], dtype=torch.int64, device=DEV))
            if bool(v[0]):
                assert torch.equal(o[0].view(torch.int32), fo.view(torch.int32)), (i, k)
                checked += 1
        assert checked >= 1
        runs.append(rec)
        env.close()
    for (oa, ia), (ob, ib) in zip(*runs):
        assert torch.equal(oa, ob) and torch.equal(ia, ib)
    env = _vec_env(True, 0)
    _, info = env.reset()
    assert env.history is None and "history_index" not in info
    _, _, _, _, info = env.step({"motor_action": np.zeros(N, np.int64), "sensory_action": np.zeros((N, 2), np.float32)})
    assert "history_index" not in info
    env.close()


def test_vec_env_refuses_unsupported_history():
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", history_len=8)
    with pytest.raises(ValueError, match="kind"):
        AtariVecEnv(AtariEnvArgs(peripheral_res=(20, 20), **kw), 2, kind="peripheral")
    with pytest.raises(ValueError, match="kind"):
        AtariVecEnv(AtariEnvArgs(**kw), 2, kind="flexible")
