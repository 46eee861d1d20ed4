"""GPU: the random-shift augmentation (include/agx_augment.h) through FrameHistory + RandomShift.  The oracle is the project's own
unshifted ``hist.observe(...)`` output, gathered per sample with torch index ops on the device by the header's shift map
(tests/shift_model.py states it): valid rows are bit for bit that gather, invalid rows keep the sentinel the output was pre-filled
with, and ``valid`` / ``fov_loc`` are observe's.  The draw is held against tests/shift_model.py."""
import numpy as np
import pytest
import torch

import shift_model as sm
from history_model import CLEAR, SKIP, HistoryModel
from test_gpu_history import BITS, MAIN_SEED, SENTINEL, _kinds, _pipe, _run, _samples, _t, commands

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
CORNERS = [(0, 0), (0, 8), (8, 0), (8, 8)]


def _gather(ref, shift, pad):
    """S[b][p][y][x] = ref[b][p][shift_src(y, dy_b)][shift_src(x, dx_b)] - ref [B, P, h, w], shift i32 [B, 2] - on the device."""
    B, P, h, w = ref.shape
    d = shift.to(torch.int64).clamp(0, 2 * pad)
    iy = (torch.arange(h, device=ref.device)[None, :] + d[:, :1] - pad).clamp(0, h - 1)
    ix = (torch.arange(w, device=ref.device)[None, :] + d[:, 1:] - pad).clamp(0, w - 1)
    bi = torch.arange(B, device=ref.device)[:, None, None, None]
    pi = torch.arange(P, device=ref.device)[None, :, None, None]
    return ref[bi, pi, iy[:, None, :, None], ix[:, None, None, :]]


def test_gather_is_the_models_shift_map():
    """The oracle's index arithmetic against shift_model.src_index, on the CPU."""
    ref = torch.arange(2 * 1 * 5 * 3, dtype=torch.float32).reshape(2, 1, 5, 3)
    shift = torch.tensor([[0, 3], [4, -1]], dtype=torch.int32)
    got = _gather(ref, shift, 2).numpy()
    iy, ix = sm.src_index([0, 4], 2, 5), sm.src_index([3, -1], 2, 3)
    for b in range(2):
        assert np.array_equal(got[b, 0], ref.numpy()[b, 0][iy[b]][:, ix[b]])


def test_main_seed_covers_every_kind_of_sample():
    """The seed of the main case, on the model alone (tests/test_gpu_history.py's rule): valid, zero-frame, evicted and skipped
    samples all occur, and the indices wrap."""
    cmds = commands(MAIN_SEED, 5, 13)
    m = HistoryModel(5, 4, 8)
    issued = []
    for cmd in cmds:
        idx = m.push(cmd)
        issued += [(n, int(k)) for n, k in enumerate(idx) if k >= 0]
    valid = [s for s in issued if m.valid(*s)]
    assert 3 * len(valid) >= len(issued)
    assert any(None in m.rows(*s) for s in valid) and len(valid) < len(issued) and (cmds & SKIP).any() and (cmds & CLEAR).any()
    assert int(m.count.max()) > 8


def _tensors(samples):
    return _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))


def _check(pipe, hist, aug, samples, shift, what="fovea", action=None):
    """observe and the shifted observe of `samples` into sentinel-filled outputs; returns the number of valid samples."""
    env, idx = _tensors(samples) if isinstance(samples, list) else samples
    B = int(env.shape[0])
    shape, bits = (B,) + hist.obs_row_shape(what), BITS[pipe.obs_dtype]
    if not isinstance(shift, torch.Tensor):
        shift = _t(np.broadcast_to(np.asarray(shift, np.int32), (B, 2)))
    outs = []
    for read, kw in ((hist.observe, {}), (aug.observe, {"shift": shift})):
        out = torch.full(shape, SENTINEL, dtype=pipe.obs_dtype, device=DEV)
        loc = torch.full((B, 2), -77, dtype=torch.int32, device=DEV)
        outs.append(read(env, idx, action=action, what=what, out=out, loc_out=loc, **kw))
    (ref, rloc, rvalid), (obs, loc, valid) = outs
    assert aug.last_shift is shift
    assert torch.equal(valid, rvalid), "validity differs from observe's"
    assert torch.equal(loc, rloc), "fov_loc differs from observe's (the shift must not be reflected; invalid rows stay untouched)"
    v = rvalid.bool()
    want = _gather(ref.reshape(B, -1, *shape[-2:]), shift, aug.pad).reshape(shape)
    assert torch.equal(obs[v].view(bits), want[v].view(bits)), "valid rows differ from the gather of the unshifted output"
    sent = torch.full_like(obs[~v], SENTINEL)
    assert torch.equal(obs[~v].view(bits), sent.view(bits)), "an invalid sample's row was written"
    return int(v.sum())


def _random_shifts(B, pad, seed):
    return _t(np.random.default_rng(seed).integers(0, 2 * pad + 1, (B, 2)).astype(np.int32))


# ---------------------------------------------------------------------------------------------- the main case
@gpu
@pytest.mark.parametrize("mode", ["resize", "mask", "raw", "full"])
def test_main_case(mode):
    """N = 5, fs = 4, 84 / 30 (the compile-time geometry), T = 8, 13 steps, pad = 4: the four corners, the identity and seeded
    random shifts, over every (n, k) ever issued plus one negative and one never-issued index per env."""
    from active_gym import FrameHistory, RandomShift
    what = "full" if mode == "full" else "fovea"
    pipe = _pipe(5, mode="resize" if mode == "full" else mode)
    hist = FrameHistory(pipe, 8)
    cmds = commands(MAIN_SEED, 5, 13)
    model, rec = _run(pipe, hist, cmds, MAIN_SEED)
    samples = _samples(model)
    issued, valid, zero, evicted = _kinds(model, rec, samples)
    assert 3 * valid >= issued and zero >= 1 and evicted >= 1 and (cmds & SKIP).any()
    aug = RandomShift(hist, pad=4)
    assert hist.shift(4) is hist.shift(4) and hist.shift(4) is not aug and hist.shift(4).pad == 4
    for s in CORNERS + [(4, 4)]:
        assert _check(pipe, hist, aug, samples, s, what) == valid
    assert _check(pipe, hist, aug, samples, _random_shifts(len(samples), 4, 1), what) == valid
    want_valid = np.array([model.valid(n, k) for n, k in samples])
    _, _, v = aug.observe(*_tensors(samples), what=what)                       # a drawn shift: validity is the model's
    assert np.array_equal(v.cpu().numpy().astype(bool), want_valid) and tuple(aug.last_shift.shape) == (len(samples), 2)
    pipe.close()
    assert not aug.alive and not hist.alive


@gpu
@pytest.mark.parametrize("mode", ["resize", "mask", "raw", "full"])
def test_identity(mode):
    """pad = 0 (whatever the shift values), and pad = 4 with every shift (4, 4): bit-equal to observe."""
    from active_gym import FrameHistory, RandomShift
    what = "full" if mode == "full" else "fovea"
    pipe = _pipe(5, mode="resize" if mode == "full" else mode)
    hist = FrameHistory(pipe, 8)
    model, _ = _run(pipe, hist, commands(MAIN_SEED, 5, 13), MAIN_SEED)
    samples = _samples(model)
    env, idx = _tensors(samples)
    ref, rloc, rvalid = hist.observe(env, idx, what=what)
    v, bits = rvalid.bool(), BITS[pipe.obs_dtype]
    for pad, shift in ((0, _random_shifts(len(samples), 7, 2) - 3), (4, (4, 4))):
        aug = RandomShift(hist, pad=pad)
        assert _check(pipe, hist, aug, samples, shift, what) == int(v.sum())
        obs, loc, valid = aug.observe(env, idx, what=what, shift=aug.last_shift)
        assert torch.equal(obs[v].view(bits), ref[v].view(bits)) and torch.equal(valid, rvalid), pad
        if pipe.kind == "fixed":
            assert torch.equal(loc[v], rloc[v])
    pipe.close()


# ---------------------------------------------------------------------------------------------- run-time geometry
@gpu
@pytest.mark.parametrize("kind, obs, fov, fs, mode, pad", [
    ("fixed", (100, 100), (30, 20), 3, "resize", 4),
    ("fixed", (8, 264), (4, 100), 3, "resize", 4),        # wider than a workgroup: the striding H pass reads xtab[cx(x)] itself
    ("fixed", (10, 12), (3, 5), 3, "raw", 4),             # shifts exceed the crop: the clamp saturates
    ("fixed", (100, 100), (30, 20), 1, "mask", 4),
    ("base", (10, 12), (3, 5), 1, "full", 16),            # the pad exceeds the plane
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_generic_geometry(kind, obs, fov, fs, mode, pad):
    from active_gym import FrameHistory, RandomShift
    what = "full" if mode == "full" else "fovea"
    pipe = _pipe(4, kind=kind, obs=obs, fov=fov, fs=fs, mode="resize" if mode == "full" else mode, action_mode="relative")
    hist = FrameHistory(pipe, 5)
    model, rec = _run(pipe, hist, commands(11, 4, 9), 11)
    samples = _samples(model)
    issued, valid, _, evicted = _kinds(model, rec, samples)
    assert valid >= 8 and evicted >= 1
    aug = RandomShift(hist, pad=pad)
    for s in [(0, 0), (0, 2 * pad), (2 * pad, 0), (2 * pad, 2 * pad), (pad, pad)]:
        assert _check(pipe, hist, aug, samples, s, what) == valid
    for seed in (3, 4):
        assert _check(pipe, hist, aug, samples, _random_shifts(len(samples), pad, seed), what) == valid
    pipe.close()


# ---------------------------------------------------------------------------------------------- the pad at its limit
PAD_LIMIT = 32                                             # AGX_SHIFT_PAD_LIMIT


@gpu
@pytest.mark.parametrize("obs, fov, fs, mode", [((84, 84), (30, 30), 4, m) for m in ("resize", "mask", "raw", "full")] +
                         [((10, 12), (3, 5), 3, m) for m in ("resize", "mask", "raw", "full")],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_shifted_observe_at_pad_limit(obs, fov, fs, mode):
    """pad = 32 (AGX_SHIFT_PAD_LIMIT; so far only the draw ran there), at the compile-time geometry 84 / 30 and at 10 x 12 / 3 x 5,
    where every shift but the identity leaves the 3 x 5 crop, in every mode the geometry builds: the corners, the identity and
    seeded random shifts over 0 .. 64 are bit for bit the gather of the unshifted output.  pad = 33 is refused by the library
    (AGX_E_INVALID) and by the Python surface."""
    from active_gym import FrameHistory, RandomShift
    from active_gym import _native as nat
    from active_gym import augment as ag
    import ctypes
    assert ag.PAD_LIMIT == PAD_LIMIT
    what = "full" if mode == "full" else "fovea"
    pipe = _pipe(4, obs=obs, fov=fov, fs=fs, mode="resize" if mode == "full" else mode, action_mode="relative")
    hist = FrameHistory(pipe, 5)
    model, rec = _run(pipe, hist, commands(11, 4, 9), 11)
    samples = _samples(model)
    issued, valid, _, evicted = _kinds(model, rec, samples)
    assert valid >= 8 and evicted >= 1
    aug = RandomShift(hist, pad=PAD_LIMIT)
    for s in [(0, 0), (64, 64), (0, 64), (64, 0), (32, 32)]:
        assert _check(pipe, hist, aug, samples, s, what) == valid
    for seed in (3, 4):
        shift = _random_shifts(len(samples), PAD_LIMIT, seed)
        assert int(shift.max()) > 40 and int(shift.min()) < 24
        assert _check(pipe, hist, aug, samples, shift, what) == valid
    handle = ctypes.c_void_p()
    assert ag.lib().agx_shift_create(hist.handle, PAD_LIMIT + 1, ctypes.byref(handle)) == nat.E_INVALID and not handle.value
    assert ag.lib().agx_shift_create(hist.handle, -1, ctypes.byref(handle)) == nat.E_INVALID and not handle.value
    what_code = 1 if what == "full" else 0                    # AGX_HIST_FULL / AGX_HIST_FOVEA: the pad is checked in front of the buffers
    assert ag.lib().agx_history_observe_shifted(hist.handle, what_code, None, None, 4, None, 0, PAD_LIMIT + 1, None, None, None, None,
                                                pipe._stream()) == nat.E_INVALID
    assert "pad must be 0 .. 32, got 33" in nat.last_error(pipe._ctx)
    with pytest.raises(ValueError, match="pad must be 0 .. 32"):
        RandomShift(hist, pad=PAD_LIMIT + 1)
    pipe.close()


# ---------------------------------------------------------------------------------------------- 16-bit outputs
@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("mode", ["resize", "raw"])
def test_16_bit_outputs(mode, dtype):
    """N = 3, T = 6: the one rounding at the store commutes with the move, fovea and full."""
    from active_gym import FrameHistory, RandomShift
    pipe = _pipe(3, mode=mode, dtype=dtype)
    hist = FrameHistory(pipe, 6)
    model, _ = _run(pipe, hist, commands(5, 3, 8), 5)
    samples = _samples(model)
    aug = RandomShift(hist, pad=4)
    for what in ("fovea", "full"):
        assert _check(pipe, hist, aug, samples, (0, 8), what) >= 6
        assert _check(pipe, hist, aug, samples, _random_shifts(len(samples), 4, 6), what) >= 6
    pipe.close()


# ---------------------------------------------------------------------------------------------- shift values, actions
@gpu
def test_out_of_range_shifts_are_clamped():
    """Components -3 and 99 at pad = 4 are 0 and 8."""
    from active_gym import FrameHistory, RandomShift
    pipe = _pipe(5)
    hist = FrameHistory(pipe, 8)
    model, _ = _run(pipe, hist, commands(MAIN_SEED, 5, 13), MAIN_SEED)
    samples = [s for s in _samples(model, extra=False) if model.valid(*s)]
    env, idx = _tensors(samples)
    aug = RandomShift(hist, pad=4)
    for wild, tame in (((-3, 99), (0, 8)), ((99, -3), (8, 0)), ((-2 ** 31, 2 ** 31 - 1), (0, 8))):
        assert _check(pipe, hist, aug, samples, wild) == len(samples)          # (the oracle clamps as the header says)
        a = aug.observe(env, idx, shift=_t(np.broadcast_to(np.array(wild, np.int32), (len(samples), 2))))[0]
        b = aug.observe(env, idx, shift=_t(np.broadcast_to(np.array(tame, np.int32), (len(samples), 2))))[0]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), wild
    pipe.close()


@gpu
@pytest.mark.parametrize("mode", ["resize", "mask", "raw"])
def test_counterfactual_action_and_shift(mode):
    """observe(action=a, shift=s) is the gather of observe(action=a): float32 and int64 actions, out-of-range ones included."""
    from active_gym import FrameHistory, RandomShift
    pipe = _pipe(5, mode=mode)
    hist = FrameHistory(pipe, 8)
    model, _ = _run(pipe, hist, commands(MAIN_SEED, 5, 13), MAIN_SEED)
    samples = _samples(model)
    B = len(samples)
    rng = np.random.default_rng(9)
    aug = RandomShift(hist, pad=4)
    for act in (rng.uniform(-20, 110, (B, 2)).astype(np.float32), rng.integers(-20, 110, (B, 2)).astype(np.int64)):
        _check(pipe, hist, aug, samples, _random_shifts(B, 4, 10), action=_t(act))
    pipe.close()


# ---------------------------------------------------------------------------------------------- more than one launch
@gpu
def test_more_samples_than_one_launch_takes():
    """B = 65,540 on a base (10, 12) context, fs = 1: shuffled repeats of a few valid samples, a shift of its own per sample.  The
    last five rows belong to the second launch: they expose a d_shift (or any other array) that was not advanced."""
    from active_gym import FrameHistory, RandomShift
    pipe = _pipe(4, kind="base", obs=(10, 12), fs=1)
    hist = FrameHistory(pipe, 5)
    model, _ = _run(pipe, hist, commands(11, 4, 9), 11)
    few = [s for s in _samples(model, extra=False) if model.valid(*s)][:7] + [(0, -1)]
    B = 65540
    rng = np.random.default_rng(13)
    pick = rng.integers(0, len(few), B)
    samples = (_t(np.array([few[i][0] for i in pick], np.int32)), _t(np.array([few[i][1] for i in pick], np.int64)))
    shift = rng.integers(0, 9, (B, 2)).astype(np.int32)
    assert (shift[65535:] != shift[:5]).any(axis=1).all() and (pick[65535:] != len(few) - 1).any()
    aug = RandomShift(hist, pad=4)
    assert _check(pipe, hist, aug, samples, _t(shift), "full") == int((pick != len(few) - 1).sum())
    pipe.close()


# ---------------------------------------------------------------------------------------------- the draw
@gpu
def test_draw_counter_seed_and_graph_replay():
    """Consecutive draws are the model's calls 0, 1, 2, ... at B = 1 / 257 / 70,000; B = 0 does not advance the counter; seed(s)
    restarts the sequence; draw + observe captured under torch.cuda.graph and replayed three times give the model's next three
    calls - fresh shifts - and the observations that go with them."""
    from active_gym import FrameHistory, RandomShift
    pipe = _pipe(5)
    hist = FrameHistory(pipe, 8)
    model, _ = _run(pipe, hist, commands(MAIN_SEED, 5, 13), MAIN_SEED)
    seed = (1 << 63) + 12345
    aug = RandomShift(hist, pad=4, seed=seed)
    call = 0
    for B in (1, 257, 70000):
        for _ in range(3):
            got = aug.draw(B)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), sm.draw(seed, call, B, 4)), (B, call)
            call += 1
    assert tuple(aug.draw(0).shape) == (0, 2)
    assert np.array_equal(aug.draw(300).cpu().numpy(), sm.draw(seed, call, 300, 4))
    assert np.array_equal(RandomShift(hist, pad=32).draw(300).cpu().numpy(), sm.draw(0, 0, 300, 32))       # a new source has seed 0
    aug.seed(9)
    samples = [s for s in _samples(model, extra=False) if model.valid(*s)]
    env, idx = _tensors(samples)
    B = len(samples)
    ref = hist.observe(env, idx)[0]
    shift = torch.empty((B, 2), dtype=torch.int32, device=DEV)
    out = torch.empty_like(ref)
    loc = torch.empty((B, 2), dtype=torch.int32, device=DEV)
    valid = torch.empty((B,), dtype=torch.uint8, device=DEV)

    def both():
        aug.draw(B, out=shift)
        aug.observe(env, idx, shift=shift, out=out, loc_out=loc, valid_out=valid)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both()                                               # call 0, eager, on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(shift.cpu().numpy(), sm.draw(9, 0, B, 4))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        both()                                               # captured, not run: the counter lives on the device
    seen = []
    for call in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        want = sm.draw(9, call, B, 4)
        assert np.array_equal(shift.cpu().numpy(), want), call
        assert torch.equal(out.view(torch.int32), _gather(ref, _t(want), 4).view(torch.int32)) and bool(valid.all()), call
        seen.append(want)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert np.array_equal(aug.draw(B).cpu().numpy(), sm.draw(9, 4, B, 4))      # usable one call at a time after the replays
    pipe.close()


@gpu
def test_refusals():
    from active_gym import FrameHistory, RandomShift
    from active_gym._native import AgxError, E_STATE
    pipe = _pipe(4, kind="base", obs=(10, 12), fs=1)
    hist = FrameHistory(pipe, 5)
    aug = RandomShift(hist, pad=4)
    env, idx = torch.zeros((3,), dtype=torch.int32, device=DEV), torch.zeros((3,), dtype=torch.int64, device=DEV)
    with pytest.raises(AgxError) as e:
        aug.observe(env, idx)                                # AGX_HIST_FOVEA on a base context
    assert e.value.code == E_STATE
    with pytest.raises(ValueError, match="what must be"):
        aug.observe(env, idx, what="both")
    with pytest.raises(ValueError, match="shift must have shape"):
        aug.observe(env, idx, what="full", shift=torch.zeros((2, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError, match="shift must be"):
        aug.observe(env, idx, what="full", shift=torch.zeros((3, 2), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="B must be"):
        aug.draw(-1)
    obs, _, valid = aug.observe(env[:0], idx[:0], what="full")          # B = 0
    assert tuple(obs.shape) == (0, 1, 10, 12) and valid.numel() == 0
    pipe.env_range(1, 2)                                     # a narrowed env range: refused as observe refuses it - not at B = 0
    shift3 = torch.zeros((3, 2), dtype=torch.int32, device=DEV)
    for call in (lambda: aug.observe(env, idx, what="full", shift=shift3), lambda: aug.draw(3), lambda: aug.seed(1), lambda: RandomShift(hist, pad=2)):
        with pytest.raises(AgxError, match="env range") as e:
            call()
        assert e.value.code == E_STATE
    shift0 = torch.zeros((0, 2), dtype=torch.int32, device=DEV)
    assert aug.observe(env[:0], idx[:0], what="full", shift=shift0)[0].numel() == 0 and hist.observe(env[:0], idx[:0], what="full")[0].numel() == 0
    pipe.env_range()
    hist.close()
    with pytest.raises(RuntimeError, match="closed"):
        aug.draw(4)
    pipe.close()


# ---------------------------------------------------------------------------------------------- the vector env
def _vec_env(native_loop):
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=150, native_loop=native_loop, history_len=16, step_log=True)
    return AtariVecEnv(AtariEnvArgs(**kw), 6, kind="fixed", noop_fn=lambda: 2)


@gpu
@pytest.mark.parametrize("native", [True, False], ids=["native_loop", "python_loop"])
def test_vec_env_replay_batch_with_shift_pad(native):
    """AtariVecEnv(N = 6, history_len = 16, step_log = True): replay_batch(32, nstep = 3, shift_pad = 4), uniform and prioritized -
    for ok rows obs / next_obs are the gather of history.observe at index / next_index with obs_shift / next_obs_shift, the two
    shifts are independent draws, and shift_pad = None returns the keys it returned before."""
    N = 6
    env = _vec_env(native)
    assert (env._loop is not None) == native
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(40):
        env.step({"motor_action": rng.integers(0, 4, N), "sensory_action": rng.uniform(-5, 90, (N, 2)).astype(np.float32)})
    plain = env.replay_batch(32, nstep=3)
    base_keys = ["env", "index", "next_index", "ok", "obs", "next_obs", "ret", "discount", "steps", "flags", "fov_loc", "next_fov_loc",
                 "motor_action", "sensory_action"]
    assert sorted(plain) == sorted(base_keys) and env.history._shifts == {}
    for prioritized in (False, True):
        out = env.replay_batch(32, nstep=3, shift_pad=4, prioritized=prioritized)
        assert sorted(out) == sorted(base_keys + ["obs_shift", "next_obs_shift"] + (["weight", "priority"] if prioritized else []))
        rows = out["ok"].bool()
        assert int(rows.sum()) >= 24
        for key, at in (("obs", "index"), ("next_obs", "next_index")):
            sh = out[key + "_shift"]
            assert sh.dtype == torch.int32 and tuple(sh.shape) == (32, 2) and int(sh.min()) >= 0 and int(sh.max()) <= 8
            ref, loc, _ = env.history.observe(out["env"], out[at])
            want = _gather(ref, sh, 4)
            assert torch.equal(out[key][rows].view(torch.int32), want[rows].view(torch.int32)), (prioritized, key)
            assert torch.equal(out["fov_loc" if key == "obs" else "next_fov_loc"][rows], loc[rows])
        assert not torch.equal(out["obs_shift"], out["next_obs_shift"])
    aug = env.random_shift(4)
    assert aug is env.random_shift(4) and aug is env.history.shift(4, 3) and list(env.history._shifts) == [(4, 3)]      # seed = args.seed
    with pytest.raises(ValueError, match="the glimpse memory is not shifted"):
        env.replay_batch(8, glimpses=3, shift_pad=4)
    env.close()
    assert not aug.alive
