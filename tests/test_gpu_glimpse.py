"""GPU: the glimpse memory (include/agx_glimpse.h) through ObsPipeline + FrameHistory + GlimpseMemory.  Every case drives
ingest -> fovea -> push over seeded command bytes with CLEAR and SKIP and keeps a clone of each observation and fov_loc the
step returned; the memory of a sample must equal, bit for bit, torch.maximum over the clones of its taken glimpses, which
glimpses are taken is the model's (tests/glimpse_model.py), and rows of invalid samples keep the sentinel."""
import json
import os

import numpy as np
import pytest
import torch

from glimpse_model import sample_class, taken_count
from history_model import CLEAR, SKIP, HistoryModel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -3.0                 # exact in float32, bfloat16 and float16; no observation value is negative
LOC_SENTINEL = -77
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
CASES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_cases.json")))


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pipe(N, obs=(84, 84), fov=(30, 30), fs=4, mode="resize", dtype=torch.float32, kind="fixed"):
    from active_gym import ObsPipeline
    kw = dict(num_envs=N, kind=kind, obs_size=obs, frame_stack=fs, device=DEV, obs_dtype=dtype)
    if kind != "base":
        kw.update(fov_size=fov, fov_init_loc=(min(2, obs[0] - fov[0]), min(3, obs[1] - fov[1])), sensory_action_mode="absolute",
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


def inputs(seed, N, steps, obs):
    """The frames u8 [steps][N][2][oh][ow] and sensory actions f32 [steps][N][2] of a run (NumPy: the oracle reads them too)."""
    rng = np.random.default_rng(seed + 1000)
    frames = rng.integers(0, 256, (steps, N, 2) + tuple(obs), dtype=np.uint8)
    acts = rng.uniform(-9, max(obs) + 5, (steps, N, 2)).astype(np.float32)
    return frames, acts


def _run(pipe, hist, cmds, seed):
    """Drive ingest + fovea + push over the command bytes.  Returns (model, rec): rec[(n, index)] = (obs row, fov_loc row), device
    clones of what the step returned."""
    N = pipe.num_envs
    frames, acts = inputs(seed, N, len(cmds), pipe.obs_size)
    model = HistoryModel(N, pipe.frame_stack, hist.capacity)
    rec = {}
    for step, cmd in enumerate(cmds):
        pipe.ingest_gray(_t(frames[step]), _t(cmd))
        obs, loc = pipe.fovea(_t(acts[step]))
        idx = hist.push(_t(cmd)).cpu().numpy()
        assert np.array_equal(idx, model.push(cmd)), "indices differ from the model"
        obs, loc = obs.clone(), loc.clone()
        for n in range(N):
            if idx[n] >= 0:
                rec[(n, int(idx[n]))] = (obs[n], loc[n])
    return model, rec


def _samples(model, seed=0, repeats=12):
    """Every (n, k) ever issued plus, per env, one index below 0 and one never issued, shuffled, with some repeats."""
    out = []
    for n in range(model.N):
        out += [(n, k) for k in range(-1, int(model.count[n]) + 1)]
    rng = np.random.default_rng(seed)
    out += [out[i] for i in rng.integers(0, len(out), repeats)]
    return [out[i] for i in rng.permutation(len(out))]


def _observe(pipe, hist, P, samples):
    from active_gym import GlimpseMemory
    B = len(samples)
    env = _t(np.array([s[0] for s in samples], np.int32))
    idx = _t(np.array([s[1] for s in samples], np.int64))
    out = torch.full((B,) + hist.obs_row_shape(), SENTINEL, dtype=pipe.obs_dtype, device=DEV)
    loc = torch.full((B, P, 2), LOC_SENTINEL, dtype=torch.int32, device=DEV)
    return GlimpseMemory(hist, P).observe(env, idx, out=out, loc_out=loc)


def _want(rec, n, k, count):
    """torch.maximum over the step-returned clones of glimpses 0 .. count - 1."""
    want = rec[(n, k)][0]
    for i in range(1, count):
        want = torch.maximum(want, rec[(n, k - i)][0])
    return want


def _check(pipe, hist, model, rec, P, samples):
    """observe into sentinel-filled outputs and compare everything; returns the class counts of the distinct samples."""
    obs, loc, taken = _observe(pipe, hist, P, samples)
    taken = taken.cpu().numpy()
    want_taken = np.array([taken_count(model, n, k, P) for n, k in samples])
    assert np.array_equal(taken, want_taken), "glimpses taken differ from the model"
    bits = BITS[pipe.obs_dtype]
    sent = torch.full(hist.obs_row_shape(), SENTINEL, dtype=pipe.obs_dtype, device=DEV).view(bits)
    loc = loc.cpu().numpy()
    classes = {"full": 0, "clear": 0, "evicted": 0, "invalid": 0}
    for n, k in set(samples):
        classes[sample_class(model, n, k, P)] += 1
    for b, (n, k) in enumerate(samples):
        if taken[b]:
            assert torch.equal(obs[b].view(bits), _want(rec, n, k, int(taken[b])).view(bits)), f"sample {(n, k)}: memory bits differ"
        else:
            assert torch.equal(obs[b].view(bits), sent), f"invalid sample {(n, k)}: row was written"
        for i in range(P):
            want = rec[(n, k - i)][1].tolist() if i < taken[b] else [LOC_SENTINEL, LOC_SENTINEL]
            assert loc[b, i].tolist() == want, f"sample {(n, k)}: fov_loc of glimpse {i}"
    return classes


# ---- case 1: P = 1 is hist.observe
@pytest.mark.parametrize("mode", ["mask", "resize"])
def test_one_glimpse_is_observe(mode):
    from active_gym import FrameHistory
    pipe = _pipe(3, mode=mode)
    hist = FrameHistory(pipe, 12)
    model, _ = _run(pipe, hist, commands(7, 3, 30), 7)
    samples = _samples(model)
    B = len(samples)
    env, idx = _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))
    want = torch.full((B,) + hist.obs_row_shape(), SENTINEL, device=DEV)
    wloc = torch.full((B, 2), LOC_SENTINEL, dtype=torch.int32, device=DEV)
    _, _, valid = hist.observe(env, idx, out=want, loc_out=wloc)
    got, gloc, taken = _observe(pipe, hist, 1, samples)
    assert int(valid.sum()) >= 20 and int((valid == 0).sum()) >= 6
    assert torch.equal(taken, valid)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(gloc[:, 0], wloc)
    pipe.close()


# ---- case 2: the main case.  One run per mode, shared by the P cases and the oracle check.
MAIN = dict(N=5, fs=4, T=12, steps=30, p_clear=0.1, p_skip=0.1)
MAIN_SEED = 28
MAIN_P = (2, 3, 8)


def _main_model(seed):
    cmds = commands(seed, MAIN["N"], MAIN["steps"], MAIN["p_clear"], MAIN["p_skip"])
    m = HistoryModel(MAIN["N"], MAIN["fs"], MAIN["T"])
    for cmd in cmds:
        m.push(cmd)
    return cmds, m


def _class_counts(m, P, samples):
    out = {"full": 0, "clear": 0, "evicted": 0, "invalid": 0}
    for n, k in set(samples):
        out[sample_class(m, n, k, P)] += 1
    return out


_main_runs = {}


@pytest.fixture(scope="module", autouse=True)
def _close_main_runs():
    yield
    for pipe, _, _, _ in _main_runs.values():
        pipe.close()
    _main_runs.clear()


def _main_run(mode):
    from active_gym import FrameHistory
    if mode not in _main_runs:
        pipe = _pipe(MAIN["N"], mode=mode, fs=MAIN["fs"])
        hist = FrameHistory(pipe, MAIN["T"])
        cmds, _ = _main_model(MAIN_SEED)
        model, rec = _run(pipe, hist, cmds, MAIN_SEED)
        _main_runs[mode] = (pipe, hist, model, rec)
    return _main_runs[mode]


@pytest.mark.parametrize("P", MAIN_P)
@pytest.mark.parametrize("mode", ["mask", "resize"])
def test_main_case(mode, P):
    """N = 5, fs = 4, 84 / 30 (the compile-time geometry), T = 12, 30 steps.  The seed was chosen on the model alone so that
    every class of sample occurs at least 5 times for every P; the counts are asserted on what was actually compared."""
    pipe, hist, model, rec = _main_run(mode)
    _, m = _main_model(MAIN_SEED)
    samples = _samples(model, seed=P)
    assert _class_counts(m, P, samples) == _class_counts(model, P, samples)
    assert len(set(samples)) < len(samples)                      # repeats
    classes = _check(pipe, hist, model, rec, P, samples)
    assert min(classes.values()) >= 5, classes


def _oracle_memories(mode, P, samples, model):
    """float64: the oracle's fixed-fovea observation of every taken glimpse, from the frames and actions the run was given (the ring
    and the fov_loc are re-derived here in NumPy), maxed."""
    from oracle import oracle as O
    N, fs, steps = MAIN["N"], MAIN["fs"], MAIN["steps"]
    cmds, _ = _main_model(MAIN_SEED)
    frames, acts = inputs(MAIN_SEED, N, steps, (84, 84))
    fov = [O.FixedFovealOracle((84, 84), (30, 30), (2, 3), "absolute", resize_to_full=mode == "resize", mask_out=mode == "mask") for _ in range(N)]
    stack = np.zeros((N, fs, 84, 84), np.uint8)
    count = np.zeros(N, np.int64)
    seen = {}
    for step in range(steps):
        for n in range(N):
            c = int(cmds[step, n])
            if not c & SKIP:
                if c & CLEAR:
                    stack[n] = 0
                new = frames[step, n, 0] if (c & 3) == 1 else np.maximum(frames[step, n, 0], frames[step, n, 1])
                stack[n] = np.concatenate([stack[n, 1:], new[None]], 0)
            fov[n].update_loc(acts[step, n])                      # the fovea call moves every env's fov_loc, skipped or not
            if not c & SKIP:
                seen[(n, int(count[n]))] = fov[n].get_fov_state(O.u8_to_unit(stack[n]).astype(np.float64))
                count[n] += 1
    out = {}
    for n, k in set(samples):
        t = taken_count(model, n, k, P)
        if t:
            out[(n, k)] = np.max(np.stack([seen[(n, k - i)] for i in range(t)], 0), 0)
    return out


@pytest.mark.parametrize("mode", ["mask", "resize"])
def test_main_case_against_the_float64_oracle(mode):
    """Case 7: rests neither on the new kernel nor on hist.observe - within the project's 1e-5 of the NumPy maximum of the
    oracle's observations of the taken glimpses, P = 3."""
    pipe, hist, model, _ = _main_run(mode)
    P = 3
    samples = _samples(model, seed=P)
    want = _oracle_memories(mode, P, samples, model)
    assert len(want) >= 40
    obs, _, taken = _observe(pipe, hist, P, samples)
    obs, taken = obs.cpu().numpy(), taken.cpu().numpy()
    worst = 0.0
    for b, s in enumerate(samples):
        assert (taken[b] > 0) == (s in want)
        if taken[b]:
            worst = max(worst, float(np.abs(obs[b] - want[s]).max()))
    print(f"glimpse memory vs float64 oracle ({mode}): max abs error {worst:.3g}")
    assert worst <= 1e-5


# ---- case 3: T at its minimum
@pytest.mark.parametrize("T", [6, 4], ids=["T=fs+P-1", "T=fs"])
@pytest.mark.parametrize("mode", ["mask", "resize"])
def test_smallest_capacity(mode, T):
    """fs = 4, P = 3.  T = 6: every row is rewritten every T steps and all three glimpses of the newest sample survive; T = fs:
    nothing older than glimpse 0 does, unless the episode is younger than the stack."""
    from active_gym import FrameHistory
    pipe = _pipe(3, mode=mode)
    hist = FrameHistory(pipe, T)
    model, rec = _run(pipe, hist, commands(4, 3, 17, p_clear=0.12), 4)
    assert int(model.count.min()) > 2 * T                          # wrap-around, more than once
    classes = _check(pipe, hist, model, rec, 3, _samples(model))
    assert classes["invalid"] >= 6 and classes["full"] + classes["clear"] + classes["evicted"] >= 3, classes
    if T == 6:
        assert classes["full"] >= 1, classes
    pipe.close()


# ---- case 4: low occupancy
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("mode", ["mask", "resize"])
def test_low_occupancy(mode, N):
    """B = 1 and B = 5 on N envs: one workgroup per stack position and sample, far fewer workgroups than CUs."""
    from active_gym import FrameHistory
    pipe = _pipe(N, mode=mode)
    hist = FrameHistory(pipe, 8)
    model, rec = _run(pipe, hist, commands(2, N, 9, p_clear=0.1, p_skip=0.1), 2)
    full = [(n, k) for n in range(N) for k in range(int(model.count[n])) if taken_count(model, n, k, 3) == 3]
    assert full
    assert _check(pipe, hist, model, rec, 3, full[-1:])["full"] == 1                       # B = 1
    five = [(n, int(model.count[n]) - 1 - d) for n in range(N) for d in range(5)][:5]
    assert len(set(five)) == 5 and sum(_check(pipe, hist, model, rec, 3, five).values()) == 5   # B = 5
    pipe.close()


# ---- case 5: the run-time geometry form
@pytest.mark.parametrize("mode", ["mask", "resize"])
@pytest.mark.parametrize("obs, fov, fs", [((100, 100), (30, 20), 3), ((128, 128), (31, 9), 1), ((8, 264), (4, 100), 3)],
                         ids=["100x100-30x20-fs3", "128x128-31x9-fs1", "8x264-4x100-fs3"])
def test_generic_geometry(obs, fov, fs, mode):
    """k_fovea_fixed<GeomR> geometries of tests/golden/geometry_cases.json with a non-square window: the LDS accumulator.
    8 x 264: the ow > 256 striding horizontal pass together with it."""
    from active_gym import FrameHistory
    assert any(tuple(c["obs"]) == obs and tuple(c["fov"]) == fov and c["fs"] == fs and "GeomR" in c["plan"].get("fixed_" + mode, "") for c in CASES)
    pipe = _pipe(4, obs=obs, fov=fov, fs=fs, mode=mode)
    hist = FrameHistory(pipe, 7)
    model, rec = _run(pipe, hist, commands(11, 4, 12, p_clear=0.1), 11)
    classes = _check(pipe, hist, model, rec, 3, _samples(model, repeats=4))
    assert classes["full"] >= 4 and classes["invalid"] >= 8 and classes["clear"] + classes["evicted"] >= 2, classes
    pipe.close()


# ---- case 6: 16-bit outputs
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("mode", ["mask", "resize"])
def test_16_bit_outputs(mode, dtype):
    """The 16-bit memory equals the float32 memory .to(dtype) bit for bit (the same run on a float32 and a 16-bit context), and
    the maximum of that context's own step outputs."""
    from active_gym import FrameHistory
    cmds = commands(5, 3, 14, p_clear=0.1)
    outs = []
    for dt in (torch.float32, dtype):
        pipe = _pipe(3, mode=mode, dtype=dt)
        hist = FrameHistory(pipe, 8)
        model, rec = _run(pipe, hist, cmds, 5)
        samples = _samples(model)
        classes = _check(pipe, hist, model, rec, 3, samples)
        assert classes["full"] >= 5
        obs, _, taken = _observe(pipe, hist, 3, samples)
        outs.append((obs, taken))
        pipe.close()
    (o32, t32), (o16, t16) = outs
    assert torch.equal(t32, t16)
    ok = t32 > 0
    assert torch.equal(o32[ok].to(dtype).view(torch.int16), o16[ok].view(torch.int16))


# ---- case 8: more than one launch
def test_more_samples_than_one_launch():
    """B = 65536 + 3 at obs 12 x 12, fov 4 x 4, fs = 1, mask-out (38 MB of output): the first, the 65535th, the 65536th and the
    last rows."""
    from active_gym import FrameHistory
    pipe = _pipe(4, obs=(12, 12), fov=(4, 4), fs=1, mode="mask")
    hist = FrameHistory(pipe, 8)
    model, rec = _run(pipe, hist, commands(3, 4, 8, p_clear=0.0, p_skip=0.0), 3)
    B = 65536 + 3
    rng = np.random.default_rng(1)
    env, idx = rng.integers(0, 4, B).astype(np.int32), rng.integers(2, 8, B).astype(np.int64)
    idx[65534] = 9                                                  # never issued: an invalid row right at the launch boundary
    out = torch.full((B, 1, 12, 12), SENTINEL, device=DEV)
    from active_gym import GlimpseMemory
    obs, loc, taken = GlimpseMemory(hist, 3).observe(_t(env), _t(idx), out=out)
    taken = taken.cpu().numpy()
    assert taken[65534] == 0 and bool((out[65534] == SENTINEL).all())
    assert (np.delete(taken, 65534) == 3).all()
    for b in (0, 65533, 65535, 65536, B - 1):
        n, k = int(env[b]), int(idx[b])
        assert torch.equal(obs[b].view(torch.int32), _want(rec, n, k, 3).view(torch.int32)), b
        assert loc[b].tolist() == [rec[(n, k - i)][1].tolist() for i in range(3)], b
    pipe.close()


# ---- case 9: refusals
def test_refusals():
    from active_gym import FrameHistory, GlimpseMemory
    from active_gym import _native as nat
    from active_gym.glimpse import observe_memory
    z32, z64 = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    cmd = torch.full((2,), 2, dtype=torch.uint8, device=DEV)

    def refused(pipe, hist, P, code, match, shape):
        out = torch.full((1,) + shape, SENTINEL, dtype=torch.float32, device=DEV)
        loc = torch.full((1, P, 2), LOC_SENTINEL, dtype=torch.int32, device=DEV)
        tk = torch.full((1,), 99, dtype=torch.uint8, device=DEV)
        with pytest.raises(nat.AgxError, match=match) as e:
            observe_memory(hist, P, z32, z64, out=out, loc_out=loc, taken_out=tk)
        assert e.value.code == code
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((loc == LOC_SENTINEL).all()) and int(tk[0]) == 99      # nothing was written

    base = _pipe(2, kind="base")
    hist = FrameHistory(base, 4)
    refused(base, hist, 3, nat.E_STATE, "AGX_KIND_FIXED only", (4, 84, 84))
    with pytest.raises(ValueError, match="kind 'fixed'"):
        GlimpseMemory(hist, 3)
    base.close()
    raw = _pipe(2, mode="raw")
    hist = FrameHistory(raw, 4)
    refused(raw, hist, 3, nat.E_STATE, "raw-crop mode is not served", (4, 30, 30))
    with pytest.raises(ValueError, match="raw crops"):
        GlimpseMemory(hist, 3)
    raw.close()
    pipe = _pipe(2, mode="mask")
    hist = FrameHistory(pipe, 4)
    pipe.ingest_gray(torch.zeros((2, 2, 84, 84), dtype=torch.uint8, device=DEV), cmd)
    pipe.fovea()
    hist.push(cmd)                                                              # sample (0, 0) is valid
    for P in (0, 9):
        refused(pipe, hist, P, nat.E_INVALID, "glimpses must be 1 .. 8", (4, 84, 84))
        with pytest.raises(ValueError, match="glimpses must be"):
            GlimpseMemory(hist, P)
    pipe.env_range(1, 1)                                                        # (lo, count): env 1 of the 2
    refused(pipe, hist, 3, nat.E_STATE, "env range", (4, 84, 84))
    pipe.env_range()
    _, _, taken = GlimpseMemory(hist, 3).observe(z32, z64)
    assert int(taken[0]) == 1
    o, l, t = GlimpseMemory(hist, 3).observe(z32[:0], z64[:0])                  # B = 0
    assert tuple(o.shape) == (0, 4, 84, 84) and tuple(l.shape) == (0, 3, 2) and tuple(t.shape) == (0,)
    pipe.close()


# ---- case 10: the vector env
def _vec_env(native_loop, history_len):
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=150, native_loop=native_loop)
    if history_len is not None:
        kw["history_len"] = history_len
    return AtariVecEnv(AtariEnvArgs(**kw), 6, kind="fixed", noop_fn=lambda: 2)


def test_vec_env_glimpse_memory():
    """AtariVecEnv(history_len=16).glimpse_memory(3) after every reset / step: the max over the last up-to-3 observations returned
    for that env since its last reset - just the returned observation for an env autoreset in that step; native and Python loop."""
    N, STEPS = 6, 40
    for native in (True, False):
        env = _vec_env(native, 16)
        assert (env._loop is not None) == native
        obs, _ = env.reset()
        last = [[obs[i].clone()] for i in range(N)]

        def check():
            mem = env.glimpse_memory(3)
            for i in range(N):
                want = last[i][-1]
                for o in last[i][-3:-1]:
                    want = torch.maximum(want, o)
                assert torch.equal(mem[i].view(torch.int32), want.view(torch.int32)), i
        check()
        rng = np.random.default_rng(0)
        dones = 0
        for step in range(STEPS):
            act = {"motor_action": rng.integers(0, 4, N), "sensory_action": rng.uniform(-5, 90, (N, 2)).astype(np.float32)}
            obs, _, done, _, _ = env.step(act)
            for i in range(N):
                if done[i]:
                    last[i] = []
                    dones += 1
                last[i].append(obs[i].clone())
            check()
        assert dones >= 5                        # several autoresets
        assert torch.equal(env.glimpse_memory(1), obs)
        env.close()
    env = _vec_env(True, 0)
    env.reset()
    with pytest.raises(ValueError, match="history"):
        env.glimpse_memory(3)
    env.close()
