"""GPU: sequence replay (include/agx_sequence.h) through ObsPipeline + FrameHistory + StepLog + SequenceReplay.  The oracle is the
project's own per-transition code plus a small model: a live step's rows are StepLog.gather's and FrameHistory.observe's for the
env-step (n, k + l), which steps are live is tests/sequence_model.py's (and agx_replay_inspect's), and every other step is zeros.
No tolerance anywhere: floats are compared as integer bit patterns, every (n, k) of a case is compared, and every output is
pre-filled with a sentinel that must not survive."""
import ctypes

import numpy as np
import pytest
import torch

import sequence_model as qm
import steplog_model as sm
from history_model import HistoryModel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = ctypes.c_void_p
GAMMA = 0.99
SENTINEL = -3.0                 # exact in float32, bfloat16 and float16; no observation value is negative
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
W = 12


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ptr(t):
    return None if t is None else P(t.data_ptr())


class Case:
    """A pipeline with a history, a step log and a SequenceReplay on it, driven over command bytes next to the models."""

    def __init__(self, N, fs, T, kind="fixed", obs=(84, 84), fov=(30, 30), mode="resize", dtype=torch.float32):
        from active_gym import FrameHistory, ObsPipeline, SequenceReplay, StepLog
        kw = dict(num_envs=N, kind=kind, obs_size=obs, frame_stack=fs, device=DEV, obs_dtype=dtype)
        if kind != "base":
            kw.update(fov_size=fov, fov_init_loc=(min(2, obs[0] - fov[0]), min(3, obs[1] - fov[1])), sensory_action_mode="absolute",
                      resize_to_full=mode == "resize", mask_out=mode == "mask")
        self.pipe = ObsPipeline(**kw)
        self.hist = FrameHistory(self.pipe, T)
        self.log = StepLog(self.hist, W)
        self.seq = SequenceReplay(self.log)
        self.hm = HistoryModel(N, fs, T)
        self.lm = sm.StepLogModel(self.hm, W)
        self.fs, self.bits = fs, BITS[dtype]

    def drive(self, cmds, seed, p_unrecorded=0.2):
        """ingest / observation / push over the command bytes, a record after each push: random float32 rewards, random flags, W
        random bytes, and about p_unrecorded of the pushed rows left unrecorded."""
        pipe, N = self.pipe, self.pipe.num_envs
        oh, ow = pipe.obs_size
        rng = np.random.default_rng(seed + 1000)
        for cmd in cmds:
            pipe.ingest_gray(_t(rng.integers(0, 256, (N, 2, oh, ow), dtype=np.uint8)), _t(cmd))
            if pipe.kind == "base":
                pipe.observe_full()
            else:
                pipe.fovea(_t(rng.uniform(-9, max(oh, ow) + 5, (N, 2)).astype(np.float32)))
            idx = self.hist.push(_t(cmd)).cpu().numpy()
            assert np.array_equal(idx, self.hm.push(cmd)), "indices differ from the model"
            idx[rng.random(N) < p_unrecorded] = -1
            reward = (rng.standard_normal(N) * 3).astype(np.float32)
            flags = ((rng.random(N) < 0.15) * sm.TERMINATED + (rng.random(N) < 0.05) * sm.TRUNCATED).astype(np.uint8)
            payload = rng.integers(0, 256, (N, W), dtype=np.uint8)
            self.log.record(_t(idx), _t(reward), _t(flags), _t(payload))
            self.lm.record(idx, reward, flags, payload)
        return self

    def close(self):
        self.pipe.close()


def _case(name, **kw):
    seed, N, fs, T, steps, _ = qm.CASES[name]
    return Case(N, fs, T, **kw).drive(qm.commands(seed, N, steps), seed)


def _pair(samples):
    return _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))


def _flat(samples, L, lens):
    """The B * L env-steps of the sequences in [B][L] order -> (env i32, index i64, live bool); a step that is not live is (-1, -1),
    which StepLog.gather and history.observe both take for no sample."""
    n = np.repeat(np.array([s[0] for s in samples], np.int32), L)
    k = np.repeat(np.array([s[1] for s in samples], np.int64), L)
    l = np.tile(np.arange(L, dtype=np.int64), len(samples))
    live = l < np.repeat(np.asarray(lens, np.int64), L)
    return np.where(live, n, -1).astype(np.int32), np.where(live, k + l, -1).astype(np.int64), live


def _layout(t, B, L, time_major):
    """A [B * L, ...] reference in [B][L] order -> the call's layout."""
    t = t.reshape((B, L) + tuple(t.shape[1:]))
    return t.transpose(0, 1).contiguous() if time_major else t


def _lengths(c, samples, L):
    """seq.lengths against the model and against 1 + min(inspect.ahead, L - 1) -> the model's lengths."""
    from active_gym import replay
    env, idx = _pair(samples)
    got = c.seq.lengths(env, idx, L, out=torch.full((len(samples),), -9, dtype=torch.int32, device=DEV)).cpu().numpy()
    want = np.array([qm.length(c.hm, n, k, L) for n, k in samples], np.int32)
    assert np.array_equal(got, want), f"L = {L}: lengths differ from the model"
    ahead = replay.inspect(c.hist, env, idx)[1].cpu().numpy()
    assert np.array_equal(got, np.where(ahead < 0, 0, 1 + np.minimum(ahead, L - 1))), f"L = {L}: lengths differ from inspect's ahead"
    return want


GATHER_KEYS = ("steps", "next_index", "ret", "discount", "flags", "payload")


def _gather_outs(shape):
    """The outputs of agx_sequence_gather, sentinel-filled."""
    return {"steps": torch.full(shape, -9, dtype=torch.int32, device=DEV), "next_index": torch.full(shape, -9, dtype=torch.int64, device=DEV),
            "ret": torch.full(shape, -7.5, dtype=torch.float32, device=DEV), "discount": torch.full(shape, -7.5, dtype=torch.float32, device=DEV),
            "flags": torch.full(shape, 0xAB, dtype=torch.uint8, device=DEV), "payload": torch.full(shape + (W,), 0xAB, dtype=torch.uint8, device=DEV)}


def _raw_gather(c, env, idx, L, nstep, time_major, out, length=None):
    from active_gym import _native as nat
    B = int(env.shape[0])
    rc = c.seq._lib.agx_sequence_gather(c.log._s, _ptr(env), _ptr(idx), B, L, nstep, GAMMA, int(time_major), _ptr(length), _ptr(out.get("steps")),
                                        _ptr(out.get("next_index")), _ptr(out.get("ret")), _ptr(out.get("discount")), _ptr(out.get("flags")),
                                        _ptr(out.get("payload")), c.pipe._stream())
    nat.check(rc, c.pipe._ctx)


def _same_rows(got, want, B, L, time_major, what):
    """Per-step outputs against a [B * L] reference of StepLog.gather's, floats as bit patterns."""
    for key in GATHER_KEYS:
        g, w = got[key], _layout(want[key], B, L, time_major)
        if g.dtype == torch.float32:
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert g.shape == w.shape and torch.equal(g, w), f"{key} differs from StepLog.gather ({what})"


def _gather(c, samples, L, lens, nsteps=(1, 3, 64), layouts=(False, True)):
    """agx_sequence_gather into sentinel-filled outputs against StepLog.gather on the flattened list, dead rows (-1, -1)."""
    B = len(samples)
    env, idx = _pair(samples)
    fe, fi, live = _flat(samples, L, lens)
    seen = set()
    for nstep in nsteps:
        want = c.log.gather(_t(fe), _t(fi), nstep, GAMMA)          # zeros, steps = 0 and next_index = -1 where nothing was folded
        seen.update(want["steps"].cpu().numpy()[live].tolist())
        assert not want["steps"].cpu().numpy()[~live].any()
        for tm in layouts:
            out = _gather_outs((L, B) if tm else (B, L))
            length = torch.full((B,), -9, dtype=torch.int32, device=DEV)
            _raw_gather(c, env, idx, L, nstep, tm, out, length)
            assert np.array_equal(length.cpu().numpy(), lens), f"d_len differs (L = {L}, nstep = {nstep})"
            _same_rows(out, want, B, L, tm, f"L = {L}, nstep = {nstep}, time_major = {tm}")
    return seen


def _observe(c, samples, L, lens, what="fovea", planes_list=(1, 2, None), layouts=(False, True), d_len=None, by_validity=False):
    """seq.observe into sentinel-filled outputs against history.observe of the flattened env-steps into zero-filled ones.
    by_validity: the d_len passed is not the truth - every step (n, k + l) that history.observe takes for valid is live."""
    B, fs = len(samples), c.fs
    env, idx = _pair(samples)
    if by_validity:
        fe = np.repeat(np.array([s[0] for s in samples], np.int32), L)
        fi = np.repeat(np.array([s[1] for s in samples], np.int64), L) + np.tile(np.arange(L, dtype=np.int64), B)
        live = np.array([c.hm.valid(int(n), int(k)) for n, k in zip(fe, fi)])
    else:
        fe, fi, live = _flat(samples, L, lens)
    row = c.hist.obs_row_shape(what)
    ref = torch.zeros((B * L,) + row, dtype=c.pipe.obs_dtype, device=DEV)
    refloc = torch.zeros((B * L, 2), dtype=torch.int32, device=DEV)
    ref, refloc, valid = c.hist.observe(_t(fe), _t(fi), what=what, out=ref, loc_out=refloc)
    assert np.array_equal(valid.cpu().numpy().astype(bool), live), "the live steps are not the valid ones"
    assert (ref.view(c.bits)[_t(~live)] == 0).all()
    lens_t = _t(np.asarray(lens, np.int32)) if d_len is None else d_len
    for planes in planes_list:
        p = fs if planes is None else planes
        if p > fs:
            continue
        for tm in layouts:
            shp = (L, B) if tm else (B, L)
            out = torch.full(shp + (p,) + row[1:], SENTINEL, dtype=c.pipe.obs_dtype, device=DEV)
            loc = torch.full(shp + (2,), -77, dtype=torch.int32, device=DEV)
            lv = torch.full(shp, 9, dtype=torch.uint8, device=DEV)
            got, gloc, glive = c.seq.observe(env, idx, lens_t, L, what=what, planes=planes, time_major=tm, out=out, loc_out=loc, live_out=lv)
            tag = f"{what}, L = {L}, planes = {p}, time_major = {tm}"
            assert got is out and tuple(got.shape) == shp + (p,) + row[1:]
            assert torch.equal(got.view(c.bits), _layout(ref[:, fs - p:], B, L, tm).view(c.bits)), f"observation bits differ ({tag})"
            assert torch.equal(glive, _layout(_t(live.astype(np.uint8)), B, L, tm)), f"live differs ({tag})"
            assert not (got == SENTINEL).any(), f"a sentinel survived ({tag})"
            dead = _layout(_t(~live), B, L, tm)
            assert (got.view(c.bits)[dead] == 0).all(), f"a dead step is not all-zero bytes ({tag})"
            if c.pipe.kind == "fixed":
                assert torch.equal(gloc, _layout(refloc, B, L, tm)), f"fov_loc differs ({tag})"
    return int(live.sum())


# ---------------------------------------------------------------------------------------------- the main case
MAIN_LS = (1, 3, 8)


@pytest.fixture(scope="module")
def main_resize():
    c = _case("main")
    yield c
    c.close()


def test_main_case_lengths_and_gather(main_resize):
    """N = 5, fs = 4, 84 / 30, T = 16, 25 steps with CLEAR and SKIP, a fifth of the rows unrecorded; starts: every (n, k), k in
    [-1, cnt], plus env -1 and N; L = 1, 3, 8; nstep = 1, 3, 64; both layouts."""
    c = main_resize
    samples = qm.starts(c.hm)
    assert (c.lm.stamp < 0).any() and int(c.hm.count.max()) > 16
    seen = set()
    for L in MAIN_LS:
        lens = _lengths(c, samples, L)
        seen |= _gather(c, samples, L, lens)
    assert min(qm.kinds(c.hm, 8).values()) >= 1 and {0, 1, 2, 3} <= seen
    got = c.seq.gather(*_pair(samples), 8, nstep=3, gamma=GAMMA)          # the Python surface: the same rows, freshly allocated
    fe, fi, _ = _flat(samples, 8, _lengths(c, samples, 8))
    _same_rows(got, c.log.gather(_t(fe), _t(fi), 3, GAMMA), len(samples), 8, False, "SequenceReplay.gather")


@pytest.mark.parametrize("mode", ["resize", "mask", "raw", "full"])
def test_main_case_observe(mode, main_resize):
    """observe in every mode, planes 1 / 2 / fs, both layouts, L = 1, 3, 8, into sentinel-filled outputs."""
    c = main_resize if mode in ("resize", "full") else _case("main", mode=mode)
    samples = qm.starts(c.hm)
    for L in MAIN_LS:
        lens = np.array([qm.length(c.hm, n, k, L) for n, k in samples], np.int32)
        live = _observe(c, samples, L, lens, what="full" if mode == "full" else "fovea")
        assert live == int(lens.sum()) >= len(samples) // 3
    if c is not main_resize:
        c.close()


def test_a_wrong_length_gives_a_defined_result(main_resize):
    """d_len = L for every sample, and d_len beyond L: the kernel re-checks validity, so exactly the steps (n, k + l) that
    history.observe takes for valid are written as live - another episode's included - and the others are zeros."""
    c = main_resize
    samples = qm.starts(c.hm)
    for d in (8, 1000):
        wrong = torch.full((len(samples),), d, dtype=torch.int32, device=DEV)
        live = _observe(c, samples, 8, None, planes_list=(1, None), layouts=(False,), d_len=wrong, by_validity=True)
        assert live > int(sum(qm.length(c.hm, n, k, 8) for n, k in samples))
    none = torch.zeros((len(samples),), dtype=torch.int32, device=DEV)          # ... and a d_len of 0 or below: nothing is live
    for d in (0, -5):
        _observe(c, samples, 8, np.zeros(len(samples), np.int32), planes_list=(1,), layouts=(True,), d_len=none + d)


@pytest.mark.parametrize("mode, dtype", [("resize", torch.bfloat16), ("raw", torch.float16)], ids=["resize-bf16", "raw-f16"])
def test_16_bit_outputs(mode, dtype):
    c = _case("dtype", mode=mode, dtype=dtype)
    samples = qm.starts(c.hm)
    L = qm.CASES["dtype"][5]
    lens = _lengths(c, samples, L)
    assert _observe(c, samples, L, lens) >= 10
    assert _observe(c, samples, L, lens, what="full", planes_list=(1,), layouts=(False,)) >= 10
    c.close()


def test_run_time_geometry():
    """obs 40 x 160, fov 12 x 50, fs = 3: the run-time geometry form, planes 1 / 2 / 3."""
    c = _case("geometry", obs=(40, 160), fov=(12, 50), mode="resize")
    samples = qm.starts(c.hm)
    L = qm.CASES["geometry"][5]
    lens = _lengths(c, samples, L)
    _gather(c, samples, L, lens, nsteps=(3,), layouts=(False,))
    assert _observe(c, samples, L, lens, planes_list=(1, 2, 3)) >= 8
    c.close()


def test_base_context():
    """A base context serves what = "full" only."""
    from active_gym import _native as nat
    c = _case("base", kind="base")
    samples = qm.starts(c.hm)
    L = qm.CASES["base"][5]
    lens = _lengths(c, samples, L)
    _gather(c, samples, L, lens, nsteps=(3,), layouts=(True,))
    assert _observe(c, samples, L, lens, what="full", planes_list=(1, None)) >= 8
    env, idx = _pair(samples)
    with pytest.raises(nat.AgxError, match="AGX_HIST_FULL only") as e:
        c.seq.observe(env, idx, _t(lens), L, what="fovea")
    assert e.value.code == nat.E_STATE
    c.close()


# ---------------------------------------------------------------------------------------------- L > 64
def test_sequences_longer_than_a_wave():
    """N = 2, obs 4 x 4 / fov 1 x 1 (the smallest a context accepts), T = 320, 300 appends with CLEARs placed so that lengths of 64,
    65, 70, 128 and 256 occur: the carry across 64-step chunks."""
    c = Case(qm.LONG_N, qm.LONG_FS, qm.LONG_T, obs=(4, 4), fov=(1, 1)).drive(qm.long_commands(), 17, p_unrecorded=0.1)
    samples = qm.starts(c.hm)
    env, idx = _pair(samples)
    at256 = c.seq.lengths(env, idx, 256).cpu().numpy()
    for s, want in qm.LONG_WITNESS.items():
        assert at256[samples.index(s)] == want, s
    for L in qm.LONG_LS:
        lens = _lengths(c, samples, L)
        assert L in lens and 0 in lens and ((lens > 0) & (lens < L)).any()
        seen = _gather(c, samples, L, lens, nsteps=(3, 64) if L == 70 else (3,), layouts=(False, True) if L in (70, 256) else (False,))
        assert {0, 3} <= seen
    lens = np.array([qm.length(c.hm, n, k, 70) for n, k in samples], np.int32)
    assert _observe(c, samples, 70, lens, planes_list=(1,)) == int(lens.sum())
    c.close()


# ---------------------------------------------------------------------------------------------- more rows than a grid dimension
def test_more_than_65535_rows():
    """B = 8200, L = 8 = 65600 rows, raw crop, planes = 1, bfloat16: the rows of the second launch - and the last of the first -
    against history.observe of just those env-steps."""
    c = _case("main", mode="raw", dtype=torch.bfloat16)
    starts = qm.starts(c.hm)
    B, L = 8200, 8
    samples = [starts[i % len(starts)] for i in range(B)]
    env, idx = _pair(samples)
    lens = np.array([qm.length(c.hm, n, k, L) for n, k in samples], np.int32)
    out = torch.full((B, L, 1, 30, 30), SENTINEL, dtype=torch.bfloat16, device=DEV)
    length = c.seq.lengths(env, idx, L)
    assert np.array_equal(length.cpu().numpy(), lens)
    got, loc, live = c.seq.observe(env, idx, length, L, planes=1, out=out)
    fe, fi, want_live = _flat(samples, L, lens)
    assert np.array_equal(live.reshape(-1).cpu().numpy().astype(bool), want_live) and not (got == SENTINEL).any()
    lo = 65000                                   # 535 rows of the first launch, all 65 of the second
    assert B * L - 65535 == 65
    ref = torch.zeros((B * L - lo, 4, 30, 30), dtype=torch.bfloat16, device=DEV)
    refloc = torch.zeros((B * L - lo, 2), dtype=torch.int32, device=DEV)
    c.hist.observe(_t(fe[lo:]), _t(fi[lo:]), out=ref, loc_out=refloc)
    assert want_live[65535:].any() and not want_live[65535:].all()
    assert torch.equal(got.reshape(B * L, 1, 30, 30)[lo:].view(torch.int16), ref[:, 3:].view(torch.int16))
    assert torch.equal(loc.reshape(B * L, 2)[lo:], refloc)
    c.close()


# ---------------------------------------------------------------------------------------------- edges
def test_empty_batches_null_outputs_and_refusals():
    from active_gym import _native as nat
    c = _case("graph")
    lib, st, h, s = c.seq._lib, c.pipe._stream(), c.hist.handle, c.log._s
    samples = qm.starts(c.hm)
    env, idx = _pair(samples)
    B, L = len(samples), 6
    lens = _lengths(c, samples, L)
    fe, fi, live = _flat(samples, L, lens)
    want = c.log.gather(_t(fe), _t(fi), 3, GAMMA)
    # every output but d_steps may be NULL, d_len too
    steps = torch.full((B, L), -9, dtype=torch.int32, device=DEV)
    _raw_gather(c, env, idx, L, 3, False, {"steps": steps})
    assert torch.equal(steps.reshape(-1), want["steps"])
    from active_gym import StepLog
    log0 = StepLog(c.hist, 0)                    # a log without a payload ignores d_payload
    steps0 = torch.full((B, L), -9, dtype=torch.int32, device=DEV)
    assert lib.agx_sequence_gather(log0._s, _ptr(env), _ptr(idx), B, L, 3, GAMMA, 0, None, _ptr(steps0), None, None, None, None, None, st) == nat.OK
    assert not steps0.any()                      # nothing was recorded in it
    # d_fov_loc and d_live may be NULL
    lens_t = _t(lens)
    out = torch.full((B, L, 1, 84, 84), SENTINEL, device=DEV)
    assert lib.agx_sequence_observe(h, 0, _ptr(env), _ptr(idx), _ptr(lens_t), B, L, 1, 0, _ptr(out), None, None, st) == nat.OK
    ref, _, lv = c.seq.observe(env, idx, lens_t, L, planes=1)
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32)) and np.array_equal(lv.reshape(-1).cpu().numpy().astype(bool), live)
    # planes above frame_stack: refused once the handle is known
    assert lib.agx_sequence_observe(h, 0, _ptr(env), _ptr(idx), _ptr(lens_t), B, L, 5, 0, _ptr(out), None, None, st) == nat.E_INVALID
    assert "planes = 5 exceeds frame_stack 4" in nat.last_error(c.pipe._ctx)
    # B = 0: AGX_OK without a launch, whatever the buffers
    assert lib.agx_sequence_lengths(h, None, None, 0, L, None, st) == nat.OK
    assert lib.agx_sequence_gather(s, None, None, 0, L, 3, GAMMA, 0, None, None, None, None, None, None, None, st) == nat.OK
    assert lib.agx_sequence_observe(h, 0, None, None, None, 0, L, 1, 0, None, None, None, st) == nat.OK
    e0, i0 = torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV)
    assert tuple(c.seq.lengths(e0, i0, L).shape) == (0,)
    assert tuple(c.seq.gather(e0, i0, L)["payload"].shape) == (0, L, W)
    assert tuple(c.seq.observe(e0, i0, e0, L, planes=2, time_major=True)[0].shape) == (L, 0, 2, 84, 84)
    # a narrowed env range: AGX_E_STATE, but B = 0 stays AGX_OK (it comes in front of the range check)
    c.pipe.env_range(1, 2)
    for call in (lambda: c.seq.lengths(env, idx, L), lambda: c.seq.gather(env, idx, L), lambda: c.seq.observe(env, idx, lens_t, L)):
        with pytest.raises(nat.AgxError, match="env range") as e:
            call()
        assert e.value.code == nat.E_STATE
    assert lib.agx_sequence_observe(h, 0, None, None, None, 0, L, 1, 0, None, None, None, st) == nat.OK
    c.pipe.env_range()
    assert np.array_equal(c.seq.lengths(env, idx, L).cpu().numpy(), lens)
    torch.cuda.synchronize()
    c.hist.close()
    with pytest.raises(RuntimeError, match="closed"):
        c.seq.lengths(env, idx, L)
    c.close()


def test_captured_graph_of_sample_gather_and_observe():
    """sample + gather + observe captured under torch.cuda.graph on a side stream and replayed three times equals the same calls
    issued one by one on a second sampler of the same seed: every replay draws afresh and every output is rewritten in full."""
    from active_gym import ReplaySampler
    c = _case("graph")
    B, L = 96, 6
    smp, ref = ReplaySampler(c.hist, back=0, forward=1, seed=9), ReplaySampler(c.hist, back=0, forward=1, seed=9)
    env = torch.empty((B,), dtype=torch.int32, device=DEV)
    idx = torch.empty((B,), dtype=torch.int64, device=DEV)
    ok = torch.empty((B,), dtype=torch.uint8, device=DEV)
    length = torch.empty((B,), dtype=torch.int32, device=DEV)
    outs = _gather_outs((B, L))
    obs = torch.empty((B, L, 1, 84, 84), device=DEV)
    loc = torch.empty((B, L, 2), dtype=torch.int32, device=DEV)
    live = torch.empty((B, L), dtype=torch.uint8, device=DEV)

    def work():
        smp.sample(B, env, idx, ok)
        _raw_gather(c, env, idx, L, 3, False, outs, length)
        c.seq.observe(env, idx, length, L, planes=1, out=obs, loc_out=loc, live_out=live)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        work()                                   # call 0, eager, on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        work()                                   # captured, not run: the call counter lives on the device
    ref.sample(B)                                # the reference sampler's call 0
    kinds = set()
    for call in (1, 2, 3):
        for t in (obs, loc, live, length, *outs.values()):
            t.fill_(55)                          # nothing of the replay before may pass for this one's
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        renv, ridx, rok = ref.sample(B)
        assert torch.equal(env, renv) and torch.equal(idx, ridx) and torch.equal(ok, rok), call
        want = c.seq.gather(renv, ridx, L, nstep=3, gamma=GAMMA)
        assert torch.equal(length, want["length"])
        for key in GATHER_KEYS:
            a, b = outs[key], want[key]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), (call, key)
        wobs, wloc, wlive = c.seq.observe(renv, ridx, want["length"], L, planes=1)
        assert torch.equal(obs.view(torch.int32), wobs.view(torch.int32)) and torch.equal(loc, wloc) and torch.equal(live, wlive), call
        samples = list(zip(env.cpu().tolist(), idx.cpu().tolist()))
        lens = np.array([qm.length(c.hm, n, k, L) for n, k in samples], np.int32)
        assert np.array_equal(length.cpu().numpy(), lens) and (lens[ok.cpu().numpy() == 1] >= 2).all()          # forward = 1: two steps at least
        kinds |= {qm.kind(c.hm, n, k, L) for n, k in samples}
    assert {"full", "episode", "end"} <= kinds
    c.close()


# ---------------------------------------------------------------------------------------------- the vector env
def _vec_env(native_loop):
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=30, native_loop=native_loop, history_len=16, step_log=True)
    return AtariVecEnv(AtariEnvArgs(**kw), 6, kind="fixed", noop_fn=lambda: 2)


@pytest.mark.parametrize("native", [True, False], ids=["native_loop", "python_loop"])
def test_vec_env_sequence_batch(native):
    """AtariVecEnv(history_len = 16, step_log = True), 40 random steps with autoresets, then sequence_batch(64, length = 8,
    min_length = 2, nstep = 3), uniform and prioritized: every live step holds the observation the step returned for that
    history_index (final_observation for a terminal), the actions of the step taken on seeing it and the bit-exact float32 fold of
    the rewards the steps returned; no sequence holds a reset observation after its first step; over the batch there are full
    sequences, ones an episode's end cuts and ones the end of the history cuts; update_priorities takes mixed_priority.  (The
    run was checked without a GPU: the scripted emulator's done sequence for these actions at scripted_p_over = 30, pushed on
    tests/history_model.py, leaves 66 accepted starts of which 12 are full, 36 cut by their episode and 18 by the history's end;
    the uniform draw of 64 takes 9 / 35 / 20 of them.)"""
    from active_gym import mixed_priority
    N, STEPS, B, L = 6, 40, 64, 8
    env = _vec_env(native)
    assert (env._loop is not None) == native and env.steplog is not None
    obs, info = env.reset()
    rec, resets, produced = {}, set(), {}
    hi = info["history_index"].cpu().numpy()
    obs = obs.clone()
    for i in range(N):
        rec[(i, int(hi[i]))] = obs[i]
        resets.add((i, int(hi[i])))
    rng = np.random.default_rng(0)
    for step in range(STEPS):
        act = {"motor_action": rng.integers(0, 4, N), "sensory_action": rng.uniform(-5, 90, (N, 2)).astype(np.float32)}
        obs, reward, done, _, info = env.step(act)
        obs, hi = obs.clone(), info["history_index"].cpu().numpy()
        for i in range(N):
            rec[(i, int(hi[i]))] = obs[i]
            at = int(hi[i]) - int(done[i])                     # the observation this step produced
            produced[(i, at)] = (int(act["motor_action"][i]), act["sensory_action"][i].copy(), np.float32(reward[i]), bool(done[i]))
        for i in np.nonzero(done)[0]:
            rec[(int(i), int(hi[i]) - 1)] = info["final_observation"][i].clone()
            resets.add((int(i), int(hi[i])))
    count = env.history.last_index().cpu().numpy() + 1
    with pytest.raises(ValueError, match="min_length"):
        env.sequence_batch(B, length=80)
    for prioritized in (False, True):
        out = env.sequence_batch(B, length=L, min_length=2, nstep=3, gamma=GAMMA, prioritized=prioritized)
        keys = ["env", "index", "ok", "length", "live", "obs", "fov_loc", "steps", "next_index", "ret", "discount", "flags", "next_step",
                "motor_action", "sensory_action"] + (["weight", "priority"] if prioritized else [])
        assert sorted(out) == sorted(keys)
        assert tuple(out["obs"].shape) == (B, L, 4, 84, 84) and tuple(out["motor_action"].shape) == (B, L) and out["motor_action"].dtype == torch.int32
        assert tuple(out["sensory_action"].shape) == (B, L, 2) and out["sensory_action"].dtype == torch.float32
        e, k, ok, length, live, steps, nxt, nstp, flags, motor = (out[x].cpu().numpy() for x in (
            "env", "index", "ok", "length", "live", "steps", "next_index", "next_step", "flags", "motor_action"))
        sens = out["sensory_action"].cpu().numpy().view(np.int32)
        ret, disc = out["ret"].cpu().numpy().view(np.int32), out["discount"].cpu().numpy().view(np.int32)
        assert ok.sum() >= 0.9 * B and (length[ok == 1] >= 2).all() and np.array_equal(live, np.arange(L)[None, :] < length[:, None])
        full = by_episode = by_end = 0
        for b in np.nonzero(ok)[0]:
            n, m = int(e[b]), int(length[b])
            for l in range(L):
                at = int(k[b]) + l
                if l >= m:                                     # padding: zeros, nothing else
                    assert not out["obs"][b, l].any() and steps[b, l] == 0 and nxt[b, l] == -1 and nstp[b, l] == -1
                    assert ret[b, l] == 0 and disc[b, l] == 0 and flags[b, l] == 0 and motor[b, l] == 0 and not sens[b, l].any()
                    continue
                assert l == 0 or (n, at) not in resets, f"sequence {b}: step {l} is the reset observation {(n, at)}"
                assert torch.equal(out["obs"][b, l].view(torch.int32), rec[(n, at)].view(torch.int32)), (b, l, n, at)
                rewards, terminal = [], False
                for i in range(1, 4):
                    row = produced.get((n, at + i))
                    if row is None:                            # a reset observation, or the end of the history
                        break
                    rewards.append(row[2])
                    terminal = row[3]
                    if terminal:
                        break
                f = len(rewards)
                assert steps[b, l] == f and nxt[b, l] == (at + f if f else -1), (b, l, n, at)
                assert nstp[b, l] == (l + f if f and l + f < m else -1), (b, l)
                if f == 0:
                    assert ret[b, l] == 0 and disc[b, l] == 0 and motor[b, l] == 0
                    continue
                first = produced[(n, at + 1)]
                assert motor[b, l] == first[0] and np.array_equal(sens[b, l], first[1].view(np.int32)), (b, l, n, at)
                G, d = sm.fold(rewards, GAMMA)
                assert ret[b, l] == sm.bits(G) and disc[b, l] == sm.bits(0.0 if terminal else d), (b, l, n, at)
                assert flags[b, l] == (sm.TERMINATED if terminal else 0)
            full += m == L
            by_episode += m < L and (n, int(k[b]) + m) in resets
            by_end += m < L and int(k[b]) + m == count[n]
        print(f"prioritized = {prioritized}: ok = {int(ok.sum())}, full = {full}, cut by an episode's end = {by_episode}, by the history's = {by_end}")
        assert full >= 1, "no full sequence: lengthen the run"
        assert by_episode >= 1, "no sequence is cut by its episode's end: lengthen the run"
        assert by_end >= 1, "no sequence is cut by the end of the history: lengthen the run"
        if prioritized:
            assert tuple(out["weight"].shape) == (B,) and tuple(out["priority"].shape) == (B,)
            td = torch.rand((B, L), device=DEV)
            pri = mixed_priority(td, out["live"])
            assert tuple(pri.shape) == (B,) and bool((pri[out["ok"].bool()] > 0).all())
            env.update_priorities(out, pri)
            again = env.sequence_batch(B, length=L, min_length=2, nstep=3, gamma=GAMMA, prioritized=True, time_major=True)
            assert tuple(again["obs"].shape) == (L, B, 4, 84, 84) and tuple(again["motor_action"].shape) == (L, B) and again["ok"].any()
    torch.cuda.synchronize()
    env.close()
