"""GPU: the step log (include/agx_steplog.h) through ObsPipeline + FrameHistory + StepLog.  Which rows a gather folds is a pure
function of the history's bookkeeping and of what was recorded, and the fold is float32 with one rounding per operation, so every
case compares steps, next_index, flags and payload with tests/steplog_model.py EXACTLY and ret / discount as int32 bit patterns;
rows with steps == 0 must keep the sentinel written before the call."""
import ctypes

import numpy as np
import pytest
import torch

import replay_model as rm
import steplog_model as sm
from history_model import HistoryModel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = ctypes.c_void_p
GAMMA = 0.99
NSTEPS = (1, 3, 64)
F_SENT, B_SENT = -7.5, 0xAB               # sentinels: exact in float32 and no fold's result here; no flag byte; the payload's fill
T, FS = 8, 4


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pipe(N):
    from active_gym import ObsPipeline
    return ObsPipeline(num_envs=N, kind="fixed", obs_size=(84, 84), frame_stack=FS, device=DEV, fov_size=(30, 30), fov_init_loc=(2, 3),
                       sensory_action_mode="absolute", resize_to_full=True, mask_out=False)


class Outs:
    """The six outputs of agx_steplog_gather, filled with sentinels; call() runs the C entry point on them."""

    def __init__(self, B, W):
        self.B, self.W = B, W
        self.ret = torch.empty(B, dtype=torch.float32, device=DEV)
        self.discount = torch.empty(B, dtype=torch.float32, device=DEV)
        self.steps = torch.empty(B, dtype=torch.int32, device=DEV)
        self.next_index = torch.empty(B, dtype=torch.int64, device=DEV)
        self.flags = torch.empty(B, dtype=torch.uint8, device=DEV)
        self.payload = torch.empty((B, W), dtype=torch.uint8, device=DEV)
        self.fill()

    def fill(self):
        self.ret.fill_(F_SENT)
        self.discount.fill_(F_SENT)
        self.steps.fill_(-9)
        self.next_index.fill_(-9)
        self.flags.fill_(B_SENT)
        self.payload.fill_(B_SENT)

    def call(self, log, env, index, nstep, gamma=GAMMA):
        from active_gym import _native as nat
        rc = log._lib.agx_steplog_gather(log._s, P(env.data_ptr()), P(index.data_ptr()), self.B, nstep, gamma, P(self.ret.data_ptr()),
                                         P(self.discount.data_ptr()), P(self.steps.data_ptr()), P(self.next_index.data_ptr()),
                                         P(self.flags.data_ptr()), P(self.payload.data_ptr()) if self.W else None, log.pipe._stream())
        nat.check(rc, log.pipe._ctx)

    def host(self):
        return dict(ret=self.ret.cpu().numpy().view(np.int32), discount=self.discount.cpu().numpy().view(np.int32), steps=self.steps.cpu().numpy(),
                    next_index=self.next_index.cpu().numpy(), flags=self.flags.cpu().numpy(), payload=self.payload.cpu().numpy())


def _expected(model, samples, nstep, W, gamma=GAMMA):
    """The model's outputs for a list of samples, sentinels where steps == 0."""
    B = len(samples)
    want = dict(ret=np.full(B, F_SENT, np.float32), discount=np.full(B, F_SENT, np.float32), steps=np.zeros(B, np.int32),
                next_index=np.full(B, -1, np.int64), flags=np.full(B, B_SENT, np.uint8), payload=np.full((B, W), B_SENT, np.uint8))
    for b, (n, k) in enumerate(samples):
        m, nxt, G, disc, last, pay = model.gather(n, k, nstep, gamma)
        if m:
            want["steps"][b], want["next_index"][b], want["ret"][b], want["discount"][b], want["flags"][b] = m, nxt, G, disc, last
            want["payload"][b] = pay
    want["ret"], want["discount"] = want["ret"].view(np.int32), want["discount"].view(np.int32)
    return want


def _same(got, want, what):
    for key in ("steps", "next_index", "flags", "payload", "ret", "discount"):
        assert np.array_equal(got[key], want[key]), f"{key} differs from the model ({what})"


def _all_samples(hm):
    return [(n, k) for n in range(hm.N) for k in range(-1, int(hm.count[n]) + 1)]


def _drive(pipe, hist, log, hm, lm, cmds, seed, after=None, p_unrecorded=0.2):
    """ingest / fovea / push over the command bytes, a record after each push: random float32 rewards, random flags, W random
    bytes, and a known subset of the pushed rows (about p_unrecorded of them) left unrecorded."""
    N, W = pipe.num_envs, log.payload_bytes
    rng = np.random.default_rng(seed + 1000)
    for step, cmd in enumerate(cmds):
        pipe.ingest_gray(_t(rng.integers(0, 256, (N, 2, 84, 84), dtype=np.uint8)), _t(cmd))
        pipe.fovea(_t(rng.uniform(-9, 89, (N, 2)).astype(np.float32)))
        idx = hist.push(_t(cmd)).cpu().numpy()
        assert np.array_equal(idx, hm.push(cmd)), "indices differ from the model"
        idx[rng.random(N) < p_unrecorded] = -1
        reward = (rng.standard_normal(N) * 3).astype(np.float32)
        flags = ((rng.random(N) < 0.15) * sm.TERMINATED + (rng.random(N) < 0.05) * sm.TRUNCATED).astype(np.uint8)
        payload = rng.integers(0, 256, (N, W), dtype=np.uint8)
        log.record(_t(idx), _t(reward), _t(flags), _t(payload) if W else None)
        lm.record(idx, reward, flags, payload)
        if after is not None:
            after(step)


def _setup(N, W=12, steps=13, seed=3, **kw):
    from active_gym import FrameHistory, StepLog
    pipe = _pipe(N)
    hist = FrameHistory(pipe, T)
    nbytes = hist.nbytes
    log = StepLog(hist, W)
    assert hist.nbytes == nbytes and log.bytes() >= T * N * (13 + W)          # the log's storage is its own
    hm = HistoryModel(N, FS, T)
    lm = sm.StepLogModel(hm, W)
    if steps:
        _drive(pipe, hist, log, hm, lm, rm.commands(seed, N, steps), seed, **kw)
    return pipe, hist, log, hm, lm


@pytest.mark.parametrize("N", [1, 5, 257])
def test_pipeline(N):
    """84 / 30, fs = 4, T = 8, 20 steps with random CLEAR / SKIP, W = 12: after every step the gather over ALL (n, k), k in [-1, cnt],
    equals the model for nstep 1, 3 and 64.  N = 257 crosses the record kernel's block boundary."""
    pipe, hist, log, hm, lm = _setup(N, steps=0)
    seen = set()

    def check(step):
        samples = _all_samples(hm)
        env, idx = _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))
        outs = Outs(len(samples), 12)
        for nstep in NSTEPS:
            outs.fill()
            outs.call(log, env, idx, nstep)
            want = _expected(lm, samples, nstep, 12)
            _same(outs.host(), want, f"N = {N}, step {step}, nstep = {nstep}")
            seen.update(want["steps"].tolist())
        if step == 19:                           # the Python surface returns the same rows, zeros where steps == 0
            got = log.gather(env, idx, nstep=3, gamma=GAMMA)
            want = _expected(lm, samples, 3, 12)
            none = want["steps"] == 0
            for key in ("ret", "discount"):
                want[key] = np.where(none, 0, want[key])
            want["flags"] = np.where(none, 0, want["flags"]).astype(np.uint8)
            want["payload"] = np.where(none[:, None], 0, want["payload"]).astype(np.uint8)
            host = {key: v.cpu().numpy() for key, v in got.items()}
            host["ret"], host["discount"] = host["ret"].view(np.int32), host["discount"].view(np.int32)
            _same(host, want, "StepLog.gather")

    _drive(pipe, hist, log, hm, lm, rm.commands(3, N, 20), 3, after=check)
    assert (lm.stamp >= 0).any() and (N == 1 or {0, 1, 2, 3} <= seen) and max(seen) >= 3
    pipe.close()


def test_batch_is_not_bound_by_the_grid():
    """B = 70,000 repeated samples at N = 5: more than gridDim.y holds, and more than one block's worth of every sample."""
    pipe, hist, log, hm, lm = _setup(5)
    samples = _all_samples(hm)
    want = _expected(lm, samples, 3, 12)
    B = 70_000
    rep = np.arange(B) % len(samples)
    env, idx = _t(np.array([s[0] for s in samples], np.int32)[rep]), _t(np.array([s[1] for s in samples], np.int64)[rep])
    outs = Outs(B, 12)
    outs.call(log, env, idx, 3)
    _same(outs.host(), {key: v[rep] for key, v in want.items()}, "B = 70000")
    assert (want["steps"] > 0).sum() >= 10
    pipe.close()


def test_no_payload_and_null_outputs():
    """W = 0: d_payload is ignored; every output but d_steps may be NULL; B = 0 launches nothing."""
    from active_gym import _native as nat
    pipe, hist, log, hm, lm = _setup(5, W=0)
    samples = _all_samples(hm)
    env, idx = _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))
    B = len(samples)
    want = _expected(lm, samples, 3, 0)
    outs = Outs(B, 0)
    outs.call(log, env, idx, 3)
    _same(outs.host(), want, "W = 0")
    steps = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    lib, s, st = log._lib, log._s, pipe._stream()
    assert lib.agx_steplog_gather(s, P(env.data_ptr()), P(idx.data_ptr()), B, 3, GAMMA, None, None, P(steps.data_ptr()), None, None, None, st) == nat.OK
    assert np.array_equal(steps.cpu().numpy(), want["steps"])
    assert lib.agx_steplog_gather(s, P(env.data_ptr()), P(idx.data_ptr()), B, 3, GAMMA, None, None, None, None, None, None, st) == nat.E_INVALID
    assert "d_steps" in nat.last_error(pipe._ctx)
    assert lib.agx_steplog_gather(s, None, P(idx.data_ptr()), B, 3, GAMMA, None, None, P(steps.data_ptr()), None, None, None, st) == nat.E_INVALID
    assert lib.agx_steplog_gather(s, None, None, 0, 3, GAMMA, None, None, None, None, None, None, st) == nat.OK
    assert lib.agx_steplog_gather(s, P(env.data_ptr()), P(idx.data_ptr()), B, 65, GAMMA, None, None, P(steps.data_ptr()), None, None, None, st) == nat.E_INVALID
    assert lib.agx_steplog_record(s, None, None, None, None, st) == nat.E_INVALID and "d_index" in nat.last_error(pipe._ctx)
    got = log.gather(env, idx, nstep=3)
    assert tuple(got["payload"].shape) == (B, 0) and np.array_equal(got["steps"].cpu().numpy(), want["steps"])
    # a log with a payload refuses a record without one
    from active_gym import StepLog
    log4 = StepLog(hist, 4)
    z64, zf, z8 = torch.zeros(5, dtype=torch.int64, device=DEV), torch.zeros(5, device=DEV), torch.zeros(5, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="payload"):
        log4.record(z64, zf, z8)
    assert log4._lib.agx_steplog_record(log4._s, P(z64.data_ptr()), P(zf.data_ptr()), P(z8.data_ptr()), None, st) == nat.E_INVALID
    assert "d_payload" in nat.last_error(pipe._ctx)
    torch.cuda.synchronize()
    pipe.close()


def test_clear():
    """history.clear() clears the logs on it: every sample has steps == 0 until rows are recorded again (the indices restart at 0,
    and the stamps of the rows before the clear do not pass for the new ones)."""
    pipe, hist, log, hm, lm = _setup(5)
    assert (_expected(lm, _all_samples(hm), 3, 12)["steps"] > 0).any()
    hist.clear()                                 # ... and log.clear() with it
    hm.clear()
    lm.clear()

    def gathered():
        samples = [(n, k) for n in range(5) for k in range(-1, T + 6)]
        env, idx = _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))
        outs = Outs(len(samples), 12)
        outs.call(log, env, idx, 3)
        return outs.host(), _expected(lm, samples, 3, 12)

    # push without recording: the old rows' stamps (indices 0 .. 12 of before) would match the new indices had clear not reset them
    cmds = rm.commands(11, 5, 6, p_skip=0.0)
    rng = np.random.default_rng(5)
    for cmd in cmds:
        pipe.ingest_gray(_t(rng.integers(0, 256, (5, 2, 84, 84), dtype=np.uint8)), _t(cmd))
        pipe.fovea(_t(np.zeros((5, 2), np.float32)))
        assert np.array_equal(hist.push(_t(cmd)).cpu().numpy(), hm.push(cmd))
    got, want = gathered()
    assert not want["steps"].any()
    _same(got, want, "after clear")
    _drive(pipe, hist, log, hm, lm, rm.commands(12, 5, 6), 12, p_unrecorded=0.0)
    got, want = gathered()
    assert (want["steps"] > 0).sum() >= 5
    _same(got, want, "re-recorded after clear")
    pipe.close()


def test_env_range_is_refused():
    from active_gym import StepLog
    from active_gym import _native as nat
    pipe, hist, log, hm, lm = _setup(5, steps=2)
    z32, z64 = torch.zeros(5, dtype=torch.int32, device=DEV), torch.zeros(5, dtype=torch.int64, device=DEV)
    zf, z8, zp = torch.zeros(5, device=DEV), torch.zeros(5, dtype=torch.uint8, device=DEV), torch.zeros((5, 12), dtype=torch.uint8, device=DEV)
    pipe.env_range(1, 2)
    for call in (lambda: StepLog(hist, 4), lambda: log.record(z64, zf, z8, zp), lambda: log.gather(z32, z64)):
        with pytest.raises(nat.AgxError, match="env range") as e:
            call()
        assert e.value.code == nat.E_STATE
    pipe.env_range()
    log.record(z64, zf, z8, zp)
    hist.close()
    with pytest.raises(RuntimeError, match="closed"):
        log.gather(z32, z64)
    pipe.close()


def test_captured_graph_of_sample_and_gather():
    """sample + gather captured under torch.cuda.graph on a side stream and replayed three times equals the same calls issued one
    by one (a second sampler of the same seed): the sampler draws afresh per replay, the model follows the call counter."""
    from active_gym import ReplaySampler
    pipe, hist, log, hm, lm = _setup(5, p_unrecorded=0.1)
    B = 300
    smp, ref = ReplaySampler(hist, back=0, forward=1, seed=9), ReplaySampler(hist, back=0, forward=1, seed=9)
    env = torch.empty((B,), dtype=torch.int32, device=DEV)
    idx = torch.empty((B,), dtype=torch.int64, device=DEV)
    ok = torch.empty((B,), dtype=torch.uint8, device=DEV)
    outs, routs = Outs(B, 12), Outs(B, 12)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        smp.sample(B, env, idx, ok)              # call 0, eager, on the side stream
        outs.call(log, env, idx, 3)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        smp.sample(B, env, idx, ok)              # captured, not run: the counter lives on the device
        outs.call(log, env, idx, 3)
    ref.sample(B)                                # the reference sampler's call 0
    some = 0
    for call in (1, 2, 3):
        outs.fill()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        renv, ridx, rok = ref.sample(B)
        routs.fill()
        routs.call(log, renv, ridx, 3)
        we, wi, wo, _ = rm.draw(hm, 0, 1, 16, 9, call, B)
        assert np.array_equal(env.cpu().numpy(), we) and np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(ok.cpu().numpy(), wo), call
        assert torch.equal(env, renv) and torch.equal(idx, ridx) and torch.equal(ok, rok)
        got = outs.host()
        _same(got, routs.host(), f"replay {call} against the calls issued one by one")
        _same(got, _expected(lm, list(zip(we.tolist(), wi.tolist())), 3, 12), f"replay {call}")
        some += int((got["steps"] > 0).sum())
    assert some >= B
    pipe.close()


def test_batch_reads_both_observations():
    """StepLog.batch: ok = the sampler's ok AND steps > 0, obs / next_obs are history.observe at index / next_index (and the
    glimpse memory's with glimpses = 3), the rows equal the model's."""
    from active_gym import GlimpseMemory, ReplaySampler
    pipe, hist, log, hm, lm = _setup(5, p_unrecorded=0.3)
    with pytest.raises(ValueError, match="back >= 2"):
        log.batch(ReplaySampler(hist, back=0, forward=1), 8, glimpses=3)
    with pytest.raises(ValueError, match="memory must be"):
        log.batch(ReplaySampler(hist, back=2, forward=1), 8, glimpses=3, memory=GlimpseMemory(hist, 2))
    for glimpses in (None, 3):
        smp = ReplaySampler(hist, back=2, forward=1, seed=4)
        out = log.batch(smp, 512, nstep=3, gamma=GAMMA, glimpses=glimpses)
        assert sorted(out) == sorted(["env", "index", "next_index", "ok", "obs", "next_obs", "ret", "discount", "steps", "flags", "payload",
                                      "fov_loc", "next_fov_loc"])
        we, wi, wo, _ = rm.draw(hm, 2, 1, 16, 4, 0, 512)
        assert np.array_equal(out["env"].cpu().numpy(), we) and np.array_equal(out["index"].cpu().numpy(), wi)
        want = _expected(lm, list(zip(we.tolist(), wi.tolist())), 3, 12)
        assert np.array_equal(out["steps"].cpu().numpy(), want["steps"]) and np.array_equal(out["next_index"].cpu().numpy(), want["next_index"])
        okw = (wo == 1) & (want["steps"] > 0)
        assert np.array_equal(out["ok"].cpu().numpy(), okw.astype(np.uint8)) and okw.any() and (okw != (wo == 1)).any()
        read = hist.observe if glimpses is None else GlimpseMemory(hist, 3).observe
        rows = torch.from_numpy(np.nonzero(okw)[0]).to(DEV)
        for key, at in (("obs", out["index"]), ("next_obs", out["next_index"])):
            ref, _, _ = read(out["env"], at)
            assert torch.equal(out[key][rows].view(torch.int32), ref[rows].view(torch.int32)), (glimpses, key)
        assert np.array_equal(out["ret"].cpu().numpy().view(np.int32)[okw], want["ret"][okw])
        smp.close()
    pipe.close()


# ---------------------------------------------------------------------------------------------- the vector env
def _vec_env(native_loop, history_len, **extra):
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=150, native_loop=native_loop, history_len=history_len, **extra)
    return AtariVecEnv(AtariEnvArgs(**kw), 6, kind="fixed", noop_fn=lambda: 2)


@pytest.mark.parametrize("native", [True, False], ids=["native_loop", "python_loop"])
def test_vec_env_replay_batch(native):
    """AtariVecEnv(history_len = 16, step_log = True), 40 random steps with autoresets, then replay_batch(2048, nstep = 3): per ok row
    the actions are those of the step that produced index + 1, ret / discount are bit-equal to the float32 fold of the rewards
    the steps returned, next_obs is bit for bit the observation recorded for next_index (final_observation for a terminal) and no
    next_index is a reset observation; over the batch there are full 3-step rows, rows a terminal cuts short (discount 0) and
    rows the end of the history cuts short.  (The run's seed was checked without a GPU: the scripted emulator's done sequence for
    these actions, pushed and recorded on tests/history_model.py + tests/steplog_model.py and drawn with tests/replay_model.py, gives
    2048 ok rows of which 576 fold three steps, 1326 end at a terminal and 146 at the end of the history.)"""
    N, STEPS = 6, 40
    env = _vec_env(native, 16, step_log=True)
    assert (env._loop is not None) == native and env.steplog is not None and env.steplog.payload_bytes == 12
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
    assert not set(produced) & resets
    B = 2048
    out = env.replay_batch(B, nstep=3, gamma=GAMMA)
    assert sorted(out) == sorted(["env", "index", "next_index", "ok", "obs", "next_obs", "ret", "discount", "steps", "flags", "fov_loc", "next_fov_loc",
                                  "motor_action", "sensory_action"])
    assert out["motor_action"].dtype == torch.int32 and out["sensory_action"].dtype == torch.float32 and tuple(out["sensory_action"].shape) == (B, 2)
    e, k, k1, ok, steps, flags, motor = (out[x].cpu().numpy() for x in ("env", "index", "next_index", "ok", "steps", "flags", "motor_action"))
    sens = out["sensory_action"].cpu().numpy().view(np.int32)
    ret, disc = out["ret"].cpu().numpy().view(np.int32), out["discount"].cpu().numpy().view(np.int32)
    print(f"ok = {int(ok.sum())} of {B}; steps histogram = {np.bincount(steps[ok == 1], minlength=4).tolist()}")
    assert ok.sum() >= 0.99 * B
    full = by_terminal = by_end = 0
    for b in np.nonzero(ok)[0]:
        n, at = int(e[b]), int(k[b])
        rewards, terminal = [], False
        for i in range(1, 4):
            row = produced.get((n, at + i))
            if row is None:                                    # a reset observation, or the end of the history
                break
            rewards.append(row[2])
            terminal = row[3]
            if terminal:
                break
        m = len(rewards)
        assert m >= 1 and steps[b] == m and k1[b] == at + m, (b, n, at, steps[b], m)
        first = produced[(n, at + 1)]
        assert motor[b] == first[0] and np.array_equal(sens[b], first[1].view(np.int32)), (b, n, at)
        G, d = sm.fold(rewards, GAMMA)
        assert ret[b] == sm.bits(G) and disc[b] == sm.bits(0.0 if terminal else d), (b, n, at)
        assert flags[b] == (sm.TERMINATED if terminal else 0)
        nxt = (n, at + m)
        assert nxt not in resets, f"row {b}: next_index is the reset observation {nxt}"
        assert torch.equal(out["obs"][b].view(torch.int32), rec[(n, at)].view(torch.int32)), (n, at)
        assert torch.equal(out["next_obs"][b].view(torch.int32), rec[nxt].view(torch.int32)), nxt
        full += m == 3
        by_terminal += m < 3 and terminal and disc[b] == 0
        by_end += m < 3 and not terminal and (n, at + m + 1) not in resets
    assert full >= 1, "no row with steps == 3: lengthen the run"
    assert by_terminal >= 1, "no row is cut short by a terminal: lengthen the run"
    assert by_end >= 1, "no row is cut short by the end of the history: lengthen the run"
    with pytest.raises(ValueError, match="nstep"):
        env.replay_batch(8, nstep=0)
    # glimpses = P reads through the env's own glimpse memory (the one glimpse_memory(P) uses), not a second one
    gb = env.replay_batch(64, nstep=3, gamma=GAMMA, glimpses=3)
    mem, used = env.history._memories[3], []
    mem.observe = lambda *a, _observe=mem.observe, **kw: used.append(mem) or _observe(*a, **kw)       # spy: who serves glimpse_memory(3)
    env.glimpse_memory(3)
    del mem.observe
    assert list(env.history._memories) == [3] and used == [mem] and env.replay_sampler(back=2).back == 2
    rows = gb["ok"].bool()
    assert rows.any() and tuple(gb["fov_loc"].shape) == (64, 3, 2)
    ref, _, _ = env.history.memory(3).observe(gb["env"], gb["next_index"])
    assert torch.equal(gb["next_obs"][rows].view(torch.int32), ref[rows].view(torch.int32))
    env.close()


def test_vec_env_without_step_log_records_nothing():
    env = _vec_env(True, 16)
    assert env.steplog is None and env.step_log is False
    with pytest.raises(ValueError, match="step_log"):
        env.replay_batch(8)
    env.close()
