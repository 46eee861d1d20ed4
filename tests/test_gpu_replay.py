"""GPU: the replay sampler (include/agx_replay.h) through ObsPipeline + FrameHistory + ReplaySampler.  The draw is a pure integer
function of (seed, call number) and the history's bookkeeping, so every case compares env, index, ok and total with
tests/replay_model.py EXACTLY; the read-path cases also keep a clone of what each step returned (as tests/test_gpu_history.py
does) and compare the re-created observations of the drawn samples bit for bit."""
import numpy as np
import pytest
import torch

import replay_model as rm
from history_model import HistoryModel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -3.0                 # exact in float32; no observation value is negative
CONFIGS = [(0, 0), (0, 1), (2, 1), (0, 3)]          # (back, forward)
MAIN_SEED = 3


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pipe(N, kind="fixed", obs=(84, 84), fov=(30, 30), fs=4, mode="resize"):
    from active_gym import ObsPipeline
    kw = dict(num_envs=N, kind=kind, obs_size=obs, frame_stack=fs, device=DEV)
    if kind != "base":
        kw.update(fov_size=fov, fov_init_loc=(2, 3), sensory_action_mode="absolute", resize_to_full=mode == "resize", mask_out=mode == "mask")
    return ObsPipeline(**kw)


def _steps(pipe, hist, model, cmds, seed, rec=None, after=None):
    """Drive ingest + observation + push over the command bytes; rec[(n, index)] = (obs row, fov_loc row) clones of what the step
    returned; after(step) runs behind every push."""
    N = pipe.num_envs
    oh, ow = pipe.obs_size
    rng = np.random.default_rng(seed + 1000)
    for step, cmd in enumerate(cmds):
        pipe.ingest_gray(_t(rng.integers(0, 256, (N, 2, oh, ow), dtype=np.uint8)), _t(cmd))
        if pipe.kind == "base":
            obs, loc = pipe.observe_full(), None
        else:
            obs, loc = pipe.fovea(_t(rng.uniform(-9, max(oh, ow) + 5, (N, 2)).astype(np.float32)))
        idx = hist.push(_t(cmd)).cpu().numpy()
        assert np.array_equal(idx, model.push(cmd)), "indices differ from the model"
        if rec is not None:
            obs, loc = obs.clone(), loc.clone()
            for n in range(N):
                if idx[n] >= 0:
                    rec[(n, int(idx[n]))] = (obs[n], loc[n])
        if after is not None:
            after(step)


def _equals_model(smp, model, seed, call, B):
    """One sample(B) == the model's call `call`; returns the model's (env, index, ok)."""
    env, idx, ok = smp.sample(B)
    we, wi, wo, wt = rm.draw(model, smp.back, smp.forward, smp.attempts, seed, call, B)
    assert int(smp.total()) == wt, f"total differs from the model (call {call})"
    assert np.array_equal(ok.cpu().numpy(), wo), f"ok differs from the model (call {call})"
    assert np.array_equal(env.cpu().numpy(), we), f"env differs from the model (call {call})"
    assert np.array_equal(idx.cpu().numpy(), wi), f"index differs from the model (call {call})"
    return we, wi, wo


def test_main_case():
    """N = 5, T = 8, fs = 4, 84 / 30, commands(3, 5, 13) incl. CLEAR / SKIP: before any push and after every step, each of the four
    configs draws exactly the model's samples; an empty history gives total = 0 and no ok."""
    from active_gym import FrameHistory, ReplaySampler
    pipe = _pipe(5)
    hist = FrameHistory(pipe, 8)
    nbytes = hist.nbytes
    model = HistoryModel(5, 4, 8)
    smps = [ReplaySampler(hist, back=b, forward=f, attempts=16, seed=7) for b, f in CONFIGS]
    assert hist.nbytes == nbytes                     # the sampler's scratch is its own
    calls = [0] * len(smps)
    cmds = rm.commands(MAIN_SEED, 5, 13)

    def check(B):
        out = []
        for i, smp in enumerate(smps):
            out.append(_equals_model(smp, model, 7, calls[i], B))
            calls[i] += 1
        return out

    for _, _, ok in check(512):
        assert not ok.any()
    assert all(int(s.total()) == 0 for s in smps)
    _steps(pipe, hist, model, cmds, MAIN_SEED, after=lambda step: check(512))
    last = check(4096)
    assert all(ok.sum() >= 0.99 * 4096 for _, _, ok in last) and not last[3][2].all()      # (0, 3) has failed samples: the -1 path
    for (back, forward), (env, idx, ok) in zip(CONFIGS, last):
        assert {(int(n), int(k)) for n, k, o in zip(env, idx, ok) if o} == set(rm.accepted_set(model, back, forward))
    pipe.close()


@pytest.mark.parametrize("N", [1, 257, 700])
def test_scan_across_chunks_and_waves(N):
    """kind base, 12 x 12, fs = 2, T = 4, 6 steps with p_skip = 0.3 (counts differ between envs): the offsets of N = 700 cross
    two chunk carries and every wave boundary, N = 257 leaves a last chunk of one env, N = 1 is one lane."""
    from active_gym import FrameHistory, ReplaySampler
    pipe = _pipe(N, kind="base", obs=(12, 12), fs=2)
    hist = FrameHistory(pipe, 4)
    model = HistoryModel(N, 2, 4)
    _steps(pipe, hist, model, rm.commands(21, N, 6, p_skip=0.3), 21)
    assert N == 1 or len(set(model.count.tolist())) > 1
    smp = ReplaySampler(hist, back=0, forward=1, seed=11)
    env, _, ok = _equals_model(smp, model, 11, 0, 2048)
    assert ok.sum() >= 0.9 * 2048 and (N == 1 or len(set(env[ok == 1].tolist())) > min(N, 2048) // 3)
    pipe.close()


@pytest.mark.parametrize("mode", ["resize", "mask"])
def test_consistency_with_the_read_path(mode):
    """back = 2, forward = 1: every ok sample is valid under history.observe at index and index + 1, both observations are bit
    for bit what the steps returned, GlimpseMemory(hist, 3) is full at both, and a row with ok = 0 keeps its sentinel."""
    from active_gym import FrameHistory, GlimpseMemory, ReplaySampler
    pipe = _pipe(5, mode=mode)
    hist = FrameHistory(pipe, 8)
    model, rec = HistoryModel(5, 4, 8), {}
    _steps(pipe, hist, model, rm.commands(MAIN_SEED, 5, 13), MAIN_SEED, rec=rec)
    B = 512
    # attempts = 1 gives up after one rejected candidate: rows with ok = 0 among the accepted ones
    for attempts, some_fail in ((16, False), (1, True)):
        smp = ReplaySampler(hist, back=2, forward=1, attempts=attempts, seed=5)
        we, wi, wo = _equals_model(smp, model, 5, 0, B)
        assert (wo == 0).any() == some_fail and wo.sum() >= B // 4
        env, idx = _t(we), _t(wi)
        mem = GlimpseMemory(hist, 3)
        age, ahead = smp.inspect(env, idx)
        age, ahead = age.cpu().numpy(), ahead.cpu().numpy()
        for step in (0, 1):
            at = torch.where(idx >= 0, idx + step, idx)
            out = torch.full((B,) + hist.obs_row_shape(), SENTINEL, dtype=torch.float32, device=DEV)
            loc = torch.full((B, 2), -77, dtype=torch.int32, device=DEV)
            obs, loc, valid = hist.observe(env, at, out=out, loc_out=loc)
            assert np.array_equal(valid.cpu().numpy(), wo)
            _, _, taken = mem.observe(env, at)
            taken = taken.cpu().numpy()
            for b in range(B):
                if wo[b]:
                    o, l = rec[(int(we[b]), int(wi[b]) + step)]
                    assert torch.equal(obs[b].view(torch.int32), o.view(torch.int32)), (b, step)
                    assert torch.equal(loc[b], l)
                    assert taken[b] == min(3, rm.age(model, int(we[b]), int(wi[b]) + step) + 1)
                    assert age[b] == rm.age(model, int(we[b]), int(wi[b])) and ahead[b] >= 1
                else:
                    assert bool((obs[b] == SENTINEL).all()) and loc[b].tolist() == [-77, -77] and taken[b] == 0
                    assert (age[b], ahead[b]) == (-1, -1)
        smp.close()
    pipe.close()


def test_inspect():
    """Every (n, k) ever issued plus, per env, an index below 0 and a never-issued one; and envs that are none."""
    from active_gym import FrameHistory
    from active_gym import replay as rp
    pipe = _pipe(5)
    hist = FrameHistory(pipe, 8)
    model = HistoryModel(5, 4, 8)
    _steps(pipe, hist, model, rm.commands(MAIN_SEED, 5, 13), MAIN_SEED)
    samples = [(n, k) for n in range(5) for k in range(-1, int(model.count[n]) + 1)] + [(-1, 0), (5, 0)]
    want = [rm.inspect(model, n, k) for n, k in samples]
    assert sum(a >= 0 for a, _ in want) >= 10 and len({f for _, f in want}) >= 4
    age, ahead = rp.inspect(hist, _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64)))
    assert list(zip(age.tolist(), ahead.tolist())) == want
    pipe.close()


def test_counter_seed_and_graph_replay():
    """Two consecutive calls are the model's calls 0 and 1; seed(s) restarts the sequence; B = 0 does not advance it; one sample
    captured under torch.cuda.graph on a side stream draws the model's next three calls in three replays."""
    from active_gym import FrameHistory, ReplaySampler
    pipe = _pipe(5)
    hist = FrameHistory(pipe, 8)
    model = HistoryModel(5, 4, 8)
    _steps(pipe, hist, model, rm.commands(MAIN_SEED, 5, 13), MAIN_SEED)
    B = 300
    smp = ReplaySampler(hist, back=0, forward=1)
    a = _equals_model(smp, model, 0, 0, B)                    # a new sampler has seed 0
    b = _equals_model(smp, model, 0, 1, B)
    assert not np.array_equal(a[1], b[1])
    smp.seed((1 << 63) + 12345)
    smp.sample(0)
    _equals_model(smp, model, (1 << 63) + 12345, 0, B)
    smp.seed(9)
    env = torch.empty((B,), dtype=torch.int32, device=DEV)
    idx = torch.empty((B,), dtype=torch.int64, device=DEV)
    ok = torch.empty((B,), dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        smp.sample(B, env, idx, ok)                          # call 0, eager, on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        smp.sample(B, env, idx, ok)                          # captured, not run: the counter lives on the device
    for call in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        we, wi, wo, wt = rm.draw(model, 0, 1, 16, 9, call, B)
        assert np.array_equal(env.cpu().numpy(), we) and np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(ok.cpu().numpy(), wo), call
        assert int(smp.total()) == wt
    _equals_model(smp, model, 9, 4, B)                       # usable one call at a time after the replays
    pipe.close()


def test_refusals():
    import ctypes
    from active_gym import FrameHistory, ReplaySampler
    from active_gym import _native as nat
    from active_gym import replay as rp
    pipe = _pipe(4)
    hist = FrameHistory(pipe, 8)
    pipe.env_range(1, 2)
    with pytest.raises(nat.AgxError, match="env range") as e:
        ReplaySampler(hist)
    assert e.value.code == nat.E_STATE
    pipe.env_range()
    smp = ReplaySampler(hist)
    z32, z64 = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    pipe.env_range(1, 2)
    for call in (lambda: smp.sample(4), lambda: smp.inspect(z32, z64), lambda: smp.seed(1)):
        with pytest.raises(nat.AgxError, match="env range") as e:
            call()
        assert e.value.code == nat.E_STATE
    pipe.env_range()
    lib, P = rp.lib(), ctypes.c_void_p
    assert lib.agx_replay_sample(smp._r, -1, P(z32.data_ptr()), P(z64.data_ptr()), None, None, pipe._stream()) == nat.E_INVALID
    assert lib.agx_replay_sample(smp._r, 4, None, P(z64.data_ptr()), None, None, pipe._stream()) == nat.E_INVALID
    assert lib.agx_replay_sample(smp._r, 4, P(z32.data_ptr()), None, None, None, pipe._stream()) == nat.E_INVALID
    assert lib.agx_replay_inspect(hist.handle, None, P(z64.data_ptr()), 4, None, None, pipe._stream()) == nat.E_INVALID
    assert lib.agx_replay_inspect(hist.handle, P(z32.data_ptr()), P(z64.data_ptr()), -1, None, None, pipe._stream()) == nat.E_INVALID
    # d_ok and d_total may be NULL; B = 0 launches nothing
    assert lib.agx_replay_sample(smp._r, 4, P(z32.data_ptr()), P(z64.data_ptr()), None, None, pipe._stream()) == nat.OK
    assert lib.agx_replay_sample(smp._r, 0, None, None, None, None, pipe._stream()) == nat.OK
    torch.cuda.synchronize()
    assert z32.tolist() == [-1] * 4 and z64.tolist() == [-1] * 4          # an empty history: nothing to draw
    with pytest.raises(ValueError):
        smp.sample(-1)
    with pytest.raises(ValueError, match="forward >= 1"):
        ReplaySampler(hist, forward=0).transitions(4)
    with pytest.raises(ValueError, match="back >= 2"):
        smp.transitions(4, glimpses=3)
    hist.close()
    with pytest.raises(RuntimeError, match="closed"):
        smp.sample(4)
    pipe.close()


def _vec_env(native_loop, history_len):
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=150, native_loop=native_loop, history_len=history_len)
    return AtariVecEnv(AtariEnvArgs(**kw), 6, kind="fixed", noop_fn=lambda: 2)


@pytest.mark.parametrize("native", [True, False], ids=["native_loop", "python_loop"])
def test_vec_env_transitions(native):
    """AtariVecEnv(history_len = 16), 40 random steps with autoresets: every ok row of replay_sampler(forward=1).transitions(2048)
    has as next_obs, bit for bit, the observation recorded for (env, index + 1) - info["final_observation"] for a terminal step -
    no row's next_obs is a reset observation, and at least one row ends in a terminal observation."""
    N, STEPS = 6, 40
    env = _vec_env(native, 16)
    assert (env._loop is not None) == native
    obs, info = env.reset()
    rec, resets, terminals = {}, set(), set()
    hi = info["history_index"].cpu().numpy()
    obs = obs.clone()
    for i in range(N):
        rec[(i, int(hi[i]))] = obs[i]
        resets.add((i, int(hi[i])))
    rng = np.random.default_rng(0)
    for step in range(STEPS):
        act = {"motor_action": rng.integers(0, 4, N), "sensory_action": rng.uniform(-5, 90, (N, 2)).astype(np.float32)}
        obs, _, done, _, info = env.step(act)
        obs, hi = obs.clone(), info["history_index"].cpu().numpy()
        for i in range(N):
            rec[(i, int(hi[i]))] = obs[i]
        for i in np.nonzero(done)[0]:
            rec[(int(i), int(hi[i]) - 1)] = info["final_observation"][i].clone()
            terminals.add((int(i), int(hi[i]) - 1))
            resets.add((int(i), int(hi[i])))
    smp = env.replay_sampler(forward=1)
    assert env.replay_sampler(forward=1) is smp and env.replay_sampler(forward=1, back=1) is not smp      # cached per argument tuple
    assert (smp.back, smp.forward, smp.attempts) == (0, 1, 16)
    tr = smp.transitions(2048)
    assert sorted(tr) == ["env", "fov_loc", "index", "next_fov_loc", "next_index", "next_obs", "obs", "ok"]
    e, k, k1, ok = (tr[x].cpu().numpy() for x in ("env", "index", "next_index", "ok"))
    assert ok.sum() >= 0.99 * 2048
    assert np.array_equal(k1[ok == 1], k[ok == 1] + 1) and (k1[ok == 0] == -1).all()
    ended, pairs = 0, set()
    for b in np.nonzero(ok)[0]:
        key = (int(e[b]), int(k[b]))
        nxt = (key[0], key[1] + 1)
        assert nxt not in resets, f"row {b}: next_obs is the reset observation {nxt}"
        ended += nxt in terminals
        pairs.add(key)
        assert torch.equal(tr["obs"][b].view(torch.int32), rec[key].view(torch.int32)), key
        assert torch.equal(tr["next_obs"][b].view(torch.int32), rec[nxt].view(torch.int32)), nxt
    assert ended >= 1, "no drawn transition ends in a terminal observation: lengthen the run"
    assert len(pairs) >= 30
    env.close()


def test_vec_env_without_history_has_no_sampler():
    env = _vec_env(True, 0)
    with pytest.raises(ValueError, match="history_len"):
        env.replay_sampler()
    env.close()
