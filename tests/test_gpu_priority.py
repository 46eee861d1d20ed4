"""GPU: the prioritized sampler (include/agx_priority.h) through ObsPipeline + FrameHistory + PrioritizedSampler.  The draw is a
pure integer function of (seed, call number), the history's bookkeeping and the table, so every case compares env, index, ok,
weight, total and accepted with tests/priority_model.py EXACTLY: there is no tolerance in them.  The one floating-point output,
importance(), is compared with NumPy float64 at rtol = 1e-6 (one rounding to float32, at most 2^-24 relative, plus a few ulps of
the float64 pow)."""
import ctypes

import numpy as np
import pytest
import torch

import priority_model as pm
import replay_model as rm
import steplog_model as sm
from history_model import CLEAR, SKIP, HistoryModel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = ctypes.c_void_p
SENTINEL = -3.0                 # exact in float32; no observation value is negative
CONFIGS = [(0, 0), (0, 1), (2, 1), (0, 3)]          # (back, forward)
MAIN_SEED = 3
GAMMA = 0.99
SPECIAL = [0.0, float("nan"), 2.0 ** -17, 1.0, 3.7, 65536.0]


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


def _equals_model(per, model, table, seed, call, B):
    """One sample(B) == the model's call `call`, in all six outputs; returns the model's draw."""
    env, idx, ok = per.sample(B)
    want = pm.draw(model, table, per.back, per.forward, seed, call, B)
    we, wi, wo, ww, wt, wa = want
    assert int(per.total()) == wt, f"total differs from the model (call {call})"
    assert int(per.accepted()) == wa, f"accepted differs from the model (call {call})"
    assert np.array_equal(ok.cpu().numpy(), wo), f"ok differs from the model (call {call})"
    assert np.array_equal(env.cpu().numpy(), we), f"env differs from the model (call {call})"
    assert np.array_equal(idx.cpu().numpy(), wi), f"index differs from the model (call {call})"
    assert np.array_equal(per.weight.cpu().numpy(), ww), f"weight differs from the model (call {call})"
    return want


def _update(per, model, table, env, index, priority):
    env, index, priority = np.asarray(env, np.int32), np.asarray(index, np.int64), np.asarray(priority, np.float32)
    per.update(_t(env), _t(index), _t(priority))
    pm.update(model, table, env, index, priority)


def _lookup_all(per, model, table):
    """lookup over every (n, k), k in [-1, cnt], and an env on either side == the model."""
    samples = [(n, k) for n in range(-1, model.N + 1) for k in range(-1, int(model.count[n]) + 2 if 0 <= n < model.N else 2)]
    got = per.lookup(_t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64)))
    assert got.tolist() == [pm.lookup(model, table, n, k) for n, k in samples]


def _update_all(per, model, table, rng, weight=None):
    """Every retained row gets a priority: random over 2^-18 .. 2^14, or `weight` for all."""
    rows = [(n, k) for n in range(model.N) for k in range(max(int(model.count[n]) - model.T, 0), int(model.count[n]))]
    prio = np.full(len(rows), weight, np.float32) if weight is not None else (2.0 ** rng.uniform(-18, 14, len(rows))).astype(np.float32)
    _update(per, model, table, [r[0] for r in rows], [r[1] for r in rows], prio)


def test_main_case():
    """N = 5, T = 8, fs = 4, 84 / 30, commands(3, 5, 13) incl. CLEAR / SKIP (the rows wrap, lo mod T != 0): before any push (total =
    0, nothing ok) and after every step each of the four configs draws exactly the model's samples; between the steps 64
    distinct samples - retained, evicted, never issued, -1, envs that are none - are updated with priorities that include 0, NaN,
    2^-17, 1.0, 3.7 and 65536.0; lookup over all (n, k) equals the model; and with equal weights B = 4096 draws exactly the
    uniform sampler's accepted set."""
    from active_gym import FrameHistory, PrioritizedSampler
    pipe = _pipe(5)
    hist = FrameHistory(pipe, 8)
    nbytes = hist.nbytes
    model = HistoryModel(5, 4, 8)
    pers = [PrioritizedSampler(hist, back=b, forward=f, seed=7) for b, f in CONFIGS]
    tables = [pm.Table(model) for _ in CONFIGS]
    assert hist.nbytes == nbytes and pers[0].bytes() >= 5 * 8 * 20          # the table and its scratch are the sampler's own
    calls = [0] * len(pers)
    cmds = rm.commands(MAIN_SEED, 5, 13)
    rng = np.random.default_rng(17)

    def check(B):
        out = []
        for i, per in enumerate(pers):
            out.append(_equals_model(per, model, tables[i], 7, calls[i], B))
            calls[i] += 1
        return out

    def after(step):
        check(512)
        pool = [(n, k) for n in range(-1, 6) for k in range(-1, int(model.count[n]) + 2 if 0 <= n < 5 else 3)]
        pick = [pool[i] for i in rng.permutation(len(pool))[:64]]
        prio = np.where(rng.random(len(pick)) < 0.5, rng.choice(SPECIAL, len(pick)), 2.0 ** rng.uniform(-18, 6, len(pick))).astype(np.float32)
        for per, table in zip(pers, tables):
            _update(per, model, table, [s[0] for s in pick], [s[1] for s in pick], prio)
            _lookup_all(per, model, table)

    for _, _, ok, wt, total, acc in check(512):
        assert not ok.any() and not wt.any() and total == 0 and acc == 0
    _steps(pipe, hist, model, cmds, MAIN_SEED, after=after)
    assert any((int(c) - 8) % 8 for c in model.count if c > 8)          # the rows wrap, and lo mod T != 0
    assert all(len(set(t.weight[t.stamp >= 0].tolist())) >= 8 for t in tables)
    last = check(4096)
    assert all(ok.all() for _, _, ok, _, _, _ in last)                  # no rejection: a sample fails only on an empty set
    for per in pers:
        per.close()
    for back, forward in CONFIGS:
        per = PrioritizedSampler(hist, back=back, forward=forward, seed=5)
        env, idx, ok, wt, total, acc = _equals_model(per, model, pm.Table(model), 5, 0, 4096)
        V = rm.accepted_set(model, back, forward)
        assert sorted(set(zip(env.tolist(), idx.tolist()))) == V and acc == len(V) and total == 65536 * len(V)
    pipe.close()


@pytest.mark.parametrize("N", [1, 257, 700])
def test_scan_across_chunks_and_waves(N):
    """kind base, 12 x 12, fs = 2, T = 4, 6 steps with p_skip = 0.3 (counts differ between envs): the offsets of N = 700 cross two
    chunk carries of the env scan and every wave boundary, N = 257 leaves a last group of one env, N = 1 is one lane."""
    from active_gym import FrameHistory, PrioritizedSampler
    pipe = _pipe(N, kind="base", obs=(12, 12), fs=2)
    hist = FrameHistory(pipe, 4)
    model = HistoryModel(N, 2, 4)
    _steps(pipe, hist, model, rm.commands(21, N, 6, p_skip=0.3), 21)
    assert N == 1 or len(set(model.count.tolist())) > 1
    per = PrioritizedSampler(hist, back=0, forward=1, seed=11)
    table = pm.Table(model)
    _update_all(per, model, table, np.random.default_rng(N))
    env, _, ok, _, _, _ = _equals_model(per, model, table, 11, 0, 2048)
    assert ok.all() and (N == 1 or len(set(env.tolist())) > min(N, 2048) // 8)
    _lookup_all(per, model, table)
    pipe.close()


@pytest.mark.parametrize("saturated", [False, True], ids=["random_weights", "all_0xFFFFFFFF"])
def test_rows_of_one_env_across_chunks(saturated):
    """N = 3, kind base, 12 x 12, fs = 2, T = 600, 700 steps: more rows per env than a workgroup has threads, ten chunks of 64 per
    env with a last one of 24, a wrapped ring.  Once with random weights, once with every row at 0xFFFFFFFF: the prefixes inside
    an env and the env offsets cross 2^32 and reach about 2^41."""
    from active_gym import FrameHistory, PrioritizedSampler
    pipe = _pipe(3, kind="base", obs=(12, 12), fs=2)
    hist = FrameHistory(pipe, 600)
    model = HistoryModel(3, 2, 600)
    _steps(pipe, hist, model, rm.commands(9, 3, 700, p_clear=0.02, p_skip=0.1), 9)
    assert all(int(c) > 600 for c in model.count) and len(set(model.count.tolist())) > 1
    for back, forward in ((0, 1), (2, 1)):
        per = PrioritizedSampler(hist, back=back, forward=forward, seed=13)
        table = pm.Table(model)
        _update_all(per, model, table, np.random.default_rng(4), weight=float("inf") if saturated else None)
        env, idx, ok, wt, total, acc = _equals_model(per, model, table, 13, 0, 4096)
        assert ok.all() and set(env.tolist()) == {0, 1, 2} and acc > 1500
        assert len({int(k - max(int(model.count[n]) - 600, 0)) // 64 for n, k in zip(env, idx)}) == 10        # every chunk is drawn from
        if saturated:
            assert (wt == 0xFFFFFFFF).all() and total == acc * 0xFFFFFFFF > 1 << 42
        per.close()
    pipe.close()


@pytest.mark.parametrize("T", [5, 1])
def test_capacity_that_is_no_power_of_two(T):
    """T = 5: the rows wrap at a capacity that is no power of two.  T = 1 with forward = 1: nothing is accepted, total = 0 and
    every sample is -1."""
    from active_gym import FrameHistory, PrioritizedSampler
    pipe = _pipe(4, kind="base", obs=(12, 12), fs=1)
    hist = FrameHistory(pipe, T)
    model = HistoryModel(4, 1, T)
    _steps(pipe, hist, model, rm.commands(2, 4, 9, p_skip=0.2), 2)
    per = PrioritizedSampler(hist, back=0, forward=1, seed=3)
    table = pm.Table(model)
    _update_all(per, model, table, np.random.default_rng(T))
    env, idx, ok, wt, total, acc = _equals_model(per, model, table, 3, 0, 1024)
    if T == 1:
        assert total == 0 and acc == 0 and not ok.any() and (env == -1).all() and (idx == -1).all() and not wt.any()
    else:
        assert ok.all() and acc >= 8
    _lookup_all(per, model, table)
    pipe.close()


def _main_setup(seed=9):
    from active_gym import FrameHistory, PrioritizedSampler
    pipe = _pipe(5)
    hist = FrameHistory(pipe, 8)
    model = HistoryModel(5, 4, 8)
    _steps(pipe, hist, model, rm.commands(MAIN_SEED, 5, 13), MAIN_SEED)
    per = PrioritizedSampler(hist, back=0, forward=1, seed=seed)
    table = pm.Table(model)
    _update_all(per, model, table, np.random.default_rng(8))
    return pipe, hist, model, per, table


def test_large_batch_and_null_outputs():
    """B = 70,000 (more samples than a 16-bit grid dimension); d_ok, d_weight, d_total, d_accepted NULL; B = 0 launches nothing
    and does not advance the call counter."""
    from active_gym import _native as nat
    from active_gym import priority as pr
    pipe, hist, model, per, table = _main_setup()
    _equals_model(per, model, table, 9, 0, 70_000)
    lib = pr.lib()
    env, idx = torch.empty(300, dtype=torch.int32, device=DEV), torch.empty(300, dtype=torch.int64, device=DEV)
    assert lib.agx_priority_sample(per._t, 0, None, None, None, None, None, None, pipe._stream()) == nat.OK
    assert lib.agx_priority_sample(per._t, 300, P(env.data_ptr()), P(idx.data_ptr()), None, None, None, None, pipe._stream()) == nat.OK
    we, wi, _, _, _, _ = pm.draw(model, table, 0, 1, 9, 1, 300)
    assert np.array_equal(env.cpu().numpy(), we) and np.array_equal(idx.cpu().numpy(), wi)
    assert lib.agx_priority_sample(per._t, 4, None, P(idx.data_ptr()), None, None, None, None, pipe._stream()) == nat.E_INVALID
    assert "d_env" in nat.last_error(pipe._ctx)
    assert lib.agx_priority_sample(per._t, 4, P(env.data_ptr()), None, None, None, None, None, pipe._stream()) == nat.E_INVALID
    assert lib.agx_priority_update(per._t, P(env.data_ptr()), P(idx.data_ptr()), None, 4, pipe._stream()) == nat.E_INVALID
    assert "d_priority" in nat.last_error(pipe._ctx)
    assert lib.agx_priority_lookup(per._t, P(env.data_ptr()), P(idx.data_ptr()), 4, None, pipe._stream()) == nat.E_INVALID
    assert lib.agx_priority_update(per._t, None, None, None, 0, pipe._stream()) == nat.OK
    _equals_model(per, model, table, 9, 2, 64)
    with pytest.raises(ValueError):
        per.sample(-1)
    pipe.close()


def test_clear_reseed_and_history_clear():
    """clear(): the stamps are gone and wmax is 65536 again; seed(s) restarts the sequence; FrameHistory.clear() clears the table,
    so a stamp from before does not pass for the same index issued again."""
    pipe, hist, model, per, table = _main_setup()
    assert table.wmax > 65536
    _equals_model(per, model, table, 9, 0, 256)
    per.clear()
    table.clear()
    env, idx, ok, wt, total, acc = _equals_model(per, model, table, 9, 1, 256)
    assert (wt == 65536).all() and total == 65536 * acc
    _lookup_all(per, model, table)
    _update_all(per, model, table, np.random.default_rng(1))
    per.seed((1 << 63) + 12345)
    per.sample(0)
    _equals_model(per, model, table, (1 << 63) + 12345, 0, 256)
    hist.clear()
    model.clear()
    table.clear()
    _equals_model(per, model, table, (1 << 63) + 12345, 1, 64)
    _steps(pipe, hist, model, rm.commands(12, 5, 11, p_clear=0.3), 12)      # the same indices again, every episode begun by a CLEAR
    env, idx, ok, wt, total, acc = _equals_model(per, model, table, (1 << 63) + 12345, 2, 256)
    assert acc > 0 and (wt == 65536).all()
    _lookup_all(per, model, table)
    pipe.close()


def test_env_range_and_closed_history_are_refused():
    from active_gym import FrameHistory, PrioritizedSampler
    from active_gym import _native as nat
    pipe = _pipe(4)
    hist = FrameHistory(pipe, 8)
    pipe.env_range(1, 2)
    with pytest.raises(nat.AgxError, match="env range") as e:
        PrioritizedSampler(hist)
    assert e.value.code == nat.E_STATE
    pipe.env_range()
    per = PrioritizedSampler(hist)
    assert hist.prioritized(0, 1, 0) is hist.prioritized(0, 1, 0) and hist.prioritized(0, 1, 0) is not per
    z32, z64, zf = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), torch.ones(4, device=DEV)
    pipe.env_range(1, 2)
    for call in (lambda: per.sample(4), lambda: per.update(z32, z64, zf), lambda: per.lookup(z32, z64), lambda: per.seed(1), lambda: per.clear()):
        with pytest.raises(nat.AgxError, match="env range") as e:
            call()
        assert e.value.code == nat.E_STATE
    pipe.env_range()
    env, idx, ok = per.sample(4)
    assert env.tolist() == [-1] * 4 and idx.tolist() == [-1] * 4 and ok.tolist() == [0] * 4 and per.weight.tolist() == [0] * 4
    assert per.importance(0.4).tolist() == [0.0] * 4
    cached = hist.prioritized(0, 1, 0)
    hist.close()
    assert not cached.alive
    with pytest.raises(RuntimeError, match="closed"):
        per.sample(4)
    pipe.close()


def test_captured_graph_replays_draw_anew():
    """One sample captured under torch.cuda.graph on a side stream and replayed three times draws the model's calls 1, 2, 3 - and
    what a second sampler of the same seed draws in the same calls issued one by one."""
    from active_gym import PrioritizedSampler
    pipe, hist, model, per, table = _main_setup()
    ref = PrioritizedSampler(hist, back=0, forward=1, seed=9)
    _update_all(ref, model, pm.Table(model), np.random.default_rng(8))            # the same priorities as per's
    B = 300
    env = torch.empty((B,), dtype=torch.int32, device=DEV)
    idx = torch.empty((B,), dtype=torch.int64, device=DEV)
    ok = torch.empty((B,), dtype=torch.uint8, device=DEV)
    wt = torch.empty((B,), dtype=torch.int64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        per.sample(B, env, idx, ok, wt)                      # call 0, eager, on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        per.sample(B, env, idx, ok, wt)                      # captured, not run: the counter lives on the device
    ref.sample(B)
    for call in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        we, wi, wo, ww, wtot, wacc = pm.draw(model, table, 0, 1, 9, call, B)
        assert np.array_equal(env.cpu().numpy(), we) and np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(ok.cpu().numpy(), wo), call
        assert np.array_equal(wt.cpu().numpy(), ww) and int(per.total()) == wtot and int(per.accepted()) == wacc
        renv, ridx, rok = ref.sample(B)
        assert torch.equal(env, renv) and torch.equal(idx, ridx) and torch.equal(ok, rok) and torch.equal(wt, ref.weight)
    _equals_model(per, model, table, 9, 4, B)                # usable one call at a time after the replays
    pipe.close()


def test_duplicates_within_one_update():
    """A sample that occurs several times in one update, every time with the same priority, is written once; wmax follows."""
    pipe, hist, model, per, table = _main_setup()
    V = rm.accepted_set(model, 0, 1)
    env = [V[i % 3][0] for i in range(200)] + [-1] * 56
    idx = [V[i % 3][1] for i in range(200)] + [-1] * 56
    prio = [(40000.0, 0.001, 2.5)[i % 3] for i in range(200)] + [60000.0] * 56
    _update(per, model, table, env, idx, prio)
    assert table.wmax == 40000 * 65536                   # (the skipped samples' 60000.0 does not count)
    _lookup_all(per, model, table)
    _equals_model(per, model, table, 9, 0, 1024)
    pipe.close()


@pytest.mark.parametrize("mode", ["resize", "mask"])
def test_consistency_with_the_read_path(mode):
    """back = 2, forward = 1: every sample is ok and valid under history.observe at index and index + 1, both observations are bit
    for bit what the steps returned, and GlimpseMemory(hist, 3) is full at both."""
    from active_gym import FrameHistory, GlimpseMemory, PrioritizedSampler
    pipe = _pipe(5, mode=mode)
    hist = FrameHistory(pipe, 8)
    model, rec = HistoryModel(5, 4, 8), {}
    _steps(pipe, hist, model, rm.commands(MAIN_SEED, 5, 13), MAIN_SEED, rec=rec)
    B = 512
    per = PrioritizedSampler(hist, back=2, forward=1, seed=5)
    table = pm.Table(model)
    _update_all(per, model, table, np.random.default_rng(6))
    we, wi, wo, _, _, _ = _equals_model(per, model, table, 5, 0, B)
    assert wo.all() and len(set(zip(we.tolist(), wi.tolist()))) >= 5
    env, idx = _t(we), _t(wi)
    mem = GlimpseMemory(hist, 3)
    for step in (0, 1):
        out = torch.full((B,) + hist.obs_row_shape(), SENTINEL, dtype=torch.float32, device=DEV)
        obs, loc, valid = hist.observe(env, idx + step, out=out)
        assert valid.cpu().numpy().all()
        _, _, taken = mem.observe(env, idx + step)
        taken = taken.cpu().numpy()
        for b in range(B):
            o, l = rec[(int(we[b]), int(wi[b]) + step)]
            assert torch.equal(obs[b].view(torch.int32), o.view(torch.int32)), (b, step)
            assert torch.equal(loc[b], l)
            assert taken[b] == min(3, rm.age(model, int(we[b]), int(wi[b]) + step) + 1)
    pipe.close()


def test_skew():
    """One accepted row at 0xFFFFFFFF, the rest at 1: the model says how many of B = 4096 land on that row; so does the device."""
    pipe, hist, model, per, table = _main_setup()
    _update_all(per, model, table, None, weight=2.0 ** -16)
    n, k = rm.accepted_set(model, 0, 1)[7]
    _update(per, model, table, [n], [k], [float("inf")])
    we, wi, _, ww, total, acc = _equals_model(per, model, table, 9, 0, 4096)
    assert total == 0xFFFFFFFF + acc - 1
    hits = int(((we == n) & (wi == k)).sum())
    assert hits == int((ww == 0xFFFFFFFF).sum()) >= 4090
    env, idx, _ = per.sample(4096)                      # the model's next call, counted on the device's own outputs
    we, wi, _, _, _, _ = pm.draw(model, table, 0, 1, 9, 1, 4096)
    assert int(((env == n) & (idx == k)).sum()) == int(((we == n) & (wi == k)).sum())
    pipe.close()


@pytest.mark.parametrize("beta", [0.4, 1.0])
def test_importance(beta):
    """importance(beta) == ((accepted * weight / total) ** -beta) / max over the ok rows, from the integer outputs in NumPy
    float64, at rtol = 1e-6; the maximum is exactly 1.0; probability() is weight / total."""
    pipe, hist, model, per, table = _main_setup()
    _, _, ok, ww, total, acc = _equals_model(per, model, table, 9, 0, 2048)
    raw = (acc * ww.astype(np.float64) / total) ** -beta
    want = raw / raw.max()
    got = per.importance(beta)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2048,)
    got = got.cpu().numpy()
    assert np.allclose(got, want, rtol=1e-6, atol=0.0) and got.max() == 1.0 and len(set(got.tolist())) >= 4
    assert np.allclose(per.probability().cpu().numpy(), ww / total, rtol=1e-15, atol=0.0)
    pipe.close()


# ---------------------------------------------------------------------------------------------- the vector env
def _vec_env(native_loop, history_len, **extra):
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=150, native_loop=native_loop, history_len=history_len, **extra)
    return AtariVecEnv(AtariEnvArgs(**kw), 6, kind="fixed", noop_fn=lambda: 2)


@pytest.mark.parametrize("native", [True, False], ids=["native_loop", "python_loop"])
def test_vec_env_prioritized_replay_batch(native):
    """AtariVecEnv(history_len = 64, step_log = True), 40 random steps with autoresets.  Every ok row of replay_batch(2048, nstep = 3,
    prioritized = True) passes the checks tests/test_gpu_steplog.py makes on the uniform batch (the actions of the producing step,
    the bit-exact fold, the recorded next_obs, no reset observation as next_index) and the draw is the model's; update_priorities
    followed by lookup shows the written weights; a second batch equals the model's draw on the updated table; and replay_batch
    without `prioritized` returns the keys it always did."""
    N, STEPS = 6, 40
    env = _vec_env(native, 64, step_log=True)
    assert (env._loop is not None) == native
    model = HistoryModel(N, 4, 64)
    obs, info = env.reset()
    model.push(np.full(N, 2 | CLEAR, np.uint8))
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
        model.push(np.full(N, 2, np.uint8))                        # the step's observation; then the reset one of an autoreset env
        if done.any():
            model.push(np.where(done, 2 | CLEAR, SKIP).astype(np.uint8))
        assert np.array_equal(hi, model.count - 1), "the model's pushes are not the env's"
        for i in range(N):
            rec[(i, int(hi[i]))] = obs[i]
            at = int(hi[i]) - int(done[i])                     # the observation this step produced
            produced[(i, at)] = (int(act["motor_action"][i]), act["sensory_action"][i].copy(), np.float32(reward[i]), bool(done[i]))
        for i in np.nonzero(done)[0]:
            rec[(int(i), int(hi[i]) - 1)] = info["final_observation"][i].clone()
            resets.add((int(i), int(hi[i])))
    B = 2048
    uniform_keys = ["env", "index", "next_index", "ok", "obs", "next_obs", "ret", "discount", "steps", "flags", "fov_loc", "next_fov_loc",
                    "motor_action", "sensory_action"]
    assert sorted(env.replay_batch(8, nstep=3, gamma=GAMMA)) == sorted(uniform_keys)
    with pytest.raises(ValueError, match="prioritized=True"):
        env.update_priorities({}, torch.zeros(8, device=DEV))
    per = env.prioritized_sampler()
    assert env.prioritized_sampler() is per and env.prioritized_sampler(back=1) is not per and (per.back, per.forward) == (0, 1)
    table = pm.Table(model)
    out = env.replay_batch(B, nstep=3, gamma=GAMMA, prioritized=True, beta=0.4)
    assert sorted(out) == sorted(uniform_keys + ["weight", "priority"])
    we, wi, wo, ww, total, acc = pm.draw(model, table, 0, 1, 3, 0, B)               # seed = args.seed
    e, k, k1, ok, steps, flags, motor = (out[x].cpu().numpy() for x in ("env", "index", "next_index", "ok", "steps", "flags", "motor_action"))
    assert np.array_equal(e, we) and np.array_equal(k, wi) and np.array_equal(out["priority"].cpu().numpy(), ww) and wo.all()
    raw = (acc * ww.astype(np.float64) / total) ** -0.4
    assert np.allclose(out["weight"].cpu().numpy(), raw / raw.max(), rtol=1e-6, atol=0.0)
    sens = out["sensory_action"].cpu().numpy().view(np.int32)
    ret, disc = out["ret"].cpu().numpy().view(np.int32), out["discount"].cpu().numpy().view(np.int32)
    assert ok.sum() >= 0.99 * B
    full = by_terminal = 0
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
    assert full >= 1 and by_terminal >= 1
    # new priorities from a made-up TD error; a row with ok = 0 is passed as -1 and skipped
    td = torch.from_numpy(np.random.default_rng(1).normal(0, 3, B).astype(np.float32)).to(DEV)
    out["ok"][5] = 0
    env.update_priorities(out, td, alpha=0.6, eps=1e-6)
    prio = ((td.abs() + 1e-6) ** 0.6).cpu().numpy()
    seen = {}
    for b in range(B):                                          # a pair drawn twice keeps one of its priorities: make the model agree
        if b != 5:
            seen.setdefault((int(e[b]), int(k[b])), []).append(b)
    got = per.lookup(out["env"], out["index"]).cpu().numpy()
    for (n, at), rows in seen.items():
        stored = [b for b in rows if pm.quantise(prio[b]) == got[rows[0]]]
        assert stored, (n, at)
        pm.update(model, table, [n], [at], [prio[stored[0]]])
    table.wmax = max([table.wmax] + [pm.quantise(p) for b, p in enumerate(prio) if b != 5])      # every weight written counts, stored or not
    assert np.array_equal(got, np.array([pm.lookup(model, table, int(n), int(at)) for n, at in zip(e, k)]))
    assert len(set(got.tolist())) >= 20
    second = env.replay_batch(B, nstep=3, gamma=GAMMA, prioritized=True, beta=1.0)
    we, wi, wo, ww, total, acc = pm.draw(model, table, 0, 1, 3, 1, B)
    assert np.array_equal(second["env"].cpu().numpy(), we) and np.array_equal(second["index"].cpu().numpy(), wi)
    assert np.array_equal(second["priority"].cpu().numpy(), ww) and int(per.total()) == total and int(per.accepted()) == acc
    env.close()


def test_vec_env_without_history_has_no_prioritized_sampler():
    env = _vec_env(True, 0)
    with pytest.raises(ValueError, match="history_len"):
        env.prioritized_sampler()
    env.close()
