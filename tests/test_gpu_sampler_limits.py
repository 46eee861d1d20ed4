"""GPU: the replay sampler (K7) and the prioritized sampler (K9) at AGX_REPLAY_SPAN_LIMIT = 64, and agx_replay_inspect at the 255 of
the age byte and of `ahead`.  The scenarios are tests/limit_cases.py's `span` and `span17` (tests/test_limit_cases_cpu.py pins what
they hold): back / forward windows that fill k_priority_weights' LDS age tile to its last byte (64 + 64 + 64 of kPrioRow = 196),
reach into the chunk of 64 rows before and a whole chunk ahead, and an episode longer than 255 appends.  Every output is compared
with tests/replay_model.py / tests/priority_model.py EXACTLY, as tests/test_gpu_replay.py and tests/test_gpu_priority.py do at small
spans.  One run per scenario (a module fixture) collects the device's outputs next to snapshots of the models."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import limit_cases as lc
import priority_model as pm
import replay_model as rm
from history_model import HistoryModel
from test_gpu_replay import _pipe, _steps, _t

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SET_SEED = 5


def _host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def _pairs(samples):
    return _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))


def _all_pairs(model):
    """Every (n, k), k in [-1, cnt + 1), and an env on either side."""
    return [(n, k) for n in range(-1, model.N + 1) for k in range(-1, int(model.count[n]) + 2 if 0 <= n < model.N else 2)]


def _run(name, configs, uniform):
    """Drive the scenario on a base 12 x 12 pipeline next to the model.  At each draw point every retained row of every
    prioritized table gets a fresh random priority (device and model), then every sampler draws B = SPAN_B: the outputs go into
    the record with a snapshot of the model and the tables.  After the last step: lookup and inspect over every (n, k), and an
    equally weighted draw of SPAN_SET_B per config from a new prioritized sampler."""
    from active_gym import FrameHistory, PrioritizedSampler, ReplaySampler
    from active_gym import replay as rp
    N, fs, T, steps, at = lc.SPAN[name]
    pipe = _pipe(N, kind="base", obs=(12, 12), fs=fs)
    hist = FrameHistory(pipe, T)
    model = HistoryModel(N, fs, T)
    smps = [ReplaySampler(hist, back=b, forward=f, attempts=16, seed=lc.SAMPLER_SEED) for b, f in configs] if uniform else []
    pers = [PrioritizedSampler(hist, back=b, forward=f, seed=lc.SAMPLER_SEED) for b, f in configs]
    tables = [pm.Table(model) for _ in configs]
    points = []

    def after(step):
        if step not in at:
            return
        rows, prio = lc.span_priorities(model, np.random.default_rng(100 + len(points)))
        env, idx = [r[0] for r in rows], [r[1] for r in rows]
        for per, table in zip(pers, tables):
            per.update(_t(np.array(env, np.int32)), _t(np.array(idx, np.int64)), _t(prio))
            pm.update(model, table, env, idx, prio)
        snap_model, snap_tables = copy.deepcopy((model, tables))
        point = dict(model=snap_model, tables=snap_tables, uniform=[], prioritized=[])
        for smp in smps:
            point["uniform"].append(_host(*smp.sample(lc.SPAN_B)) + [int(smp.total())])
        for per in pers:
            got = _host(*per.sample(lc.SPAN_B))
            point["prioritized"].append(got + [per.weight.cpu().numpy(), int(per.total()), int(per.accepted())])
        points.append(point)

    _steps(pipe, hist, model, lc.span_commands(name), lc.SPAN_SEED, after=after)
    assert len(points) == len(at)
    pairs = _all_pairs(model)
    out = dict(points=points, model=model, pairs=pairs, configs=configs)
    out["lookup"] = [per.lookup(*_pairs(pairs)).tolist() for per in pers]
    out["inspect"] = [t.tolist() for t in rp.inspect(hist, *_pairs(pairs))]
    out["set"] = []
    for b, f in configs:
        per = PrioritizedSampler(hist, back=b, forward=f, seed=SET_SEED)
        got = _host(*per.sample(lc.SPAN_SET_B))
        out["set"].append(got + [per.weight.cpu().numpy(), int(per.total()), int(per.accepted())])
        per.close()
    out["refusals"] = _refusals(pipe, hist)
    pipe.close()
    return out


def _refusals(pipe, hist):
    """back / forward of 65 and of -1 on a LIVE history (tests/test_replay_cpu.py and tests/test_priority_cpu.py cover the null
    handle): (rc, the handle written, the message) per create call."""
    from active_gym import _native as nat
    from active_gym import priority as pr
    from active_gym import replay as rp
    out = []
    for back, forward in ((65, 1), (-1, 1), (0, 65), (0, -1), (64, 65), (65, 64)):
        h = ctypes.c_void_p()
        rc = rp.lib().agx_replay_create(hist.handle, back, forward, 16, ctypes.byref(h))
        out.append(("replay", back, forward, rc, h.value, nat.last_error(pipe._ctx)))
        h = ctypes.c_void_p()
        rc = pr.lib().agx_priority_create(hist.handle, back, forward, ctypes.byref(h))
        out.append(("priority", back, forward, rc, h.value, nat.last_error(pipe._ctx)))
    return out


@pytest.fixture(scope="module")
def span():
    return _run("span", lc.SPAN_CONFIGS, uniform=True)


@pytest.fixture(scope="module")
def span17():
    return _run("span17", [(64, 64)], uniform=False)


CONFIG_IDS = [f"back{b}_forward{f}" for b, f in lc.SPAN_CONFIGS]


@pytest.mark.parametrize("ci", range(len(lc.SPAN_CONFIGS)), ids=CONFIG_IDS)
def test_uniform_draw_at_the_span_limit(span, ci):
    """K7: env, index, ok and total of B = 2048 at each of the three draw points equal replay_model.draw; at the spans with
    forward = 64 samples fail (the -1 path) while the history is short."""
    back, forward = lc.SPAN_CONFIGS[ci]
    compared = 0
    for call, point in enumerate(span["points"]):
        env, idx, ok, total = point["uniform"][ci]
        we, wi, wo, wt = rm.draw(point["model"], back, forward, 16, lc.SAMPLER_SEED, call, lc.SPAN_B)
        assert total == wt and np.array_equal(ok, wo) and np.array_equal(env, we) and np.array_equal(idx, wi), (back, forward, call)
        assert set(zip(env[ok == 1].tolist(), idx[ok == 1].tolist())) <= set(rm.accepted_set(point["model"], back, forward))
        compared += lc.SPAN_B
    assert wo.sum() >= 0.99 * lc.SPAN_B
    print(f"uniform ({back}, {forward}): {compared} samples compared")


@pytest.mark.parametrize("ci", range(len(lc.SPAN_CONFIGS)), ids=CONFIG_IDS)
def test_prioritized_draw_at_the_span_limit(span, ci):
    """K9: env, index, ok, weight, total and accepted of B = 2048 at each draw point, every retained row holding a random
    priority (rows of earlier points evicted and overwritten by the last one), equal priority_model.draw; lookup over all (n, k)
    equals the model."""
    back, forward = lc.SPAN_CONFIGS[ci]
    for call, point in enumerate(span["points"]):
        env, idx, ok, weight, total, acc = point["prioritized"][ci]
        we, wi, wo, ww, wt, wa = pm.draw(point["model"], point["tables"][ci], back, forward, lc.SAMPLER_SEED, call, lc.SPAN_B)
        assert (total, acc) == (wt, wa), (back, forward, call)
        assert np.array_equal(ok, wo) and np.array_equal(env, we) and np.array_equal(idx, wi) and np.array_equal(weight, ww), (back, forward, call)
    assert wo.all() and wa == len(rm.accepted_set(span["model"], back, forward)) and len(set(ww.tolist())) > 100
    last = span["points"][-1]
    assert span["lookup"][ci] == [pm.lookup(last["model"], last["tables"][ci], n, k) for n, k in span["pairs"]]


@pytest.mark.parametrize("ci", range(len(lc.SPAN_CONFIGS)), ids=CONFIG_IDS)
def test_equal_weights_draw_exactly_the_accepted_set(span, ci):
    """A new table (every weight 65536): the draw of SPAN_SET_B equals the model's, and its sample set is rm.accepted_set - a
    tile byte read from the wrong place would admit or drop a row."""
    back, forward = lc.SPAN_CONFIGS[ci]
    model = span["model"]
    env, idx, ok, weight, total, acc = span["set"][ci]
    we, wi, wo, ww, wt, wa = pm.draw(model, pm.Table(model), back, forward, SET_SEED, 0, lc.SPAN_SET_B)
    assert np.array_equal(env, we) and np.array_equal(idx, wi) and np.array_equal(ok, wo) and np.array_equal(weight, ww)
    V = rm.accepted_set(model, back, forward)
    assert sorted(set(zip(env.tolist(), idx.tolist()))) == V and acc == wa == len(V) and total == wt == 65536 * len(V)


def test_prioritized_draw_with_a_last_group_of_one_env(span17):
    """span17, (64, 64): N = 17 leaves k_priority_weights' last group of 16 envs with one env; all six outputs, the lookup and the
    accepted set equal the models."""
    model = span17["model"]
    point = span17["points"][0]
    env, idx, ok, weight, total, acc = point["prioritized"][0]
    we, wi, wo, ww, wt, wa = pm.draw(point["model"], point["tables"][0], 64, 64, lc.SAMPLER_SEED, 0, lc.SPAN_B)
    assert (total, acc) == (wt, wa) and wo.all() and 16 in we
    assert np.array_equal(ok, wo) and np.array_equal(env, we) and np.array_equal(idx, wi) and np.array_equal(weight, ww)
    assert span17["lookup"][0] == [pm.lookup(point["model"], point["tables"][0], n, k) for n, k in span17["pairs"]]
    env, idx, ok, weight, total, acc = span17["set"][0]
    V = rm.accepted_set(model, 64, 64)
    assert set(zip(env.tolist(), idx.tolist())) <= set(V) and acc == len(V) and total == 65536 * len(V)
    we, wi, _, _, _, _ = pm.draw(model, pm.Table(model), 64, 64, SET_SEED, 0, lc.SPAN_SET_B)
    assert np.array_equal(env, we) and np.array_equal(idx, wi)


def test_inspect_at_the_saturated_age(span):
    """agx_replay_inspect over every (n, k), k in [-1, cnt], of `span`: age and ahead equal the model, the 255s included."""
    model = span["model"]
    want = [rm.inspect(model, n, k) if 0 <= n < model.N else (-1, -1) for n, k in span["pairs"]]
    age, ahead = span["inspect"]
    assert list(zip(age, ahead)) == want
    env0 = [w for (n, _), w in zip(span["pairs"], want) if n == 0]
    assert sum(a == 255 for a, _ in want) >= 30 and sum(f == 255 for _, f in env0) == 62
    print(f"inspect: {len(want)} samples compared, {sum(a == 255 for a, _ in want)} with age 255, {sum(f == 255 for _, f in want)} with ahead 255")


def test_spans_outside_the_limit_are_refused_on_a_live_history(span):
    from active_gym import _native as nat
    assert len(span["refusals"]) == 12
    for who, back, forward, rc, handle, msg in span["refusals"]:
        assert rc == nat.E_INVALID and not handle, (who, back, forward)
        bad = "back" if not 0 <= back <= 64 else "forward"
        assert f"agx_{who}_create" in msg and f"{bad} must be" in msg, (who, back, forward, msg)
