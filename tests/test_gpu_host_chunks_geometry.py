"""GPU: the chunked host step (args.host_obs_chunks, agx_loop_step_host) off the compile-time geometry.

tests/test_gpu_host_chunks.py runs at 84 x 84 / 30 x 30 / fs 4.  Here three geometries of the range cover
(tests/range_cases.py) run through the same method - the digests of everything reset() / step() return, compared with
host_obs_chunks = 0 on the same native scripted source: k_fovea_fixed<GeomR> with a raw-crop row that is not a multiple of
16 B, k_fovea_flexible2, and k_fovea_peripheral3 off the headline geometry.  N = 13 in C = 3 chunks (5 + 4 + 4 envs) and in
C = 13 chunks (one env each), 6 steps with episode ends, float32 and float16.  A geometry that AtariVecEnv keeps on the Python
loop (host_obs_chunks in effect 0) is passed over for the next one of the cover in table order."""
import functools
import json
import os
import random
import time

import numpy as np
import pytest

import range_cases as R
from test_gpu_host_chunks import _digest

pytestmark = pytest.mark.gpu

N = 13
STEPS = 6
MODES = {"fixed_raw": ("fixed", False, False), "flex_resize": ("flexible", True, False), "peripheral": ("peripheral", True, False)}
# name -> the cover entries that qualify, in table order (the ingest needs a square obs_size)
WANT = {
    "fixed_GeomR_odd_row": lambda e: e["key"] == "fixed_raw" and R.arith_class(e["case"], e["key"])[3] and R.arith_class(e["case"], e["key"])[4],
    "flexible2": lambda e: e["key"] == "flex_resize" and e["label"].startswith("flexible2 "),
    "per3_off_headline": lambda e: e["key"] == "peripheral" and e["label"].startswith("per3 ") and e["case"]["obs"] != [84, 84],
}


def _candidates(name):
    seen, out = set(), []
    for e in R.fovea_cover():
        c = e["case"]
        if WANT[name](e) and c["obs"][0] == c["obs"][1] and R.case_name(c) not in seen:
            seen.add(R.case_name(c))
            out.append(e)
    return out


def _args(entry, dtype, chunks):
    from active_gym import AtariEnvArgs
    c = entry["case"]
    kind, resize, mask = MODES[entry["key"]]
    kw = dict(game="g", seed=11, obs_size=tuple(c["obs"]), frame_stack=c["fs"], frame_source="native", frame_format="gray",
              compact_rows=True, obs_dtype=dtype, num_workers=4, scripted_actions=4, scripted_lives=2, scripted_p_life=80,
              scripted_p_over=10, host_obs_chunks=chunks, fov_size=tuple(c["fov"]), fov_init_loc=(1, 2),
              sensory_action_mode="absolute", resize_to_full=resize, mask_out=mask, antialias=bool(c["aa"]))
    if kind == "peripheral":
        kw.update(peripheral_res=tuple(c["per"]))
    return kind, AtariEnvArgs(**kw)


def _actions(kind, case, seed):
    rng = np.random.default_rng(seed)
    (oh, ow) = case["obs"]
    for _ in range(STEPS):
        motor = rng.integers(0, 4, N)
        types = rng.integers(0, 2, N)
        res = np.stack([rng.integers(1, oh + 1, N), rng.integers(1, ow + 1, N)], 1)
        sens = np.where(types[:, None] == 1, res, rng.integers(-5, max(oh, ow) + 5, (N, 2))).astype(np.int64)
        act = {"motor_action": motor, "sensory_action": sens}
        if kind == "flexible":
            act["sensory_action_type"] = types
        yield act


def _run(entry, dtype, chunks):
    """reset + STEPS steps -> (the digests of everything returned, step for step; the number of episode ends), or None where
    AtariVecEnv does not put this geometry on the chunked step."""
    from active_gym import AtariVecEnv
    kind, args = _args(entry, dtype, chunks)
    random.seed(1234)
    env = AtariVecEnv(args, N, kind=kind)
    if env.host_obs_chunks != chunks:
        env.close()
        return None
    assert (env._loop is not None) == (chunks > 0)
    log, ends = [], 0
    obs, info = env.reset()
    assert isinstance(obs, np.ndarray)
    log.append(("reset", _digest(obs), {k: _digest(v) for k, v in info.items()}))
    held = []
    for t, act in enumerate(_actions(kind, entry["case"], 7)):
        obs, reward, done, trunc, info = env.step(act)
        assert isinstance(obs, np.ndarray) and obs.shape[0] == N
        for s, arr, copy in held:
            assert np.array_equal(arr, copy), f"the observation of step {s} changed during step {t}"
        held = [h for h in held if h[0] > t - 2] + [(t, obs, obs.copy())]
        rec = {"obs": _digest(obs), "reward": _digest(reward), "done": _digest(done), "trunc": _digest(trunc)}
        for key, val in info.items():
            if key not in ("final_observation", "final_info"):
                rec[key] = _digest(val)
        if done.any():
            ends += int(done.sum())
            for i in np.nonzero(done)[0]:
                rec[f"final_observation[{i}]"] = _digest(info["final_observation"][i])
                fi = info["final_info"][i]
                rec[f"final_info[{i}]"] = {k: (_digest(v) if isinstance(v, np.ndarray) else (type(v).__name__, v)) for k, v in fi.items()}
            assert all(info["final_observation"][i] is None for i in np.nonzero(~done)[0])
        log.append((t, rec))
        del obs
    if chunks > 0:
        assert env._host_step.steps == STEPS, f"{env._host_step.steps} of {STEPS} steps took the chunked path"
    else:
        assert env._host_step is None
    env.close()
    return log, ends


@functools.lru_cache(None)
def _accepted(name, dtype):
    """The first qualifying geometry AtariVecEnv runs on the chunked step, and its unchunked reference run."""
    for e in _candidates(name):
        probe = _run(e, dtype, 1)
        if probe is not None:
            return e, _run(e, dtype, 0), probe
    raise AssertionError(f"{name}: AtariVecEnv puts no qualifying geometry on the chunked step")


def test_the_three_geometries_are_in_the_cover():
    for name in WANT:
        assert _candidates(name), name
    e = _candidates("fixed_GeomR_odd_row")[0]
    assert R.obs_elems(e["case"], e["key"]) * 4 % 16 != 0 and R.obs_elems(e["case"], e["key"]) * 2 % 16 != 0


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("chunks", [3, 13])
@pytest.mark.parametrize("name", list(WANT))
def test_chunked_host_step_equals_unchunked_off_the_headline_geometry(name, chunks, dtype):
    t0 = time.time()
    entry, (want, ends0), one = _accepted(name, dtype)
    got, ends1 = _run(entry, dtype, chunks)
    # episode ends and steps without one both occur (the emulator's odds are per frame; 73 of 78 env-steps ended at 400 / 60)
    assert ends0 == ends1 == one[1] and 0 < ends0 < N * STEPS // 2, f"autoreset fired for {ends0} of {N * STEPS} env-steps"
    assert len(want) == len(got) == STEPS + 1
    for ref in (got, one[0]):
        for w, g in zip(want, ref):
            assert w[0] == g[0]
            if w[0] == "reset":
                assert w[1:] == g[1:], "reset differs"
                continue
            assert set(w[1]) == set(g[1]), (w[0], sorted(set(w[1]) ^ set(g[1])))
            for key in w[1]:
                assert w[1][key] == g[1][key], (R.case_name(entry["case"]), f"step {w[0]}", key, w[1][key], g[1][key])
    if os.environ.get("AGX_RANGE_STATS"):                         # which geometry ran (DESIGN.md section 25 quotes a run)
        with open(os.environ["AGX_RANGE_STATS"], "a") as f:
            f.write(json.dumps(dict(test=f"host_chunks[{name}-{chunks}-{dtype}]", case=R.case_name(entry["case"]), key=entry["key"],
                                    ends=ends0, seconds=round(time.time() - t0, 2))) + "\n")
