"""GPU: host (NumPy) observations from the native loop in env chunks (args.host_obs_chunks, agx_loop_step_host).  The reference
is the unchunked path of the same env (host_obs_chunks = 0: the Python loop + one device-to-host copy), same native runner, same
seeds, Python's `random` seeded identically: everything a step returns must be exactly equal."""
import random
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 12


def _args(kind, fmt, compact, dtype, chunks, **over):
    from active_gym import AtariEnvArgs
    kw = dict(game="g", seed=11, obs_size=(84, 84), frame_source="native", frame_format=fmt, compact_rows=compact, obs_dtype=dtype,
              num_workers=4, scripted_actions=4, scripted_lives=2, scripted_p_life=250, scripted_p_over=60,   # many episode ends per step
              host_obs_chunks=chunks)
    if kind != "base":
        kw.update(fov_size=(30, 30), fov_init_loc=(2, 3), sensory_action_mode="absolute", resize_to_full=True)
    if kind == "peripheral":
        kw.update(peripheral_res=(20, 20))
    kw.update(over)
    return AtariEnvArgs(**kw)


def _actions(kind, N, seed):
    rng = np.random.default_rng(seed)
    for _ in range(STEPS):
        motor = rng.integers(0, 4, N)
        if kind == "base":
            yield motor
            continue
        types = rng.integers(0, 2, N)
        sens = np.where(types[:, None] == 1, rng.integers(8, 70, (N, 2)), rng.integers(-5, 60, (N, 2))).astype(np.int64)
        act = {"motor_action": motor, "sensory_action": sens}
        if kind == "flexible":
            act["sensory_action_type"] = types
        yield act


def _digest(v):
    """What is compared of one returned value: (dtype, shape, crc of the bytes) of an array - exact equality, without keeping the
    115 MB observations (a kept pool array would not go back to the pool) - or the value itself."""
    if isinstance(v, np.ndarray) and v.dtype != object:
        return (str(v.dtype), v.shape, zlib.crc32(np.ascontiguousarray(v).tobytes()))
    return v


def _run(kind, N, chunks, args, hold=2):
    """reset + STEPS steps; returns the digests of everything returned, step for step, and the number of episode ends.  Every
    observation is held for `hold` more steps and must not change meanwhile (fresh-array semantics: 2 and more; the pinned pair
    of args.copy_obs = False: valid until the step after next, i.e. 1)."""
    from active_gym import AtariVecEnv
    random.seed(1234)
    env = AtariVecEnv(args, N, kind=kind)
    assert env.host_obs_chunks == chunks
    assert (env._loop is not None) == (chunks > 0)
    log, ends = [], 0
    obs, info = env.reset()
    assert isinstance(obs, np.ndarray)
    log.append(("reset", _digest(obs), {k: _digest(v) for k, v in info.items()}))
    held = []                                               # (step, array, copy of it)
    for t, act in enumerate(_actions(kind, N, 7)):
        obs, reward, done, trunc, info = env.step(act)
        assert isinstance(obs, np.ndarray) and obs.shape[0] == N
        for s, arr, copy in held:
            assert np.array_equal(arr, copy), f"the observation of step {s} changed during step {t}"
        held = [h for h in held if h[0] > t - hold] + [(t, obs, obs.copy())]
        rec = {"obs": _digest(obs), "reward": _digest(reward), "done": _digest(done), "trunc": _digest(trunc)}
        for key, val in info.items():
            if key in ("final_observation", "final_info"):
                continue
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
    # the path under test ran: every step went through agx_loop_step_host (at most hold + 1 of the 4 pool buffers are out, so
    # no step may have taken the unchunked copy)
    if chunks > 0:
        assert env._host_step.steps == STEPS, f"{env._host_step.steps} of {STEPS} steps took the chunked path"
    else:
        assert env._host_step is None
    env.close()
    return log, ends


CASES = [
    # kind, frame format, compact staging, obs dtype, N, chunks
    ("fixed", "rgb", True, "float32", 700, 3),
    ("flexible", "gray", False, "float32", 700, 4),
    ("peripheral", "gray", True, "float16", 700, 1),
    ("base", "rgb", False, "float16", 1024, 4),
    ("fixed", "gray", True, "float32", 1024, 3),
    ("flexible", "rgb", True, "float16", 1024, 1),
    ("peripheral", "rgb", False, "float32", 700, 4),
    ("base", "gray", True, "float32", 700, 3),
]


@pytest.mark.parametrize("kind,fmt,compact,dtype,N,chunks", CASES)
def test_chunked_host_step_equals_unchunked(kind, fmt, compact, dtype, N, chunks):
    want, ends0 = _run(kind, N, 0, _args(kind, fmt, compact, dtype, 0))
    got, ends1 = _run(kind, N, chunks, _args(kind, fmt, compact, dtype, chunks))
    assert ends0 == ends1 and ends0 > N // 4, f"autoreset fired for {ends0} envs only"
    assert len(want) == len(got) == STEPS + 1
    for w, g in zip(want, got):
        assert w[0] == g[0]
        if w[0] == "reset":
            assert w[1:] == g[1:], "reset differs"
            continue
        assert set(w[1]) == set(g[1]), (w[0], sorted(set(w[1]) ^ set(g[1])))
        for key in w[1]:
            assert w[1][key] == g[1][key], (f"step {w[0]}", key, w[1][key], g[1][key])


def test_pinned_pair_and_raw_crop_rows():
    """args.copy_obs = False (two pinned buffers used alternately) as the destination, and a raw-crop context whose observation
    row (4 * 31 * 29 floats) is not a multiple of 16 bytes."""
    kind, N, chunks = "fixed", 700, 4
    over = dict(copy_obs=False, fov_size=(31, 29), resize_to_full=False, mask_out=False)
    want, ends0 = _run(kind, N, 0, _args(kind, "gray", True, "float32", 0, **over), hold=1)
    got, ends1 = _run(kind, N, chunks, _args(kind, "gray", True, "float32", chunks, **over), hold=1)
    assert ends0 == ends1 > 0 and want == got


def test_option_falls_back_where_it_does_not_apply():
    """host_obs_chunks is the value IN EFFECT: 0 with device outputs, with the Python loop forced, and with packed ragged crops."""
    from active_gym import AtariVecEnv
    for over in (dict(device="cuda:0"), dict(native_loop=False), dict(resize_to_full=False, mask_out=False, ragged_obs="packed")):
        env = AtariVecEnv(_args("flexible", "gray", True, "float32", 4, **over), 8, kind="flexible")
        assert env.host_obs_chunks == 0 and env._host_step is None
        env.close()
    with pytest.raises(ValueError):
        AtariVecEnv(_args("fixed", "gray", True, "float32", -1), 8, kind="fixed")


def test_pool_budget_spent_takes_the_unchunked_copy():
    """A caller that keeps every observation exhausts the pool's pinned buffers: those calls take the unchunked copy, with the
    same results."""
    from active_gym import AtariVecEnv
    N = 700
    outs = []
    for chunks in (0, 3):
        random.seed(99)
        env = AtariVecEnv(_args("fixed", "gray", True, "float32", chunks, host_obs_buffers=2), N, kind="fixed")
        kept = [env.reset()[0]]
        for act in list(_actions("fixed", N, 5))[:5]:
            kept.append(env.step(act)[0])
        outs.append([zlib.crc32(o.tobytes()) for o in kept])
        if chunks:
            # reset() took one of the two pinned buffers, the first step the other (chunked); the four steps after found the
            # budget spent and took the unchunked copy: both paths ran
            assert env._host_step.steps == 1, env._host_step.steps
        env.close()
    assert outs[0] == outs[1]


@pytest.mark.parametrize("kind,chunks", [("flexible", 3), ("base", 8)])
def test_c_abi_step_host_equals_step_plus_copy(kind, chunks):
    """The C entry points themselves (through ctypes, no AtariVecEnv logic in between): agx_loop_step_host + agx_loop_host_wait into
    a caller-owned pinned buffer against agx_loop_step + a device-to-host copy, on two loops fed identically; the terminal rows of
    agx_loop_host_final against res->d_final_*; the device buffers hold what agx_loop_step leaves in them."""
    from active_gym import AtariVecEnv
    from active_gym.native_hostout import HostOutStep
    from active_gym.pipeline import _DT
    N = 700
    envs = []
    for _ in range(2):
        rnd = random.Random(5)
        e = AtariVecEnv(_args(kind, "gray", True, "float32", 0, device="cuda:0"), N, kind=kind, noop_fn=lambda r=rnd: r.randrange(30))
        assert e._loop is not None
        e.reset()
        envs.append(e)
    a, b = envs
    host = HostOutStep(a._loop, chunks)
    fov, flex = kind != "base", kind == "flexible"
    h_obs = [torch.full(tuple(a._obs.shape), -7.0, dtype=torch.float32).pin_memory() for _ in range(2)]
    ends = 0
    for t, act in enumerate(_actions(kind, N, 21)):
        motor = (act if kind == "base" else act["motor_action"]).astype(np.int32)
        sens = torch.from_numpy(act["sensory_action"]).to("cuda:0") if fov else None
        stype = torch.from_numpy(act["sensory_action_type"].astype(np.int32)).to("cuda:0") if flex else None
        dt = _DT[sens.dtype] if fov else 0
        h = h_obs[t & 1]
        ra = host.step(motor, sens, dt, stype, a._obs, a._loc if fov else None, a._res if flex else None, h)
        rb = b._loop.step(motor, sens, dt, stype, b._obs, b._loc if fov else None, b._res if flex else None)
        torch.cuda.synchronize()
        assert np.array_equal(h.numpy(), b._obs.cpu().numpy()), t
        assert torch.equal(a._obs, b._obs), t
        for x, y in zip(ra[:4], rb[:4]):
            assert np.array_equal(x, y), t
        k = len(rb[3])
        ends += k
        if k:
            assert np.array_equal(ra[4], rb[4].cpu().numpy()), t
            if fov:
                assert np.array_equal(ra[5], rb[5].cpu().numpy()), t
            if flex:
                assert np.array_equal(ra[6], rb[6].cpu().numpy()), t
        if fov:
            assert np.array_equal(ra[7], b._loc.cpu().numpy()) and torch.equal(a._loc, b._loc), t
        if flex:
            assert np.array_equal(ra[8], b._res.cpu().numpy()) and torch.equal(a._res, b._res), t
    assert ends > N // 4
    assert torch.equal(a.pipe.stack_u8(), b.pipe.stack_u8())
    a.close()
    b.close()
