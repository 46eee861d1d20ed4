"""GPU: on-policy rollouts (include/agx_rollout.h) through ObsPipeline + FrameHistory + StepLog + Rollout.  Which rows a rollout
holds is a pure function of the history's bookkeeping and of what was recorded, and the GAE fold is float32 with one rounding per
operation, so every case compares every element of every output with tests/rollout_model.py EXACTLY - floats as int32 bit
patterns - in buffers pre-filled with a sentinel that must not survive.  The scripted scenarios and their seeds are
tests/rollout_model.py's; tests/test_rollout_cpu.py checks on the model alone that they hold what the cases are there for.
N = 5 envs at the small geometry (10 x 12, fovea 3 x 5, fs = 3), T = 16, and T = 160 for the rollouts longer than a wave: the
gather walks 64 rows per pass, so L = 64 and 65 sit on that edge."""
import ctypes

import numpy as np
import pytest
import torch

import rollout_model as rm
from steplog_model import TERMINATED, bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = ctypes.c_void_p
OBS, FOV = (10, 12), (3, 5)
F_SENT, B_SENT, I_SENT = -7.5, 0xAB, -9     # exact in float32 and no reward here; no ends byte; no index and no length


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ptr(t):
    return None if t is None else P(t.data_ptr())


class Case:
    """A pipeline with a history, a step log and a Rollout on it, driven over a scripted scenario next to the models."""

    def __init__(self, name):
        from active_gym import FrameHistory, ObsPipeline, Rollout, StepLog
        self.seed, N, fs, T, _, self.Ls, _, _ = rm.CASES[name]
        self.pipe = ObsPipeline(num_envs=N, kind="fixed", obs_size=OBS, frame_stack=fs, device=DEV, fov_size=FOV, fov_init_loc=(2, 3),
                                sensory_action_mode="absolute", antialias=True, resize_to_full=True, mask_out=False)
        self.hist = FrameHistory(self.pipe, T)
        self.log = StepLog(self.hist, rm.W)
        self.roll = Rollout(self.log)
        self.N, self.fs, self.T = N, fs, T
        self.rng = np.random.default_rng(self.seed + 2000)
        _, self.hm, self.lm = rm.case_models(name, push=self.push)

    def push(self, cmd, idx, rec):
        """What rm.play does to the models, on the device: a clear (cmd is None), or ingest / fovea / push and the record."""
        if cmd is None:
            self.hist.clear()
            return
        N = self.N
        self.pipe.ingest_gray(_t(self.rng.integers(0, 256, (N, 2) + OBS, dtype=np.uint8)), _t(cmd))
        self.pipe.fovea(_t(self.rng.uniform(-3, 14, (N, 2)).astype(np.float32)))
        got = self.hist.push(_t(cmd)).cpu().numpy()
        assert np.array_equal(got, idx), "indices differ from the model"
        if rec is not None:
            index, reward, flags, payload = rec
            self.log.record(_t(index), _t(reward), _t(flags), _t(payload))

    def more(self, steps, seed):
        """Further scripted steps on the same history and models."""
        kind = rm.scenario(seed, self.N, steps + 1)[1:]
        rm.play(kind, self.fs, self.T, rm.W, seed, push=self.push, models=(self.hm, self.lm))

    def close(self):
        self.pipe.close()


@pytest.fixture(scope="module", params=sorted(rm.CASES))
def case(request):
    c = Case(request.param)
    yield c
    c.close()


class Outs:
    """The six outputs of agx_rollout_gather, filled with sentinels; call() runs the C entry point on them."""

    def __init__(self, L, N, W):
        self.L, self.W = L, W
        self.t = dict(len=torch.full((N,), I_SENT, dtype=torch.int32, device=DEV), obs_index=torch.full((L, N), I_SENT, dtype=torch.int64, device=DEV),
                      next_index=torch.full((L, N), I_SENT, dtype=torch.int64, device=DEV), reward=torch.full((L, N), F_SENT, device=DEV),
                      ends=torch.full((L, N), B_SENT, dtype=torch.uint8, device=DEV), payload=torch.full((L, N, W), B_SENT, dtype=torch.uint8, device=DEV))

    def call(self, c, log=None, keys=("len", "obs_index", "next_index", "reward", "ends", "payload")):
        from active_gym import _native as nat
        t = self.t
        a = [_ptr(t[k]) if k in keys else None for k in ("len", "obs_index", "next_index", "reward", "ends", "payload")]
        rc = c.roll._lib.agx_rollout_gather((log or c.log)._s, self.L, *a, c.pipe._stream())
        nat.check(rc, c.pipe._ctx)
        return self

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def _same(got, want, what, keys=("len", "obs_index", "next_index", "ends", "payload", "reward")):
    for key in keys:
        a, b = (got[key].view(np.int32), want[key].view(np.int32)) if key == "reward" else (got[key], want[key])
        assert np.array_equal(a, b), f"{key} differs from the model ({what})"


# ---------------------------------------------------------------------------------------------- 1. the gather
def test_gather_equals_the_model_in_every_element(case):
    c = case
    for L in c.Ls:
        want = rm.gather(c.lm, L)
        _same(Outs(L, c.N, rm.W).call(c).host(), want, f"L = {L}")
        got = c.roll.gather(L)                    # the Python surface: the same arrays and the live mask
        _same({k: v.cpu().numpy() for k, v in got.items()}, want, f"Rollout.gather, L = {L}")
        live = np.arange(L)[:, None] >= L - want["len"][None, :]
        assert got["live"].dtype == torch.bool and np.array_equal(got["live"].cpu().numpy(), live)
        assert np.array_equal(want["obs_index"] >= 0, live)
        env, index = c.roll.flat(got)
        tt, nn = np.nonzero(live)
        assert np.array_equal(env.cpu().numpy(), nn.astype(np.int32)) and np.array_equal(index.cpu().numpy(), want["obs_index"][tt, nn])
        env, index = c.roll.flat(got, "next")
        assert np.array_equal(index.cpu().numpy(), want["next_index"][tt, nn])
        at, env, index = c.roll.boot_rows(got)
        bt, bn = np.nonzero(want["ends"] & rm.BOOT)
        assert np.array_equal(at.cpu().numpy(), np.stack([bt, bn], 1)) and np.array_equal(env.cpu().numpy(), bn.astype(np.int32))
        assert np.array_equal(index.cpu().numpy(), want["next_index"][bt, bn]) and len(bt) >= 1
        _, _, valid = c.hist.observe(*c.roll.flat(got))          # every live observation and next observation can be re-created
        _, _, valid2 = c.hist.observe(*c.roll.flat(got, "next"))
        assert bool(valid.all()) and bool(valid2.all())


def test_null_outputs_and_a_log_without_payload(case):
    """Every output but d_obs_index may be NULL and is then left alone; a log without payload bytes ignores d_payload."""
    from active_gym import StepLog
    c = case
    L = c.Ls[-1]
    want = rm.gather(c.lm, L)
    got = Outs(L, c.N, rm.W).call(c, keys=("obs_index",)).host()
    _same(got, want, "obs_index alone", keys=("obs_index",))
    assert (got["len"] == I_SENT).all() and (got["next_index"] == I_SENT).all() and (got["ends"] == B_SENT).all() and (got["payload"] == B_SENT).all()
    log0 = StepLog(c.hist, 0)                     # nothing was recorded in it: every env stops at its newest row
    got = Outs(L, c.N, rm.W).call(c, log=log0).host()
    assert not got["len"].any() and (got["obs_index"] == -1).all() and (got["next_index"] == -1).all() and not got["ends"].any()
    assert not got["reward"].any() and (got["payload"] == B_SENT).all()


# ---------------------------------------------------------------------------------------------- 2, 3. GAE
def _raw_gae(c, L, length, reward, ends, value, boot, gamma, lam):
    from active_gym import _native as nat
    adv, ret = torch.full((L, c.N), F_SENT, device=DEV), torch.full((L, c.N), F_SENT, device=DEV)
    t = [_t(length), _t(reward), _t(ends), _t(value), None if boot is None else _t(boot)]
    rc = c.roll._lib.agx_rollout_gae(c.hist.handle, L, *[_ptr(x) for x in t], gamma, lam, _ptr(adv), _ptr(ret), c.pipe._stream())
    nat.check(rc, c.pipe._ctx)
    return adv.cpu().numpy(), ret.cpu().numpy()


def test_gae_equals_the_model_bit_for_bit(case):
    """Random-normal values, boot values and rewards of mixed magnitude; the boot values are NaN wherever BOOT is not set, so a
    finite output proves that they are used only there."""
    c = case
    for L in c.Ls:
        want = rm.gather(c.lm, L)
        value, boot = rm.gae_inputs(want, L)
        assert np.isnan(boot).any() and np.isfinite(boot[(want["ends"] & rm.BOOT) != 0]).all()
        for gamma, lam in rm.GAMMA_LAMBDA:
            adv, ret = rm.gae(want["len"], want["reward"], want["ends"], value, boot, gamma, lam)
            ga, gr = _raw_gae(c, L, want["len"], want["reward"], want["ends"], value, boot, gamma, lam)
            assert np.isfinite(ga).all() and np.isfinite(gr).all(), (L, gamma, lam)
            assert np.array_equal(bits(ga), bits(adv)) and np.array_equal(bits(gr), bits(ret)), (L, gamma, lam)
            live = np.arange(L)[:, None] >= L - want["len"][None, :]
            assert not ga[~live].any() and not gr[~live].any()
        # the Python surface on the gathered batch
        batch = c.roll.gather(L)
        pa, pr = c.roll.gae(batch, _t(value), _t(boot), 0.99, 0.95)
        adv, ret = rm.gae(want["len"], want["reward"], want["ends"], value, boot, 0.99, 0.95)
        assert np.array_equal(bits(pa.cpu().numpy()), bits(adv)) and np.array_equal(bits(pr.cpu().numpy()), bits(ret))


def test_gae_without_a_boot_buffer(case):
    """d_boot_value = NULL for a caller that passes no row with BOOT: the ends bytes with that bit taken out."""
    c = case
    L = c.Ls[-1]
    want = rm.gather(c.lm, L)
    ends = (want["ends"] & 7).astype(np.uint8)
    value, _ = rm.gae_inputs(want, 5)
    adv, ret = rm.gae(want["len"], want["reward"], ends, value, None, 0.99, 0.95)
    ga, gr = _raw_gae(c, L, want["len"], want["reward"], ends, value, None, 0.99, 0.95)
    assert np.array_equal(bits(ga), bits(adv)) and np.array_equal(bits(gr), bits(ret))
    got = c.roll.gae({"len": _t(want["len"]), "reward": _t(want["reward"]), "ends": _t(ends)}, _t(value), None)
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(adv))
    # a length outside 0 .. L is clamped
    wild = np.array([-3, L + 7, 0, L, 1][:c.N], np.int32)
    adv, ret = rm.gae(wild, want["reward"], ends, value, None, 0.99, 0.95)
    ga, gr = _raw_gae(c, L, wild, want["reward"], ends, value, None, 0.99, 0.95)
    assert np.array_equal(bits(ga), bits(adv)) and np.array_equal(bits(gr), bits(ret))


# ---------------------------------------------------------------------------------------------- 5. a captured graph
def test_captured_graph_of_gather_and_gae():
    """gather + gae captured under torch.cuda.graph on one side stream: after further steps every replay equals the eager calls
    and the model, in outputs that were overwritten in between."""
    c = Case("small")
    L = 5
    value, boot = (torch.randn((L, c.N), device=DEV) for _ in range(2))
    out = c.roll.gather(L)
    adv, ret = c.roll.gae(out, value, boot, 0.99, 0.95)

    def work():
        c.roll.gather(L, out=out)
        c.roll.gae(out, value, boot, 0.99, 0.95, adv_out=adv, ret_out=ret)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        work()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        work()
    seen = set()
    for call in (1, 2, 3):
        c.more(4, 50 + call)
        for t in (*out.values(), adv, ret):
            t.fill_(1)                            # nothing of the replay before may pass for this one's
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = rm.gather(c.lm, L)
        _same({k: v.cpu().numpy() for k, v in out.items()}, want, f"replay {call}")
        assert np.array_equal(out["live"].cpu().numpy(), want["obs_index"] >= 0)
        wa, wr = rm.gae(want["len"], want["reward"], want["ends"], value.cpu().numpy(), boot.cpu().numpy(), 0.99, 0.95)
        assert np.array_equal(bits(adv.cpu().numpy()), bits(wa)) and np.array_equal(bits(ret.cpu().numpy()), bits(wr)), call
        eager = c.roll.gather(L)
        ea, er = c.roll.gae(eager, value, boot, 0.99, 0.95)
        assert all(torch.equal(out[k], eager[k]) for k in eager) and torch.equal(adv.view(torch.int32), ea.view(torch.int32))
        assert torch.equal(ret.view(torch.int32), er.view(torch.int32))
        seen.add(tuple(want["obs_index"].reshape(-1).tolist()))
    assert len(seen) == 3                         # the replays saw three different histories
    c.close()


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_in_the_stated_order():
    from active_gym import _native as nat
    c = Case("small")
    lib, st, h, s, N = c.roll._lib, c.pipe._stream(), c.hist.handle, c.log._s, c.N
    L = 5
    o = Outs(L, N, rm.W).t
    f = torch.zeros((L, N), device=DEV)

    def gather(log=s, L=L, obs=o["obs_index"]):
        return lib.agx_rollout_gather(log, L, _ptr(o["len"]), _ptr(obs), None, None, None, None, st)

    def gae(hist=h, L=L, length=o["len"], reward=f, ends=o["ends"], value=f, adv=f, ret=f):
        return lib.agx_rollout_gae(hist, L, _ptr(length), _ptr(reward), _ptr(ends), _ptr(value), None, 0.99, 0.95, _ptr(adv), _ptr(ret), st)

    cases = [
        (gather, dict(L=0), "L must be 1 .. 4096", True), (gather, dict(L=4097), "L must be 1 .. 4096", True),
        (gather, dict(L=0, obs=None), "L must be 1 .. 4096", True),                   # L comes before the buffer
        (gather, dict(obs=None), "null buffer (d_obs_index)", True),
        (gather, dict(log=None), "null argument (log)", False), (gather, dict(log=None, L=0, obs=None), "null argument (log)", False),
        (gae, dict(L=0), "L must be 1 .. 4096", True), (gae, dict(L=4097, value=None), "L must be 1 .. 4096", True),
        (gae, dict(length=None), "null buffer (d_len)", True), (gae, dict(reward=None), "null buffer (d_reward)", True),
        (gae, dict(ends=None), "null buffer (d_ends)", True), (gae, dict(value=None), "null buffer (d_value)", True),
        (gae, dict(adv=None), "null buffer (d_adv)", True), (gae, dict(ret=None), "null buffer (d_ret)", True),
        (gae, dict(hist=None, L=0, value=None), "null argument (h)", False),
    ]
    for call, kw, named, has_ctx in cases:
        assert call(**kw) == nat.E_INVALID, (call.__name__, kw)
        msg = nat.last_error(c.pipe._ctx if has_ctx else None)
        assert named in msg and "agx_rollout_" + call.__name__ in msg, (call.__name__, kw, msg)
    assert (o["obs_index"] == I_SENT).all()       # no refused call launched anything
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="L must be"):
            c.roll.gather(bad)
    # a narrowed env range: AGX_E_STATE from both
    batch = c.roll.gather(L)
    c.pipe.env_range(1, 2)
    for call in (lambda: c.roll.gather(L), lambda: c.roll.gae(batch, f, f)):
        with pytest.raises(nat.AgxError, match="env range") as e:
            call()
        assert e.value.code == nat.E_STATE
    c.pipe.env_range()
    assert torch.equal(c.roll.gather(L)["obs_index"], batch["obs_index"])
    torch.cuda.synchronize()
    c.hist.close()
    with pytest.raises(RuntimeError, match="closed"):
        c.roll.gather(L)
    c.close()


# ---------------------------------------------------------------------------------------------- 4. the vector env
def _vec_env(native_loop):
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=30, native_loop=native_loop, history_len=16, step_log=True)
    return AtariVecEnv(AtariEnvArgs(**kw), 6, kind="fixed", noop_fn=lambda: 2)


@pytest.mark.parametrize("native", [True, False], ids=["native_loop", "python_loop"])
def test_vec_env_rollout_batch(native):
    """AtariVecEnv(history_len = 16, step_log = True) with the synthetic frame source, 40 random steps with autoresets, then
    rollout_batch(12): history.observe at every live slot's obs_index and next_index is bit for bit the observation the steps
    returned - at a TERMINATED slot next_index is the terminal observation the step handed out as final_observation, never the
    reset observation - the slot carries the reward and the actions of the step between the two, slots chain except across resets,
    and rollout_gae equals the model's fold."""
    from active_gym import Rollout
    N, STEPS, L = 6, 40, 12
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
    batch = env.rollout_batch(L)
    keys = ["len", "obs_index", "next_index", "reward", "ends", "live", "motor_action", "sensory_action"]
    assert sorted(batch) == sorted(keys)
    assert tuple(batch["motor_action"].shape) == (L, N) and batch["motor_action"].dtype == torch.int32
    assert tuple(batch["sensory_action"].shape) == (L, N, 2) and batch["sensory_action"].dtype == torch.float32
    roll = Rollout(env.steplog)
    length, oi, ni, ends, motor = (batch[k].cpu().numpy() for k in ("len", "obs_index", "next_index", "ends", "motor_action"))
    rew, sens = batch["reward"].cpu().numpy().view(np.int32), batch["sensory_action"].cpu().numpy().view(np.int32)
    live = batch["live"].cpu().numpy()
    assert np.array_equal(live, np.arange(L)[:, None] >= L - length[None, :]) and (length >= 1).all()
    terminated = chained = 0
    for which, index in (("obs", oi), ("next", ni)):
        e, k = roll.flat(batch, which)
        got, _, valid = env.history.observe(e, k)
        assert bool(valid.all())
        e, k = e.cpu().numpy(), k.cpu().numpy()
        for row, (t, n) in enumerate(zip(*np.nonzero(live))):
            assert int(k[row]) == index[t, n] and int(e[row]) == n
            assert torch.equal(got[row].view(torch.int32), rec[(n, int(index[t, n]))].view(torch.int32)), (which, t, n, int(index[t, n]))
    for n in range(N):
        newest = int(count[n]) - 1 - ((n, int(count[n]) - 1) in resets)
        assert ni[L - 1, n] == newest, "the newest slot is the newest step"
        for t in range(L):
            if not live[t, n]:
                assert oi[t, n] == -1 and ni[t, n] == -1 and rew[t, n] == 0 and ends[t, n] == 0 and motor[t, n] == 0 and not sens[t, n].any()
                continue
            a, b = int(oi[t, n]), int(ni[t, n])
            m, s, r, done = produced[(n, b)]
            assert a == b - 1 and (n, b) not in resets, "next_index is never a reset observation"
            assert rew[t, n] == bits(r) and motor[t, n] == m and np.array_equal(sens[t, n], s.view(np.int32)), (t, n)
            assert bool(ends[t, n] & TERMINATED) == done and not ends[t, n] & (rm.CUT | 2)
            assert bool(ends[t, n] & rm.BOOT) == (t == L - 1 and not done)
            terminated += done
            if t < L - 1:
                if done:
                    assert (n, b + 1) in resets and oi[t + 1, n] == b + 1, "behind a terminal step the next slot starts at the reset observation"
                else:
                    assert oi[t + 1, n] == b
                    chained += 1
    print(f"len = {length.tolist()}, terminated slots = {terminated}, chained = {chained}")
    assert terminated >= 1, "no terminal step in the rollouts: lengthen the run"
    assert chained >= N
    value, boot = (torch.randn((L, N), device=DEV) for _ in range(2))
    adv, ret = env.rollout_gae(batch, value, boot, 0.99, 0.95)
    wa, wr = rm.gae(length, batch["reward"].cpu().numpy(), ends, value.cpu().numpy(), boot.cpu().numpy(), 0.99, 0.95)
    assert np.array_equal(bits(adv.cpu().numpy()), bits(wa)) and np.array_equal(bits(ret.cpu().numpy()), bits(wr))
    at, be, bk = roll.boot_rows(batch)
    assert len(at) == int((ends & rm.BOOT != 0).sum()) and bool(env.history.observe(be, bk)[2].all())
    torch.cuda.synchronize()
    env.close()
