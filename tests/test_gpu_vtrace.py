"""GPU: V-trace over a gathered rollout (include/agx_vtrace.h, K13) and the BehaviourLog.  The fold is float32 with one rounding
per operation, so every case compares every element of both outputs with tests/vtrace_model.py EXACTLY - floats as int32 bit
patterns - in buffers pre-filled with a sentinel that must not survive.  The synthetic cases are vtrace_model.case's (tests/
test_vtrace_cpu.py holds on the model alone what they are there for, and runs them through the host side of the same fold): N = 5
and N = 70 - a second workgroup with 6 live threads - at L = 1, 5, 8, 9, 16, 17, 33 and 130: at the kernel's set depth of 8 a short
set, one full register set, a full set and a short one of one slot, two full sets, two and one slot, four and one slot, many sets
(at a depth of 16, which was measured too, 16, 17 and 33 are those edges).  The kernel needs a history for N, the device and the error
channel only: a base 12 x 12 pipeline that never steps."""
import ctypes

import numpy as np
import pytest
import torch

import rollout_model as ro
import vtrace_model as vm
from steplog_model import bits
from test_gpu_rollout import F_SENT, Case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = ctypes.c_void_p
ONE = (1.0, 1.0, 1.0)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ptr(t):
    return None if t is None else P(t.data_ptr())


class Context:
    def __init__(self, N):
        from active_gym import FrameHistory, ObsPipeline
        from active_gym import rollout as rl
        from active_gym import vtrace as vt
        self.N = N
        self.pipe = ObsPipeline(num_envs=N, kind="base", obs_size=(12, 12), frame_stack=1, device=DEV)
        self.hist = FrameHistory(self.pipe, 1)
        self.lib, self.gae_lib = vt.lib(), rl.lib()

    def returns(self, L, length, reward, ends, value, boot, rho, gamma, lam, bars):
        from active_gym import _native as nat
        vs, pg = torch.full((L, self.N), F_SENT, device=DEV), torch.full((L, self.N), F_SENT, device=DEV)
        t = [_t(length), _t(reward), _t(ends), _t(value), None if boot is None else _t(boot), _t(rho)]
        rc = self.lib.agx_vtrace_returns(self.hist.handle, L, *[_ptr(x) for x in t], gamma, lam, *bars, _ptr(vs), _ptr(pg), self.pipe._stream())
        nat.check(rc, self.pipe._ctx)
        return vs.cpu().numpy(), pg.cpu().numpy()

    def gae(self, L, length, reward, ends, value, boot, gamma, lam):
        from active_gym import _native as nat
        adv, ret = torch.full((L, self.N), F_SENT, device=DEV), torch.full((L, self.N), F_SENT, device=DEV)
        t = [_t(length), _t(reward), _t(ends), _t(value), None if boot is None else _t(boot)]
        rc = self.gae_lib.agx_rollout_gae(self.hist.handle, L, *[_ptr(x) for x in t], gamma, lam, _ptr(adv), _ptr(ret), self.pipe._stream())
        nat.check(rc, self.pipe._ctx)
        return adv.cpu().numpy(), ret.cpu().numpy()


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(N):
        if N not in made:
            made[N] = Context(N)
        return made[N]

    yield get
    for c in made.values():
        c.pipe.close()


# ---------------------------------------------------------------------------------------------- 1. the fold
@pytest.mark.parametrize("N", vm.NS)
def test_vtrace_equals_the_model_bit_for_bit(contexts, N):
    """Every L, every (gamma, lambda, levels) of vtrace_model.PARAMS: rewards and values of mixed magnitude, rho in [0, 4] with exact
    0, 1 and 4, boot NaN wherever BOOT is unset, reward / value / rho NaN in every slot that is not live, len with -3, L + 7, 0, L and
    1: vs and pg_adv equal the model in every element, are finite, and are +0.0 in the slots that are not live."""
    ctx, compared = contexts(N), 0
    for L in vm.LS:
        length, reward, ends, value, boot, rho, live = vm.case(N, L, 1000 * N + L)
        assert np.isnan(boot).any() or (ends & ro.BOOT).all()
        for gamma, lam, bars in vm.PARAMS:
            want = vm.vtrace(length, reward, ends, value, boot, rho, gamma, lam, bars)
            got = ctx.returns(L, length, reward, ends, value, boot, rho, gamma, lam, bars)
            for g, w, name in zip(got, want, ("vs", "pg_adv")):
                what = (name, N, L, gamma, lam, bars)
                assert np.isfinite(g).all(), what               # no NaN of a dead slot or an unused boot value came through, no sentinel
                assert np.array_equal(bits(g), bits(w)), what
                assert not bits(g)[~live].any(), what
                compared += L * N
    print(f"N = {N}: {compared} vs / pg_adv elements compared")


@pytest.mark.parametrize("N", vm.NS)
def test_null_boot_buffer_reads_as_zero(contexts, N):
    """d_boot_value = NULL (k_slot_fold<VtraceFold, false>): the model without a boot array, on ends bytes with and without the BOOT bit."""
    ctx = contexts(N)
    for L in vm.LS:
        length, reward, ends, value, boot, rho, live = vm.case(N, L, 1000 * N + L)
        for e in (ends, (ends & 7).astype(np.uint8)):
            want = vm.vtrace(length, reward, e, value, None, rho, 0.99, 0.5, (2.0, 0.5, 1.0))
            got = ctx.returns(L, length, reward, e, value, None, rho, 0.99, 0.5, (2.0, 0.5, 1.0))
            assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want)), (N, L)


@pytest.mark.parametrize("N", vm.NS)
def test_on_policy_equals_gae_on_the_device(contexts, N):
    """rho = 1 (and rho = 3 cut to 1) under levels 1: vs is agx_rollout_gae's ret bit for bit, launched on the same arrays.  A = vs -
    value before its last rounding is no output of the kernel; it is held to GAE's adv through vs at value = 0, where vs =
    fadd(A, 0) is A itself (a -0.0 comes out as +0.0: compared as numbers there, as bits everywhere else)."""
    ctx = contexts(N)
    for L in vm.LS:
        length, reward, ends, value, boot, rho, live = vm.case(N, L, 1000 * N + L)
        for gamma, lam in ro.GAMMA_LAMBDA + ((0.99, 1.0),):
            adv, ret = ctx.gae(L, length, reward, ends, value, boot, gamma, lam)
            for ratio in (1.0, 3.0):
                vs, _ = ctx.returns(L, length, reward, ends, value, boot, np.full((L, N), ratio, np.float32), gamma, lam, ONE)
                assert np.array_equal(bits(vs), bits(ret)), (N, L, gamma, lam, ratio)
            zero = np.where(live, np.float32(0), np.float32(np.nan)).astype(np.float32)
            adv0, _ = ctx.gae(L, length, reward, ends, zero, boot, gamma, lam)
            vs0, _ = ctx.returns(L, length, reward, ends, zero, boot, np.ones((L, N), np.float32), gamma, lam, ONE)
            nz = adv0 != 0
            assert np.array_equal(vs0, adv0) and np.array_equal(bits(vs0)[nz], bits(adv0)[nz]), (N, L, gamma, lam)


def test_a_nan_ratio_at_a_live_slot_reads_as_the_level(contexts):
    ctx, N, L = contexts(70), 70, 33
    length, reward, ends, value, boot, rho, live = vm.case(N, L, 9)
    hole = live & (np.random.default_rng(9).random((L, N)) < 0.3)
    bars = (2.0, 0.5, 1.0)
    a = ctx.returns(L, length, reward, ends, value, boot, np.where(hole, np.float32(np.nan), rho).astype(np.float32), 0.99, 0.5, bars)
    b = ctx.returns(L, length, reward, ends, value, boot, np.where(hole, np.float32(7), rho).astype(np.float32), 0.99, 0.5, bars)
    assert hole.sum() > 100 and all(np.isfinite(x).all() and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 2. refusals
def test_refusals_in_the_stated_order():
    from active_gym import VTrace
    from active_gym import _native as nat
    c = Case("small")
    vt = VTrace(c.log)
    lib, st, h, N, L = vt._lib, c.pipe._stream(), c.hist.handle, c.N, 5
    f = torch.full((L, N), F_SENT, device=DEV)
    ln, en = torch.zeros((N,), dtype=torch.int32, device=DEV), torch.zeros((L, N), dtype=torch.uint8, device=DEV)
    nan, inf = float("nan"), float("inf")

    def call(hist=h, L=L, length=ln, reward=f, ends=en, value=f, rho=f, bars=ONE, vs=f, pg=f):
        return lib.agx_vtrace_returns(hist, L, _ptr(length), _ptr(reward), _ptr(ends), _ptr(value), None, _ptr(rho), 0.99, 1.0, *bars, _ptr(vs), _ptr(pg), st)

    cases = [
        (dict(hist=None, L=0, value=None, bars=(0.0, 1.0, 1.0)), "null argument (h)", False),
        (dict(L=0, value=None, bars=(0.0, 1.0, 1.0)), "L must be 1 .. 4096", True), (dict(L=4097, bars=(nan, 1.0, 1.0)), "L must be 1 .. 4096", True),
        (dict(length=None, bars=(1.0, -1.0, 1.0)), "null buffer (d_len)", True), (dict(reward=None), "null buffer (d_reward)", True),
        (dict(ends=None), "null buffer (d_ends)", True), (dict(value=None), "null buffer (d_value)", True),
        (dict(rho=None, bars=(1.0, 1.0, 0.0)), "null buffer (d_rho)", True), (dict(vs=None), "null buffer (d_vs)", True),
        (dict(pg=None), "null buffer (d_pg_adv)", True),
        (dict(bars=(0.0, 1.0, 1.0)), "rho_bar must be > 0", True), (dict(bars=(nan, 1.0, 1.0)), "rho_bar must be > 0", True),
        (dict(bars=(1.0, -2.0, 0.0)), "c_bar must be > 0", True), (dict(bars=(inf, inf, -inf)), "pg_rho_bar must be > 0", True),
        (dict(bars=(1.0, 1.0, nan)), "pg_rho_bar must be > 0", True),
    ]
    for kw, named, has_ctx in cases:
        assert call(**kw) == nat.E_INVALID, kw
        msg = nat.last_error(c.pipe._ctx if has_ctx else None)
        assert named in msg and "agx_vtrace_returns" in msg, (kw, msg)
    torch.cuda.synchronize()
    assert bool((f == F_SENT).all())               # no refused call launched anything
    assert call(bars=(inf, inf, inf)) == nat.OK    # +inf is legal: no clipping
    batch = c.roll.gather(L)
    value = torch.zeros((L, N), device=DEV)
    for bad in ({"rho_bar": 0.0}, {"c_bar": nan}, {"pg_rho_bar": -1.0}):
        with pytest.raises(ValueError, match="must be > 0"):
            vt.returns(batch, value, value, value, **bad)
    with pytest.raises(ValueError, match="rho must have shape"):
        vt.returns(batch, value, value, value[:2])
    with pytest.raises(TypeError, match="value must be torch.float32"):
        vt.returns(batch, value.double(), value, value)
    # a narrowed env range: AGX_E_STATE, behind the argument checks
    c.pipe.env_range(1, 2)
    with pytest.raises(nat.AgxError, match="env range") as e:
        vt.returns(batch, value, value, value)
    assert e.value.code == nat.E_STATE
    assert call(bars=(0.0, 1.0, 1.0)) == nat.E_INVALID
    c.pipe.env_range()
    vt.returns(batch, value, None, value)
    torch.cuda.synchronize()
    c.hist.close()
    with pytest.raises(RuntimeError, match="closed"):
        vt.returns(batch, value, value, value)
    c.close()


# ---------------------------------------------------------------------------------------------- 3. a captured graph
def test_captured_graph_of_gather_and_vtrace():
    """gather + BehaviourLog.read + exp + returns captured under torch.cuda.graph on one side stream: after further steps every
    replay equals the eager calls and the model, in outputs that were overwritten in between."""
    from active_gym import BehaviourLog, VTrace
    c = Case("small")
    vt, mu = VTrace(c.log), BehaviourLog(c.hist)
    L, bars = 5, (2.0, 0.5, 1.0)
    mu.values.copy_(torch.rand(mu.values.shape, device=DEV) - 0.5)
    value, boot, logp = (torch.randn((L, c.N), device=DEV) for _ in range(3))
    out = c.roll.gather(L)
    rho = torch.empty((L, c.N), device=DEV)
    vs, pg = vt.returns(out, value, boot, torch.ones((L, c.N), device=DEV), 0.99, 0.95, *bars)

    def work():
        c.roll.gather(L, out=out)
        torch.exp(logp - mu.read(out["obs_index"])[..., 0], out=rho)
        vt.returns(out, value, boot, rho, 0.99, 0.95, *bars, vs_out=vs, pg_adv_out=pg)

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
        for t in (*out.values(), rho, vs, pg):
            t.fill_(1)                            # nothing of the replay before may pass for this one's
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = ro.gather(c.lm, L)
        assert np.array_equal(out["obs_index"].cpu().numpy(), want["obs_index"]) and np.array_equal(out["ends"].cpu().numpy(), want["ends"])
        got_rho = rho.cpu().numpy()
        wv, wp = vm.vtrace(want["len"], want["reward"], want["ends"], value.cpu().numpy(), boot.cpu().numpy(), got_rho, 0.99, 0.95, bars)
        assert np.array_equal(bits(vs.cpu().numpy()), bits(wv)) and np.array_equal(bits(pg.cpu().numpy()), bits(wp)), call
        eager = c.roll.gather(L)
        erho = torch.exp(logp - mu.read(eager["obs_index"])[..., 0])
        ev, ep = vt.returns(eager, value, boot, erho, 0.99, 0.95, *bars)
        assert torch.equal(rho.view(torch.int32), erho.view(torch.int32))
        assert torch.equal(vs.view(torch.int32), ev.view(torch.int32)) and torch.equal(pg.view(torch.int32), ep.view(torch.int32))
        seen.add(tuple(want["obs_index"].reshape(-1).tolist()))
    assert len(seen) == 3                         # the replays saw three different histories
    c.close()


# ---------------------------------------------------------------------------------------------- 4. the vector env
def _vec_env(native_loop, N):
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(12, 12), frame_stack=3, fov_size=(3, 5), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=30, native_loop=native_loop, history_len=16, step_log=True)
    return AtariVecEnv(AtariEnvArgs(**kw), N, kind="fixed", noop_fn=lambda: 2)


@pytest.mark.parametrize("native", [True, False], ids=["native_loop", "python_loop"])
def test_vec_env_behaviour_log_and_vtrace(native):
    """AtariVecEnv(history_len = 16, step_log = True), N = 5 at 12 x 12 / 3 x 5, fs = 3 (the small geometry of the rollout tests is
    10 x 12, which an Atari env refuses: its observation is square, as the reference's is), 40 random steps across autoresets.  At
    every act BehaviourLog.write(info["history_index"], value) with a value that encodes (env, step); after rollout_batch(12),
    read(obs_index) is exactly the value written when the policy acted on that observation at every live slot - found again
    through the index the env reported then - and 0 at padding; rollout_vtrace equals the model, and with rho = 1 its vs equals
    rollout_gae's ret."""
    N, STEPS, L = 5, 40, 12
    env = _vec_env(native, N)
    assert (env._loop is not None) == native and env.steplog is not None
    mu = env.behaviour_log()
    assert env.behaviour_log() is mu and env.behaviour_log(2) is not mu and tuple(mu.values.shape) == (16, N, 1)
    obs, info = env.reset()
    rng = np.random.default_rng(0)
    acted = {}                                     # (env, index of the observation acted on) -> the value written
    for step in range(STEPS):
        index = info["history_index"]
        code = (torch.arange(N, device=DEV, dtype=torch.float32) * 1000 + step + 1)[:, None]
        mu.write(index, code)
        for n, k in enumerate(index.cpu().numpy()):
            acted[(n, int(k))] = float(n * 1000 + step + 1)
        act = {"motor_action": rng.integers(0, 4, N), "sensory_action": rng.uniform(-3, 14, (N, 2)).astype(np.float32)}
        obs, reward, done, _, info = env.step(act)
    batch = env.rollout_batch(L)
    got = mu.read(batch["obs_index"])
    assert tuple(got.shape) == (L, N, 1) and got.dtype == torch.float32
    got, oi, live, ends = got[..., 0].cpu().numpy(), batch["obs_index"].cpu().numpy(), batch["live"].cpu().numpy(), batch["ends"].cpu().numpy()
    assert live.sum() >= 3 * N and (ends[live] & 1).any(), "no terminal step in the rollouts: lengthen the run"
    for t in range(L):
        for n in range(N):
            assert got[t, n] == (acted[(n, int(oi[t, n]))] if live[t, n] else 0.0), (t, n, int(oi[t, n]))
    flat_t, flat_n = np.nonzero(live)
    flat = mu.read(batch["obs_index"][batch["live"]], torch.from_numpy(flat_n.astype(np.int32)).to(DEV))
    assert np.array_equal(flat[:, 0].cpu().numpy(), got[flat_t, flat_n])
    # the fold through the env
    value, boot = (torch.randn((L, N), device=DEV) for _ in range(2))
    rho = torch.rand((L, N), device=DEV) * 4
    bars = (2.0, 0.5, 1.0)
    vs, pg = env.rollout_vtrace(batch, value, boot, rho, 0.99, 0.95, *bars)
    wv, wp = vm.vtrace(batch["len"].cpu().numpy(), batch["reward"].cpu().numpy(), ends, value.cpu().numpy(), boot.cpu().numpy(), rho.cpu().numpy(),
                       0.99, 0.95, bars)
    assert np.array_equal(bits(vs.cpu().numpy()), bits(wv)) and np.array_equal(bits(pg.cpu().numpy()), bits(wp))
    vs1, _ = env.rollout_vtrace(batch, value, boot, torch.ones_like(rho), 0.99, 0.95)
    _, ret = env.rollout_gae(batch, value, boot, 0.99, 0.95)
    assert torch.equal(vs1.view(torch.int32), ret.view(torch.int32))
    torch.cuda.synchronize()
    env.close()
