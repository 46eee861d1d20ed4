"""GPU: the V-trace kernel (K13, include/agx_vtrace.h) at the limits its header states and on special floats.
tests/test_gpu_vtrace.py holds it to tests/vtrace_model.py at N = 5 and 70 and L <= 130, on ordinary normals.  Here: N = 1, 63, 64,
65, 257 and 4097 (one lane up to 65 blocks with one lane in the last) at every set edge of depths 8 and 16; L = AGX_VTRACE_LIMIT =
4096 (512 register sets, element numbers up to 266,239); the device's own output against the paper's definition in float64;
+-0, subnormals, 3.4e38, infinities and NaN in live reward / value / boot_value / rho, against finite, infinite and subnormal
levels; the arrays agx_rollout_gather itself writes at L = 1000, 1024 and 4096; and the BehaviourLog on device tensors.  The
scenarios are tests/vtrace_limit_cases.py's (tests/test_vtrace_limits_cpu.py pins what they hold).  Every output lies between
4096 sentinel elements in front and 4096 behind, which every call must leave untouched: nothing is written outside [L][N]."""
import ctypes

import numpy as np
import pytest
import torch

import limit_cases as lc
import rollout_model as ro
import vtrace_limit_cases as vl
import vtrace_model as vm
from steplog_model import bits
from test_gpu_rollout import F_SENT, Outs
from test_gpu_rollout_launch import Roll

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = ctypes.c_void_p
F32 = np.float32
ONE = (1.0, 1.0, 1.0)
G = vl.GUARD


def _t(x):
    return torch.from_numpy(np.array(x)).to(DEV)          # (a copy: the shared cases are read-only)


def _ptr(t):
    return None if t is None else P(t.data_ptr())


class Guarded:
    """An [L, N] float32 output between G sentinel elements in front and G behind, all of it pre-filled with the sentinel."""

    def __init__(self, L, N):
        self.L, self.N = L, N
        self.buf = torch.full((2 * G + L * N,), F_SENT, device=DEV)
        self.out = self.buf[G:G + L * N].view(L, N)

    def host(self, what):
        buf = self.buf.cpu().numpy()
        assert (buf[:G] == F32(F_SENT)).all(), f"written in front of [L][N] ({what})"
        assert (buf[G + self.L * self.N:] == F32(F_SENT)).all(), f"written behind [L][N] ({what})"
        return buf[G:G + self.L * self.N].reshape(self.L, self.N)


class Context:
    """agx_vtrace_returns and agx_rollout_gae need a history for N, the device and the error channel only: a base 12 x 12 pipeline
    that never steps."""

    def __init__(self, N):
        from active_gym import FrameHistory, ObsPipeline
        from active_gym import rollout as rl
        from active_gym import vtrace as vt
        self.N = N
        self.pipe = ObsPipeline(num_envs=N, kind="base", obs_size=(12, 12), frame_stack=1, device=DEV)
        self.hist = FrameHistory(self.pipe, 1)
        self.lib, self.gae_lib = vt.lib(), rl.lib()

    def upload(self, case):
        """The device copies of one case, made once: with its boot buffer, and the ends bytes of a call without one."""
        length, reward, ends, value, boot, rho, live = case
        return dict(len=_t(length), reward=_t(reward), ends=_t(ends), bare=_t(vl.no_boot(ends)), value=_t(value), boot=_t(boot), rho=_t(rho))

    def returns(self, d, gamma, lam, bars, boot=True, value=None, rho=None):
        """-> (vs, pg_adv) on the host, from guarded outputs; boot = False: a NULL boot buffer on the ends bytes without BOOT."""
        from active_gym import _native as nat
        L = d["reward"].shape[0]
        vs, pg = Guarded(L, self.N), Guarded(L, self.N)
        a = [d["len"], d["reward"], d["ends"] if boot else d["bare"], d["value"] if value is None else value, d["boot"] if boot else None,
             d["rho"] if rho is None else rho]
        rc = self.lib.agx_vtrace_returns(self.hist.handle, L, *[_ptr(x) for x in a], gamma, lam, *bars, _ptr(vs.out), _ptr(pg.out), self.pipe._stream())
        nat.check(rc, self.pipe._ctx)
        what = (self.N, L, gamma, lam, bars, boot)
        return vs.host(what), pg.host(what)

    def gae(self, d, gamma, lam):
        from active_gym import _native as nat
        L = d["reward"].shape[0]
        adv, ret = Guarded(L, self.N), Guarded(L, self.N)
        a = [d["len"], d["reward"], d["ends"], d["value"], d["boot"]]
        rc = self.gae_lib.agx_rollout_gae(self.hist.handle, L, *[_ptr(x) for x in a], gamma, lam, _ptr(adv.out), _ptr(ret.out), self.pipe._stream())
        nat.check(rc, self.pipe._ctx)
        return adv.host("gae"), ret.host("gae")


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


def _equals_the_model(ctx, N, L, seed):
    """One case, every parameter set, with the boot buffer and with NULL on the ends bytes without BOOT: both outputs equal the
    model as int32 bits, are finite, and are +0.0 bits where the slot is not live -> elements compared."""
    case = vl.case(N, L, seed)
    boot, ends, live = case[4], case[2], case[6]
    assert np.isnan(boot).any() or (ends & ro.BOOT).all()
    d, compared = ctx.upload(case), 0
    for gamma, lam, bars in vm.PARAMS:
        for with_boot in (True, False):
            want = vl.model(N, L, seed, gamma, lam, bars, with_boot)[:2]
            got = ctx.returns(d, gamma, lam, bars, with_boot)
            for g, w, name in zip(got, want, ("vs", "pg_adv")):
                what = (name, N, L, gamma, lam, bars, with_boot)
                assert np.isfinite(g).all(), what              # no NaN of a dead slot or an unused boot value came through, no sentinel
                assert np.array_equal(bits(g), bits(w)), what
                assert not bits(g)[~live].any(), what
                compared += L * N
    return compared


# ---------------------------------------------------------------------------------------------- 1. launch geometry
@pytest.mark.parametrize("N", vl.LIMIT_NS)
def test_vtrace_by_blocks_and_register_sets(contexts, N):
    """N = 1, 63, 64, 65, 257: one lane, a wave short of one lane (the n >= N exit taken by one), a full block (not taken), a block
    and one lane, four blocks and one lane.  L = 1 .. 48: at the kernel's set depth of 8 a short only set (1, 7), exactly one set
    (8), full sets and a short last one of 1, 7, 0, 1 slots (9, 15, 16, 17), up to six sets (48); at a depth of 16 the same edges
    at 15 .. 33.  len random in [0, L] with -3, L + 7, 0, L and 1 among them and L in the last lane of the last block."""
    ctx = contexts(N)
    compared = sum(_equals_the_model(ctx, N, L, vl.limit_seed(N, L)) for L in vl.LIMIT_LS)
    print(f"N = {N}: {compared} vs / pg_adv elements compared")


def test_vtrace_across_many_blocks(contexts):
    """N = 4097: 65 blocks, the last with one lane, which folds every slot, at L = 9 and 17 (a full set and one slot, at both depths)."""
    N, Ls = vl.MANY_BLOCKS
    ctx = contexts(N)
    compared = sum(_equals_the_model(ctx, N, L, vl.limit_seed(N, L)) for L in Ls)
    print(f"N = {N}: {compared} vs / pg_adv elements compared")


def test_vtrace_at_the_rollout_limit(contexts):
    """L = AGX_VTRACE_LIMIT = 4096 at N = 65: 512 full register sets at depth 8, the element number steps down from 266,239 by
    65; every parameter set, both boot forms.  And the on-policy identity at that size: rho = 1 (and rho = 3 cut to 1) under levels
    1 gives vs equal to agx_rollout_gae's ret bit for bit, launched on the same arrays."""
    N, L, seed = vl.LIMIT_CASE
    ctx = contexts(N)
    compared = _equals_the_model(ctx, N, L, seed)
    d = ctx.upload(vl.case(N, L, seed))
    for gamma, lam in ro.GAMMA_LAMBDA + ((0.99, 1.0),):
        adv, ret = ctx.gae(d, gamma, lam)
        for ratio in (1.0, 3.0):
            vs, _ = ctx.returns(d, gamma, lam, ONE, rho=torch.full((L, N), ratio, device=DEV))
            assert np.array_equal(bits(vs), bits(ret)), (gamma, lam, ratio)
            compared += L * N
    print(f"L = {L}, N = {N}: {compared} elements compared")


# ---------------------------------------------------------------------------------------------- 2. the definition
@pytest.mark.parametrize("gamma, lam, bars", vm.PARAMS)
def test_targets_against_the_definition_in_float64(contexts, gamma, lam, bars):
    """The device's vs and pg_adv against vtrace_model.definition - the paper's explicit sum in float64, which shares nothing with the
    fold - for every live slot of (N, L) = (65, 48), (257, 33) and (65, 4096), within vtrace_model.bounds (derived from the
    operation count: a term meets at most 5 roundings in its own slot and 4 per slot it is carried over).  A = vs - value before its
    last rounding is no output of the kernel: it is held to the definition's A, within A's own bound, through a second call at
    value = 0 on the live slots, where vs = fadd(A, 0) is A itself.  No live slot has a non-zero term below 2^-100 in either call, so
    none is left out.  The worst error / bound is printed."""
    worst, checked, longest = dict(A=0.0, vs=0.0, pg_adv=0.0), 0, 0
    for N, L, seed in vl.DEFINITION_CASES:
        case = vl.case(N, L, seed)
        live = case[6]
        ctx = contexts(N)
        dev = ctx.upload(case)
        vs, pg = ctx.returns(dev, gamma, lam, bars)
        d, (bA, bvs, bpg) = vl.defined(N, L, seed, gamma, lam, bars)
        vs0, pg0 = ctx.returns(dev, gamma, lam, bars, value=_t(vl.zero_value(live)))
        d0, (bA0, _, bpg0) = vl.defined(N, L, seed, gamma, lam, bars, True)
        for dd in (d, d0):
            assert np.array_equal(dd["live"], live) and not (dd["smallest"][live] < lc.TINY).any(), (N, L)
        for name, got, want, bound in (("vs", vs, d["vs"], bvs), ("pg_adv", pg, d["pg"], bpg), ("A", vs0, d0["A"], bA0), ("pg_adv", pg0, d0["pg"], bpg0)):
            ok, ratio = vl.ratios(got, want, bound, live)
            assert ok, (name, N, L, ratio)
            worst[name] = max(worst[name], ratio)
        checked, longest = checked + int(live.sum()), max(longest, int(d["chain"][live].max()))
    print(f"gamma = {gamma}, lambda = {lam}, levels = {bars}: {checked} live slots, none left out, longest chain {longest}; worst error / "
          f"bound A {worst['A']:.3f}, vs {worst['vs']:.3f}, pg_adv {worst['pg_adv']:.3f}")
    assert checked > 100_000 and longest >= 10 and max(worst.values()) < 1


# ---------------------------------------------------------------------------------------------- 3. special floats
def test_vtrace_special_floats(contexts):
    """N = 65, L = 33: +-0, +-2^-149, +-2^-126, +-3.4e38, +-inf, NaN and ordinary normals in reward, value and boot of the live slots;
    0, -0.0, 2^-149, 2^-126, 1, 4, 3.4e38, +inf and NaN among their ratios; levels that are infinite, 1, ordinary, and 3.4e38 /
    2^-149 / 2^-126.  Where the model's vs / pg_adv is NaN the device's is NaN (any payload); every other element is bit-equal:
    subnormals are not flushed - not in the products, not in the clip -, infinities and signed zeros come out as the header's
    operations give them, and the slots that are not live are +0.0 whatever was folded through them."""
    N, L = vl.SPECIAL_NL
    case = vl.case(N, L, vl.SPECIAL_SEED, True)
    live = case[6]
    ctx = contexts(N)
    d = ctx.upload(case)
    total, compared = dict(nan=0, inf=0, subnormal=0, negzero=0), 0
    for gamma, lam, bars in vl.SPECIAL_PARAMS:
        for with_boot in (True, False):
            want = vl.model(N, L, vl.SPECIAL_SEED, gamma, lam, bars, with_boot, True)[:2]
            got = ctx.returns(d, gamma, lam, bars, with_boot)
            for g, w, name in zip(got, want, ("vs", "pg_adv")):
                what = f"{name} ({gamma}, {lam}, {bars}, boot buffer {with_boot})"
                nan = np.isnan(w)
                assert np.array_equal(np.isnan(g), nan), f"NaN-ness differs from the model: {what}"
                assert np.array_equal(bits(g)[~nan], bits(w)[~nan]), f"bit patterns differ from the model: {what}"
                assert not bits(g)[~live].any(), what
                seen = vl.kinds(g)
                assert all(v >= 1 for v in seen.values()), (what, seen)        # each kind came out of the device in this very output
                for k, v in seen.items():
                    total[k] += v
                compared += L * N
    print(f"special floats: {compared} elements compared; {total}")


# ---------------------------------------------------------------------------------------------- 4. the gather's own arrays
@pytest.fixture(scope="module")
def deeproll():
    r = Roll("deeproll")
    yield r
    r.dev.pipe.close()


@pytest.mark.parametrize("L", [1000, 1024, 4096])
def test_vtrace_on_gathered_rollouts(deeproll, L):
    """limit_cases' `deeproll` on the device (N = 9, T = 1100, one env with 1026 live slots): agx_rollout_gather at L = 1000, 1024 and
    4096, then VTrace.returns on the len, reward and ends bytes the gather wrote - padding included - with random value /
    boot_value / rho: the result equals the model on those very arrays, with and without the boot buffer.  At L = 4096 more than
    80 % of the slots are padding, and all of it comes out +0.0."""
    from active_gym import VTrace
    r, N = deeproll, deeproll.d.N
    batch = Outs(L, N, 4).call(r.case).t
    length, reward, ends = (batch[k].cpu().numpy() for k in ("len", "reward", "ends"))
    assert int(length.max()) == min(L, 1026) and int(length.min()) < 64
    live = np.arange(L)[:, None] >= L - np.clip(length, 0, L)[None, :]
    rng = np.random.default_rng(L)
    value, boot = (rng.standard_normal((L, N)).astype(F32) for _ in range(2))
    rho = rng.uniform(0.0, 4.0, (L, N)).astype(F32)
    gamma, lam, bars = 0.99, 0.95, (2.0, 0.5, 1.0)
    vt = VTrace(r.dev.logs[4])
    for b in (boot, None):
        vs, pg = Guarded(L, N), Guarded(L, N)
        vt.returns(batch, _t(value), None if b is None else _t(b), _t(rho), gamma, lam, *bars, vs_out=vs.out, pg_adv_out=pg.out)
        want = vm.vtrace(length, reward, ends, value, b, rho, gamma, lam, bars)
        for g, w, name in zip((vs.host(L), pg.host(L)), want, ("vs", "pg_adv")):
            assert np.array_equal(bits(g), bits(w)), (name, L, b is not None)
            assert not bits(g)[~live].any() and g[live].any(), (name, L)
    if L == 4096:
        assert (~live).mean() > 0.8
    print(f"L = {L}: {4 * L * N} elements compared, {int(live.sum())} live, len = {length.tolist()}")


# ---------------------------------------------------------------------------------------------- 5. the behaviour log
def test_behaviour_log_on_the_device():
    """BehaviourLog(hist, width = 3) at N = 70, T = 7 on device tensors: 40 writes, -1 at a fifth of the envs each time, so every env
    wraps its rows at least three times and the envs stand at different indices; read([L, N]) over every retained index and -1, and read([B], env) with int32 env ids that
    include out-of-range ones (they are clamped): what a dict of the rows kept in NumPy says, 0 where the index is -1."""
    from active_gym import BehaviourLog, FrameHistory, ObsPipeline
    N, T, W = 70, 7, 3
    pipe = ObsPipeline(num_envs=N, kind="base", obs_size=(12, 12), frame_stack=1, device=DEV)
    mu = BehaviourLog(FrameHistory(pipe, T), width=W)
    assert mu.values.device.type == DEV.type and tuple(mu.values.shape) == (T, N, W)
    rng = np.random.default_rng(5)
    index, rows = np.zeros(N, np.int64), {}            # rows: (env, index mod T) -> the last vector written there
    for step in range(40):
        skip = rng.random(N) < 0.2
        vals = rng.standard_normal((N, W)).astype(F32)
        mu.write(_t(np.where(skip, -1, index)), _t(vals))
        for n in np.nonzero(~skip)[0]:
            rows[(int(n), int(index[n]) % T)] = vals[n]
        index += ~skip
    assert int(index.min()) >= 3 * T and len(set(index.tolist())) > 3

    def want(n, k):
        return np.zeros(W, F32) if k < 0 else rows[(n, k % T)]

    L = T + 1
    obs_index = index[None, :] - T + np.arange(L)[:, None]          # every retained index, then a row of -1 next to the oldest retained one
    obs_index[L - 1] = np.where(np.arange(N) % 2 == 0, -1, index - T)
    got = mu.read(_t(obs_index))
    assert got.device.type == DEV.type and tuple(got.shape) == (L, N, W)
    got = got.cpu().numpy()
    for t in range(L):
        for n in range(N):
            assert np.array_equal(bits(got[t, n]), bits(want(n, int(obs_index[t, n])))), (t, n)
    B = 300
    env = rng.integers(-5, N + 5, B).astype(np.int32)
    env[:4] = (-1, N, 0, N - 1)
    clamped = np.clip(env, 0, N - 1)
    k = index[clamped] - 1 - rng.integers(0, T, B)
    k[::7] = -1
    flat = mu.read(_t(k), _t(env)).cpu().numpy()
    assert flat.shape == (B, W) and ((env < 0) | (env >= N)).sum() > 10
    for i in range(B):
        assert np.array_equal(bits(flat[i]), bits(want(int(clamped[i]), int(k[i])))), (i, int(env[i]), int(k[i]))
    torch.cuda.synchronize()
    pipe.close()
