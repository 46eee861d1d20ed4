"""GPU: rollout gather and GAE (K12) by launch geometry.  tests/test_gpu_rollout.py runs every case at N = 5 - two blocks of
k_rollout_gather (a wave per env, four per block) and seven lanes of one wave of k_slot_fold<GaeFold> (an env per thread, 64 per block) -
and at L <= 130 of AGX_ROLLOUT_LIMIT = 4096.  Here: GAE on synthetic arrays at N = 1, 63, 64, 65, 257 and every L mod 16 the short
last register set can have, L = 4096, special floats, and the advantage against its DEFINITION in float64; the gather at N = 1, 4,
9 and 257 and at L = 1000, 1024 and 4096 on tests/limit_cases.py's `deeproll` and `wide` (tests/test_limit_cases_cpu.py pins what
they hold).  Every element of every output is compared with tests/rollout_model.py EXACTLY, floats as bit patterns, in buffers
pre-filled with a sentinel."""
import ctypes
import types

import numpy as np
import pytest
import torch

import limit_cases as lc
import rollout_model as ro
from steplog_model import bits
from test_gpu_rollout import F_SENT, I_SENT, Outs, _same
from test_gpu_steplog_limits import Device

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = ctypes.c_void_p
GAE_NS = (1, 63, 64, 65, 257)
GAE_LS = (1, 15, 16, 17, 31, 32, 33, 48)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ptr(t):
    return None if t is None else P(t.data_ptr())


# ---------------------------------------------------------------------------------------------- GAE on synthetic arrays
class GaeContext:
    """agx_rollout_gae needs a history for N, the device and the error channel only: a base 12 x 12 pipeline that never steps."""

    def __init__(self, N):
        from active_gym import FrameHistory, ObsPipeline
        from active_gym import rollout as rl
        self.N = N
        self.pipe = ObsPipeline(num_envs=N, kind="base", obs_size=(12, 12), frame_stack=1, device=DEV)
        self.hist = FrameHistory(self.pipe, 1)
        self.lib = rl.lib()

    def gae(self, L, length, reward, ends, value, boot, gamma, lam):
        from active_gym import _native as nat
        adv, ret = torch.full((L, self.N), F_SENT, device=DEV), torch.full((L, self.N), F_SENT, device=DEV)
        t = [_t(length), _t(reward), _t(ends), _t(value), None if boot is None else _t(boot)]
        rc = self.lib.agx_rollout_gae(self.hist.handle, L, *[_ptr(x) for x in t], gamma, lam, _ptr(adv), _ptr(ret), self.pipe._stream())
        nat.check(rc, self.pipe._ctx)
        return adv.cpu().numpy(), ret.cpu().numpy()


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(N):
        if N not in made:
            made[N] = GaeContext(N)
        return made[N]

    yield get
    for c in made.values():
        c.pipe.close()


def _gae_equals_the_model(ctx, N, L, seed):
    """One synthetic case, every (gamma, lambda), with d_boot_value and - the BOOT bits taken out - without -> slots compared."""
    length, reward, ends, value, boot, live = lc.gae_case(N, L, seed)
    assert np.isnan(boot).any() or not ((ends & ro.BOOT) == 0).any()
    slots = 0
    for gamma, lam in ro.GAMMA_LAMBDA:
        for b, e in ((boot, ends), (None, (ends & 7).astype(np.uint8))):
            want_adv, want_ret = ro.gae_vec(length, reward, e, value, b, gamma, lam)
            adv, ret = ctx.gae(L, length, reward, e, value, b, gamma, lam)
            what = (N, L, gamma, lam, b is not None)
            assert np.isfinite(adv).all() and np.isfinite(ret).all(), what      # no NaN of a dead slot or an unused boot value came through
            assert np.array_equal(bits(adv), bits(want_adv)) and np.array_equal(bits(ret), bits(want_ret)), what
            assert not adv[~live].any() and not ret[~live].any(), what           # +0.0 in every slot that is not live: no sentinel either
            slots += 2 * L * N
    return slots


@pytest.mark.parametrize("N", GAE_NS)
def test_gae_by_blocks_and_register_sets(contexts, N):
    """N = 1, 63, 64, 65, 257: one lane, a wave short of one lane, one full block, a block and one lane, four blocks and one
    lane.  L = 1 .. 48: a short first set (1, 15), exactly one set (16), full sets and a short last one of 1, 15, 0 and 1 slots
    (17, 31, 32, 33), three full sets (48).  len random in [0, L] with -3, L + 7, 0, L and 1 among them; reward and value are NaN
    in the slots that are not live, boot is NaN wherever BOOT is unset: adv / ret equal the model bit for bit and are finite."""
    ctx = contexts(N)
    slots = sum(_gae_equals_the_model(ctx, N, L, 1000 * N + L) for L in GAE_LS)
    print(f"N = {N}: {slots} adv / ret elements compared")


def test_gae_at_the_rollout_limit(contexts):
    """L = AGX_ROLLOUT_LIMIT = 4096 at N = 65: 256 full register sets, the element number steps down from 266 239 by 65."""
    slots = _gae_equals_the_model(contexts(65), 65, ro.ROLLOUT_LIMIT, 7)
    print(f"L = 4096, N = 65: {slots} adv / ret elements compared")


@pytest.mark.parametrize("gamma, lam", ro.GAMMA_LAMBDA)
def test_advantage_against_the_definition_in_float64(contexts, gamma, lam):
    """For every live slot t of finite inputs, with g = float64(float32(gamma)), gl = g * float64(float32(lambda)), as
    include/agx_rollout.h states it and in float64 throughout (limit_cases.gae_definition; nothing from rollout_model's fold):

        adv_t = sum_{l = 0 .. c - 1} gl^l delta_(t+l),   delta_t = r_t + g nv_t - v_t,   nv_t = boot_t | 0 | v_(t+1)

    over the chain of c slots from t to the first one that breaks it (ends & 7, or t = L - 1), and

        |adv32_t - adv_t| <= (4 c + 4) 2^-24 S_t,        S_t = sum_l gl^l (|r| + |g nv| + |v|)_(t+l).

    Derivation (limit_cases.gae_bound): a term of delta_(t+l) takes at most one rounding when it is formed (the product g nv), two
    in the additions of its delta and one in the addition of the carry; each of the l slots it is then carried over multiplies
    it by fl(gamma lambda) - one rounding off g lam itself - rounds the product and rounds the next addition: 4 + 3 l <= 4 c + 4
    relative errors of at most u = 2^-24 on a term of magnitude gl^l |x|; to first order in u their sum is bounded as stated.
    ret is fl(adv + v), one operation: it is held exactly to that.  The bound is derived, not measured; the worst ratio of error
    to bound is printed.  No slot has a non-zero term below 2^-100, so none is left out."""
    worst, checked, longest = 0.0, 0, 0
    for N, L, seed in ((65, 48, 3), (257, 33, 4), (65, 4096, 7)):
        length, reward, ends, value, boot, live = lc.gae_case(N, L, seed)
        adv, ret = contexts(N).gae(L, length, reward, ends, value, boot, gamma, lam)
        want, S, chain, smallest, dlive = lc.gae_definition(length, reward, ends, value, boot, gamma, lam)
        assert np.array_equal(dlive, live) and not (smallest[live] < lc.TINY).any()
        err, bound = np.abs(adv.astype(np.float64) - want)[live], lc.gae_bound(S, chain)[live]
        assert (bound > 0).all() and (err <= bound).all(), (N, L, float((err / bound).max()))
        assert np.array_equal(bits(ret[live]), bits((adv[live] + value[live]).astype(np.float32)))
        worst, checked, longest = max(worst, float((err / bound).max())), checked + int(live.sum()), max(longest, int(chain[live].max()))
    print(f"gamma = {gamma}, lambda = {lam}: {checked} live slots checked, longest chain {longest}; worst error / bound {worst:.4f}")
    assert checked > 100_000 and longest >= 10 and worst < 1


def test_gae_special_floats(contexts):
    """N = 65, L = 33: +-0, +-2^-149, +-2^-126, +-3.4e38, +-inf, NaN and ordinary normals in reward, value and boot of the live
    slots.  Where the model's adv / ret is NaN the device's is NaN (any payload); every other element is bit-equal: subnormals are
    not flushed, signed zeros keep their sign, and the slots that are not live are +0.0 whatever was folded through them."""
    N, L = 65, 33
    length, reward, ends, value, boot, live = lc.gae_case(N, L, 1, special=True)
    seen = dict(nan=0, inf=0, subnormal=0)
    for gamma, lam in ro.GAMMA_LAMBDA:
        want = ro.gae_vec(length, reward, ends, value, boot, gamma, lam)
        got = contexts(N).gae(L, length, reward, ends, value, boot, gamma, lam)
        for g, w, name in zip(got, want, ("adv", "ret")):
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), f"{name}: NaN-ness differs from the model ({gamma}, {lam})"
            assert np.array_equal(bits(g)[~nan], bits(w)[~nan]), f"{name}: bit patterns differ from the model ({gamma}, {lam})"
            assert not nan[~live].any() and not bits(g)[~live].any()
            seen["nan"] += int(nan.sum())
            seen["inf"] += int(np.isinf(w).sum())
            seen["subnormal"] += int(((w != 0) & (np.abs(w) < 2.0 ** -126)).sum())
    print(f"special floats: {6 * L * N} elements compared; {seen}")
    assert all(v >= 1 for v in seen.values()), seen


# ---------------------------------------------------------------------------------------------- the gather
class Roll:
    """A scripted limit_cases.Deep run at the small geometry with one log (W = 4), on the device and on the models."""

    def __init__(self, name, N=None):
        _, full_N, T, _, _ = lc.DEEP[name]
        self.dev = Device(full_N if N is None else N, T, widths=(4,), special=False)
        self.d = lc.Deep(name, device=self.dev, N=N)
        self.lm = self.d.logs[4]
        self.case = types.SimpleNamespace(roll=self.dev.roll, log=self.dev.logs[4], pipe=self.dev.pipe)

    def check(self, L):
        """agx_rollout_gather into sentinel-filled outputs == rm.gather in every element -> (the model's arrays, elements)."""
        want = ro.gather(self.lm, L)
        got = Outs(L, self.d.N, 4).call(self.case).host()
        _same(got, want, f"{self.d.name}, N = {self.d.N}, L = {L}")
        assert (got["len"] != I_SENT).all() and (got["obs_index"] != I_SENT).all() and (got["next_index"] != I_SENT).all()
        assert not (got["reward"] == F_SENT).any()
        return want, sum(v.size for v in want.values())


@pytest.fixture(scope="module")
def deeproll():
    r = Roll("deeproll")
    yield r
    r.dev.pipe.close()


@pytest.mark.parametrize("N", [1, 4, 9])
def test_gather_across_waves_and_blocks(deeproll, N):
    """The first N envs of `deeproll` (N = 1: one wave of one block; 4: one full block; 9: two blocks and one wave) at L = 5, 65
    and 1024: every element of every output equals rm.gather, no sentinel survives."""
    r = deeproll if N == 9 else Roll("deeproll", N)
    compared = 0
    for L in (5, 65, 1024):
        want, n = r.check(L)
        compared += n
    assert int(want["len"].max()) > 64
    if r is not deeproll:
        r.dev.pipe.close()
    print(f"N = {N}: {compared} elements compared")


def test_gather_across_many_blocks():
    """`wide`: N = 257, T = 16, 24 steps - 65 blocks, the last one with one wave; full, partial and empty envs and every ends bit."""
    r = Roll("wide")
    compared = 0
    for L in (1, 8, 20):
        want, n = r.check(L)
        compared += n
    assert set(np.unique(want["len"])) >= {0, 1, 2} and int(want["len"][256]) >= 0
    r.dev.pipe.close()
    print(f"N = 257: {compared} elements compared")


@pytest.mark.parametrize("L", [1000, 1024, 4096])
def test_gather_depth(deeproll, L):
    """`deeproll` (N = 9, T = 1100, an env with more than 1024 live slots) at L = 1000, at L = 1024 - 16 full passes of 64 rows with the
    walk cut by L - and at L = 4096 = AGX_ROLLOUT_LIMIT, which is almost all padding: the padding loop, every element written
    exactly once (a sentinel would survive, or a live slot would be overwritten)."""
    want, n = deeproll.check(L)
    lens = want["len"]
    assert int(lens.max()) == min(L, 1026) and int(lens.min()) < 64
    if L == 4096:
        assert (want["obs_index"] == -1).mean() > 0.8
    print(f"L = {L}: {n} elements compared, len = {lens.tolist()}")


# ---------------------------------------------------------------------------------------------- refusals
def test_l_times_n_cannot_exceed_int32_max_on_a_context():
    """tests/test_gpu_rollout.py covers L = 0 and 4097, the null buffers and the null handles, in the header's order.  What is left
    of that order, L * N above INT32_MAX, cannot be reached through a context: agx_create refuses num_envs above 65535, and
    4096 * 65535 = 268 431 360 < 2^31.  So the check is held from both sides: a context of 65536 envs is refused, and at the largest
    product a context of the small kind can be asked for here, L = 4096 (the limit) is not refused for L * N but for its null
    buffer, behind L = 4097 which is refused for L.  Nothing is launched."""
    from active_gym import FrameHistory, ObsPipeline, StepLog
    from active_gym import _native as nat
    from active_gym import rollout as rl
    assert ro.ROLLOUT_LIMIT * 65535 < 2 ** 31 - 1
    with pytest.raises(nat.AgxError, match="num_envs must be in \\[1, 65535\\]"):
        ObsPipeline(num_envs=65536, kind="base", obs_size=(4, 4), frame_stack=1, device=DEV)
    N = 4096
    pipe = ObsPipeline(num_envs=N, kind="base", obs_size=(4, 4), frame_stack=1, device=DEV)
    hist = FrameHistory(pipe, 1)
    log = StepLog(hist, 0)
    lib, st = rl.lib(), pipe._stream()

    def gather(L):
        return lib.agx_rollout_gather(log._s, L, None, None, None, None, None, None, st), nat.last_error(pipe._ctx)

    def gae(L):
        return lib.agx_rollout_gae(hist.handle, L, None, None, None, None, None, 0.99, 0.95, None, None, st), nat.last_error(pipe._ctx)

    for call in (gather, gae):
        rc, msg = call(4097)
        assert rc == nat.E_INVALID and "L must be 1 .. 4096" in msg, msg
        rc, msg = call(4096)
        assert rc == nat.E_INVALID and "null buffer" in msg and "exceeds" not in msg, msg
    assert rl.check_rollout_length(4096, N) == 4096
    torch.cuda.synchronize()
    pipe.close()
