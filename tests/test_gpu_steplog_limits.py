"""GPU: the step log's gather (K8) and the gather half of sequence replay (K11) at AGX_STEPLOG_NSTEP_LIMIT = 64 and
AGX_STEPLOG_PAYLOAD_LIMIT = 64, on tests/limit_cases.py's `deepfold` (tests/test_limit_cases_cpu.py pins what it holds): folds of
exactly 64 rows, every stop reason below that, a wave that holds a 64-row fold next to a 0-row one, payloads of 4 and 64 bytes,
rewards that are subnormal, infinite, NaN and negative zero - and the n-step return against its DEFINITION in float64, which
shares nothing with tests/steplog_model.py.  One scripted run (a module fixture) serves every test: the small geometry 10 x 12 /
3 x 5, fs = 3, N = 5, T = 160, 200 steps, three logs on one history."""
import ctypes
import types

import numpy as np
import pytest
import torch

import limit_cases as lc
import rollout_model as ro
import sequence_model as qm
import steplog_model as sm
from test_gpu_rollout import Outs as RolloutOuts
from test_gpu_rollout import _same as _same_rollout
from test_gpu_steplog import B_SENT, F_SENT, Outs, _expected, _same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = ctypes.c_void_p
GAMMA = 0.99
SEQ_W = 4                             # the log the sequences are gathered from


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pair(samples):
    return _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))


class Device:
    """What limit_cases.Deep does to the models, on the device: ingest / fovea / push, and a record into every log."""

    def __init__(self, N, T, widths=lc.WIDTHS, special=True):
        from active_gym import FrameHistory, ObsPipeline, Rollout, SequenceReplay, StepLog
        self.pipe = ObsPipeline(num_envs=N, kind="fixed", obs_size=lc.OBS, frame_stack=lc.FS, device=DEV, fov_size=lc.FOV, fov_init_loc=(2, 3),
                                sensory_action_mode="absolute", antialias=True, resize_to_full=True, mask_out=False)
        self.hist = FrameHistory(self.pipe, T)
        self.logs = {W: StepLog(self.hist, W) for W in widths}
        self.special = StepLog(self.hist, 0) if special else None
        self.seq = SequenceReplay(self.logs[SEQ_W])
        self.roll = Rollout(self.logs[SEQ_W])
        self.N = N
        self.rng = np.random.default_rng(2000)

    def push(self, cmd, idx):
        N = self.N
        self.pipe.ingest_gray(_t(self.rng.integers(0, 256, (N, 2) + lc.OBS, dtype=np.uint8)), _t(cmd))
        self.pipe.fovea(_t(self.rng.uniform(-3, 14, (N, 2)).astype(np.float32)))
        assert np.array_equal(self.hist.push(_t(cmd)).cpu().numpy(), idx), "indices differ from the model"

    def record(self, index, reward, flags, payload, special):
        index, reward, flags, payload = _t(index), _t(reward), _t(flags), _t(payload)
        for W, log in self.logs.items():
            log.record(index, reward, flags, payload[:, :W].contiguous())
        if self.special is not None:
            self.special.record(index, _t(special), flags)


@pytest.fixture(scope="module")
def run():
    _, N, T, _, _ = lc.DEEP["deepfold"]
    dev = Device(N, T)
    d = lc.Deep("deepfold", device=dev)
    samples = d.samples()
    yield types.SimpleNamespace(dev=dev, d=d, samples=samples, pair=_pair(samples), cache={})
    dev.pipe.close()


def _gathered(run, log, W, nstep, gamma):
    """agx_steplog_gather over every sample into sentinel-filled outputs -> host arrays (ret / discount as int32 patterns)."""
    outs = Outs(len(run.samples), W)
    outs.call(log, *run.pair, nstep, gamma)
    return outs.host()


# ---------------------------------------------------------------------------------------------- fold depth
@pytest.mark.parametrize("nstep", [1, 63, 64])
def test_fold_depth_equals_the_model(run, nstep):
    """Every (n, k), k in [-1, cnt]: steps, next_index, flags, payload and the bit patterns of ret / discount equal
    StepLogModel.gather; at nstep = 64 the early-exit loop runs all 64 rounds in the waves that hold a 64-row fold."""
    got = _gathered(run, run.dev.logs[4], 4, nstep, GAMMA)
    want = _expected(run.d.logs[4], run.samples, nstep, 4, GAMMA)
    _same(got, want, f"nstep = {nstep}")
    assert int(want["steps"].max()) == nstep and (want["steps"] == 0).any()
    if nstep == 64:
        waves = want["steps"][:len(run.samples) // 64 * 64].reshape(-1, 64)
        assert ((waves == 64).any(1) & (waves == 0).any(1)).any()          # the __any exit: a lane done at once next to one that goes on
    print(f"nstep = {nstep}: {len(run.samples)} samples compared, {int((want['steps'] == nstep).sum())} full folds")


def _composition(run, samples, L):
    """The sequence tests' composition from the models alone: the length rule (tests/sequence_model.py) plus
    StepLogModel.gather of every live step (n, k + l) at nstep = 64; every other step is zeros and next_index -1.  [B][L]."""
    d = run.d
    if "table" not in run.cache:
        run.cache["table"] = lc.gather_table(d.hm, d.logs[SEQ_W], lc.NSTEP_LIMIT, GAMMA)
    table = run.cache["table"]
    B = len(samples)
    lens = np.array([qm.length(d.hm, n, k, L) for n, k in samples], np.int32)
    want = dict(steps=np.zeros((B, L), np.int32), next_index=np.full((B, L), -1, np.int64), ret=np.zeros((B, L), np.float32),
                discount=np.zeros((B, L), np.float32), flags=np.zeros((B, L), np.uint8), payload=np.zeros((B, L, SEQ_W), np.uint8))
    for b, ((n, k), m) in enumerate(zip(samples, lens)):
        for key in want if m else ():
            want[key][b, :m] = table[key][n][k:k + m]
    return lens, want


@pytest.mark.parametrize("L", [1, 64, 65])
def test_sequence_gather_depth(run, L):
    """agx_sequence_gather at nstep = 64, L = 1, 64 and 65 (one step past a wave of steps), both layouts, into sentinel-filled
    outputs: d_len and every element of every output equal the composition."""
    from active_gym import _native as nat
    dev = run.dev
    samples = qm.starts(run.d.hm)
    B = len(samples)
    env, idx = _pair(samples)
    lens, want = _composition(run, samples, L)
    assert (lens == L).any() and (lens == 0).any() and int(want["steps"].max()) == 64
    for tm in (False, True):
        shape = (L, B) if tm else (B, L)
        out = {"steps": torch.full(shape, -9, dtype=torch.int32, device=DEV), "next_index": torch.full(shape, -9, dtype=torch.int64, device=DEV),
               "ret": torch.full(shape, F_SENT, dtype=torch.float32, device=DEV), "discount": torch.full(shape, F_SENT, dtype=torch.float32, device=DEV),
               "flags": torch.full(shape, B_SENT, dtype=torch.uint8, device=DEV), "payload": torch.full(shape + (SEQ_W,), B_SENT, dtype=torch.uint8, device=DEV)}
        length = torch.full((B,), -9, dtype=torch.int32, device=DEV)
        rc = dev.seq._lib.agx_sequence_gather(dev.logs[SEQ_W]._s, P(env.data_ptr()), P(idx.data_ptr()), B, L, lc.NSTEP_LIMIT, GAMMA, int(tm),
                                              P(length.data_ptr()), *[P(out[k].data_ptr()) for k in ("steps", "next_index", "ret", "discount", "flags", "payload")],
                                              dev.pipe._stream())
        nat.check(rc, dev.pipe._ctx)
        assert np.array_equal(length.cpu().numpy(), lens), f"d_len differs (L = {L})"
        for key, w in want.items():
            g = out[key].cpu().numpy()
            g = np.swapaxes(g, 0, 1) if tm else g
            if g.dtype == np.float32:
                g, w = g.view(np.int32), w.view(np.int32)
            assert np.array_equal(g, w), f"{key} differs from the composition (L = {L}, time_major = {tm})"
    print(f"L = {L}: {B} sequences, {B * L} steps compared in both layouts, {int(lens.sum())} live")


# ---------------------------------------------------------------------------------------------- payload width
@pytest.mark.parametrize("W", lc.WIDTHS)
def test_payload_width(run, W):
    """W = 4 and W = 64 (AGX_STEPLOG_PAYLOAD_LIMIT), logs on the same history recorded with the same rows: the payload bytes of
    agx_steplog_gather (the row of index + 1) and of agx_rollout_gather (the row of next_index) equal the model, rows that
    folded nothing keep the sentinel, and the sentinel rows in front of and behind the output buffer are untouched."""
    from active_gym import _native as nat
    dev, d = run.dev, run.d
    log, lm = dev.logs[W], d.logs[W]
    B = len(run.samples)
    for nstep in (1, 64):
        _same(_gathered(run, log, W, nstep, GAMMA), _expected(lm, run.samples, nstep, W, GAMMA), f"W = {W}, nstep = {nstep}")
    want = _expected(lm, run.samples, 64, W, GAMMA)
    guard = torch.full((B + 2, W), B_SENT, dtype=torch.uint8, device=DEV)
    steps = torch.empty(B, dtype=torch.int32, device=DEV)
    rc = log._lib.agx_steplog_gather(log._s, P(run.pair[0].data_ptr()), P(run.pair[1].data_ptr()), B, 64, GAMMA, None, None, P(steps.data_ptr()),
                                     None, None, P(guard[1:].data_ptr()), dev.pipe._stream())
    nat.check(rc, dev.pipe._ctx)
    guard = guard.cpu().numpy()
    assert np.array_equal(guard[1:-1], want["payload"]) and (guard[0] == B_SENT).all() and (guard[-1] == B_SENT).all()
    assert len({bytes(r) for r in want["payload"][want["steps"] > 0]}) > 100
    case = types.SimpleNamespace(roll=dev.roll, log=log, pipe=dev.pipe)
    for L in lc.WIDTH_LS:
        model = ro.gather(lm, L)
        got = RolloutOuts(L, d.N, W).call(case).host()
        _same_rollout(got, model, f"W = {W}, L = {L}")
        assert model["payload"].shape == (L, d.N, W) and model["payload"][model["obs_index"] >= 0].any()
    print(f"W = {W}: {B} gather rows and {sum(lc.WIDTH_LS) * d.N} rollout slots compared")


# ---------------------------------------------------------------------------------------------- the definition
WORST = {}


@pytest.mark.parametrize("gamma", [0.99, 1.0, 0.5])
def test_return_and_discount_against_the_definition_in_float64(run, gamma):
    """For every sample that folded m > 0 rows (m, and TERMINATED, are the device's own outputs, held to the model elsewhere):

        |ret - sum_{i=1..m} g^(i-1) r_i| <= 2 m 2^-24 sum_i |g^(i-1) r_i|        |discount - g^m| <= m 2^-24 g^m,  or discount == 0

    with g = float64(float32(gamma)) and the recorded float32 rewards r_i widened, all in float64; the rewards come from the
    scenario's own record of what was recorded, nothing from tests/steplog_model.py.  Derivation (limit_cases.nstep_bounds): the
    kernel's disc before row i is g multiplied i - 1 times, i - 1 roundings; the product with r_i is one more; the term then
    passes m - i + 1 additions, one rounding each: at most m + 1 <= 2 m relative errors of at most u = 2^-24 on a term of
    magnitude g^(i-1) |r_i|, and summed over the terms, to first order in u, 2 m u sum |g^(i-1) r_i|.  discount is m products, m
    roundings.  The bounds are derived, not measured; the worst observed ratio of error to bound is printed.  A sample with a
    non-zero term below 2^-100 would be left out (the bounds do not model underflow): there is none in this case."""
    d = run.d
    got = _gathered(run, run.dev.logs[4], 4, lc.NSTEP_LIMIT, gamma)
    ret, disc = got["ret"].view(np.float32), got["discount"].view(np.float32)
    checked = left_out = 0
    worst_ret = worst_disc = 0.0
    for b, (n, k) in enumerate(run.samples):
        m = int(got["steps"][b])
        if m == 0:
            continue
        want, gm, terminated, S, smallest = lc.nstep_definition(d.rows, n, k, m, gamma)
        if smallest < lc.TINY:
            left_out += 1
            continue
        rb, db = lc.nstep_bounds(m, S, gm)
        err = abs(float(ret[b]) - want)
        assert err <= rb, (n, k, m, float(ret[b]), want, rb)
        assert terminated == bool(got["flags"][b] & sm.TERMINATED)
        if terminated:
            assert disc[b] == 0.0 and not np.signbit(disc[b]), (n, k)
        else:
            assert abs(float(disc[b]) - gm) <= db, (n, k, m, float(disc[b]), gm)
            worst_disc = max(worst_disc, abs(float(disc[b]) - gm) / db)
        worst_ret = max(worst_ret, err / rb if rb else 0.0)
        checked += 1
    print(f"gamma = {gamma}: {checked} samples checked, {left_out} left out; worst error / bound: ret {worst_ret:.4f}, discount {worst_disc:.4f}")
    assert checked > 500 and left_out == 0 and worst_ret < 1 and worst_disc < 1


# ---------------------------------------------------------------------------------------------- special floats
@pytest.mark.parametrize("gamma", lc.SPECIAL_GAMMAS)
def test_special_floats_go_through_the_fold_unchanged(run, gamma):
    """The special log - rewards +-0, +-2^-149, +-2^-126, +-3.4e38, +-inf, NaN and ordinary normals on the same rows - at nstep = 64:
    where the model's ret / discount is NaN the device's is NaN (any payload), everywhere else the bit patterns are equal:
    subnormal sums and discounts are not flushed, signed zeros keep their sign, overflow gives inf, inf - inf and 0 * inf give
    NaN.  (tests/test_limit_cases_cpu.py runs the host side of the same fold on the same rows.)"""
    d = run.d
    got = _gathered(run, run.dev.special, 0, lc.NSTEP_LIMIT, gamma)
    with np.errstate(all="ignore"):
        want = _expected(d.special, run.samples, lc.NSTEP_LIMIT, 0, gamma)
    for key in ("steps", "next_index", "flags"):
        assert np.array_equal(got[key], want[key]), key
    seen = {}
    for key in ("ret", "discount"):
        g, w = got[key].view(np.float32), want[key].view(np.float32)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), f"{key}: NaN-ness differs from the model"
        assert np.array_equal(got[key][~nan], want[key][~nan]), f"{key}: bit patterns differ from the model"
        folded = want["steps"] > 0
        seen[key] = dict(nan=int(nan.sum()), inf=int(np.isinf(w[folded]).sum()), subnormal=int(((w != 0) & (np.abs(w) < 2.0 ** -126))[folded].sum()),
                         zero=int((w == 0)[folded].sum()))
    print(f"gamma = {gamma}: {len(run.samples)} samples compared; {seen}")
    assert seen["ret"]["nan"] >= 1 and seen["ret"]["inf"] >= 1
    if gamma == lc.SPECIAL_GAMMA:
        assert seen["ret"]["subnormal"] >= 1 and seen["discount"]["subnormal"] >= 1 and seen["discount"]["zero"] >= 1
