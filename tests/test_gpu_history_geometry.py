"""GPU: every reader of the frame history - FrameHistory.observe, RandomShift.observe, SequenceReplay.observe, GlimpseMemory.observe
and the counterfactual ``action=`` path - by geometry, type and launch edge.  The sweep is tests/history_cases.py's, derived from
tests/golden/geometry_cases.json (tests/test_history_cases_cpu.py says what it reaches and pins every seed on the model alone).

One run per (case, mode): N = 3, T = fs + 2, seeded CLEAR and SKIP, enough steps for every env's indices to wrap.  Every output
is allocated with a sentinel tail behind it and pre-filled with the sentinel.  Within the run each reader is held against the
step's own clones bit for bit, and observe - with and without a read-time action - against oracle.FixedFovealOracle in float64,
fed the NumPy frames and actions alone: raw crops, masks and full frames bit-exact, resampled values within FLOAT_TOL.  The seed
of a test is derived from its id, so one case can be re-run alone:
``pytest tests/test_gpu_history_geometry.py -k o64x64_f21x19_fs3_aa0-fixed_resize``."""
import numpy as np
import pytest
import torch

import history_cases as hc
import sequence_model as qm
from glimpse_model import taken_count
from history_model import HistoryModel
from test_gpu_augment import _gather
from test_gpu_geometry import FLOAT_TOL, SENTINEL, _bits, _guarded, _tail_ok

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOC_SENTINEL = -77
PAD = 4
assert FLOAT_TOL == 1e-5               # history_cases.check_obs states the same bar


def _t(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)         # (a copy: a broadcast view is not writable)


def _untouched(t):
    """Every element still holds the sentinel the output was pre-filled with (in the output's own type)."""
    return torch.equal(t, torch.full_like(t, SENTINEL))


def _pipe(c, N, mode="absolute", dtype=torch.float32):
    from active_gym import ObsPipeline
    kw = dict(num_envs=N, kind=c.kind, obs_size=c.obs, frame_stack=c.fs, device=DEV, obs_dtype=dtype)
    if c.kind == "fixed":
        kw.update(fov_size=c.fov, fov_init_loc=hc.init_loc(c), sensory_action_mode=mode, antialias=bool(c.aa),
                  sensory_action_space=(-7.0, 9.0) if mode == "relative" else None, resize_to_full=c.mode == "resize",
                  mask_out=c.mode == "mask")
    return ObsPipeline(**kw)


class Run:
    """A case driven through ingest -> fovea (observe_full on a base context) -> push over hc.inputs(case, seed), with a device
    clone of what every step returned: rec[(n, index)] = (obs row, fov_loc row or None)."""

    def __init__(self, c, seed, dtype=torch.float32, shape=None):
        from active_gym import FrameHistory
        self.c, self.seed, self.dtype, self.shape = c, seed, dtype, shape or hc.shape_of_run(c)
        N, T, _ = self.shape
        self.pipe = _pipe(c, N, hc.action_mode(seed), dtype)
        self.hist = FrameHistory(self.pipe, T)
        self.model = HistoryModel(N, c.fs, T)
        self.rec = {}
        cmds, frames, acts = hc.inputs(c, seed, self.shape)
        for step, cmd in enumerate(cmds):
            self.push(frames[step], cmd, acts[step])
        self.what = "full" if c.kind == "base" else "fovea"
        self.row = tuple(self.hist.obs_row_shape(self.what))
        self.samples = [(n, k) for n in range(N) for k in range(-1, int(self.model.count[n]) + 1)]     # one below 0, one never issued
        self.env, self.idx = self.tensors(self.samples)
        self.valid = np.array([self.model.valid(n, k) for n, k in self.samples])
        self.vt = _t(self.valid)

    def push(self, frames, cmd, act=None, fovea=True):
        N = self.shape[0]
        self.pipe.ingest_gray(_t(frames), _t(cmd))
        obs = loc = None
        if self.c.kind == "base":
            obs = self.pipe.observe_full().clone()
        elif fovea:
            obs, loc = (x.clone() for x in self.pipe.fovea(None if act is None else _t(act)))
        idx = self.hist.push(_t(cmd)).cpu().numpy()
        assert np.array_equal(idx, self.model.push(cmd)), "indices differ from the model"
        for n in range(N):
            if idx[n] >= 0 and obs is not None:
                self.rec[(n, int(idx[n]))] = (obs[n], None if loc is None else loc[n])
        return idx

    @staticmethod
    def tensors(samples):
        return _t(np.array([s[0] for s in samples], np.int32)), _t(np.array([s[1] for s in samples], np.int64))

    def read(self, read=None, env=None, idx=None, lead=None, loc_shape=None, row=None, **kw):
        """read(env, idx, out=..., loc_out=..., **kw) into a guarded, sentinel-filled output [B, *lead, *row] and a fov_loc filled
        with LOC_SENTINEL; the tail is checked before the triple comes back."""
        env, idx = (self.env, self.idx) if env is None else (env, idx)
        B = int(env.shape[0])
        buf, out = _guarded((B,) + tuple(lead or ()) + tuple(row or self.row), self.dtype)
        loc = torch.full((B,) + tuple(loc_shape or (2,)), LOC_SENTINEL, dtype=torch.int32, device=DEV)
        got = (read or self.hist.observe)(env, idx, out=out, loc_out=loc, **kw)
        torch.cuda.synchronize()
        assert got[0] is out and got[1] is loc
        assert _tail_ok(buf, out.numel()), "the launch wrote behind its output"
        return got

    def close(self):
        self.pipe.close()


# ---------------------------------------------------------------------------------------------- the checks of one run
def check_observe(run):
    """Valid rows are the step's clones bit for bit, with the same fov_loc; validity is the model's; invalid rows keep the
    sentinel.  Returns the triple for the other checks."""
    obs, loc, valid = run.read(what=run.what)
    assert np.array_equal(valid.cpu().numpy().astype(bool), run.valid), "validity differs from the model"
    assert int(run.valid.sum()) >= 8
    for b, s in enumerate(run.samples):
        if run.valid[b]:
            o, l = run.rec[s]
            assert torch.equal(_bits(obs[b]), _bits(o)), f"sample {s}: observation bits differ from the step's"
            if l is not None:
                assert torch.equal(loc[b], l), f"sample {s}: fov_loc differs from the step's"
    assert _untouched(obs[~run.vt]), "an invalid sample's row was written"
    assert bool((loc[~run.vt] == LOC_SENTINEL).all()) and (run.c.kind == "fixed" or bool((loc == LOC_SENTINEL).all()))
    return obs, loc, valid


def check_oracle(run, obs, loc, seen, wrong=None):
    """observe's valid rows against the float64 oracle of the sample's own NumPy stack at the oracle's own fov_loc.  Returns
    (rows compared, worst resize error).  wrong: keyword of hc.oracle_obs for a deliberately wrong oracle."""
    got, gloc = obs.float().cpu().numpy(), loc.cpu().numpy()
    n, worst = 0, 0.0
    for b, s in enumerate(run.samples):
        if not run.valid[b]:
            continue
        stack, oloc = seen[s]
        ok, err = hc.check_obs(run.c, got[b], hc.oracle_obs(run.c, stack, oloc, **(wrong or {})))
        assert ok, (hc.case_id(run.c), s, err)
        if oloc is not None:
            assert tuple(gloc[b]) == oloc, (s, gloc[b], oloc)
        n, worst = n + 1, max(worst, err)
    assert n >= 8
    return n, worst


def check_shifted(run, ref, loc, valid):
    """pad = 4: the four corners, the identity and one seeded random shift per sample are the gather of the unshifted output;
    valid and fov_loc are observe's; pad = 0 is observe whatever the shift values."""
    from active_gym import RandomShift
    B, shape = len(run.samples), (len(run.samples),) + run.row
    rng = np.random.default_rng(run.seed + 7)
    aug = RandomShift(run.hist, pad=PAD)
    for s in [(0, 0), (0, 2 * PAD), (2 * PAD, 0), (2 * PAD, 2 * PAD), (PAD, PAD), rng.integers(0, 2 * PAD + 1, (B, 2))]:
        sh = _t(np.broadcast_to(np.asarray(s, np.int32), (B, 2)))
        got, gloc, gvalid = run.read(aug.observe, what=run.what, shift=sh)
        assert torch.equal(gvalid, valid) and torch.equal(gloc, loc), "valid / fov_loc differ from observe's"
        want = _gather(ref.reshape(B, -1, *shape[-2:]), sh, PAD).reshape(shape)
        assert torch.equal(_bits(got[run.vt]), _bits(want[run.vt])), f"shift {s if isinstance(s, tuple) else 'random'}: not the gather"
        assert _untouched(got[~run.vt])
    got, gloc, gvalid = run.read(RandomShift(run.hist, pad=0).observe, what=run.what, shift=_t(rng.integers(-3, 12, (B, 2)).astype(np.int32)))
    assert torch.equal(_bits(got), _bits(ref)) and torch.equal(gloc, loc) and torch.equal(gvalid, valid), "pad = 0 is not observe"
    return 7 * int(run.valid.sum())


def check_sequence(run, ref, loc, valid):
    """L = 1, planes = fs: observe on the live rows; L = 3, planes = 1: step l is hist.observe's newest plane of (n, k + l).  Dead
    steps are all-zero bytes with fov_loc (0, 0) (a base context writes no fov_loc).  Returns the live steps compared."""
    from active_gym import SequenceReplay, StepLog
    c, m, B = run.c, run.model, len(run.samples)
    fixed = c.kind == "fixed"
    seq = SequenceReplay(StepLog(run.hist, 0))
    length = seq.lengths(run.env, run.idx, 1)
    assert np.array_equal(length.cpu().numpy(), run.valid.astype(np.int32))
    o, l, live = run.read(seq.observe, lead=(1,), loc_shape=(1, 2), length=length, L=1, what=run.what, planes=c.fs)
    assert torch.equal(live[:, 0], valid)
    assert torch.equal(_bits(o[:, 0][run.vt]), _bits(ref[run.vt])), "L = 1: a live step differs from observe"
    assert not bool(_bits(o[:, 0][~run.vt]).any()), "L = 1: a dead step is not all-zero bytes"
    if fixed:
        assert torch.equal(l[:, 0][run.vt], loc[run.vt]) and not bool(l[:, 0][~run.vt].any())
    else:
        assert bool((l == LOC_SENTINEL).all())
    L = 3
    lens = np.array([qm.length(m, n, k, L) for n, k in run.samples], np.int32)
    length = seq.lengths(run.env, run.idx, L)
    assert np.array_equal(length.cpu().numpy(), lens), "lengths differ from the model"
    o, l, live = run.read(seq.observe, lead=(L, 1), loc_shape=(L, 2), row=run.row[1:], length=length, L=L, what=run.what, planes=1)
    want_live = np.arange(L)[None, :] < lens[:, None]
    assert np.array_equal(live.cpu().numpy().astype(bool), want_live)
    fe = _t(np.repeat([s[0] for s in run.samples], L).astype(np.int32))
    fi = _t((np.array([s[1] for s in run.samples], np.int64)[:, None] + np.arange(L)[None, :]).reshape(-1))
    fo, fl, fv = run.read(env=fe, idx=fi, what=run.what)
    lv = _t(want_live.reshape(-1))
    assert int(lv.sum()) >= 8 and bool((~lv).any()) and bool(fv.bool()[lv].all())
    o, l = o.reshape((B * L, 1) + run.row[1:]), l.reshape(B * L, 2)
    assert torch.equal(_bits(o[lv]), _bits(fo[:, c.fs - 1:][lv])), "L = 3: a live step is not observe's newest plane"
    assert not bool(_bits(o[~lv]).any()), "L = 3: a dead step is not all-zero bytes"
    if fixed:
        assert torch.equal(l[lv], fl[lv]) and not bool(l[~lv].any())
    return int(run.valid.sum()) + int(lv.sum())


def _memory_want(run, n, k, count):
    want = run.rec[(n, k)][0]
    for i in range(1, count):
        want = torch.maximum(want, run.rec[(n, k - i)][0])
    return want


def check_memory(run, P, samples=None):
    """GlimpseMemory(P).observe: taken and the per-glimpse fov_loc are the model's, a taken row is torch.maximum over the step's
    clones bit for bit, an invalid one keeps the sentinel.  Returns (obs, loc, taken)."""
    from active_gym import GlimpseMemory
    samples = run.samples if samples is None else samples
    env, idx = run.tensors(samples)
    obs, loc, taken = run.read(GlimpseMemory(run.hist, P).observe, env=env, idx=idx, loc_shape=(P, 2))
    taken = taken.cpu().numpy()
    assert np.array_equal(taken, np.array([taken_count(run.model, n, k, P) for n, k in samples])), "glimpses taken differ from the model"
    gl = loc.cpu().numpy()
    for b, (n, k) in enumerate(samples):
        if taken[b]:
            assert torch.equal(_bits(obs[b]), _bits(_memory_want(run, n, k, int(taken[b])))), f"sample {(n, k)}: memory bits differ"
        else:
            assert _untouched(obs[b]), f"invalid sample {(n, k)}: row was written"
        for i in range(P):
            want = run.rec[(n, k - i)][1].tolist() if i < taken[b] else [LOC_SENTINEL, LOC_SENTINEL]
            assert gl[b, i].tolist() == want, f"sample {(n, k)}: fov_loc of glimpse {i}"
    return obs, loc, taken


def check_glimpse(run, ref, loc, valid):
    """P = 1 is observe; P = 3 is the maximum over the step's clones.  A P whose LDS is over the limit must be refused with
    memory_lds's number (none of the sweep's is, at P <= 3)."""
    from active_gym import GlimpseMemory
    from active_gym._native import AgxError
    n = 0
    for P in (1, 3):
        need = hc.memory_lds(run.c, P)
        if need > hc.K_MAX_LDS:
            with pytest.raises(AgxError, match=f"need {need} B of LDS"):
                GlimpseMemory(run.hist, P).observe(run.env, run.idx)
            continue
        obs, gl, taken = check_memory(run, P)
        if P == 1:
            assert torch.equal(_bits(obs), _bits(ref)) and torch.equal(gl[:, 0], loc), "P = 1 is not observe"
            assert np.array_equal(taken, valid.cpu().numpy())
        else:
            assert int(taken.max()) >= 2
        n += int((taken > 0).sum())
    return n


def action_values(c, B, seed):
    """float64 [B, 2] read-time actions: out of range on both sides, exact .5 ties (at both bounds: the two bounds differ
    wherever oh - fh != ow - fw, so an exchange of them, or of (r, c), shows), the rest uniform over the frame and beyond."""
    br, bc = c.obs[0] - c.fov[0], c.obs[1] - c.fov[1]
    a = np.random.default_rng(seed + 11).uniform(-12.0, max(c.obs) + 12.0, (B, 2))
    edge = [[0.5, 1.5], [2.5, bc + 0.5], [br + 0.5, bc], [-0.5, bc + 6.0], [1e9, -1e9], [br - 0.5, 0.49999], [-1e9, 1e9], [br, bc - 0.5]]
    a[:len(edge)] = edge[:B]
    return a


def check_action(run, seen, wrong=None):
    """observe(action=a), a in float32 / float64 / int32 / int64: the oracle at update_loc(a) on the sample's own NumPy stack,
    fov_loc exact.  Returns (rows compared, worst resize error)."""
    c = run.c
    samples = [s for s in run.samples if run.model.valid(*s)]
    env, idx = run.tensors(samples)
    base = action_values(c, len(samples), run.seed)
    n, worst = 0, 0.0
    for dt in (np.float32, np.float64, np.int32, np.int64):
        a = np.rint(base).astype(dt) if np.issubdtype(dt, np.integer) else base.astype(dt)
        obs, loc, valid = run.read(env=env, idx=idx, action=_t(a))
        assert bool(valid.all())
        got, gloc = obs.float().cpu().numpy(), loc.cpu().numpy()
        for b, s in enumerate(samples):
            want_loc = hc.action_loc(c, a[b])
            assert tuple(gloc[b]) == want_loc, (dt.__name__, s, a[b], gloc[b], want_loc)
            ok, err = hc.check_obs(c, got[b], hc.oracle_obs(c, seen[s][0], want_loc, **(wrong or {})))
            assert ok, (hc.case_id(c), dt.__name__, s, a[b], err)
            n, worst = n + 1, max(worst, err)
    return n, worst


# ---------------------------------------------------------------------------------------------- 1: the sweep
@pytest.mark.parametrize("case", hc.SWEEP, ids=hc.case_id)
def test_readers_by_geometry(case):
    seed = hc.seed_of(case)
    run = Run(case, seed)
    seen = hc.replay(case, seed)
    assert sorted(seen) == sorted(run.rec)
    ref, loc, valid = check_observe(run)
    counts = {"observe": int(run.valid.sum())}
    counts["oracle"], worst = check_oracle(run, ref, loc, seen)
    counts["shifted"] = check_shifted(run, ref, loc, valid)
    counts["sequence"] = check_sequence(run, ref, loc, valid)
    if case.kind == "fixed":
        if case.mode != "raw":
            counts["glimpse"] = check_glimpse(run, ref, loc, valid)
        counts["action"], w = check_action(run, seen)
        worst = max(worst, w)
    print(f"{hc.case_id(case)}: compared {counts}, worst error against the float64 oracle {worst:.3g}")
    run.close()


# ---------------------------------------------------------------------------------------------- 2: 16-bit outputs
def _pick(**want):
    return next(c for c in hc.SWEEP if all(getattr(c, k) == v for k, v in want.items()))


# one run-time geometry per mode (each with oh - fh != ow - fw), "full", and the compile-time geometry in resize and mask-out
SUBSET_16 = [_pick(obs=(64, 64), mode="resize", aa=0), _pick(obs=(40, 160), mode="raw", aa=1), _pick(obs=(120, 40), mode="mask", aa=0),
             _pick(obs=(64, 64), kind="base"), _pick(obs=(84, 84), fov=(30, 30), mode="resize", aa=1),
             _pick(obs=(84, 84), fov=(30, 30), mode="mask", aa=0)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", SUBSET_16, ids=hc.case_id)
def test_16_bit_readers_are_the_f32_readers_cast_once(case, dtype):
    """The three plane readers on a float32 and on a 16-bit context over the same inputs: the 16-bit bits are o32.to(dtype)'s, and
    observe's are that context's own step clones."""
    from active_gym import RandomShift, SequenceReplay, StepLog
    seed = hc.seed_of(case)
    r32, r16 = Run(case, seed), Run(case, seed, dtype)
    B, L = len(r32.samples), 3
    sh = _t(np.random.default_rng(seed + 7).integers(0, 2 * PAD + 1, (B, 2)).astype(np.int32))
    outs = []
    for run in (r32, r16):
        obs, loc, valid = check_observe(run)                       # (the step's own clones, in the context's own type)
        sobs, sloc, svalid = run.read(RandomShift(run.hist, pad=PAD).observe, what=run.what, shift=sh)
        seq = SequenceReplay(StepLog(run.hist, 0))
        length = seq.lengths(run.env, run.idx, L)
        qobs, qloc, live = run.read(seq.observe, lead=(L, 1), loc_shape=(L, 2), row=run.row[1:], length=length, L=L, what=run.what, planes=1)
        outs.append((obs, loc, valid, sobs, sloc, svalid, qobs, qloc, live))
    a, b = outs
    vt = r32.vt
    for i in (1, 2, 4, 5, 7, 8):
        assert torch.equal(a[i], b[i]), "fov_loc / valid / live differ between the two contexts"
    assert int(vt.sum()) >= 8 and int(a[8].sum()) >= 8
    assert torch.equal(_bits(b[0][vt]), _bits(a[0][vt].to(dtype))), "observe"
    assert torch.equal(_bits(b[3][vt]), _bits(a[3][vt].to(dtype))), "shifted observe"
    assert _untouched(b[0][~vt]) and _untouched(b[3][~vt])
    assert torch.equal(_bits(b[6]), _bits(a[6].to(dtype))), "sequence observe (dead steps are zero bytes in both)"
    r32.close()
    r16.close()


# ---------------------------------------------------------------------------------------------- 3: launch edges
EDGE = hc.Case((12, 12), (3, 5), 1, 1, "fixed", "raw", "edge")
EDGE_SHAPE, EDGE_SEED = (4, 5, 9), 11


def _shift_np(x, d, pad):
    """NumPy: the plane [h][w] moved by d = (dy, dx) - tests/shift_model.py's map, output (y, x) = input (clamp(y + dy - pad), ..)."""
    h, w = x.shape
    iy = np.clip(np.arange(h) + int(d[0]) - pad, 0, h - 1)
    ix = np.clip(np.arange(w) + int(d[1]) - pad, 0, w - 1)
    return x[iy][:, ix]


@pytest.mark.parametrize("adt", [np.float64, np.int32], ids=["f64_16B_stride", "i32_8B_stride"])
def test_more_than_65535_rows_advance_every_per_row_array(adt):
    """B = 65,540 on a fixed 12 x 12 / 3 x 5 context, fs = 1, raw crops: a few valid samples in shuffled repeats, an invalid one at
    row 65534, an action of its own per row (float64: 16 bytes a row; int32: 8), loc_out and valid, and for the shifted reader a
    shift of its own per row.  Rows 65000 .. B - 1 are held against a single-launch call on just those rows - the last five
    belong to the second launch, and take other actions and shifts than rows 0 .. 4, so an array that was not advanced shows
    there - and rows 0, 65534, 65535, 65536 and B - 1 against the float64 oracle."""
    from active_gym import RandomShift
    c = EDGE
    run = Run(c, EDGE_SEED, shape=EDGE_SHAPE)
    seen = hc.replay(c, EDGE_SEED, EDGE_SHAPE)
    few = [s for s in run.samples if run.model.valid(*s)][:7]
    assert len(few) >= 4
    few.append((0, -1))
    B, lo, cut = 65540, 65000, 65535
    rng = np.random.default_rng(13)
    pick = rng.integers(0, len(few) - 1, B)
    pick[cut - 1] = len(few) - 1                                   # an invalid row, the last of the first launch
    env = _t(np.array([few[i][0] for i in pick], np.int32))
    idx = _t(np.array([few[i][1] for i in pick], np.int64))
    act = rng.uniform(-3.0, 15.0, (B, 2))
    act = np.rint(act).astype(adt) if np.issubdtype(adt, np.integer) else act.astype(adt)
    shift = rng.integers(0, 2 * PAD + 1, (B, 2)).astype(np.int32)
    want_loc = np.rint(np.clip(act.astype(np.float64), 0, [c.obs[0] - c.fov[0], c.obs[1] - c.fov[1]])).astype(np.int32)
    # the second launch's rows differ from the rows an unadvanced array would hand them: action (through its fov_loc) and shift
    assert (want_loc[cut:] != want_loc[:B - cut]).any(axis=1).all() and (shift[cut:] != shift[:B - cut]).any(axis=1).all()
    valid_want = pick != len(few) - 1
    aug = RandomShift(run.hist, pad=PAD)
    plain = None
    for name, read, kw, kw_ref in (("observe", run.hist.observe, {}, {}),
                                   ("shifted", aug.observe, {"shift": _t(shift)}, {"shift": _t(shift[lo:])})):
        obs, loc, valid = run.read(read, env=env, idx=idx, action=_t(act), **kw)
        robs, rloc, rvalid = run.read(read, env=env[lo:], idx=idx[lo:], action=_t(act[lo:]), **kw_ref)
        differ = (_bits(obs[lo:]) != _bits(robs)).flatten(1).any(1) | (loc[lo:] != rloc).any(1) | (valid[lo:] != rvalid)
        rows = (torch.nonzero(differ).flatten() + lo).tolist()
        assert not rows, f"{name}: rows {rows} differ from the single-launch call on rows {lo} .. {B - 1}"
        assert np.array_equal(valid.cpu().numpy().astype(bool), valid_want)
        got, gloc = obs.cpu().numpy(), loc.cpu().numpy()
        assert np.array_equal(gloc[valid_want], want_loc[valid_want]), f"{name}: fov_loc is not the oracle's"
        for b in (0, cut - 1, cut, cut + 1, B - 1):
            if not valid_want[b]:
                assert b == cut - 1 and (got[b] == SENTINEL).all() and gloc[b].tolist() == [LOC_SENTINEL] * 2
                continue
            assert hc.action_loc(c, act[b]) == tuple(want_loc[b])
            want = hc.oracle_obs(c, seen[few[pick[b]]][0], tuple(want_loc[b])).astype(np.float32)
            if name == "shifted":
                want = np.stack([_shift_np(p, shift[b], PAD) for p in want])
            assert np.array_equal(got[b], want), f"{name}: row {b} is not the oracle's"
        if plain is None:
            plain = obs
        else:
            v = _t(valid_want)
            assert torch.equal(_bits(obs[v]), _bits(_gather(plain, _t(shift), PAD)[v])), "shifted rows are not the gather of observe's"
    run.close()


WILD = hc.Case((40, 160), (12, 50), 4, 1, "fixed", None, "wild")


@pytest.mark.parametrize("mode", ["resize", "mask", "raw"])
def test_out_of_range_recorded_position_is_clamped(mode):
    """40 x 160 / 12 x 50 (the bounds are 28 and 110).  How the recorded row comes to hold a raw value: agx_set_fov_state copies the
    caller's locations into the context's fov_loc as they are, and a push straight after it - with no fovea call in between,
    which would clip them - copies that fov_loc into the history row as it is.  observe, the shifted observe, the sequence
    observe and the glimpse memory then clamp at read time: nothing behind their outputs, the clamped fov_loc, and the bits of
    observe(action = the clamped location)."""
    from active_gym import GlimpseMemory, RandomShift, SequenceReplay, StepLog
    c = WILD._replace(mode=mode)
    assert any((s.obs, s.fov, s.mode) == (c.obs, c.fov, mode) for s in hc.SWEEP)
    N, T = 4, 6
    run = Run(c, 2, shape=(N, T, 0))                              # no seeded steps: the run below is plain
    rng = np.random.default_rng(5)
    plain = np.full(N, 2, np.uint8)
    frames = rng.integers(0, 256, (c.fs + 2, N, 2) + c.obs, dtype=np.uint8)
    for step in range(c.fs + 1):
        run.push(frames[step], plain, rng.uniform(-5, 170, (N, 2)).astype(np.float32))
    wild = np.array([[-5, 200], [40, -3], [29, 111], [3, 7]], np.int32)
    tame = np.array([[0, 110], [28, 0], [28, 110], [3, 7]], np.int32)
    run.pipe.ingest_gray(_t(frames[-1]), _t(plain))
    run.pipe.set_fov_state(_t(wild))
    k = run.hist.push(_t(plain)).cpu().numpy()
    assert (k == c.fs + 1).all() and np.array_equal(k, run.model.push(plain))
    env, idx = run.tensors([(n, int(k[n])) for n in range(N)])
    row = tuple(run.hist.obs_row_shape())
    obs, loc, valid = run.read(env=env, idx=idx)
    assert bool(valid.all()) and np.array_equal(loc.cpu().numpy(), tame), loc
    want, wloc, _ = run.read(env=env, idx=idx, action=_t(tame))
    assert torch.equal(_bits(obs), _bits(want)) and torch.equal(loc, wloc), "observe is not observe(action = the clamped location)"
    stack = np.maximum(frames[-c.fs:, :, 0], frames[-c.fs:, :, 1]).transpose(1, 0, 2, 3)     # cmd 2: the maximum of the two frames
    for n in range(N):
        ok, err = hc.check_obs(c, obs[n].cpu().numpy(), hc.oracle_obs(c, stack[n], tuple(tame[n])))
        assert ok, (n, err)
    aug = RandomShift(run.hist, pad=PAD)
    for sh in (np.full((N, 2), PAD, np.int32), rng.integers(0, 2 * PAD + 1, (N, 2)).astype(np.int32)):
        got, gloc, _ = run.read(aug.observe, env=env, idx=idx, shift=_t(sh))
        assert torch.equal(gloc, loc) and torch.equal(_bits(got), _bits(_gather(want, _t(sh), PAD))), "shifted observe"
    seq = SequenceReplay(StepLog(run.hist, 0))
    got, gloc, live = run.read(seq.observe, env=env, idx=idx, lead=(1,), loc_shape=(1, 2), length=seq.lengths(env, idx, 1), L=1, planes=c.fs)
    assert bool(live.all()) and torch.equal(gloc[:, 0], loc) and torch.equal(_bits(got[:, 0]), _bits(want)), "sequence observe"
    if mode != "raw":
        got, gloc, taken = run.read(GlimpseMemory(run.hist, 1).observe, env=env, idx=idx, loc_shape=(1, 2))
        assert bool((taken == 1).all()) and torch.equal(gloc[:, 0], loc) and torch.equal(_bits(got), _bits(want)), "glimpse memory, P = 1"
        got, gloc, taken = run.read(GlimpseMemory(run.hist, 2).observe, env=env, idx=idx, loc_shape=(2, 2))
        older = torch.stack([run.rec[(n, int(k[n]) - 1)][0] for n in range(N)])
        oloc = torch.stack([run.rec[(n, int(k[n]) - 1)][1] for n in range(N)])
        assert bool((taken == 2).all()) and torch.equal(gloc[:, 0], loc) and torch.equal(gloc[:, 1], oloc)
        assert torch.equal(_bits(got), _bits(torch.maximum(want, older))), "glimpse memory, P = 2"
    run.close()


def _plain_run(c, N, T, steps, seed):
    """No CLEAR, no SKIP: every env appends at every step."""
    run = Run(c, seed, shape=(N, T, 0))
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        run.push(rng.integers(0, 256, (N, 2) + c.obs, dtype=np.uint8), np.full(N, 2, np.uint8),
                 rng.uniform(-5, max(c.obs) + 5, (N, 2)).astype(np.float32))
    return run


def test_glimpse_memory_at_the_lds_limit():
    """256 x 256 / 200 x 200 mask-out, fs = 1: three glimpses take 128 + 3 x 51200 B of the 163840 a workgroup has - the maximum
    of the step's clones, nothing behind the output; four are refused with memory_lds's own number and nothing is written."""
    from active_gym import _native as nat
    from active_gym.glimpse import observe_memory
    c = _pick(obs=(256, 256), mode="mask")
    run = _plain_run(c, 2, 4, 6, 3)
    samples = [(n, k) for n in range(2) for k in range(1, 7)]
    assert hc.memory_lds(c, 3) == 153728 <= hc.K_MAX_LDS
    _, _, taken = check_memory(run, 3, samples)
    assert sorted(set(taken.tolist())) == [0, 1, 2, 3]             # evicted, and memories of one, two and three glimpses
    need = hc.memory_lds(c, 4)
    assert need == 204928 > hc.K_MAX_LDS
    env, idx = run.tensors(samples)
    B = len(samples)
    buf, out = _guarded((B,) + run.row)
    loc = torch.full((B, 4, 2), LOC_SENTINEL, dtype=torch.int32, device=DEV)
    tk = torch.full((B,), 99, dtype=torch.uint8, device=DEV)
    with pytest.raises(nat.AgxError, match=f"4 glimpses of this geometry need {need} B of LDS per workgroup") as e:
        observe_memory(run.hist, 4, env, idx, out=out, loc_out=loc, taken_out=tk)
    assert e.value.code == nat.E_STATE
    torch.cuda.synchronize()
    assert _untouched(buf) and bool((loc == LOC_SENTINEL).all()) and bool((tk == 99).all())
    run.close()


def test_glimpse_memory_of_eight_glimpses_with_the_lds_accumulator():
    """84 x 84 / 83 x 83 resize, fs = 1, P = 8: 141,280 B - eight window images, two H buffers and the 28 KB accumulator."""
    c = _pick(obs=(84, 84), fov=(83, 83), mode="resize")
    assert hc.memory_lds(c, 8) == 141280 <= hc.K_MAX_LDS
    run = _plain_run(c, 2, 10, 12, 4)
    _, _, taken = check_memory(run, 8, [(n, k) for n in range(2) for k in range(1, 13)])
    assert int(taken.max()) == 8 and int((taken == 8).sum()) >= 2 and int((taken == 0).sum()) >= 2
    run.close()
