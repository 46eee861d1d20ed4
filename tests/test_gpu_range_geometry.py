"""GPU: launches over a range of envs (agx_env_range) at every kernel form and every awkward size of the case tables.

tests/test_gpu_env_range.py walks partitions at 84 x 84 / 30 x 30 / fs 4 alone, where every frame and every observation row
is a multiple of 16 B and obs_h == obs_w.  Here the cover of tests/range_cases.py (pinned on the CPU by
tests/test_range_cases_cpu.py) runs: per (kind-mode, plan label) and per arithmetic class one geometry, per geometry two
contexts built from the same arguments - `whole` never sees a range, `ranged` walks the run's partitions, one call of an
entry point per range, then env_range() again.  After every step

(a) `ranged` is bit for bit `whole`: observations, loc_out / res_out, fov_state() and stack_u8();
(b) every env of a float32 `ranged` context matches the float64 oracle at the bars of tests/test_gpu_geometry.py (crops,
    masks, windows, fov_loc, fov_res bit-exact; resampled values within FLOAT_TOL) - independently of any kernel of ours;
(c) a 16-bit `ranged` context holds the bits of ``o32.to(dtype)`` of that float32 `ranged` context;
(d) masked-out rows are still the sentinel and nothing is written behind any output.

No knob is set.  The seed of a run and its partitions are functions of the test id (range_cases.run_plan).  With
AGX_RANGE_STATS=<file> every test appends one JSON line of what it compared (DESIGN.md section 25 quotes a run)."""
import json
import os
import time

import numpy as np
import pytest
import torch

import range_cases as R
import test_gpu_geometry as G
import test_gpu_ingest_geometry as I
from golden_util import unit64
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = G.DEV
SENT = G.SENTINEL
ISENT = -12345
TDT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def _stats(name, **kw):
    path = os.environ.get("AGX_RANGE_STATS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(test=name, **kw)) + "\n")


def _u8(x, offset):
    """A u8 device tensor of `x`; with `offset` a view at byte offset 1 of a larger allocation, so that the aligned dword
    around its byte `lo` starts in front of the view for lo < 3 (uniform_load_u8's contract: it reads the aligned dword that
    contains the byte - the same 4-byte word, inside the allocation - so any byte address inside an allocation is legal)."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    if not offset:
        return G._t(x)
    big = torch.full((x.size + 16,), 0xFF, dtype=torch.uint8, device=DEV)
    view = big[1:1 + x.size]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    return view


def _iguard(N):
    buf = torch.full((2 * N + G.TAIL,), ISENT, dtype=torch.int32, device=DEV)
    return buf, buf[:2 * N].view(N, 2)


def _itail_ok(buf, n):
    return bool((buf[n:] == ISENT).all())


class _Ctx:
    """One context and the guarded outputs of its current call."""

    def __init__(self, pipe, flexible):
        self.p, self.flexible = pipe, flexible

    def fresh(self, loc_fill=None):
        self.obuf, self.o = G._guarded(self.p.obs_shape, self.p.obs_dtype)
        self.lbuf, self.loc = _iguard(self.p.num_envs)
        self.rbuf, self.res = _iguard(self.p.num_envs)
        if loc_fill is not None:
            self.loc.copy_(loc_fill)

    def fovea(self, a, types, mask):
        kw = dict(mask=mask, out=self.o, loc_out=self.loc)
        if self.flexible:
            kw.update(action_type=types, res_out=self.res)
        self.p.fovea(a, **kw)

    def tails_ok(self):
        n = self.p.num_envs
        return G._tail_ok(self.obuf, self.o.numel()) and _itail_ok(self.lbuf, 2 * n) and _itail_ok(self.rbuf, 2 * n)


def _walk(ctx, ranges, call):
    for lo, n in ranges:
        ctx.p.env_range(lo, n)
        call(ctx)
    ctx.p.env_range()


def _same(a, b, what):
    """(a): everything the two contexts hold and wrote, bit for bit, guard tails included; returns the elements compared."""
    assert torch.equal(G._bits(a.obuf), G._bits(b.obuf)), (what, "observations differ")
    assert torch.equal(a.lbuf, b.lbuf), (what, "loc_out differs")
    assert torch.equal(a.rbuf, b.rbuf), (what, "res_out differs")
    n = a.o.numel() + a.loc.numel() + a.res.numel()
    return n + _same_state(a.p, b.p, what)


def _same_state(p, q, what):
    sa, sb = p.stack_u8(), q.stack_u8()
    assert torch.equal(sa, sb), (what, "ring differs")
    n = sa.numel()
    if p.kind != "base":
        (la, ra), (lb, rb) = p.fov_state(), q.fov_state()
        assert torch.equal(la, lb), (what, "fov_loc state differs")
        assert torch.equal(ra, rb), (what, "fov_res state differs")
        n += la.numel() + ra.numel()
    return n


def _actions(rng, kind, N, case, mode, step, int_dtype):
    """The action generator of tests/test_gpu_geometry.py (out-of-range values, .5 ties, f32 / f64, the special resolutions
    1, fov, fov + 1, obs per axis for flexible); the last step's actions are floored to an integer type."""
    (oh, ow), (fh, fw) = case["obs"], case["fov"]
    types = None
    if kind == "flexible":
        a, types = G._flex_actions(rng, N, oh, ow, fh, fw, mode, step, None)
    else:
        a = G._loc_actions(rng, N, oh, ow, mode, step)
    if step == R.STEPS - 1:
        a = np.floor(a).astype(int_dtype)
    return a, types


def _run_fovea(entry, name, N, plan, offset_views=False, single=True):
    case, key = entry["case"], entry["key"]
    mode = "relative" if R.seed_of(name, "mode") & 1 else "absolute"
    int_dtype = np.int32 if R.seed_of(name, "int") & 1 else np.int64
    kind, out, okw, pkw = G._kw(case, key, mode)
    (oh, ow), (fh, fw), fs = case["obs"], case["fov"], case["fs"]
    dt = TDT[entry["dtype"]]
    flexible = kind == "flexible"
    rng = np.random.default_rng(R.seed_of(name, N))
    whole = _Ctx(G._pipe(N, pkw, obs_dtype=dt), flexible)
    ranged = _Ctx(G._pipe(N, pkw, obs_dtype=dt), flexible)
    r32 = ranged if dt == torch.float32 else _Ctx(G._pipe(N, pkw), flexible)      # the float32 ranged context of (b) and (c)
    ctxs = [whole, ranged] + ([r32] if r32 is not ranged else [])
    orcs = [G._oracle(kind, okw) for _ in range(N)]
    envs = bits = 0
    worst = 0.0
    loc_prev = None

    def step_oracle(i, st, a, types):
        fr = unit64(st[i]).reshape(-1, oh, ow)
        return orcs[i].step(fr, a[i], np.array((types[i],))) if flexible else orcs[i].step(fr, a[i])

    def check_env(i, obs, st, a, types, what):
        nonlocal worst
        want = step_oracle(i, st, a, types)
        got = obs[i].reshape((-1,) + obs[i].shape[-2:])
        G._check_obs(kind, out, got, want, orcs[i], (fh, fw), what)
        if want.shape == got.shape or (flexible and out == "raw"):
            g = got[..., :want.shape[-2], :want.shape[-1]]
            worst = max(worst, float(np.abs(g - want).max()) if g.size else 0.0)

    def check_16(what):
        if r32 is not ranged:
            assert torch.equal(G._bits(ranged.o), G._bits(r32.o.to(dt))), (what, "16-bit bits are not the float32 output cast once")
            assert torch.equal(ranged.lbuf, r32.lbuf) and torch.equal(ranged.rbuf, r32.rbuf), (what, "16-bit fov rows")

    for step in range(R.STEPS):
        what = (entry["id"], f"N={N}", mode, f"step {step}")
        st = rng.integers(0, 256, (N, fs, oh, ow), dtype=np.uint8)
        a, types = _actions(rng, kind, N, case, mode, step, int_dtype)
        ta, tt = G._t(a), None if types is None else G._t(types)
        mask = plan["mask"] if step == R.MASKED_STEP else None
        tm = None if mask is None else _u8(mask, offset_views)
        for c in ctxs:
            c.p.set_stack_u8(G._t(st))
        if step == R.RESET_STEP:
            rs = plan["reset"]
            trs = _u8(rs, offset_views)
            whole.p.fovea_reset(trs)
            for c in ctxs[1:]:
                _walk(c, plan["parts"][0], lambda c: c.p.fovea_reset(trs))
            for i in np.nonzero(rs)[0]:
                orcs[i].init_loc()
                if flexible:
                    orcs[i].init_res()
            bits += _same_state(whole.p, ranged.p, what + ("fovea_reset",))
        for c in ctxs:
            c.fresh(loc_prev if mask is not None else None)
        whole.fovea(ta, tt, tm)
        for c in ctxs[1:]:
            _walk(c, plan["walk"](step), lambda c: c.fovea(ta, tt, tm))
        torch.cuda.synchronize()
        for c in ctxs:
            assert c.tails_ok(), (what, "a launch wrote behind an output")                       # (d)
        bits += _same(whole, ranged, what)                                                         # (a)
        check_16(what)                                                                             # (c)
        if r32 is not ranged:
            bits += ranged.o.numel()
        obs, loc, res = r32.o.cpu().numpy(), r32.loc.cpu().numpy(), r32.res.cpu().numpy()
        st_loc, st_res = (x.cpu().numpy() for x in r32.p.fov_state())
        o16, sent16 = ranged.o.float().cpu().numpy(), float(torch.tensor(SENT, dtype=dt))     # the sentinel as the type holds it
        for i in range(N):                                                                         # (b)
            w = what + (f"env {i}",)
            if mask is not None and not mask[i]:
                assert (obs[i] == SENT).all() and (o16[i] == sent16).all(), (w, "a masked-out env was written")     # (d)
            else:
                check_env(i, obs, st, a, types, w)
                envs += 1
                if flexible:
                    assert np.array_equal(res[i], orcs[i].fov_res), (w, res[i], orcs[i].fov_res)
            assert np.array_equal(loc[i], orcs[i].fov_loc), (w, loc[i], orcs[i].fov_loc)
            assert np.array_equal(st_loc[i], orcs[i].fov_loc), (w, "state", st_loc[i], orcs[i].fov_loc)
            if flexible:
                assert np.array_equal(st_res[i], orcs[i].fov_res), (w, "state", st_res[i], orcs[i].fov_res)
        loc_prev = r32.loc.clone()

    if single and plan["single"] is not None:
        # one ranged call on the contexts as they stand: nothing of an env outside [lo, lo + n) changes
        lo, n = plan["single"]
        what = (entry["id"], f"single range ({lo}, {n})")
        st = rng.integers(0, 256, (N, fs, oh, ow), dtype=np.uint8)
        a, types = _actions(rng, kind, N, case, mode, 1, int_dtype)
        ta, tt = G._t(a), None if types is None else G._t(types)
        inside = np.zeros(N, bool)
        inside[lo:lo + n] = True
        tin = torch.from_numpy(inside).to(DEV)
        for c in ctxs[1:]:
            c.p.set_stack_u8(G._t(st))
            state0 = [t.clone() for t in c.p.fov_state()]
            c.fresh()
            _walk(c, [(lo, n)], lambda c: c.fovea(ta, tt, None))
            torch.cuda.synchronize()
            assert c.tails_ok(), (what, "a launch wrote behind an output")
            assert bool((c.o[~tin] == torch.tensor(SENT, dtype=c.o.dtype)).all()), (what, "an observation row outside the range was written")
            assert bool((c.loc[~tin] == ISENT).all()) and bool((c.res[~tin] == ISENT).all()), (what, "a fov row outside the range was written")
            assert not bool((c.loc[tin] == ISENT).any()), (what, "a fov row inside the range was not written")
            assert flexible == (not bool((c.res[tin] == ISENT).any())), (what, "res_out rows inside the range")
            l1, r1 = c.p.fov_state()
            assert torch.equal(l1[~tin], state0[0][~tin]) and torch.equal(r1[~tin], state0[1][~tin]), (what, "fov state outside the range changed")
            assert torch.equal(l1[tin], c.loc[tin]), (what, "fov state inside the range")
            assert torch.equal(c.p.stack_u8(), G._t(st)), (what, "the ring changed")
        check_16(what)
        obs, loc = r32.o.cpu().numpy(), r32.loc.cpu().numpy()
        for i in range(lo, lo + n):
            w = what + (f"env {i}",)
            check_env(i, obs, st, a, types, w)
            envs += 1
            assert np.array_equal(loc[i], orcs[i].fov_loc), (w, loc[i], orcs[i].fov_loc)
            if flexible:
                assert np.array_equal(r32.res.cpu().numpy()[i], orcs[i].fov_res), w
    for c in ctxs:
        c.p.close()
    return dict(envs=envs, bits=bits, worst=worst)


# ---------------------------------------------------------------- fovea kinds
@pytest.mark.parametrize("entry", [pytest.param(e, id=e["id"]) for e in R.fovea_cover()])
def test_ranged_form_equals_whole_batch_and_oracle(request, entry):
    assert request.node.name == R.node(R.T_FOVEA, entry)
    t0 = time.time()
    N = entry["n"]
    got = _run_fovea(entry, request.node.name, N, R.run_plan(request.node.name, N))
    assert got["envs"] >= 3 * N and got["bits"] > 0
    _stats(request.node.name, seconds=round(time.time() - t0, 2), **got)


@pytest.mark.parametrize("entry", [pytest.param(e, id=e["id"]) for e in R.full_cover()])
def test_ranged_observe_full(request, entry):
    """agx_observe_full over the partitions of two steps and over one single range: bit for bit the whole-batch context's
    rows, which are ``float32(u8) / 255`` exactly (16-bit: that value cast once); rows outside the single range stay the
    sentinel."""
    assert request.node.name == R.node(R.T_FULL, entry)
    t0 = time.time()
    N, fs, (oh, ow), dt = entry["n"], entry["fs"], entry["obs"], TDT[entry["dtype"]]
    plan = R.run_plan(request.node.name, N, R.INGEST_STEPS, masked=False)
    rng = np.random.default_rng(R.seed_of(request.node.name, N))
    kw = dict(kind="base", obs_size=(oh, ow), frame_stack=fs, device=DEV, obs_dtype=dt)
    whole, ranged = G._pipe(N, kw), G._pipe(N, kw)
    bits = 0
    walks = [plan["walk"](s) for s in range(R.INGEST_STEPS)] + [[plan["single"]]]
    for step, walk in enumerate(walks):
        st = rng.integers(0, 256, (N, fs, oh, ow), dtype=np.uint8)
        whole.set_stack_u8(G._t(st))
        ranged.set_stack_u8(G._t(st))
        (bw, ow_), (br, or_) = G._guarded(whole.full_shape, dt), G._guarded(ranged.full_shape, dt)
        whole.observe_full(ow_)
        for lo, n in walk:
            ranged.env_range(lo, n)
            ranged.observe_full(or_)
        ranged.env_range()
        torch.cuda.synchronize()
        want = torch.from_numpy(O.u8_to_unit(st)).to(DEV).to(dt)
        assert G._tail_ok(bw, ow_.numel()) and G._tail_ok(br, or_.numel()), step
        assert torch.equal(G._bits(ow_), G._bits(want)), (entry["id"], step, "whole batch vs u8 / 255")
        inside = torch.zeros(N, dtype=torch.bool, device=DEV)
        for lo, n in walk:
            inside[lo:lo + n] = True
        assert torch.equal(G._bits(or_[inside]), G._bits(want[inside])), (entry["id"], step, "ranged rows")
        assert bool((or_[~inside] == torch.tensor(SENT, dtype=dt)).all()), (entry["id"], step, "a row outside the range was written")
        assert bool(inside.all()) == (step < R.INGEST_STEPS)
        bits += or_.numel() + _same_state(whole, ranged, (entry["id"], step))
    whole.close()
    ranged.close()
    _stats(request.node.name, seconds=round(time.time() - t0, 2), envs=0, bits=bits, worst=0.0)


# ---------------------------------------------------------------- ingests
def _ingest_call(p, form, whole, rows, cmd):
    if form == "small":
        p.ingest_gray(G._t(whole), cmd)
    else:
        I._ingest(p, form, whole, rows, cmd)


def _run_ingest(entry, name, n, plan, offset_views=False):
    """INGEST_STEPS steps (the second appends at a non-zero head) of one ingest form, walked by range on one context and whole
    on its twin, then a third step as the single range: rings bit-equal (agx_get_stack_u8 reads the ring through the heads,
    oldest frame first, so a wrong head shows as a wrong order), and equal to the oracle's ring byte for byte."""
    c, form = entry["row"], entry["form"]
    obs, fs = c["obs"], c["fs"]
    gray = form != "rgb" and form != "rgb-compact"
    rng = np.random.default_rng(R.seed_of(name, n))
    whole, ranged = I._pipe(n, obs, fs), I._pipe(n, obs, fs)
    rows = I._check_rows(whole, obs)
    ring = O.RingOracle(n, fs, (obs, obs))
    walks = [plan["walk"](s) for s in range(R.INGEST_STEPS)] + ([[plan["single"]]] if plan["single"] is not None else [])
    bits = 0
    for step, walk in enumerate(walks):
        if form == "small":
            scr = rng.integers(0, 256, (n, 2, obs, obs), dtype=np.uint8)
        else:
            scr = I._screens(rng, n, gray)
        nvalid, clear, skip = I._commands(rng, n, fs, step)
        code = (nvalid | clear * I.CMD_CLEAR | skip * I.CMD_SKIP).astype(np.uint8)
        cmd = _u8(code, offset_views)
        inside = np.zeros(n, bool)
        for lo, k in walk:
            inside[lo:lo + k] = True
        assert inside.all() == (step < R.INGEST_STEPS)
        before = ranged.stack_u8().cpu().numpy()
        if inside.all():
            _ingest_call(whole, form, scr, rows, cmd)
        for lo, k in walk:
            ranged.env_range(lo, k)
            _ingest_call(ranged, form, scr, rows, cmd)
        ranged.env_range()
        ring.ingest(scr, nvalid, clear=clear, skip=np.where(inside, skip, 1), gray=gray)
        got, want = ranged.stack_u8().cpu().numpy(), ring.stack_u8()
        if inside.all():
            assert torch.equal(whole.stack_u8(), ranged.stack_u8()), (entry["id"], step, "ranged ring != whole-batch ring")
        else:
            assert np.array_equal(got[~inside], before[~inside]), (entry["id"], step, "the ring of an env outside the range changed")
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{entry['id']} step {step}: {len(bad)} bytes differ from the oracle, first at (env, slot, row, col) "
                                 f"{bad[0].tolist()}; cmd {code.tolist()}; walk {walk}")
        bits += got.size
    assert ring.stack_u8().any()
    whole.close()
    ranged.close()
    return dict(envs=n * len(walks), bits=bits, worst=0.0)


@pytest.mark.parametrize("entry", [pytest.param(e, id=e["id"]) for e in R.ingest_cover()])
def test_ranged_ingest_equals_whole_batch_and_oracle(request, entry):
    assert request.node.name == R.node(R.T_INGEST, entry)
    t0 = time.time()
    n = entry["n"]
    got = _run_ingest(entry, request.node.name, n, R.run_plan(request.node.name, n, R.INGEST_STEPS, masked=False))
    _stats(request.node.name, seconds=round(time.time() - t0, 2), **got)


# ---------------------------------------------------------------- launch edges
def _first(key, start):
    return next(e for e in R.fovea_cover() if e["key"] == key and e["label"].startswith(start))


def _edge_plan(N, parts, steps=R.STEPS):
    rng = np.random.default_rng(N)
    plan = dict(steps=steps, parts=[parts, parts], descending=1, mask=(np.arange(N) % 2).astype(np.uint8),
                reset=(rng.random(N) < 0.5).astype(np.uint8), single=None)
    plan["walk"] = lambda step: parts[::-1] if step == 1 else parts
    return plan


EDGE_FORMS = [("fixed_raw", "fixed<GeomR>"), ("flex_resize", "flexible2 "), ("peripheral", "generic ")]


@pytest.mark.parametrize("key,start", EDGE_FORMS, ids=[k for k, s in EDGE_FORMS])
def test_one_env_with_the_explicit_range(request, key, start):
    """N = 1 and agx_env_range(0, 1) set explicitly before every call: the whole batch, stated as a range."""
    got = _run_fovea(_first(key, start), request.node.name, 1, _edge_plan(1, [(0, 1)]))
    assert got["envs"] >= 3


@pytest.mark.parametrize("key,start", EDGE_FORMS[1:], ids=[k for k, s in EDGE_FORMS[1:]])
def test_a_walk_of_one_env_per_range(request, key, start):
    """N = 11 walked as 11 ranges of one env each (step 1 from the top down), on one flexible2 and one generic case."""
    N = R.N_FOVEA
    got = _run_fovea(_first(key, start), request.node.name, N, _edge_plan(N, [(i, 1) for i in range(N)]))
    assert got["envs"] >= 3 * N


@pytest.mark.parametrize("key,start", [("fixed_mask", "fixed<GeomR>"), ("flex_raw", "raw3 "), ("peripheral", "per3 ")],
                         ids=["fixed_mask", "flex_raw", "peripheral"])
def test_mask_as_a_view_at_byte_offset_1(request, key, start):
    """The mask of the masked call and of fovea_reset is a view at byte offset 1 of a larger allocation: advanced by `lo` it is
    at any alignment, and the aligned dword around byte `lo` starts in front of the view.  uniform_load_u8 reads the aligned
    dword that contains the byte - legal for any byte inside an allocation - so the results are those of an aligned mask."""
    entry = _first(key, start)
    name = request.node.name
    got = _run_fovea(entry, name, entry["n"], R.run_plan(name, entry["n"]), offset_views=True, single=False)
    assert got["envs"] >= 3 * entry["n"]


@pytest.mark.parametrize("obs,form", [(48, "rgb"), (20, "gray-compact"), (212, "rgb-compact"), (12, "small")])
def test_cmd_as_a_view_at_byte_offset_1(request, obs, form):
    """The ingests read cmd through uniform_load_u8 (the band kernels; k_ingest_gray reads the byte): the same walk with cmd a
    view at byte offset 1 of a larger allocation."""
    entry = next(e for e in R.ingest_cover() if e["row"]["obs"] == obs and e["form"] == form)
    name = request.node.name
    _run_ingest(entry, name, entry["n"], R.run_plan(name, entry["n"], R.INGEST_STEPS, masked=False), offset_views=True)
