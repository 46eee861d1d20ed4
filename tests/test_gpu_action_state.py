"""GPU: the fovea state update - sensory action -> fov_loc (and fov_res) - of every live kernel form, on special action values
and on set state outside the frame, against the definition tests/action_cases.py:next_state (held to the oracle on the CPU by
tests/test_action_cases_cpu.py).

Every form is reached by geometry alone (no knob): the rows come from tests/golden/geometry_cases.json through
action_cases.FORMS - the smallest row per kernel family in each output mode, the three packed forms, agx_step_fixed,
agx_step_flexible_packed with and without the band12 ingest plan, and the history's read-time observe(action=).

What is compared, all of it exactly (no tolerance anywhere in this module):
  state        loc_out, res_out and fov_state() equal next_state; envs the mask leaves out keep their stored state and their
               output rows stay sentinel; TAIL sentinel elements behind every output stay sentinel.
  observation  bit-equal to that of a second, tame context of the same config, which is given the definition's (loc, res) as plain
               int32 actions (FOV_RES first, then FOV_LOC).  The tame context is always in absolute mode - the mode is a run-time
               parameter of the state update alone, the kernel instantiation is the same.  tests/test_gpu_geometry.py holds the
               tame context's observations against the float64 oracle.

Wild set states stay within a few rows / columns of the frame (at most 40 columns) and sit in the middle of the batch: a copy of
the state update that missed the clamp-on-read rule would read its neighbours' ring slots - inside the allocation - and fail here
on values."""
import math
import zlib

import numpy as np
import pytest
import torch

import action_cases as ac

pytestmark = pytest.mark.gpu
SENTINEL = -12345
TAIL = 4096
DEV = torch.device("cuda:0")
CMD_CLEAR, CMD_SKIP = 4, 8
WIDE_SAS = [(-3e9, 3e9), (-math.inf, math.inf)]
FORM_IDS = [f.name for f in ac.FORMS]
NO_MASK = ("fovea_packed", "step_fixed", "step_flexible_packed", "history_observe")     # entry points without a mask argument


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _guarded(shape, dtype=torch.float32):
    """An output of `shape` whose storage continues with TAIL sentinel elements; everything starts as SENTINEL."""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def _all_sentinel(t):
    return bool((t == SENTINEL).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


_SCREENS = {}


def _screens(n):
    """Whole RGB screens u8 [n, 2, 210, 160, 3], made once per batch size and shared (never written)."""
    if n not in _SCREENS:
        _SCREENS[n] = _t(np.random.default_rng(n).integers(0, 256, (n, 2, 210, 160, 3), dtype=np.uint8))
    return _SCREENS[n]


def _kw(form, mode, sas):
    kind, out = ac.MODES[form.key]
    (oh, ow), (fh, fw) = form.obs, form.fov
    kw = dict(kind=kind, obs_size=form.obs, fov_size=form.fov, fov_init_loc=(min(2, oh - fh), min(3, ow - fw)), frame_stack=form.fs,
              sensory_action_mode=mode, sensory_action_space=sas if mode == "relative" else None, antialias=bool(form.aa),
              resize_to_full=out == "resize", mask_out=out == "mask", device=DEV)
    if kind == "peripheral":
        kw["peripheral_res"] = form.per
    return kw


class Pair:
    """The context under test and the tame one, fed the same frames, with the definition's state next to them."""

    def __init__(self, form, n, mode, sas, seed):
        from active_gym import ObsPipeline
        self.form, self.n, self.sas = form, n, sas
        self.kind = ac.MODES[form.key][0]
        self.flex = self.kind == "flexible"
        # the history's read-time action is absolute whatever the context's mode (include/agx_history.h)
        self.mode = "absolute" if form.entry == "history_observe" else mode
        self.rng = np.random.default_rng(seed)
        kw = _kw(form, mode, sas)
        self.main = ObsPipeline(num_envs=n, **kw)
        self.tame = ObsPipeline(num_envs=n, **_kw(form, "absolute", None))
        self.loc = [tuple(int(v) for v in kw["fov_init_loc"])] * n
        self.res = [tuple(form.fov)] * n
        self.hist = None
        if form.entry == "history_observe":
            from active_gym.history import FrameHistory
            self.hist = FrameHistory(self.main, capacity=form.fs + 2)
            for _ in range(form.fs):
                self._push()
        else:
            st = _t(self.rng.integers(0, 256, (n, form.fs) + form.obs, dtype=np.uint8))
            self.main.set_stack_u8(st)
            self.tame.set_stack_u8(st)

    def _push(self):
        """One append to the history: a new random frame for every env, recorded with the env's stored fov_loc."""
        cmd = torch.full((self.n,), 1, dtype=torch.uint8, device=DEV)
        self.main.ingest_gray(_t(self.rng.integers(0, 256, (self.n, 2) + self.form.obs, dtype=np.uint8)), cmd)
        self.hist.push(cmd)

    def close(self):
        if self.hist is not None:
            self.hist.close()
        self.main.close()
        self.tame.close()

    def set_state(self, loc, res=None):
        self.main.set_fov_state(_t(np.array(loc, np.int32)), _t(np.array(res, np.int32)) if self.flex else None)
        self.loc = [tuple(map(int, v)) for v in loc]
        if self.flex:
            self.res = [tuple(map(int, v)) for v in res]
        if self.hist is not None:
            self._push()                                   # the history reads the fov_loc a push recorded

    def _cmd(self):
        cmd = np.full(self.n, 2, np.uint8)
        cmd[0] |= CMD_CLEAR
        cmd[1] = CMD_SKIP
        return _t(cmd)

    def call(self, action, dtype, types=None, mask=None, what=""):
        """One call of the form's entry point with `action` ([n, 2] NumPy of `dtype`, or None), compared in full."""
        form, n, main, tame = self.form, self.n, self.main, self.tame
        entry = form.entry
        if entry in NO_MASK:
            mask = None
        want = [ac.next_state(self.kind, self.mode, self.sas, form.obs, form.fov, self.loc[i], self.res[i],
                              None if action is None else action[i], dtype, 0 if types is None else int(types[i]),
                              mask is not None and not mask[i]) for i in range(n)]
        live = np.ones(n, bool) if mask is None else mask.astype(bool)
        at = None if action is None else _t(action)
        tt = None if types is None or action is None else _t(types)
        lbuf, lo = _guarded((n, 2), torch.int32)
        rbuf, ro = _guarded((n, 2), torch.int32)
        bufs = [(lbuf, lo, "loc_out")] + ([(rbuf, ro, "res_out")] if self.flex else [])
        # ---- the call under test
        if entry == "fovea":
            obuf, o = _guarded(main.obs_shape)
            extra = dict(action_type=tt, res_out=ro) if self.flex else {}
            main.fovea(at, mask=None if mask is None else _t(mask), out=o, loc_out=lo, **extra)
        elif entry == "step_fixed":
            obuf, o = _guarded(main.obs_shape)
            main.step_fixed(_screens(n), self._cmd(), at, out=o, loc_out=lo)
        elif entry == "history_observe":
            obuf, o = _guarded(main.obs_shape)
            env = torch.arange(n, dtype=torch.int32, device=DEV)
            vbuf = torch.full((n + TAIL,), 199, dtype=torch.uint8, device=DEV)
            self.hist.observe(env, self.hist.last_index(), action=at, out=o, loc_out=lo, valid_out=vbuf[:n])
            assert bool((vbuf[:n] == 1).all()) and bool((vbuf[n:] == 199).all()), (form.name, what, "valid")
        else:
            cap = n * form.fs * form.obs[0] * form.obs[1]
            obuf, o = _guarded((cap,))
            fbuf, off = _guarded((n + 1,), torch.int64)
            bufs.append((fbuf, off, "offsets"))
            if entry == "fovea_packed":
                main.fovea_packed(at, action_type=tt, packed=o, offsets=off, loc_out=lo, res_out=ro)
            else:
                main.step_flexible_packed(_screens(n), self._cmd(), at, action_type=tt, packed=o, offsets=off, loc_out=lo, res_out=ro)
        torch.cuda.synchronize()
        bufs.append((obuf, o, "obs"))
        for buf, view, name in bufs:
            assert _all_sentinel(buf[view.numel():]), (form.name, what, f"the call wrote behind {name}")
        # ---- state
        w_loc = np.array([w[0] for w in want], np.int32)
        w_res = np.array([w[1] for w in want], np.int32) if self.flex else None
        g_loc = lo.cpu().numpy()
        bad = [i for i in range(n) if live[i] and tuple(g_loc[i]) != tuple(w_loc[i])]
        assert not bad, (form.name, what, "loc_out", [(i, self._say(action, types, i), g_loc[i].tolist(), w_loc[i].tolist()) for i in bad[:6]])
        assert _all_sentinel(lo[_t(~live)]), (form.name, what, "loc_out of a masked-out env was written")
        if self.flex:
            g_res = ro.cpu().numpy()
            bad = [i for i in range(n) if live[i] and tuple(g_res[i]) != tuple(w_res[i])]
            assert not bad, (form.name, what, "res_out", [(i, self._say(action, types, i), g_res[i].tolist(), w_res[i].tolist()) for i in bad[:6]])
            assert _all_sentinel(ro[_t(~live)]), (form.name, what, "res_out of a masked-out env was written")
        if self.hist is None:
            s_loc, s_res = (x.cpu().numpy() for x in main.fov_state())
            assert np.array_equal(s_loc, w_loc), (form.name, what, "fov_state loc", np.argwhere(s_loc != w_loc)[:4].tolist())
            if self.flex:
                assert np.array_equal(s_res, w_res), (form.name, what, "fov_state res", np.argwhere(s_res != w_res)[:4].tolist())
            self.loc = [w[0] for w in want]
            self.res = [w[1] for w in want] if self.flex else self.res
        # ---- the tame context: the definition's state as plain int32 actions, clamped into the frame for the envs left out
        t_res = np.array([w[1] if live[i] else (1, 1) for i, w in enumerate(want)], np.int32) if self.flex else None
        t_loc = np.array([w[0] if live[i] else (0, 0) for i, w in enumerate(want)], np.int32)
        if entry in ("fovea", "step_fixed", "history_observe"):
            if entry == "step_fixed":
                tame.ingest(_screens(n), self._cmd())
            elif entry == "history_observe":
                tame.set_stack_u8(main.stack_u8())
            if self.flex:
                tame.fovea(_t(t_res), action_type=torch.ones(n, dtype=torch.int32, device=DEV))
                r = tame.fovea(_t(t_loc), action_type=torch.zeros(n, dtype=torch.int32, device=DEV))
                assert np.array_equal(r[2].cpu().numpy(), t_res), (form.name, what, "the tame context did not take the resolution")
            else:
                r = tame.fovea(_t(t_loc))
            assert np.array_equal(r[1].cpu().numpy(), t_loc), (form.name, what, "the tame context did not take the location")
            idx = _t(live)
            same = torch.equal(_bits(o[idx]), _bits(r[0][idx]))
            assert same, (form.name, what, "observation differs from the tame context's, envs",
                          [i for i in range(n) if live[i] and not torch.equal(_bits(o[i]), _bits(r[0][i]))][:8])
            assert _all_sentinel(o[_t(~live)]), (form.name, what, "a masked-out env's observation was written")
        else:
            tame.fovea_packed(_t(t_res), action_type=torch.ones(n, dtype=torch.int32, device=DEV))
            if entry == "step_flexible_packed":
                tame.ingest(_screens(n), self._cmd())
            tbuf, tp = _guarded((o.numel(),))
            _, t_off, tl, tr = tame.fovea_packed(_t(t_loc), action_type=torch.zeros(n, dtype=torch.int32, device=DEV), packed=tp)
            assert np.array_equal(tl.cpu().numpy(), t_loc) and np.array_equal(tr.cpu().numpy(), t_res), (form.name, what, "tame state")
            sizes = form.fs * t_res[:, 0].astype(np.int64) * t_res[:, 1].astype(np.int64)
            assert np.array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum(sizes)])), (form.name, what, "offsets")
            assert torch.equal(off, t_off) and torch.equal(_bits(o), _bits(tp)), (form.name, what, "packed crops differ from the tame context's")
        if entry in ("step_fixed", "step_flexible_packed"):
            assert torch.equal(main.stack_u8(), tame.stack_u8()), (form.name, what, "ring")

    def _say(self, action, types, i):
        a = None if action is None else [repr(v) for v in action[i].tolist()]
        return (a, None if types is None else int(types[i]), "from", self.loc[i], self.res[i] if self.flex else None)


def _seed(request, *more):
    return zlib.crc32("/".join([request.node.name, *map(str, more)]).encode())


def _bounds(form, mode, sas):
    """The `bound` of the value table: the upper bound of the clip an action element meets first - the relative delta's where that
    is a small number ((-7, 9)), else the window's range (with the wide action spaces the delta passes its clip unchanged)."""
    if mode == "relative" and math.isfinite(sas[1]) and sas[1] < 2 ** 20:
        return int(sas[1]), int(sas[1])
    return form.obs[0] - form.fov[0], form.obs[1] - form.fov[1]


def _special(request, form, dtype, mode, sas):
    a, mask, names = ac.batch(dtype, *_bounds(form, mode, sas))
    n = len(a)
    pair = Pair(form, n, mode, sas, _seed(request, mode, sas))
    what = (dtype, mode, sas)
    pair.call(a, dtype, None, mask, what + ("FOV_LOC",))
    if pair.flex:
        # the same table with the bound of the clip a FOV_RES action meets (obs), the types mixing 0, 1, 2 and -1: twice, with
        # complementary types, so that every value meets both branches in both elements
        a2 = ac.batch(dtype, *form.obs)[0]
        for which in (0, 1):
            pair.call(a2, dtype, ac.mixed_types(n, which), mask, what + (f"mixed types {which}",))
    pair.close()


@pytest.mark.parametrize("dtype", ac.DTYPES)
@pytest.mark.parametrize("form", ac.FORMS, ids=FORM_IDS)
def test_special_actions(request, form, dtype):
    """batch(dtype) through the form, absolute and relative with sas = (-7, 9); the flexible kind goes on with mixed types."""
    for mode, sas in (("absolute", None), ("relative", ac.REL_SAS)):
        _special(request, form, dtype, mode, sas)


@pytest.mark.parametrize("sas", WIDE_SAS, ids=["sas3e9", "sasinf"])
@pytest.mark.parametrize("form", [f for f in ac.FORMS if f.entry != "history_observe"], ids=[n for n in FORM_IDS if not n.startswith("history")])
def test_relative_sum_has_no_32_bit_limit(request, form, sas):
    """Relative mode with an action space wider than int32: the f32 / f64 tables equal the definition (the sum is formed in
    double; as int32 it wraps and lands on 0 where the reference's int64 lands on the bound)."""
    for dtype in ("f32", "f64"):
        _special(request, form, dtype, "relative", sas)


def _states(form, flex):
    """(loc [N][2], res [N][2]) with the wild envs in the middle of the batch (two tame envs at each end)."""
    (oh, ow), (fh, fw) = form.obs, form.fov
    br, bc = oh - fh, ow - fw
    home = (min(2, br), min(3, bc))
    loc = [home, (0, 0), (-5, ow + 40), (oh, -3), (br + 1, bc + 1), (br, 0)]
    res = [(fh, fw)] * len(loc)
    if flex:
        loc += [(1, 1), (2, 1), (1, 2), home]
        res += [(0, 0), (-3, ow + 9), (oh + 1, 1), (oh - 1, ow - 1)]       # the last: in range, its loc valid only for a smaller res
    loc += [(0, bc), home]
    res += [(fh, fw), (fh, fw)]
    return loc, res


@pytest.mark.parametrize("form", ac.FORMS, ids=FORM_IDS)
def test_set_state_outside_the_frame_is_clamped_as_it_is_read(request, form):
    """set_fov_state(out of range), then in turn fovea(None), a location action (absolute and relative: both modes run), a
    resolution action, a masked call: the state out is next_state's, the observation the tame context's, nothing is written
    behind an output.  A masked-out env keeps the wild state it was given."""
    flex = ac.MODES[form.key][0] == "flexible"
    loc, res = _states(form, flex)
    n = len(loc)
    assert n >= 5 and all(0 <= v[0] <= form.obs[0] - form.fov[0] and 0 <= v[1] <= form.obs[1] - form.fov[1] for v in loc[:2] + loc[-2:])
    (oh, ow) = form.obs
    for mode, sas in (("absolute", None), ("relative", ac.REL_SAS)):
        pair = Pair(form, n, mode, sas, _seed(request, mode))
        rng = pair.rng
        lo_a, hi_a = ((-4.0, max(oh, ow) + 4.0) if pair.mode == "absolute" else (-9.0, 11.0))
        follow = [("no action", None, "f32", None, None),
                  ("location action", np.floor(rng.uniform(lo_a, hi_a, (n, 2))).astype(np.float32) + np.float32(0.5), "f32",
                   np.zeros(n, np.int32) if flex else None, None)]
        if flex:
            follow.append(("resolution action", np.stack([rng.integers(0, oh + 3, n), rng.integers(0, ow + 3, n)], 1).astype(np.int64), "i64",
                           np.ones(n, np.int32), None))
        if form.entry not in NO_MASK:
            mask = (np.arange(n) % 2).astype(np.uint8)             # wild envs on both sides of the mask
            follow.append(("masked call", rng.uniform(lo_a, hi_a, (n, 2)), "f64", ac.mixed_types(n, 0) if flex else None, mask))
        for name, action, dtype, types, mask in follow:
            pair.set_state(loc, res)
            pair.call(action, dtype, types, mask, (mode, name))
        pair.close()
