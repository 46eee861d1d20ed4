"""GPU: device-side minibatches on a rollout (include/agx_minibatch.h) through ObsPipeline + FrameHistory + StepLog + Rollout +
Minibatcher.  Which slot a row of a take holds is a pure integer function of (seed, list, the number of selects before, len, ends),
so every case compares every element of every output with tests/minibatch_model.py EXACTLY - floats as int32 bit patterns - in
buffers pre-filled with sentinels that must not survive, between guard regions that must.  The kernels need nothing of the
history but N, so the shape cases run on synthetic len / ends / index arrays at the small geometry (10 x 12, fovea 3 x 5,
fs = 3); the end-to-end cases run two scenarios of tests/rollout_model.py and a small AtariVecEnv."""
import ctypes

import numpy as np
import pytest
import torch

import minibatch_model as mm
import rollout_model as rm
from steplog_model import bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = ctypes.c_void_p
OBS, FOV = (10, 12), (3, 5)
F_SENT, B_SENT, I_SENT = -7.5, 0xAB, -9     # exact in float32 and no stream value; no payload-wide pattern; no slot, env or index
GUARD = 64                                   # elements on either side of every output


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ptr(t):
    return None if t is None else P(t.data_ptr())


class Rig:
    """A pipeline of N envs with a history, a step log, a Rollout and a Minibatcher on it."""

    def __init__(self, N, seed=5, T=8):
        from active_gym import FrameHistory, ObsPipeline, Rollout, StepLog
        self.pipe = ObsPipeline(num_envs=N, kind="fixed", obs_size=OBS, frame_stack=3, device=DEV, fov_size=FOV, fov_init_loc=(2, 3),
                                sensory_action_mode="absolute", antialias=True, resize_to_full=True, mask_out=False)
        self.hist = FrameHistory(self.pipe, T)
        self.log = StepLog(self.hist, rm.W)
        self.roll = Rollout(self.log)
        self.mb = self.roll.minibatcher(seed)
        self.model = mm.Model(N, seed)
        self.N, self.lib = N, self.mb._lib

    def close(self):
        self.pipe.close()


RIGS = {}


@pytest.fixture(scope="module")
def rigs():
    """One Rig per N, made at first use and shared by the shape cases: its model counts the selects with it."""
    def get(N):
        if N not in RIGS:
            RIGS[N] = Rig(N)
        return RIGS[N]
    yield get
    torch.cuda.synchronize()
    for r in RIGS.values():
        r.close()
    RIGS.clear()


class Guarded:
    """An output of `count` elements between two guard regions, all filled with the sentinel."""

    def __init__(self, count, dtype, sentinel):
        self.count, self.sentinel = count, sentinel
        self.t = torch.full((count + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        return P(self.t.data_ptr() + GUARD * self.t.element_size())

    def host(self):
        """The interior; the guards are checked on the way."""
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == self.sentinel).all() and (a[GUARD + self.count:] == self.sentinel).all(), "a guard region was written"
        return a[GUARD:GUARD + self.count]


def _device(a):
    return dict(len=_t(a["len"]), ends=_t(a["ends"]), obs_index=_t(a["obs_index"]), next_index=_t(a["next_index"]), payload=_t(a["payload"]),
                streams=[_t(s) for s in a["streams"]])


def _select(rig, which, a, d, L):
    total = torch.full((1,), I_SENT, dtype=torch.int32, device=DEV)
    from active_gym import _native as nat
    nat.check(rig.lib.agx_minibatch_select(rig.mb._m, which, L, _ptr(d["len"]), _ptr(d["ends"]), _ptr(total), rig.pipe._stream()), rig.pipe._ctx)
    want = rig.model.select(which, a["len"], a["ends"], L)
    assert int(total.item()) == want
    return want


# what a take passes: (n_f32, W, the outputs left NULL, the index inputs left NULL)
CONFIGS = ((8, 12, (), ()), (1, 4, ("env", "next_index", "valid"), ()), (0, 0, ("obs_index", "payload"), ("next_index",)))


def _take(rig, which, permute, a, d, L, first, S, config, what):
    """agx_minibatch_take on sentinel-filled, guarded outputs against the model, element for element."""
    from active_gym import _native as nat
    from active_gym.minibatch import MinibatchIo
    n_f32, W, null_out, null_in = config
    payload = a["payload"][..., :W]
    d_payload = _t(payload) if W else None
    outs = dict(slot=Guarded(S, torch.int32, I_SENT), env=Guarded(S, torch.int32, I_SENT), obs_index=Guarded(S, torch.int64, I_SENT),
                next_index=Guarded(S, torch.int64, I_SENT), payload=Guarded(S * W, torch.uint8, B_SENT), valid=Guarded(S, torch.uint8, B_SENT))
    streams = [Guarded(S, torch.float32, F_SENT) for _ in range(n_f32)]
    io = MinibatchIo()
    io.d_obs_index = None if "obs_index" in null_in else _ptr(d["obs_index"])
    io.d_next_index = None if "next_index" in null_in else _ptr(d["next_index"])
    io.d_payload, io.payload_bytes, io.n_f32 = _ptr(d_payload), W, n_f32
    for key, field in (("slot", "d_slot"), ("env", "d_env"), ("obs_index", "d_obs_index_out"), ("next_index", "d_next_index_out"),
                       ("payload", "d_payload_out"), ("valid", "d_valid")):
        setattr(io, field, None if key in null_out or (key == "payload" and not W) else outs[key].ptr)
    for k in range(n_f32):
        io.src_f32[k], io.dst_f32[k] = d["streams"][k].data_ptr(), streams[k].ptr.value
    rc = rig.lib.agx_minibatch_take(rig.mb._m, which, permute, L, _ptr(d["len"]), _ptr(d["ends"]), first, S, ctypes.byref(io), rig.pipe._stream())
    nat.check(rc, rig.pipe._ctx)
    want = rig.model.take(which, bool(permute), a["len"], a["ends"], L, first, S, None if "obs_index" in null_in else a["obs_index"],
                          None if "next_index" in null_in else a["next_index"], payload if W else None, a["streams"][:n_f32])
    for key, g in outs.items():
        got = g.host()
        if key in null_out or (key == "payload" and not W):
            assert (got == g.sentinel).all(), f"{key} was passed as NULL and written ({what})"
        else:
            assert np.array_equal(got, want[key].reshape(-1)), f"{key} differs from the model ({what})"
    for k, g in enumerate(streams):
        assert np.array_equal(g.host().view(np.int32), want["streams"][k].view(np.int32)), f"stream {k} differs from the model ({what})"
    return want


def _forms(total):
    """(first, S): one row; a range crossing total; more than two lists; a start behind the list."""
    return ((total // 2, 1), (max(total - 2, 0), 5), (0, 2 * total + 3), (total + 1, 4))


# ---------------------------------------------------------------------------------------------- 1. shapes
SHAPES = [(N, L) for N in (1, 3, 64, 65, 130) for L in (1, 2, 37)] + [(3, 65)]


@pytest.mark.parametrize("N,L", SHAPES)
def test_take_equals_the_model_in_every_element(rigs, N, L):
    rig = rigs(N)
    a = mm.rollout_arrays(100 + N * 131 + L, N, L)
    d = _device(a)
    live = np.arange(L)[:, None] >= L - np.clip(a["len"], 0, L)[None, :]
    if N >= 64:
        assert ((a["ends"] & 8 != 0) & ~live).any(), "no BOOT bit on a slot that is not live: it must be there and not be counted"
    for which in (mm.LIVE, mm.BOOT):
        total = _select(rig, which, a, d, L)
        for permute in (0, 1):
            for i, (first, S) in enumerate(_forms(total)):
                config = CONFIGS[(i + permute + which) % 3]
                want = _take(rig, which, permute, a, d, L, first, S, config, f"which {which}, permute {permute}, first {first}, S {S}, config {config[:2]}")
                if total:
                    assert want["valid"].tolist() == [int(first + j < total) for j in range(S)] and (want["slot"] >= 0).all()
        if total > 8:                              # a second epoch of the same list is another order of the same slots
            before = rig.model.take(which, True, a["len"], a["ends"], L, 0, total)["slot"]
            _select(rig, which, a, d, L)
            after = _take(rig, which, 1, a, d, L, 0, total, CONFIGS[1], "the second epoch")["slot"]
            assert sorted(before.tolist()) == sorted(after.tolist()) and before.tolist() != after.tolist()


@pytest.mark.parametrize("N", [1, 65])
def test_an_empty_list(rigs, N):
    """total == 0 - no live slot, or live slots without BOOT: slot -1, env 0, indices -1, zeros, valid 0 in every row."""
    rig, L = rigs(N), 3
    a = mm.rollout_arrays(40 + N, N, L)
    a["len"][:] = 0
    b = dict(a, len=np.full(N, L, np.int32), ends=(a["ends"] & 7).astype(np.uint8))
    for which, arrays in ((mm.LIVE, a), (mm.BOOT, a), (mm.BOOT, b)):
        d = _device(arrays)
        assert _select(rig, which, arrays, d, L) == 0
        for permute in (0, 1):
            want = _take(rig, which, permute, arrays, d, L, 0, 7, CONFIGS[0], f"empty list {which}")
            assert (want["slot"] == -1).all() and not want["env"].any() and not want["valid"].any() and (want["obs_index"] == -1).all()
            assert not want["payload"].any() and not any(s.any() for s in want["streams"])


@pytest.mark.parametrize("N,L", [(5, 37), (65, 2), (130, 37)])
def test_other_arrays_than_select_saw_are_invalid_rather_than_wrong(rigs, N, L):
    """take with other len / ends than select saw: the rows whose slot no longer exists are invalid, every other row is the
    model's, and nothing outside the outputs is written (the guard regions of every buffer)."""
    rig = rigs(N)
    a, b = mm.rollout_arrays(100 + N * 131 + L, N, L), mm.rollout_arrays(900 + N * 131 + L, N, L)
    da, db = _device(a), _device(b)
    lost = 0
    for which in (mm.LIVE, mm.BOOT):
        total = _select(rig, which, a, da, L)
        for permute in (0, 1):
            want = _take(rig, which, permute, b, db, L, 0, total + 5, CONFIGS[0], f"mismatched, which {which}, permute {permute}")
            gone = want["slot"][:total] < 0
            assert not want["valid"][:total][gone].any() and want["valid"][:total][~gone].all() and not want["env"][:total][gone].any()
            lost += int(gone.sum())
    assert lost > 0, "the second arrays lose no slot: the case shows nothing"


# ---------------------------------------------------------------------------------------------- 2. scatter
def test_scatter_skips_invalid_rows_and_slots_out_of_range(rigs):
    from active_gym import _native as nat
    N, L = 65, 3
    rig = rigs(N)
    cells = L * N
    rng = np.random.default_rng(3)
    good = rng.permutation(cells)[:40].astype(np.int32)
    slot = np.concatenate([good[:20], [-1, cells, cells + 7, -5, 2 ** 31 - 1], good[20:]]).astype(np.int32)
    valid = np.ones(len(slot), np.uint8)
    valid[[3, 30]] = 0
    src = rng.standard_normal(len(slot)).astype(np.float32)
    dst = Guarded(cells, torch.float32, F_SENT)
    d_slot, d_valid, d_src = _t(slot), _t(valid), _t(src)          # (named: a temporary's memory is the next temporary's)
    rc = rig.lib.agx_minibatch_scatter(rig.mb._m, len(slot), _ptr(d_slot), _ptr(d_valid), _ptr(d_src), L, dst.ptr, rig.pipe._stream())
    nat.check(rc, rig.pipe._ctx)
    want = mm.scatter(slot, valid, src, np.full((L, N), F_SENT, np.float32))
    got = dst.host()
    assert np.array_equal(got.view(np.int32), want.reshape(-1).view(np.int32))
    assert int((got != F_SENT).sum()) == 38        # 40 good slots, two of them in rows that are not valid
    # the Python surface
    out = torch.full((L, N), F_SENT, device=DEV)
    rig.mb.scatter({"slot": _t(slot), "valid": _t(valid)}, _t(src)[:, None], out)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


# ---------------------------------------------------------------------------------------------- 3. a captured graph
def test_captured_graph_of_select_and_take():
    """select + take captured under torch.cuda.graph on one side stream: replay k equals the model at call k, and two replays
    are two different orders of the same slots."""
    N, L, seed = 65, 37, 11
    rig = Rig(N, seed)
    a = mm.rollout_arrays(77, N, L)
    batch = {k: _t(a[k]) for k in ("len", "ends", "obs_index", "next_index", "payload")}
    adv = _t(a["streams"][0])
    S = L * N
    out = rig.mb.take(batch, 0, S, streams={"adv": adv})          # before any select: total is 0, every row invalid
    assert not out["valid"].any() and (out["slot"] == -1).all()

    def work():
        rig.mb.select(batch)
        rig.mb.take(batch, 0, S, streams={"adv": adv}, out=out)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        work()                                    # call 0
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        work()                                    # captured, not run
    rig.model.select(mm.LIVE, a["len"], a["ends"], L)
    seen = []
    for call in (1, 2):
        for t in out.values():
            t.fill_(1)                            # nothing of the replay before may pass for this one's
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        total = rig.model.select(mm.LIVE, a["len"], a["ends"], L)
        assert int(rig.mb.total().item()) == total and rig.model.calls[0] == call + 1
        want = rig.model.take(mm.LIVE, True, a["len"], a["ends"], L, 0, S, a["obs_index"], a["next_index"], a["payload"], [a["streams"][0]])
        for key in ("slot", "env", "obs_index", "next_index", "payload", "valid"):
            assert np.array_equal(out[key].cpu().numpy(), want[key]), (key, call)
        assert np.array_equal(bits(out["adv"].cpu().numpy()), bits(want["streams"][0])), call
        seen.append(want["slot"][:total].tolist())
    assert seen[0] != seen[1] and sorted(seen[0]) == sorted(seen[1])
    torch.cuda.synchronize()
    rig.close()


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_in_the_stated_order():
    from active_gym import _native as nat
    from active_gym.minibatch import MinibatchIo
    N, L = 3, 4
    rig = Rig(N)
    lib, st, m = rig.lib, rig.pipe._stream(), rig.mb._m
    a = mm.rollout_arrays(1, N, L)
    d = _device(a)
    slot = torch.full((8,), I_SENT, dtype=torch.int32, device=DEV)
    f = torch.zeros((L, N), device=DEV)
    total = torch.full((1,), I_SENT, dtype=torch.int32, device=DEV)

    def io(n_f32=0, slot_=slot):
        x = MinibatchIo()
        x.n_f32, x.d_slot = n_f32, _ptr(slot_)
        return ctypes.byref(x)

    def select(mb=m, which=0, L=L, length=d["len"], ends=d["ends"]):
        return lib.agx_minibatch_select(mb, which, L, _ptr(length), _ptr(ends), _ptr(total), st)

    def take(mb=m, which=0, L=L, length=d["len"], ends=d["ends"], first=0, S=8, io_=None):
        return lib.agx_minibatch_take(mb, which, 1, L, _ptr(length), _ptr(ends), first, S, io() if io_ is None else io_, st)

    def scatter(mb=m, S=8, slot_=slot, valid=d["ends"], src=f, L=L, dst=f):
        return lib.agx_minibatch_scatter(mb, S, _ptr(slot_), _ptr(valid), _ptr(src), L, _ptr(dst), st)

    big = 2 ** 31 - 1
    cases = [
        # 1. the handle, whatever else is wrong
        (select, dict(mb=None, which=5, L=0, length=None), "null argument (mb)", False),
        (take, dict(mb=None, which=5, L=0, S=-1, io_=io(9, None)), "null argument (mb)", False),
        (scatter, dict(mb=None, S=-1, L=0, dst=None), "null argument (mb)", False),
        # 2. which, before L
        (select, dict(which=2, L=0), "which must be", True), (select, dict(which=-1), "which must be", True),
        (take, dict(which=2, L=0, S=-1), "which must be", True),
        # 3. L, before S and first
        (select, dict(L=0, length=None), "L must be 1 .. 4096", True), (select, dict(L=4097), "L must be 1 .. 4096", True),
        (take, dict(L=0, S=-1), "L must be 1 .. 4096", True), (take, dict(L=4097, first=-1), "L must be 1 .. 4096", True),
        (scatter, dict(L=0, S=-1), "L must be 1 .. 4096", True), (scatter, dict(L=4097, dst=None), "L must be 1 .. 4096", True),
        # 4. S and first, before n_f32
        (take, dict(S=-1, io_=io(9)), "first = 0, S = -1", True), (take, dict(first=-1, io_=io(9)), "first = -1", True),
        (take, dict(first=big, S=1, io_=io(-1)), "first + S", True), (take, dict(first=big - 7, S=8, length=None), "first + S", True),
        (scatter, dict(S=-1, dst=None), "S = -1", True),
        # 5. n_f32, before the buffers
        (take, dict(io_=io(9, None)), "n_f32 must be 0 .. 8", True), (take, dict(io_=io(-1), length=None), "n_f32 must be 0 .. 8", True),
        (take, dict(io_=ctypes.POINTER(MinibatchIo)()), "null argument (io)", True),
        # 6. the required buffers
        (select, dict(length=None), "null buffer (d_len)", True), (select, dict(which=1, ends=None), "null buffer (d_ends)", True),
        (take, dict(length=None), "null buffer (d_len)", True), (take, dict(io_=io(0, None)), "null buffer (d_slot)", True),
        (take, dict(which=1, ends=None), "null buffer (d_ends)", True),
        (scatter, dict(slot_=None), "null buffer (d_slot)", True), (scatter, dict(valid=None), "null buffer (d_valid)", True),
        (scatter, dict(src=None), "null buffer (d_src)", True), (scatter, dict(dst=None), "null buffer (d_dst)", True),
    ]
    for call, kw, named, has_ctx in cases:
        assert call(**kw) == nat.E_INVALID, (call.__name__, kw)
        msg = nat.last_error(rig.pipe._ctx if has_ctx else None)
        assert named in msg and "agx_minibatch_" + call.__name__ in msg, (call.__name__, kw, msg)
    torch.cuda.synchronize()
    assert (slot == I_SENT).all() and int(total.item()) == I_SENT and not f.any()       # no refused call launched anything
    assert select(ends=None) == nat.OK            # LIVE reads no ends byte
    assert take(S=0, io_=io(0, None)) == nat.E_INVALID and take(S=0) == nat.OK and scatter(S=0) == nat.OK
    torch.cuda.synchronize()
    assert (slot == I_SENT).all(), "S == 0 launches nothing"
    # the Python surface refuses before any GPU work
    batch = {k: d[k] for k in ("len", "ends", "obs_index", "next_index", "payload")}
    for call in (lambda: rig.mb.select(batch, "dead"), lambda: rig.mb.take(batch, 0, -1), lambda: rig.mb.take(batch, -1, 4),
                 lambda: rig.mb.take(batch, 0, 4, streams={f"s{k}": f for k in range(9)}), lambda: rig.mb.take(batch, 0, 4, streams={"slot": f})):
        with pytest.raises(ValueError):
            call()
    # a narrowed env range: AGX_E_STATE from every call
    rows = rig.mb.take(batch, 0, 4)
    rig.pipe.env_range(1, 2)
    for call in (lambda: rig.mb.select(batch), lambda: rig.mb.take(batch, 0, 4), lambda: rig.mb.scatter(rows, torch.zeros(4, device=DEV), f),
                 lambda: rig.roll.minibatcher(1)):
        with pytest.raises(nat.AgxError, match="env range") as e:
            call()
        assert e.value.code == nat.E_STATE
    rig.pipe.env_range()
    rig.mb.select(batch)
    torch.cuda.synchronize()
    rig.hist.close()                              # the history closes its minibatchers first
    assert not rig.mb.alive
    with pytest.raises(RuntimeError, match="closed"):
        rig.mb.select(batch)
    rig.close()


# ---------------------------------------------------------------------------------------------- 5. end to end
class Case:
    """A pipeline with a history, a step log and a Rollout on it, driven over a scripted scenario of tests/rollout_model.py."""

    def __init__(self, name):
        from active_gym import FrameHistory, ObsPipeline, Rollout, StepLog
        seed, N, fs, T, _, self.Ls, _, _ = rm.CASES[name]
        self.pipe = ObsPipeline(num_envs=N, kind="fixed", obs_size=OBS, frame_stack=fs, device=DEV, fov_size=FOV, fov_init_loc=(2, 3),
                                sensory_action_mode="absolute", antialias=True, resize_to_full=True, mask_out=False)
        self.hist = FrameHistory(self.pipe, T)
        self.log = StepLog(self.hist, rm.W)
        self.roll = Rollout(self.log)
        self.N = N
        self.rng = np.random.default_rng(seed + 2000)
        _, self.hm, self.lm = rm.case_models(name, push=self.push)

    def push(self, cmd, idx, rec):
        if cmd is None:
            self.hist.clear()
            return
        N = self.N
        self.pipe.ingest_gray(_t(self.rng.integers(0, 256, (N, 2) + OBS, dtype=np.uint8)), _t(cmd))
        self.pipe.fovea(_t(self.rng.uniform(-3, 14, (N, 2)).astype(np.float32)))
        self.hist.push(_t(cmd))
        if rec is not None:
            index, reward, flags, payload = rec
            self.log.record(_t(index), _t(reward), _t(flags), _t(payload))

    def close(self):
        self.pipe.close()


def _critic(env, index):
    """A synthetic critic: a function of (env, index), exact in float32."""
    return (env.to(torch.float32) * 64.0 + (index % 64).to(torch.float32) + 0.5) * (index >= 0).to(torch.float32)


@pytest.mark.parametrize("name", ["small", "long"])
def test_the_lists_are_flat_and_boot_rows(name):
    """On a scripted scenario: (env, index) of the LIVE list equals Rollout.flat as a set, and a boot_value built by BOOT take +
    scatter gives agx_rollout_gae the same bits as the one built through boot_rows."""
    c = Case(name)
    mb = c.roll.minibatcher(3)
    for L in c.Ls:
        N = c.N
        batch = c.roll.gather(L)
        env, index = c.roll.flat(batch)
        flat = sorted(zip(env.cpu().tolist(), index.cpu().tolist()))
        total = mb.select(batch)
        rows = mb.take(batch, 0, L * N + 3, streams={"reward": batch["reward"]})
        total = int(total.item())
        valid = rows["valid"].cpu().numpy().astype(bool)
        assert total == len(flat) and valid.tolist() == [True] * total + [False] * (L * N + 3 - total)
        assert sorted(zip(rows["env"].cpu().numpy()[valid].tolist(), rows["obs_index"].cpu().numpy()[valid].tolist())) == flat
        slot = rows["slot"].cpu().numpy()
        assert (slot >= 0).all() and np.array_equal(bits(rows["reward"].cpu().numpy()), bits(batch["reward"].cpu().numpy().reshape(-1)[slot]))
        assert np.array_equal(rows["payload"].cpu().numpy(), batch["payload"].cpu().numpy().reshape(L * N, -1)[slot])
        _, _, ok = c.hist.observe(rows["env"], rows["obs_index"])          # every row, wrapped ones included, can be re-created
        assert bool(ok.all())
        # boot_value, both ways
        at, benv, bindex = c.roll.boot_rows(batch)
        old = torch.zeros((L, N), device=DEV)
        old[at[:, 0], at[:, 1]] = _critic(benv, bindex)
        mb.select(batch, "boot")
        boot = mb.take(batch, 0, L * N, which="boot", permute=False)
        assert int(mb.total("boot").item()) == len(at) >= 1
        in_list_order = sorted((at[:, 0] * N + at[:, 1]).cpu().tolist(), key=lambda e: (e % N, e // N))       # env-major, ascending t
        assert boot["slot"].cpu().tolist()[:len(at)] == in_list_order and boot["valid"].cpu().tolist() == [1] * len(at) + [0] * (L * N - len(at))
        new = mb.scatter(boot, _critic(boot["env"], boot["next_index"]), torch.zeros((L, N), device=DEV))
        assert torch.equal(new.view(torch.int32), old.view(torch.int32)) and bool((new != 0).any())
        value = torch.randn((L, N), device=DEV)
        a0, r0 = c.roll.gae(batch, value, old, 0.99, 0.95)
        a1, r1 = c.roll.gae(batch, value, new, 0.99, 0.95)
        assert torch.equal(a0.view(torch.int32), a1.view(torch.int32)) and torch.equal(r0.view(torch.int32), r1.view(torch.int32))
    torch.cuda.synchronize()
    c.close()


def test_vec_env_minibatches_cover_every_live_slot_once():
    """AtariVecEnv(history_len = 16, step_log = True), 40 random steps with autoresets, rollout_batch(12): one epoch of
    rollout_minibatches covers every live slot exactly once, its actions and streams are rollout_batch's at the same slots, a
    second epoch is another order, and rollout_boot is boot_rows without the wait."""
    from active_gym import AtariEnvArgs, AtariVecEnv, Rollout
    N, STEPS, L, SIZE = 6, 40, 12, 16
    kw = dict(game="g", seed=3, obs_size=(84, 84), frame_stack=4, fov_size=(30, 30), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=30, native_loop=True, history_len=16, step_log=True)
    env = AtariVecEnv(AtariEnvArgs(**kw), N, kind="fixed", noop_fn=lambda: 2)
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(STEPS):
        env.step({"motor_action": rng.integers(0, 4, N), "sensory_action": rng.uniform(-5, 90, (N, 2)).astype(np.float32)})
    batch = env.rollout_batch(L)
    live = batch["live"].cpu().numpy()
    want = sorted((np.nonzero(live)[0] * N + np.nonzero(live)[1]).tolist())
    assert 0 < len(want) <= L * N < 5 * SIZE, "the last minibatch must reach past the list"
    adv = torch.randn((L, N), device=DEV)
    motor, sens = batch["motor_action"].cpu().numpy().reshape(-1), batch["sensory_action"].cpu().numpy().reshape(-1, 2)
    orders = []
    for epoch in range(2):
        got = list(env.rollout_minibatches(batch, SIZE, {"adv": adv, "reward": batch["reward"]}))
        assert len(got) == -(-L * N // SIZE)
        slots = []
        for rows in got:
            assert sorted(rows) == sorted(["slot", "env", "obs_index", "next_index", "valid", "motor_action", "sensory_action", "adv", "reward"])
            assert all(int(v.shape[0]) == SIZE for v in rows.values()) and tuple(rows["sensory_action"].shape) == (SIZE, 2)
            slot, valid = rows["slot"].cpu().numpy(), rows["valid"].cpu().numpy().astype(bool)
            assert (slot >= 0).all()
            assert np.array_equal(rows["motor_action"].cpu().numpy(), motor[slot]) and rows["motor_action"].dtype == torch.int32
            assert np.array_equal(bits(rows["sensory_action"].cpu().numpy()), bits(sens[slot]))
            assert np.array_equal(bits(rows["adv"].cpu().numpy()), bits(adv.cpu().numpy().reshape(-1)[slot]))
            assert np.array_equal(rows["env"].cpu().numpy(), slot % N)
            assert np.array_equal(rows["obs_index"].cpu().numpy(), batch["obs_index"].cpu().numpy().reshape(-1)[slot])
            assert bool(env.history.observe(rows["env"], rows["obs_index"])[2].all())
            slots += slot[valid].tolist()
        assert sorted(slots) == want, "an epoch covers every live slot exactly once"
        orders.append(slots)
    assert orders[0] != orders[1]
    rows = env.rollout_boot(batch)
    at, benv, bindex = Rollout(env.steplog).boot_rows(batch)
    k = len(at)
    assert int(rows["total"].item()) == k and int(rows["slot"].shape[0]) == 2 * N and rows["valid"].cpu().tolist() == [1] * k + [0] * (2 * N - k)
    assert sorted(zip(rows["env"].cpu().tolist()[:k], rows["next_index"].cpu().tolist()[:k])) == sorted(zip(benv.cpu().tolist(), bindex.cpu().tolist()))
    boot = env.rollout_scatter(rows, _critic(rows["env"], rows["next_index"]), torch.zeros((L, N), device=DEV))
    old = torch.zeros((L, N), device=DEV)
    old[at[:, 0], at[:, 1]] = _critic(benv, bindex)
    assert torch.equal(boot.view(torch.int32), old.view(torch.int32))
    torch.cuda.synchronize()
    env.close()
