"""GPU: device-side minibatches of chunks on a rollout (include/agx_chunks.h) through ObsPipeline + FrameHistory + StepLog +
Rollout + Chunker.  Which chunk a row of a take holds is a pure integer function of (seed, the number of selects before, len), so
every case compares every element of every output with tests/chunks_model.py EXACTLY - floats as int32 bit patterns - in buffers
pre-filled with sentinels that must not survive, between guard regions that must.  The kernels need nothing of the history but N,
so the shape cases run on synthetic len / ends / index arrays at the small geometry (10 x 12, fovea 3 x 5, fs = 3); the end-to-end
case runs a small AtariVecEnv under both step loops."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import chunks_model as cm
from steplog_model import bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = ctypes.c_void_p
OBS, FOV = (10, 12), (3, 5)
F_SENT, B_SENT, I_SENT = -7.5, 0xAB, -9     # exact in float32 and no stream value; no payload-wide pattern; no slot, env or index
GUARD = 64                                   # elements on either side of every output
STEP_OUT = (("slot", "d_slot", torch.int32), ("env", "d_env", torch.int32), ("obs_index", "d_obs_index_out", torch.int64),
            ("next_index", "d_next_index_out", torch.int64), ("ends", "d_ends_out", torch.uint8), ("start", "d_start", torch.uint8),
            ("mask", "d_mask", torch.uint8))
CHUNK_OUT = (("chunk", "d_chunk", torch.int32), ("first", "d_first", torch.int32), ("steps", "d_steps", torch.int32),
             ("state_index", "d_state_index", torch.int64), ("valid", "d_valid", torch.uint8))


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ptr(t):
    return None if t is None else P(t.data_ptr())


class Rig:
    """A pipeline of N envs with a history, a step log, a Rollout and a Chunker on it."""

    def __init__(self, N, seed=5, T=8):
        from active_gym import FrameHistory, ObsPipeline, Rollout, StepLog
        self.pipe = ObsPipeline(num_envs=N, kind="fixed", obs_size=OBS, frame_stack=3, device=DEV, fov_size=FOV, fov_init_loc=(2, 3),
                                sensory_action_mode="absolute", antialias=True, resize_to_full=True, mask_out=False)
        self.hist = FrameHistory(self.pipe, T)
        self.log = StepLog(self.hist, 12)
        self.roll = Rollout(self.log)
        self.ch = self.roll.chunker(seed)
        self.model = cm.Model(N, seed)
        self.N, self.lib = N, self.ch._lib

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


class Inputs:
    """The arrays of a rollout (tests/chunks_model.py's rollout_arrays) on the host, as `a`, and on the device."""

    def __init__(self, a):
        self.a = a
        self.len, self.ends = _t(a["len"]), _t(a["ends"])
        self.obs_index, self.next_index, self.payload = _t(a["obs_index"]), _t(a["next_index"]), _t(a["payload"])
        self.streams = [_t(s) for s in a["streams"]]


def _select(rig, inp, L, C):
    from active_gym import _native as nat
    total = torch.full((1,), I_SENT, dtype=torch.int32, device=DEV)
    nat.check(rig.lib.agx_chunks_select(rig.ch._c, L, C, _ptr(inp.len), _ptr(total), rig.pipe._stream()), rig.pipe._ctx)
    want = rig.model.select(inp.a["len"], L, C)
    assert int(total.item()) == want
    return want


# what a take passes: n_f32, W, the outputs left NULL, the inputs left NULL, the stream sources / destinations left NULL
CONFIGS = (
    dict(n_f32=8, W=12, null_out=(), null_in=(), null_src=(), null_dst=()),
    dict(n_f32=1, W=4, null_out=("env", "next_index", "valid", "ends", "first", "mask"), null_in=(), null_src=(), null_dst=()),
    dict(n_f32=0, W=0, null_out=("obs_index", "payload", "start", "chunk", "steps", "state_index"), null_in=("next_index",), null_src=(), null_dst=()),
    dict(n_f32=8, W=12, null_out=(), null_in=("obs_index", "payload"), null_src=(2,), null_dst=(5,)),
)


def _take(rig, permute, inp, L, C, first, S, config, what):
    """agx_chunks_take on sentinel-filled, guarded outputs against the model, element for element."""
    from active_gym import _native as nat
    from active_gym.chunks import ChunkIo
    a = inp.a
    n_f32, W, null_out, null_in = config["n_f32"], config["W"], config["null_out"], config["null_in"]
    payload = a["payload"][..., :W]
    d_payload = _t(payload) if W and "payload" not in null_in else None
    outs = {key: Guarded(C * S, dtype, B_SENT if dtype == torch.uint8 else I_SENT) for key, _, dtype in STEP_OUT}
    outs.update({key: Guarded(S, dtype, B_SENT if dtype == torch.uint8 else I_SENT) for key, _, dtype in CHUNK_OUT})
    outs["payload"] = Guarded(C * S * W, torch.uint8, B_SENT)
    streams = [Guarded(C * S, torch.float32, F_SENT) for _ in range(n_f32)]
    io = ChunkIo()
    io.d_obs_index = None if "obs_index" in null_in else _ptr(inp.obs_index)
    io.d_next_index = None if "next_index" in null_in else _ptr(inp.next_index)
    io.d_payload, io.payload_bytes, io.n_f32 = _ptr(d_payload), W, n_f32
    skipped = set(null_out) | ({"payload"} if not W else set())
    for key, field, _ in STEP_OUT + CHUNK_OUT + (("payload", "d_payload_out", None),):
        setattr(io, field, None if key in skipped else outs[key].ptr)
    for k in range(n_f32):
        io.src_f32[k] = None if k in config["null_src"] else inp.streams[k].data_ptr()
        io.dst_f32[k] = None if k in config["null_dst"] else streams[k].ptr.value
    rc = rig.lib.agx_chunks_take(rig.ch._c, permute, L, C, _ptr(inp.len), _ptr(inp.ends), first, S, ctypes.byref(io), rig.pipe._stream())
    nat.check(rc, rig.pipe._ctx)
    want = rig.model.take(bool(permute), a["len"], a["ends"], L, C, first, S, None if "obs_index" in null_in else a["obs_index"],
                          None if "next_index" in null_in else a["next_index"],
                          (np.zeros_like(payload) if "payload" in null_in else payload) if W else None,
                          [np.zeros_like(a["streams"][k]) if k in config["null_src"] else a["streams"][k] for k in range(n_f32)])
    for key, g in outs.items():
        got = g.host()
        if key in skipped:
            assert (got == g.sentinel).all(), f"{key} was passed as NULL and written ({what})"
        else:
            assert np.array_equal(got, want[key].reshape(-1)), f"{key} differs from the model ({what})"
    for k, g in enumerate(streams):
        got = g.host()
        if k in config["null_dst"]:
            assert (got == F_SENT).all(), f"stream {k} was passed as NULL and written ({what})"
        else:
            assert np.array_equal(got.view(np.int32), want["streams"][k].reshape(-1).view(np.int32)), f"stream {k} differs from the model ({what})"
            assert np.isfinite(got).all(), f"stream {k}: a value of a slot that is not live reached the output ({what})"
    return want


# ---------------------------------------------------------------------------------------------- 1. shapes
SHAPES = [(1, 1), (3, 2), (5, 37), (64, 2), (65, 5), (130, 37), (3, 65)]
LENGTHS = (1, 2, 5, 37, 64, None)            # C; None: L
SIZES = (1, 63, 64, 65, 300)                 # S


def _lengths(L):
    return sorted({L if c is None else c for c in LENGTHS if (c or L) <= L})


def _plan(N, L):
    """[(C, [(S, where, permute, config)])] of a shape: every C of the list that fits L and, per C, one take per S whose `where`
    (first = 0, mid-list, past total: every row wrapped), permute and config rotate with a counter."""
    turn = itertools.count(SHAPES.index((N, L)))
    plan = []
    for C in _lengths(L):
        takes = []
        for j, S in enumerate(SIZES):
            k = next(turn)
            takes.append((S, (k + j) % 3, (k // 3 + j) % 2, (k + 2 * j) % 4))
        plan.append((C, takes))
    return plan


def test_the_plan_crosses_every_size_with_every_first_permute_and_config():
    takes = [t for N, L in SHAPES for _, ts in _plan(N, L) for t in ts]
    assert {t[:3] for t in takes} == {(S, w, p) for S in SIZES for w in range(3) for p in range(2)}
    assert {(t[0], t[3]) for t in takes} == {(S, c) for S in SIZES for c in range(4)}
    assert {C for N, L in SHAPES for C, _ in _plan(N, L)} == {1, 2, 5, 37, 64, 65}


@pytest.mark.parametrize("N,L", SHAPES)
def test_take_equals_the_model_in_every_element(rigs, N, L):
    rig = rigs(N)
    inp = Inputs(cm.rollout_arrays(100 + N * 131 + L, N, L))
    live = np.arange(L)[:, None] >= L - np.clip(inp.a["len"], 0, L)[None, :]
    assert all(np.isfinite(s[live]).all() and not np.isfinite(s[~live]).any() for s in inp.a["streams"])
    for C, takes in _plan(N, L):
        total = _select(rig, inp, L, C)
        for S, where, permute, config in takes:
            first = (0, total // 2, total + 1)[where]
            want = _take(rig, permute, inp, L, C, first, S, CONFIGS[config], f"N {N}, L {L}, C {C}, S {S}, first {first}, permute {permute}")
            if total:
                assert want["valid"].tolist() == [int(first + s < total) for s in range(S)] and (want["chunk"] >= 0).all()
                assert ((want["slot"] >= 0).sum(0) == want["steps"]).all() and (want["steps"] >= 1).all()
                if where == 2:
                    assert not want["mask"].any() and (want["slot"] >= 0).any(), "a wrapped row holds a real chunk with mask 0"
        if total > 8:                              # a second epoch is another order of the same chunks
            before = rig.model.take(True, inp.a["len"], inp.a["ends"], L, C, 0, total)
            _select(rig, inp, L, C)
            after = _take(rig, 1, inp, L, C, 0, total, CONFIGS[0], "the second epoch")
            order = [list(zip(w["env"][0].tolist(), w["chunk"].tolist())) for w in (before, after)]
            assert sorted(order[0]) == sorted(order[1]) and order[0] != order[1]


@pytest.mark.parametrize("N", [1, 65])
def test_an_empty_list(rigs, N):
    """Every len is 0 (or below): total == 0 and every row is the null row."""
    rig, L, C = rigs(N), 5, 2
    inp = Inputs(cm.rollout_arrays(40 + N, N, L, empty=True))
    if N > 2:
        inp.a["len"][2] = -3
        inp = Inputs(inp.a)
    assert _select(rig, inp, L, C) == 0
    for permute, S, config in ((0, 7, CONFIGS[0]), (1, 65, CONFIGS[3])):
        want = _take(rig, permute, inp, L, C, 0, S, config, "empty list")
        assert (want["slot"] == -1).all() and not want["env"].any() and not want["valid"].any() and (want["obs_index"] == -1).all()
        assert (want["chunk"] == -1).all() and not want["first"].any() and not want["steps"].any() and (want["state_index"] == -1).all()
        assert not want["payload"].any() and not any(s.any() for s in want["streams"]) and not want["mask"].any() and not want["start"].any()


@pytest.mark.parametrize("N,L,C", [(5, 37, 5), (65, 5, 2), (130, 37, 37)])
def test_other_arguments_than_select_saw_are_invalid_rather_than_wrong(rigs, N, L, C):
    """take with another d_len than select saw: the rows whose chunk no longer exists are null rows, every other row is the
    model's.  take with another (L, C): null rows throughout.  Nothing outside the outputs is written (the guard regions)."""
    rig = rigs(N)
    a, b = cm.rollout_arrays(100 + N * 131 + L, N, L), cm.rollout_arrays(900 + N * 131 + L, N, L)
    ia, ib = Inputs(a), Inputs(b)
    total = _select(rig, ia, L, C)
    lost = 0
    for permute in (0, 1):
        want = _take(rig, permute, ib, L, C, 0, total + 5, CONFIGS[0], f"another len, permute {permute}")
        gone = want["chunk"][:total] < 0
        assert not want["valid"][:total][gone].any() and want["valid"][:total][~gone].all() and not want["env"][:, :total][:, gone].any()
        lost += int(gone.sum())
    assert lost > 0, "the second arrays lose no chunk: the case shows nothing"
    for L2, C2 in ((L, C - 1), (L, min(C + 1, L)), (L - 1, min(C, L - 1))):
        if (L2, C2) == (L, C):
            continue
        short = Inputs({k: v if k == "len" else [s[:L2] for s in v] if k == "streams" else v[:L2] for k, v in a.items()})
        want = _take(rig, 1, short, L2, C2, 0, 70, CONFIGS[0], f"(L, C) = {(L2, C2)} after select({(L, C)})")
        assert (want["chunk"] == -1).all() and (want["slot"] == -1).all() and not want["valid"].any()


# ---------------------------------------------------------------------------------------------- 2. a captured graph
def test_captured_graph_of_select_and_takes():
    """select + two takes captured under torch.cuda.graph on one side stream: replay k equals the model at call k, and two
    replays are two different orders of the same chunks."""
    N, L, C, seed = 65, 37, 5, 11
    rig = Rig(N, seed)
    a = cm.rollout_arrays(77, N, L)
    batch = {k: _t(a[k]) for k in ("len", "ends", "obs_index", "next_index", "payload")}
    adv = _t(np.nan_to_num(a["streams"][0], nan=0.0, posinf=0.0, neginf=0.0))
    half = (N * -(-L // C) + 1) // 2
    outs = [rig.ch.take(batch, k * half, half, C, streams={"adv": adv}) for k in range(2)]        # before any select: null rows
    assert not outs[0]["valid"].any() and (outs[0]["slot"] == -1).all() and (outs[1]["chunk"] == -1).all()

    def work():
        rig.ch.select(batch, C)
        for k in range(2):
            rig.ch.take(batch, k * half, half, C, streams={"adv": adv}, out=outs[k])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        work()                                    # call 0
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        work()                                    # captured, not run
    rig.model.select(a["len"], L, C)
    seen = []
    for call in (1, 2):
        for out in outs:
            for t in out.values():
                t.fill_(1)                        # nothing of the replay before may pass for this one's
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        total = rig.model.select(a["len"], L, C)
        assert int(rig.ch.total().item()) == total and rig.model.calls == call + 1
        order = []
        for k in range(2):
            want = rig.model.take(True, a["len"], a["ends"], L, C, k * half, half, a["obs_index"], a["next_index"], a["payload"], [adv.cpu().numpy()])
            for key in [x[0] for x in STEP_OUT + CHUNK_OUT] + ["payload"]:
                assert np.array_equal(outs[k][key].cpu().numpy(), want[key]), (key, call, k)
            assert np.array_equal(bits(outs[k]["adv"].cpu().numpy()), bits(want["streams"][0])), (call, k)
            order += [x for x, v in zip(zip(want["env"][0].tolist(), want["chunk"].tolist()), want["valid"].tolist()) if v]
        assert len(order) == total == len(set(order))
        seen.append(order)
    assert seen[0] != seen[1] and sorted(seen[0]) == sorted(seen[1])
    torch.cuda.synchronize()
    rig.close()


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_in_the_stated_order():
    from active_gym import _native as nat
    from active_gym.chunks import ChunkIo
    N, L, C = 3, 4, 2
    rig = Rig(N)
    lib, st, c = rig.lib, rig.pipe._stream(), rig.ch._c
    inp = Inputs(cm.rollout_arrays(1, N, L))
    slot = torch.full((C * 8,), I_SENT, dtype=torch.int32, device=DEV)
    total = torch.full((1,), I_SENT, dtype=torch.int32, device=DEV)

    def io(n_f32=0, slot_=slot):
        x = ChunkIo()
        x.n_f32, x.d_slot = n_f32, _ptr(slot_)
        return ctypes.byref(x)

    def select(c=c, L=L, C=C, length=inp.len):
        return lib.agx_chunks_select(c, L, C, _ptr(length), _ptr(total), st)

    def take(c=c, L=L, C=C, length=inp.len, ends=inp.ends, first=0, S=8, io_=None):
        return lib.agx_chunks_take(c, 1, L, C, _ptr(length), _ptr(ends), first, S, io() if io_ is None else io_, st)

    big = 2 ** 31 - 1
    cases = [
        # 1. the handle, whatever else is wrong
        (select, dict(c=None, L=0, C=0, length=None), "null argument (c)", False),
        (take, dict(c=None, L=0, C=0, S=-1, io_=io(9, None)), "null argument (c)", False),
        # 2. L, before C
        (select, dict(L=0, C=0), "L must be 1 .. 4096", True), (select, dict(L=4097, C=300, length=None), "L must be 1 .. 4096", True),
        (take, dict(L=0, C=0, S=-1), "L must be 1 .. 4096", True), (take, dict(L=4097, first=-1), "L must be 1 .. 4096", True),
        # 3. C, before S and first
        (select, dict(C=0, length=None), "C must be 1 .. min(L, 256) = 4", True), (select, dict(C=5), "C must be", True),
        (select, dict(L=300, C=257), "C must be 1 .. min(L, 256) = 256", True),
        (take, dict(C=0, S=-1), "C must be", True), (take, dict(C=5, first=-1), "C must be", True), (take, dict(L=300, C=257, S=-1), "C must be", True),
        # 4. S and first, then C * S, before io and n_f32
        (take, dict(S=-1, io_=io(9)), "first = 0, S = -1", True), (take, dict(first=-1, io_=io(9)), "first = -1", True),
        (take, dict(first=big, S=1, io_=io(-1)), "first + S", True), (take, dict(first=big - 7, S=8, length=None), "first + S", True),
        (take, dict(S=2 ** 30, io_=io(9)), "C * S", True), (take, dict(S=2 ** 30, io_=ctypes.POINTER(ChunkIo)()), "C * S", True),
        # 5. io and n_f32, before the buffers
        (take, dict(io_=ctypes.POINTER(ChunkIo)(), length=None), "null argument (io)", True),
        (take, dict(io_=io(9, None)), "n_f32 must be 0 .. 8", True), (take, dict(io_=io(-1), length=None), "n_f32 must be 0 .. 8", True),
        # 6. d_len, then d_ends and d_slot
        (select, dict(length=None), "null buffer (d_len)", True),
        (take, dict(length=None, ends=None, io_=io(0, None)), "null buffer (d_len)", True),
        (take, dict(ends=None, io_=io(0, None)), "null buffer (d_ends)", True), (take, dict(io_=io(0, None)), "null buffer (d_slot)", True),
    ]
    for call, kw, named, has_ctx in cases:
        assert call(**kw) == nat.E_INVALID, (call.__name__, kw)
        msg = nat.last_error(rig.pipe._ctx if has_ctx else None)
        assert named in msg and "agx_chunks_" + call.__name__ in msg, (call.__name__, kw, msg)
    torch.cuda.synchronize()
    assert (slot == I_SENT).all() and int(total.item()) == I_SENT       # no refused call launched anything
    assert take(S=0, io_=io(0, None)) == nat.E_INVALID and take(S=0) == nat.OK
    torch.cuda.synchronize()
    assert (slot == I_SENT).all(), "S == 0 launches nothing"
    assert select() == nat.OK and take() == nat.OK
    torch.cuda.synchronize()
    assert int(total.item()) == rig.model.select(inp.a["len"], L, C) and (slot != I_SENT).all()
    # the Python surface refuses before any GPU work
    batch = dict(len=inp.len, ends=inp.ends, obs_index=inp.obs_index, next_index=inp.next_index, payload=inp.payload)
    f = torch.zeros((L, N), device=DEV)
    for call in (lambda: rig.ch.select(batch, 0), lambda: rig.ch.select(batch, L + 1), lambda: rig.ch.take(batch, 0, -1, C),
                 lambda: rig.ch.take(batch, -1, 4, C), lambda: rig.ch.take(batch, 0, 4, L + 1), lambda: rig.ch.take(batch, 0, 2 ** 30, C),
                 lambda: rig.ch.take(batch, 0, 4, C, streams={f"s{k}": f for k in range(9)}), lambda: rig.ch.take(batch, 0, 4, C, streams={"mask": f})):
        with pytest.raises(ValueError):
            call()
    # a narrowed env range: AGX_E_STATE from every call
    rig.pipe.env_range(1, 2)
    for call in (lambda: rig.ch.select(batch, C), lambda: rig.ch.take(batch, 0, 4, C), lambda: rig.roll.chunker(1)):
        with pytest.raises(nat.AgxError, match="env range") as e:
            call()
        assert e.value.code == nat.E_STATE
    rig.pipe.env_range()
    rig.ch.select(batch, C)
    torch.cuda.synchronize()
    rig.hist.close()                              # the history closes its chunkers first
    assert not rig.ch.alive
    with pytest.raises(RuntimeError, match="closed"):
        rig.ch.select(batch, C)
    with pytest.raises(RuntimeError, match="closed"):
        rig.ch.take(batch, 0, 4, C)
    rig.close()


# ---------------------------------------------------------------------------------------------- 4. end to end
def _vec_env(native_loop, N):
    from active_gym import AtariEnvArgs, AtariVecEnv
    kw = dict(game="g", seed=3, obs_size=(12, 12), frame_stack=3, fov_size=(3, 5), fov_init_loc=(1, 2), sensory_action_mode="absolute",
              resize_to_full=True, frame_source="native", device="cuda:0", num_workers=2, scripted_actions=4, scripted_lives=1,
              scripted_p_life=0, scripted_p_over=30, native_loop=native_loop, history_len=16, step_log=True)
    return AtariVecEnv(AtariEnvArgs(**kw), N, kind="fixed", noop_fn=lambda: 2)


@pytest.mark.parametrize("native", [True, False], ids=["native_loop", "python_loop"])
def test_vec_env_chunks_cover_every_live_slot_once(native):
    """AtariVecEnv(history_len = 16, step_log = True), N = 4, 40 random steps across autoresets, rollout_batch(12), C = 5 (G = 3,
    three padded steps in the last chunk), size = 5 (12 chunks at the most: three minibatches, the last one wraps).  Over one epoch
    of rollout_chunks the steps with mask = 1 hold every live slot exactly once; the actions, the indices and the streams are
    the batch's at `slot`; history.observe of (env, obs_index) at the masked steps re-creates the observations the env returned
    with those indices; start & 2 sits exactly behind the batch's ended slots; state_index is obs_index at the chunk's first
    live step; and a second epoch is another order."""
    N, STEPS, L, C, SIZE = 4, 40, 12, 5, 5
    env = _vec_env(native, N)
    assert (env._loop is not None) == native and env.steplog is not None
    obs, info = env.reset()
    rng = np.random.default_rng(0)
    returned = {}                                  # (env, history index) -> the observation returned with it
    for step in range(STEPS + 1):
        host = torch.as_tensor(obs).cpu().numpy()
        for n, k in enumerate(info["history_index"].cpu().numpy()):
            returned[(n, int(k))] = host[n].copy()
        if step < STEPS:
            act = {"motor_action": rng.integers(0, 4, N), "sensory_action": rng.uniform(-3, 14, (N, 2)).astype(np.float32)}
            obs, _, _, _, info = env.step(act)
    batch = env.rollout_batch(L)
    live, ends = batch["live"].cpu().numpy(), batch["ends"].cpu().numpy()
    oi, ni = batch["obs_index"].cpu().numpy(), batch["next_index"].cpu().numpy()
    want = sorted((np.nonzero(live)[0] * N + np.nonzero(live)[1]).tolist())
    assert len(want) >= 3 * N and (ends[:-1][live[:-1]] & 7).any(), "no episode end inside the rollouts: lengthen the run"
    adv = torch.randn((L, N), device=DEV)
    motor, sens = batch["motor_action"].cpu().numpy().reshape(-1), batch["sensory_action"].cpu().numpy().reshape(-1, 2)
    t0 = L - np.clip(batch["len"].cpu().numpy(), 0, L)
    orders = []
    for epoch in range(2):
        got = list(env.rollout_chunks(batch, C, SIZE, {"adv": adv, "reward": batch["reward"]}))
        assert len(got) == -(-N * 3 // SIZE) == 3
        slots, order = [], []
        for rows in got:
            assert sorted(rows) == sorted(["slot", "env", "obs_index", "next_index", "ends", "start", "mask", "chunk", "first", "steps", "state_index",
                                           "valid", "motor_action", "sensory_action", "adv", "reward"])
            assert tuple(rows["slot"].shape) == (C, SIZE) and tuple(rows["sensory_action"].shape) == (C, SIZE, 2) and tuple(rows["valid"].shape) == (SIZE,)
            r = {k: v.cpu().numpy() for k, v in rows.items()}
            at = r["slot"] >= 0
            slot = r["slot"][at]
            assert np.array_equal(r["mask"] == 1, at & (r["valid"] == 1)[None, :]) and (r["env"] == r["env"][0]).all()
            assert np.array_equal(r["motor_action"][at], motor[slot]) and not r["motor_action"][~at].any() and rows["motor_action"].dtype == torch.int32
            assert np.array_equal(bits(r["sensory_action"][at]), bits(sens[slot])) and not r["sensory_action"][~at].any()
            assert np.array_equal(bits(r["adv"][at]), bits(adv.cpu().numpy().reshape(-1)[slot])) and not r["adv"][~at].any()
            assert np.array_equal(r["obs_index"][at], oi.reshape(-1)[slot]) and (r["obs_index"][~at] == -1).all()
            assert np.array_equal(r["next_index"][at], ni.reshape(-1)[slot]) and np.array_equal(r["ends"][at], ends.reshape(-1)[slot])
            assert np.array_equal(slot % N, r["env"][at])
            t, n = slot // N, slot % N
            assert np.array_equal((r["start"][at] & 2) != 0, (t > t0[n]) & ((ends[np.maximum(t - 1, 0), n] & 7) != 0)) and not r["start"][~at].any()
            assert np.array_equal((r["start"] & 1) != 0, at & (np.arange(C)[:, None] == r["first"][None, :]))
            assert np.array_equal(r["state_index"], r["obs_index"][r["first"], np.arange(SIZE)])
            seen, _, ok = env.history.observe(rows["env"].flatten(), rows["obs_index"].flatten())
            seen, ok = seen.cpu().numpy().reshape((C, SIZE) + seen.shape[1:]), ok.cpu().numpy().reshape(C, SIZE).astype(bool)
            assert np.array_equal(ok, at), "every live step can be re-created, every padded step is index -1"
            for l, s in zip(*np.nonzero(r["mask"] == 1)):
                assert np.array_equal(seen[l, s], returned[(int(r["env"][l, s]), int(r["obs_index"][l, s]))]), (l, s)
            slots += r["slot"][r["mask"] == 1].tolist()
            order += [x for x, v in zip(zip(r["env"][0].tolist(), r["chunk"].tolist()), r["valid"].tolist()) if v]
        assert sorted(slots) == want, "an epoch covers every live slot exactly once"
        orders.append(order)
    assert orders[0] != orders[1] and sorted(orders[0]) == sorted(orders[1])
    assert env.history.chunker(None, 3) is env.history.chunker(None, 3)          # cached per seed: the one the epochs used
    with pytest.raises(ValueError, match="C must be"):
        env.rollout_chunks(batch, L + 1, SIZE)
    torch.cuda.synchronize()
    env.close()
