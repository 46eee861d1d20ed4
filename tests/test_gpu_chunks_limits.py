"""GPU: the chunk kernels (K17, include/agx_chunks.h) at the limits the header states, on the scenarios of
tests/batch_limit_cases.py (tests/test_batch_limits_cpu.py pins what each holds): a scan of more than one run of 256 envs,
L = AGX_CHUNK_L_LIMIT with C = AGX_CHUNK_LIMIT, G = 4096, a short last chunk of a long rollout, the byte path of the payload copy
by odd widths and by misaligned pointers, first = INT32_MAX - S.  Every element of every output is compared EXACTLY - floats as
int32 bit patterns - with the vectorised definition batch_limit_cases.Chunks, which broadcasts the header's rule over [C][S];
every output lies between guard regions filled with a sentinel."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import batch_limit_cases as bl
import chunks_model as cm
from test_gpu_chunks import B_SENT, CHUNK_OUT, CONFIGS, DEV, F_SENT, I_SENT, STEP_OUT, Rig, _ptr, _t
from test_gpu_minibatch_limits import Out, shifted

pytestmark = pytest.mark.gpu
SEED = 5
SIZES = (1, 63, 64, 65, 300)                 # S: tests/test_gpu_chunks.py's
# tests/test_gpu_chunks.py's four and one whose payload is 5 bytes wide: the byte branch of k_chunk_take with outputs left out
CONFIGS = CONFIGS + (dict(n_f32=2, W=5, null_out=("next_index", "ends"), null_in=(), null_src=(), null_dst=(1,)),)


class Case:
    """A rig of N envs, the definition that counts its selects with it, and the arrays of one rollout on the device."""

    def __init__(self, N):
        self.rig, self.mine, self.N = Rig(N, SEED), bl.Chunks(N, SEED), N

    def load(self, a):
        self.a = a
        self.d = dict(len=_t(a["len"]), ends=_t(a["ends"]), obs_index=_t(a["obs_index"]), next_index=_t(a["next_index"]), payload=_t(a["payload"]),
                      streams=[_t(s) for s in a["streams"]])
        self.L = a["ends"].shape[0]
        return self

    def select(self, C):
        from active_gym import _native as nat
        rig = self.rig
        total = torch.full((1,), I_SENT, dtype=torch.int32, device=DEV)
        nat.check(rig.lib.agx_chunks_select(rig.ch._c, self.L, C, _ptr(self.d["len"]), _ptr(total), rig.pipe._stream()), rig.pipe._ctx)
        want = self.mine.select(self.a["len"], self.L, C)
        assert int(total.item()) == want, "d_total differs from the definition"
        return want

    def take(self, permute, C, first, S, config, what, in_shift=0, out_shift=0):
        """agx_chunks_take on sentinel-filled, guarded outputs against the definition, element for element."""
        from active_gym import _native as nat
        from active_gym.chunks import ChunkIo
        rig, a, d, L = self.rig, self.a, self.d, self.L
        n_f32, W, null_out, null_in = min(config["n_f32"], len(a["streams"])), config["W"], config["null_out"], config["null_in"]
        payload = a["payload"][..., :W]
        held, p_payload = (None, None)
        if W and "payload" not in null_in:
            held, p_payload = (d["payload"], _ptr(d["payload"])) if (W, in_shift) == (a["payload"].shape[-1], 0) else shifted(payload, in_shift)
        outs = {key: Out(C * S, dtype, B_SENT if dtype == torch.uint8 else I_SENT) for key, _, dtype in STEP_OUT}
        outs.update({key: Out(S, dtype, B_SENT if dtype == torch.uint8 else I_SENT) for key, _, dtype in CHUNK_OUT})
        outs["payload"] = Out(C * S * W, torch.uint8, B_SENT, out_shift)
        streams = [Out(C * S, torch.float32, F_SENT) for _ in range(n_f32)]
        io = ChunkIo()
        io.d_obs_index = None if "obs_index" in null_in else _ptr(d["obs_index"])
        io.d_next_index = None if "next_index" in null_in else _ptr(d["next_index"])
        io.d_payload, io.payload_bytes, io.n_f32 = p_payload, W, n_f32
        skipped = set(null_out) | ({"payload"} if not W else set())
        for key, field, _ in STEP_OUT + CHUNK_OUT + (("payload", "d_payload_out", None),):
            setattr(io, field, None if key in skipped else outs[key].ptr)
        for k in range(n_f32):
            io.src_f32[k] = None if k in config["null_src"] else d["streams"][k].data_ptr()
            io.dst_f32[k] = None if k in config["null_dst"] else streams[k].ptr.value
        rc = rig.lib.agx_chunks_take(rig.ch._c, permute, L, C, _ptr(d["len"]), _ptr(d["ends"]), first, S, ctypes.byref(io), rig.pipe._stream())
        nat.check(rc, rig.pipe._ctx)
        want = self.mine.take(bool(permute), a["ends"], L, C, first, S, None if "obs_index" in null_in else a["obs_index"],
                              None if "next_index" in null_in else a["next_index"],
                              (np.zeros_like(payload) if "payload" in null_in else payload) if W else None,
                              [np.zeros_like(a["streams"][k]) if k in config["null_src"] else a["streams"][k] for k in range(n_f32)])
        compared = 0
        for key, g in outs.items():
            got = g.host()
            if key in skipped:
                assert (got == g.sentinel).all(), f"{key} was passed as NULL and written ({what})"
            else:
                assert np.array_equal(got, np.asarray(want[key]).reshape(-1)), f"{key} differs from the definition ({what})"
                compared += got.size
        for k, g in enumerate(streams):
            got = g.host()
            if k in config["null_dst"]:
                assert (got == F_SENT).all(), f"stream {k} was passed as NULL and written ({what})"
            else:
                assert np.array_equal(got.view(np.int32), want["streams"][k].reshape(-1).view(np.int32)), f"stream {k} differs from the definition ({what})"
                assert np.isfinite(got).all(), f"stream {k}: a value of a slot that is not live reached the output ({what})"
                compared += got.size
        del held
        want["compared"] = compared
        return want

    def close(self):
        torch.cuda.synchronize()
        self.rig.close()


CASES = {}


@pytest.fixture(scope="module")
def cases():
    def get(N):
        if N not in CASES:
            CASES[N] = Case(N)
        return CASES[N]
    yield get
    for c in CASES.values():
        c.close()
    CASES.clear()


def _holds(want, total, first, S):
    """What every take of a non-empty list holds: the rows' validity, a real chunk in every row - wrapped ones included -, and
    mask only where valid."""
    assert want["valid"].tolist() == [int(first + s < total) for s in range(S)] and (want["chunk"] >= 0).all()
    assert ((want["slot"] >= 0).sum(0) == want["steps"]).all() and (want["steps"] >= 1).all()
    assert not want["mask"][:, want["valid"] == 0].any()


# ---------------------------------------------------------------------------------------------- 1. the scan beyond one run
@pytest.mark.parametrize("N", bl.SCAN_NS)
def test_scan_over_more_than_one_run(cases, N):
    """k_chunk_scan with a carried total, at C = 1 (a chunk per live step) and C = L (a chunk per live env): a full epoch and
    three wrapped rows, plain and permuted; the plain take reads off[0 .. N] back through env."""
    L, compared = bl.SCAN_L, 0
    for variant in bl.SCAN_VARIANTS:
        c = cases(N).load(bl.scan(N, variant))
        for C in (1, L):
            total = c.select(C)
            assert total > 8
            for permute in (0, 1):
                want = c.take(permute, C, 0, total + 3, CONFIGS[0], f"scan {N} {variant}, C {C}, permute {permute}")
                _holds(want, total, 0, total + 3)
                compared += want["compared"]
                if not permute:
                    env = want["env"][0, :total]
                    assert (np.diff(env) >= 0).all() and np.array_equal(np.bincount(env, minlength=N), np.bincount(c.mine.n, minlength=N))
    print(f"scan N = {N}: {compared} elements compared")


# ---------------------------------------------------------------------------------------------- 2. the chunk limits
def test_the_chunky_plan_crosses_every_size_with_every_config():
    takes = [(S, k % 3, (k // 3) % 2, (k + k // 5) % 5) for k, ((L, C), N, S) in enumerate(itertools.product(bl.CHUNKY, bl.CHUNKY_NS, SIZES))]
    assert {(S, cfg) for S, _, _, cfg in takes} == {(S, cfg) for S in SIZES for cfg in range(5)}
    assert {(w, p) for _, w, p, _ in takes} == {(w, p) for w in range(3) for p in range(2)}


@pytest.mark.parametrize("L,C", bl.CHUNKY)
def test_chunky_at_the_limits_of_l_c_and_g(cases, L, C):
    """(L, C) = (256, 256), (257, 256), (4096, 256), (4096, 255): G = 17 with a last chunk of 16 steps, (4096, 1): G = 4096,
    (4095, 256), at N = 5 and 257 and S = 1, 63, 64, 65, 300: first at 0, mid-list and past total (every row wrapped), plain and
    permuted, the five CONFIGS rotating."""
    turn = itertools.count(bl.CHUNKY.index((L, C)) * len(bl.CHUNKY_NS) * len(SIZES))
    compared = 0
    for N in bl.CHUNKY_NS:
        c = cases(N).load(bl.chunky(N, L, C))
        total = c.select(C)
        for S in SIZES:
            k = next(turn)
            where, permute, config = k % 3, (k // 3) % 2, (k + k // 5) % 5
            first = (0, total // 2, total + 1)[where]
            want = c.take(permute, C, first, S, CONFIGS[config], f"N {N}, L {L}, C {C}, S {S}, first {first}, permute {permute}, config {config}")
            _holds(want, total, first, S)
            compared += want["compared"]
        whole = c.take(0, C, 0, min(total, 300), CONFIGS[2], "the head of the list")       # envs 0 .. 3: the four t0 of the scenario
        assert whole["first"].max() > 0 or C == 1
        if L % C:
            assert (whole["steps"][whole["chunk"] == -(-L // C) - 1] <= L % C).all() and (whole["chunk"] == -(-L // C) - 1).any()
    print(f"chunky ({L}, {C}): {compared} elements compared")


# ---------------------------------------------------------------------------------------------- 3. the byte path of the payload
@pytest.mark.parametrize("W", bl.BYTE_WIDTHS)
def test_payload_of_a_width_that_is_no_multiple_of_four(cases, W):
    """W = 1, 3, 5, 6, 66 on pointers aligned to 64 bytes (and 260: 65 whole words again): the byte branch of k_chunk_take, live steps and padding (zeros),
    wrapped rows included; no byte beyond C * S * W is written.  A NULL payload input reads as zeros on the same branch."""
    N, L = bl.MID
    c = cases(N).load(bl.mid(W))
    for C in (5, L):
        total = c.select(C)
        config = dict(n_f32=1, W=W, null_out=(), null_in=(), null_src=(), null_dst=())
        want = c.take(1, C, 0, total + 5, config, f"W {W}, C {C}")
        assert want["payload"].any() and not want["payload"][want["slot"] < 0].any()
    assert not c.take(1, L, 3, 70, dict(config, null_in=("payload",)), f"W {W}, NULL payload")["payload"].any()


@pytest.mark.parametrize("W,in_shift,out_shift", bl.BYTE_SHIFTS)
def test_payload_behind_misaligned_pointers(cases, W, in_shift, out_shift):
    """W = 4 and 12 with the payload input 1 byte, the output 2 bytes, and both behind a 64-byte boundary (views into larger
    tensors): the word branch must not be taken, and the sentinels on either side of the C * S * W output bytes stay."""
    N, L = bl.MID
    c = cases(N).load(bl.mid(12))
    C = 5
    total = c.select(C)
    config = dict(n_f32=1, W=W, null_out=(), null_in=(), null_src=(), null_dst=())
    for permute in (0, 1):
        c.take(permute, C, 0, total + 5, config, f"W {W}, input + {in_shift}, output + {out_shift}", in_shift=in_shift, out_shift=out_shift)


# ---------------------------------------------------------------------------------------------- 4. first + S = INT32_MAX
@pytest.mark.parametrize("S", bl.FAR_SIZES)
def test_first_at_int32_max_less_s(cases, S):
    """first = INT32_MAX - S: every row is wrapped - valid 0, mask 0 everywhere - and holds the real chunk at p mod total."""
    N, L = bl.MID
    c = cases(N).load(bl.mid(12))
    C = 5
    total = c.select(C)
    for permute in (0, 1):
        want = c.take(permute, C, bl.INT32_MAX - S, S, CONFIGS[0], f"far, S {S}, permute {permute}")
        assert not want["valid"].any() and not want["mask"].any() and (want["chunk"] >= 0).all() and (want["steps"] >= 1).all() and total > 0


# ---------------------------------------------------------------------------------------------- 5. state_index and START
def test_state_index_and_start_bits_at_a_chunk_boundary_and_behind_an_episode_end(cases):
    """(L, C) = (257, 256), N = 5: env 0 (t0 = 0) ends an episode on the last step of chunk 0, so step 0 of its chunk 1 carries
    START_CHUNK | START_EPISODE and state_index is the observation there; env 1's t0 is chunk 1's first step: START_CHUNK alone,
    whatever the slot in front of t0 holds."""
    N, L, C = 5, 257, 256
    a = {k: (v.copy() if isinstance(v, np.ndarray) else [s.copy() for s in v]) for k, v in bl.chunky(N, L, C).items()}
    a["ends"][C - 1, 0] |= 1
    a["ends"][C - 1, 1] |= 7                                          # in front of env 1's t0: not live, never read
    c = cases(N).load(a)
    total = c.select(C)
    want = c.take(0, C, 0, total, CONFIGS[0], "the boundary")
    rows = {(int(n), int(g)): s for s, (n, g) in enumerate(zip(want["env"][0], want["chunk"]))}
    s = rows[(0, 1)]
    assert want["start"][0, s] == cm.START_CHUNK | cm.START_EPISODE and want["state_index"][s] == a["obs_index"][C, 0] and want["first"][s] == 0
    s = rows[(1, 1)]
    assert want["start"][0, s] == cm.START_CHUNK and want["state_index"][s] == a["obs_index"][C, 1] and (1, 0) not in rows
    s = rows[(2, 0)]                                                 # env 2: t0 = C - 1, the last step of chunk 0
    assert want["first"][s] == C - 1 and want["steps"][s] == 1 and want["start"][C - 1, s] == cm.START_CHUNK
