"""GPU: the minibatch kernels (K15, include/agx_minibatch.h) at the limits the header states, on the scenarios of
tests/batch_limit_cases.py (tests/test_batch_limits_cpu.py pins what each holds): a scan of more than one run of 256 envs with
empty runs across its boundaries, L = AGX_MB_LIMIT, totals past 2^20, the byte path of the payload copy by odd widths and by
misaligned pointers, first = INT32_MAX - S, scatter at 257 x 4096 cells.  Every element of every output is compared EXACTLY -
floats as int32 bit patterns - with the vectorised definition batch_limit_cases.Minibatches, a second writing of the header that
can follow the device to a million positions; every output lies between guard regions filled with a sentinel."""
import ctypes

import numpy as np
import pytest
import torch

import batch_limit_cases as bl
from test_gpu_minibatch import B_SENT, DEV, F_SENT, GUARD, I_SENT, P, Rig, _ptr, _t

pytestmark = pytest.mark.gpu
SEED = 5
LIVE, BOOT = bl.LIVE, bl.BOOT


class Out:
    """An output of `count` elements between two guard regions, all filled with the sentinel.  shift: the bytes (uint8 outputs)
    by which the output starts behind a 64-byte boundary."""

    def __init__(self, count, dtype, sentinel, shift=0):
        assert shift == 0 or dtype == torch.uint8
        self.count, self.sentinel, self.lo = count, sentinel, GUARD + shift
        self.t = torch.full((count + 2 * GUARD + shift,), sentinel, dtype=dtype, device=DEV)
        assert self.t.data_ptr() % 64 == 0

    @property
    def ptr(self):
        return P(self.t.data_ptr() + self.lo * self.t.element_size())

    def host(self):
        """The interior; the guards are checked on the way."""
        a = self.t.cpu().numpy()
        assert (a[:self.lo] == self.sentinel).all() and (a[self.lo + self.count:] == self.sentinel).all(), "a guard region was written"
        return a[self.lo:self.lo + self.count]


def shifted(payload, shift):
    """The payload bytes on the device `shift` bytes behind a 64-byte boundary: (the tensor that holds them, the pointer)."""
    flat = np.ascontiguousarray(payload).reshape(-1)
    big = torch.full((flat.size + 64,), B_SENT, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 64 == 0
    big[shift:shift + flat.size] = _t(flat)
    return big, P(big.data_ptr() + shift)


class Case:
    """A rig of N envs, the definition that counts its selects with it, and the arrays of one rollout on the device."""

    def __init__(self, N):
        self.rig, self.mine, self.N = Rig(N, SEED), bl.Minibatches(N, SEED), N

    def load(self, a):
        self.a = a
        self.d = dict(len=_t(a["len"]), ends=_t(a["ends"]), obs_index=_t(a["obs_index"]), next_index=_t(a["next_index"]), payload=_t(a["payload"]),
                      streams=[_t(s) for s in a["streams"]])
        self.L = a["ends"].shape[0]
        return self

    def select(self, which):
        from active_gym import _native as nat
        rig, d = self.rig, self.d
        total = torch.full((1,), I_SENT, dtype=torch.int32, device=DEV)
        nat.check(rig.lib.agx_minibatch_select(rig.mb._m, which, self.L, _ptr(d["len"]), _ptr(d["ends"]), _ptr(total), rig.pipe._stream()), rig.pipe._ctx)
        want = self.mine.select(which, self.a["len"], self.a["ends"], self.L)
        assert int(total.item()) == want, "d_total differs from the definition"
        return want

    def take(self, which, permute, first, S, what, W=None, in_shift=0, out_shift=0, null_payload=False):
        """agx_minibatch_take on sentinel-filled, guarded outputs against the definition, element for element."""
        from active_gym import _native as nat
        from active_gym.minibatch import MinibatchIo
        rig, a, d = self.rig, self.a, self.d
        W = a["payload"].shape[-1] if W is None else W
        payload = a["payload"][..., :W]
        held, p_payload = (d["payload"], _ptr(d["payload"])) if (W, in_shift) == (a["payload"].shape[-1], 0) else shifted(payload, in_shift)
        n_f32 = len(a["streams"])
        outs = dict(slot=Out(S, torch.int32, I_SENT), env=Out(S, torch.int32, I_SENT), obs_index=Out(S, torch.int64, I_SENT),
                    next_index=Out(S, torch.int64, I_SENT), payload=Out(S * W, torch.uint8, B_SENT, out_shift), valid=Out(S, torch.uint8, B_SENT))
        streams = [Out(S, torch.float32, F_SENT) for _ in range(n_f32)]
        io = MinibatchIo()
        io.d_obs_index, io.d_next_index = _ptr(d["obs_index"]), _ptr(d["next_index"])
        io.d_payload, io.payload_bytes, io.n_f32 = None if null_payload else p_payload, W, n_f32
        io.d_slot, io.d_env, io.d_obs_index_out, io.d_next_index_out = outs["slot"].ptr, outs["env"].ptr, outs["obs_index"].ptr, outs["next_index"].ptr
        io.d_payload_out, io.d_valid = outs["payload"].ptr, outs["valid"].ptr
        for k in range(n_f32):
            io.src_f32[k], io.dst_f32[k] = d["streams"][k].data_ptr(), streams[k].ptr.value
        rc = rig.lib.agx_minibatch_take(rig.mb._m, which, permute, self.L, _ptr(d["len"]), _ptr(d["ends"]), first, S, ctypes.byref(io), rig.pipe._stream())
        nat.check(rc, rig.pipe._ctx)
        want = self.mine.take(which, bool(permute), first, S, a["obs_index"], a["next_index"], np.zeros_like(payload) if null_payload else payload, a["streams"])
        for key, g in outs.items():
            assert np.array_equal(g.host(), np.asarray(want[key]).reshape(-1)), f"{key} differs from the definition ({what})"
        for k, g in enumerate(streams):
            assert np.array_equal(g.host().view(np.int32), want["streams"][k].view(np.int32)), f"stream {k} differs from the definition ({what})"
        del held
        want["compared"] = S * (6 + W + n_f32)
        return want

    def close(self):
        torch.cuda.synchronize()
        self.rig.close()


CASES = {}


@pytest.fixture(scope="module")
def cases():
    """One Case per N, made at first use: its definition counts the selects with it."""
    def get(N):
        if N not in CASES:
            CASES[N] = Case(N)
        return CASES[N]
    yield get
    for c in CASES.values():
        c.close()
    CASES.clear()


# ---------------------------------------------------------------------------------------------- 1. the scan beyond one run
@pytest.mark.parametrize("N", bl.SCAN_NS)
def test_scan_over_more_than_one_run(cases, N):
    """k_mb_scan with a carried total: both lists of every variant as a full epoch (and three wrapped rows), plain and permuted,
    in every output.  The plain take reads off[0 .. N] back: env is non-decreasing with the definition's run lengths, so every
    offset behind an empty run, behind wave 3's `before` and behind the carried total is the definition's.  A second select
    shuffles the same slots anew."""
    compared = 0
    for variant in bl.SCAN_VARIANTS:
        c = cases(N).load(bl.scan(N, variant))
        for which in (LIVE, BOOT):
            total = c.select(which)
            assert total > 8
            plain = c.take(which, 0, 0, total + 3, f"scan {N} {variant}, list {which}, plain")
            env = plain["env"][:total]
            assert (np.diff(env) >= 0).all() and np.array_equal(np.bincount(env, minlength=N), np.bincount(c.mine.envs[which], minlength=N))
            first = c.take(which, 1, 0, total + 3, f"scan {N} {variant}, list {which}, permuted")
            c.select(which)
            second = c.take(which, 1, 0, total, f"scan {N} {variant}, list {which}, the second epoch")
            assert np.array_equal(np.sort(first["slot"][:total]), np.sort(second["slot"])) and not np.array_equal(first["slot"][:total], second["slot"])
            assert np.array_equal(np.sort(second["slot"]), np.sort(c.mine.slots[which]))
            compared += plain["compared"] + first["compared"] + second["compared"]
    print(f"scan N = {N}: {compared} elements compared")


# ---------------------------------------------------------------------------------------------- 2. L = AGX_MB_LIMIT
@pytest.mark.parametrize("N,L", bl.DEEP)
def test_deep_live_list_as_one_take(cases, N, L):
    """L = 4096: the LIVE list as a full epoch in ONE take (668,295 positions at N = 257), plain and permuted."""
    c = cases(N).load(bl.deep(N, L))
    total = c.select(LIVE)
    compared = c.take(LIVE, 0, 0, total + 1, f"deep {N}, plain")["compared"]
    got = c.take(LIVE, 1, 0, total + 1, f"deep {N}, permuted")
    assert np.array_equal(np.sort(got["slot"][:total]), np.sort(c.mine.slots[LIVE])) and got["valid"][:total].all() and not got["valid"][total]
    print(f"deep ({N}, {L}) LIVE: total {total}, {compared + got['compared']} elements compared, walks up to {int(got['walks'].max())}")


@pytest.mark.parametrize("N,L", bl.DEEP)
def test_deep_boot_list_walks_whole_columns(cases, N, L):
    """BOOT at L = 4096: the column walk from 1 to 4096 slots deep.  N = 65 as a full epoch; N = 257 over the first and the last
    4096 positions and the two envs whose only BOOT bit is their first / their last slot."""
    c = cases(N).load(bl.deep(N, L))
    total = c.select(BOOT)
    slots = c.mine.slots[BOOT]
    at = {int(np.nonzero(slots == e)[0][0]): e for e in (0 * N + bl.DEEP_TOP, (L - 1) * N + bl.DEEP_BOTTOM)}
    compared = 0
    if N == 65:
        windows = [(0, total + 2)]
    else:
        windows = [(0, 4096), (total - 4096, 4096 + 2)] + [(m, 1) for m in at]
    for permute in (0, 1):
        for first, S in windows:
            compared += c.take(BOOT, permute, first, S, f"deep {N} BOOT, permute {permute}, first {first}, S {S}")["compared"]
    for m, e in at.items():                                          # the deepest and the shallowest walk, by position
        assert c.take(BOOT, 0, m, 1, "a column-walk extreme")["slot"].tolist() == [e]
    print(f"deep ({N}, {L}) BOOT: total {total}, {compared} elements compared")


# ---------------------------------------------------------------------------------------------- 3. totals and the Feistel domain
@pytest.mark.parametrize("total", sorted(bl.TOTALS))
def test_totals_as_a_full_permuted_epoch(cases, total):
    """LIVE totals of exactly 1 .. 2^20 + 1 (hb = 1, 2, 3, 7, 9, 10, 11): the sorted slots of a permuted epoch are the list, and
    their order is the definition's - cycle walks of up to 49 rounds included."""
    N, L = bl.TOTALS[total]
    c = cases(N).load(bl.totals(total))
    walks = 0
    for epoch in range(4 if total <= 17 else 1):
        assert c.select(LIVE) == total
        got = c.take(LIVE, 1, 0, total, f"total {total}, epoch {epoch}")
        assert np.array_equal(np.sort(got["slot"]), np.sort(c.mine.slots[LIVE])) and got["valid"].all()
        walks = max(walks, int(got["walks"].max()))
    assert walks >= 2 or total == 4 ** bl.half_bits(total)
    print(f"total {total}: hb {bl.half_bits(total)}, walks up to {walks}")


# ---------------------------------------------------------------------------------------------- 4. the byte path of the payload
@pytest.mark.parametrize("W", bl.BYTE_WIDTHS)
def test_payload_of_a_width_that_is_no_multiple_of_four(cases, W):
    """W = 1, 3, 5, 6, 66 on pointers aligned to 64 bytes (and 260: 65 whole words again): the byte branch of k_mb_take, both lists, wrapped rows included;
    no byte beyond S * W is written.  A NULL payload input reads as zeros on the same branch."""
    N, L = bl.MID
    c = cases(N).load(bl.mid(W))
    for which in (LIVE, BOOT):
        total = c.select(which)
        got = c.take(which, 1, 0, total + 5, f"W {W}, list {which}")
        assert got["payload"].any()
    assert not c.take(LIVE, 1, 3, 70, f"W {W}, NULL payload", null_payload=True)["payload"].any()


@pytest.mark.parametrize("W,in_shift,out_shift", bl.BYTE_SHIFTS)
def test_payload_behind_misaligned_pointers(cases, W, in_shift, out_shift):
    """W = 4 and 12 with the payload input 1 byte, the output 2 bytes, and both behind a 64-byte boundary (views into larger
    tensors): the word branch must not be taken, and the sentinels on either side of the S * W output bytes stay."""
    N, L = bl.MID
    c = cases(N).load(bl.mid(12))
    total = c.select(LIVE)
    for permute in (0, 1):
        c.take(LIVE, permute, 0, total + 5, f"W {W}, input + {in_shift}, output + {out_shift}", W=W, in_shift=in_shift, out_shift=out_shift)


# ---------------------------------------------------------------------------------------------- 5. first + S = INT32_MAX
@pytest.mark.parametrize("S", bl.FAR_SIZES)
def test_first_at_int32_max_less_s(cases, S):
    """first = INT32_MAX - S, the largest the header allows: every row is wrapped - valid 0 - and holds the real sample at
    p mod total."""
    N, L = bl.MID
    c = cases(N).load(bl.mid(12))
    for which in (LIVE, BOOT):
        total = c.select(which)
        for permute in (0, 1):
            got = c.take(which, permute, bl.INT32_MAX - S, S, f"far, S {S}, list {which}, permute {permute}")
            assert not got["valid"].any() and (got["slot"] >= 0).all() and total > 0


# ---------------------------------------------------------------------------------------------- 6. scatter at the limit
def test_scatter_at_the_rollout_limit(cases):
    """cells = 257 * 4096: the valid rows of a BOOT epoch (330,294 rows and three wrapped ones, which must be skipped) put their
    values at their slots in a guarded destination; every other cell keeps its sentinel."""
    from active_gym import _native as nat
    N, L = bl.DEEP[1]
    c = cases(N).load(bl.deep(N, L))
    rig = c.rig
    total = c.select(BOOT)
    S = total + 3
    slot, valid = torch.full((S,), I_SENT, dtype=torch.int32, device=DEV), torch.full((S,), B_SENT, dtype=torch.uint8, device=DEV)
    from active_gym.minibatch import MinibatchIo
    io = MinibatchIo()
    io.d_slot, io.d_valid = _ptr(slot), _ptr(valid)
    nat.check(rig.lib.agx_minibatch_take(rig.mb._m, BOOT, 1, L, _ptr(c.d["len"]), _ptr(c.d["ends"]), 0, S, ctypes.byref(io), rig.pipe._stream()), rig.pipe._ctx)
    want_rows = c.mine.take(BOOT, True, 0, S)
    assert np.array_equal(slot.cpu().numpy(), want_rows["slot"]) and np.array_equal(valid.cpu().numpy(), want_rows["valid"])
    src = np.random.default_rng(1).standard_normal(S).astype(np.float32)
    d_src = _t(src)
    dst = Out(L * N, torch.float32, F_SENT)
    nat.check(rig.lib.agx_minibatch_scatter(rig.mb._m, S, _ptr(slot), _ptr(valid), _ptr(d_src), L, dst.ptr, rig.pipe._stream()), rig.pipe._ctx)
    want = np.full(L * N, F_SENT, np.float32)
    want[c.mine.slots[BOOT][bl.permutation(c.mine.key[BOOT], total, np.arange(total))[0]]] = src[:total]
    got = dst.host()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) and int((got != F_SENT).sum()) == total
    assert int(c.mine.slots[BOOT].max()) > 2 ** 20


# ---------------------------------------------------------------------------------------------- 7. the Python surface
def test_minibatcher_take_with_a_payload_of_five_bytes(cases):
    """Minibatcher.take with a u8 [L, N, 5] payload tensor: the wrapper passes W = 5 and the rows hold the payload's bytes."""
    N, L = bl.MID
    c = cases(N).load(bl.mid(5))
    batch = {k: c.d[k] for k in ("len", "ends", "obs_index", "next_index", "payload")}
    assert tuple(batch["payload"].shape) == (L, N, 5)
    total = c.rig.mb.select(batch)
    want_total = c.mine.select(LIVE, c.a["len"], c.a["ends"], L)
    S = want_total + 4
    rows = c.rig.mb.take(batch, 0, S, streams={"adv": c.d["streams"][0]})
    assert int(total.item()) == want_total
    want = c.mine.take(LIVE, True, 0, S, c.a["obs_index"], c.a["next_index"], c.a["payload"], c.a["streams"][:1])
    assert tuple(rows["payload"].shape) == (S, 5)
    for key in ("slot", "env", "obs_index", "next_index", "payload", "valid"):
        assert np.array_equal(rows[key].cpu().numpy(), want[key]), key
    assert np.array_equal(rows["adv"].cpu().numpy().view(np.int32), want["streams"][0].view(np.int32))
