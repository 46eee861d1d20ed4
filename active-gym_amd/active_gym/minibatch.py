"""Minibatcher — ctypes view of include/agx_minibatch.h: the device-side list of a gathered rollout's LIVE or BOOT slots, a
seeded shuffle of it, and one launch per minibatch, for the epochs of a PPO learner.  Nothing here synchronises, calls
``nonzero`` or shows the host a count, so a whole update - gather, boot values, fold, every minibatch of every epoch - can be
captured in one graph::

    roll = Rollout(log)
    mb = roll.minibatcher(seed=0)
    batch = roll.gather(128)
    boot = mb.take(batch, 0, 2 * N, which="boot", permute=False)     # after mb.select(batch, "boot"): the BOOT list, padded
    boot_value = torch.zeros(128, N, device=dev)
    mb.scatter(boot, critic(hist.observe(boot["env"], boot["next_index"])[0]), boot_value)
    ...                                                              # value, then adv, ret = roll.gae(batch, value, boot_value)
    for epoch in range(4):
        mb.select(batch)                                             # a new shuffle of the live slots
        for first in range(0, 128 * N, 4096):
            rows = mb.take(batch, first, 4096, streams={"adv": adv, "ret": ret, "value": value, "logp": logp})
            obs = hist.observe(rows["env"], rows["obs_index"])[0]
            loss = (per_row_loss(obs, rows) * rows["valid"]).sum() / rows["valid"].sum().clamp(min=1)

Every ``take`` has the fixed shape ``[S]``: positions past the list's end wrap to real, finite samples with ``valid = 0``, and
a position whose slot does not exist is ``slot = -1, env = 0``, indices -1, zeros, ``valid = 0``.  The order of an epoch is the
pure integer function of (seed, list, the number of selects before it, total) the header spells out;
``tests/minibatch_model.py`` restates it in Python ints.

The entry points live in libagx.so, in a header and a binding of their own (active_gym/_native.py is unchanged)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat
from .lifetime import Owner
from .rollout import check_rollout_length

_P = C.c_void_p
MB_LIVE, MB_BOOT = 0, 1               # AGX_MB_LIVE, AGX_MB_BOOT
MB_STREAMS = 8                        # AGX_MB_STREAMS
INT32_MAX = 2 ** 31 - 1
RESERVED = ("slot", "env", "obs_index", "next_index", "payload", "valid")


class MinibatchIo(C.Structure):
    """agx_minibatch_io."""
    _fields_ = [
        ("d_obs_index", _P), ("d_next_index", _P), ("d_payload", _P), ("payload_bytes", C.c_int32), ("n_f32", C.c_int32),
        ("src_f32", _P * MB_STREAMS), ("d_slot", _P), ("d_env", _P), ("d_obs_index_out", _P), ("d_next_index_out", _P),
        ("d_payload_out", _P), ("dst_f32", _P * MB_STREAMS), ("d_valid", _P),
    ]


SIGNATURES = {
    "agx_minibatch_create": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "agx_minibatch_destroy": (C.c_int, [_P]),
    "agx_minibatch_select": (C.c_int, [_P, C.c_int, C.c_int32, _P, _P, _P, _P]),
    "agx_minibatch_take": (C.c_int, [_P, C.c_int, C.c_int, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.POINTER(MinibatchIo), _P]),
    "agx_minibatch_scatter": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_list(which) -> int:
    """ValueError, before any GPU work, for a list that is neither "live" nor "boot"; returns AGX_MB_LIVE / AGX_MB_BOOT."""
    if which not in ("live", "boot"):
        raise ValueError(f"which must be 'live' or 'boot', got {which!r}")
    return MB_LIVE if which == "live" else MB_BOOT


def check_minibatch_size(S, first=0):
    """ValueError, before any GPU work, for a take outside the header's range; returns (first, S) as ints."""
    first, S = int(first), int(S)
    if S < 0:
        raise ValueError(f"S must be >= 0, got {S}")
    if first < 0:
        raise ValueError(f"first must be >= 0, got {first}")
    if first + S > INT32_MAX:
        raise ValueError(f"first + S = {first + S} exceeds {INT32_MAX}")
    return first, S


def check_streams(streams, batch=None) -> dict:
    """ValueError, before any GPU work, for more than MB_STREAMS streams or a name a take's dict already holds.  streams: None, a
    dict name -> f32 [L, N] tensor, or names of entries of ``batch``.  Returns the dict."""
    if streams is None:
        return {}
    if not isinstance(streams, dict):
        names = list(streams)
        missing = [k for k in names if batch is None or k not in batch]
        if missing:
            raise ValueError(f"streams {missing} are not entries of the batch")
        streams = {k: batch[k] for k in names}
    if len(streams) > MB_STREAMS:
        raise ValueError(f"at most {MB_STREAMS} streams per take, got {len(streams)}")
    taken = [k for k in streams if k in RESERVED]
    if taken:
        raise ValueError(f"stream names {taken} are outputs of every take")
    return dict(streams)


def check_epoch_size(size) -> int:
    """ValueError, before any GPU work, for a minibatch size of an epoch that is not 1 .. INT32_MAX."""
    size = int(size)
    if not 1 <= size <= INT32_MAX:
        raise ValueError(f"size must be 1 .. {INT32_MAX}, got {size}")
    return size


class Minibatcher(Owner):
    _closed_what = "the minibatcher or its history"

    def __init__(self, rollout, seed: int = 0):
        """rollout: a Rollout (or VTrace); its history supplies N and the device.  seed: the shuffles' seed (u64)."""
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._lib = lib()
        self.rollout = rollout
        self.history = rollout.history
        self.pipe = rollout.pipe
        self.device = rollout.device
        self.num_envs = rollout.num_envs
        self._m = _P()
        nat.check(self._lib.agx_minibatch_create(self.history.handle, self.seed, C.byref(self._m)), self.pipe._ctx)
        # the minibatcher holds the history's raw handle: it goes before the history does
        self._own(self._m, self._lib.agx_minibatch_destroy, (self.history,))
        self._total = torch.zeros((2,), dtype=torch.int32, device=self.device)

    def _check(self, rc):
        nat.check(rc, self.pipe._ctx)

    def _rollout_args(self, batch: dict):
        """(L, the checked pointers of len and ends)."""
        L = check_rollout_length(batch["ends"].shape[0], self.num_envs)
        n, chk = self.num_envs, self.pipe._chk
        return L, chk(batch["len"], (n,), torch.int32, "len"), chk(batch["ends"], (L, n), torch.uint8, "ends")

    def select(self, batch: dict, which: str = "live") -> torch.Tensor:
        """Start an epoch over the LIVE (or BOOT) slots of a gathered ``batch``: a new shuffle.  Returns the list's length, i32
        [1] on the device - the host never waits for it."""
        w = check_list(which)
        self._live()
        L, pl, pe = self._rollout_args(batch)
        total = self._total[w:w + 1]
        self._check(self._lib.agx_minibatch_select(self._m, w, L, pl, pe, _P(total.data_ptr()), self.pipe._stream()))
        return total

    def total(self, which: str = "live") -> torch.Tensor:
        """i32 [1] on the device: the length of the list the last ``select(.., which)`` made (0 before the first)."""
        w = check_list(which)
        return self._total[w:w + 1]

    def take(self, batch: dict, first: int, S: int, which: str = "live", permute: bool = True, streams=None, out: Optional[dict] = None) -> dict:
        """Rows for the positions ``first .. first + S - 1`` of the epoch the last ``select(batch, which)`` started, as a dict:
        ``slot`` i32 [S] (t * N + n, -1 where none), ``env`` i32 [S], ``obs_index`` / ``next_index`` i64 [S], ``payload`` u8 [S, W]
        (W = 0 for a batch without one), ``valid`` u8 [S] and, per name in ``streams`` (a dict name -> f32 [L, N], or names of
        entries of ``batch``), f32 [S].  ``out``: the dict of an earlier take of the same shape to write into, so that a captured
        graph keeps its addresses."""
        w = check_list(which)
        first, S = check_minibatch_size(S, first)
        streams = check_streams(streams, batch)
        self._live()
        L, pl, pe = self._rollout_args(batch)
        n, chk, new = self.num_envs, self.pipe._chk, self.pipe._out
        out = {} if out is None else out
        io = MinibatchIo()
        io.d_obs_index = chk(batch["obs_index"], (L, n), torch.int64, "obs_index")
        io.d_next_index = chk(batch["next_index"], (L, n), torch.int64, "next_index")
        payload = batch.get("payload")
        W = 0 if payload is None else int(payload.shape[-1])
        if W:
            io.d_payload = chk(payload, (L, n, W), torch.uint8, "payload")
        io.payload_bytes, io.n_f32 = W, len(streams)
        for key, shape, dtype, field in (("slot", (S,), torch.int32, "d_slot"), ("env", (S,), torch.int32, "d_env"),
                                         ("obs_index", (S,), torch.int64, "d_obs_index_out"), ("next_index", (S,), torch.int64, "d_next_index_out"),
                                         ("payload", (S, W), torch.uint8, "d_payload_out"), ("valid", (S,), torch.uint8, "d_valid")):
            out[key], ptr = new(out.get(key), shape, dtype, key)
            setattr(io, field, ptr)
        for k, (name, src) in enumerate(streams.items()):
            io.src_f32[k] = chk(src, (L, n), torch.float32, name).value
            out[name], ptr = new(out.get(name), (S,), torch.float32, name)
            io.dst_f32[k] = ptr.value
        self._check(self._lib.agx_minibatch_take(self._m, w, int(bool(permute)), L, pl, pe, first, S, C.byref(io), self.pipe._stream()))
        return out

    def scatter(self, rows: dict, values: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        """``dst.view(-1)[rows["slot"]] = values`` where ``rows["valid"]`` is set and the slot lies in ``dst`` (f32 [L, N]);
        every other row is skipped.  values: f32 [S] or [S, 1].  With the rows of the BOOT list and the critic's values of their
        ``next_index`` this fills a zeroed ``boot_value``."""
        self._live()
        S = int(rows["slot"].shape[0])
        n, chk = self.num_envs, self.pipe._chk
        if not isinstance(dst, torch.Tensor) or dst.dim() != 2:
            raise ValueError("dst must be f32 [L, N]")
        L = check_rollout_length(dst.shape[0], n)
        if isinstance(values, torch.Tensor) and values.dim() == 2 and values.shape[1] == 1:
            values = values.reshape(-1)
        self._check(self._lib.agx_minibatch_scatter(self._m, S, chk(rows["slot"], (S,), torch.int32, "slot"), chk(rows["valid"], (S,), torch.uint8, "valid"),
                                                    chk(values, (S,), torch.float32, "values"), L, chk(dst, (L, n), torch.float32, "dst"),
                                                    self.pipe._stream()))
        return dst
