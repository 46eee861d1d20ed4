"""Chunker — ctypes view of include/agx_chunks.h: the device-side list of a gathered rollout's chunks (runs of C consecutive steps
of one env that hold a live step), a seeded shuffle of it, and one launch per minibatch of S chunks, time-major ``[C, S]``, for
the epochs of a recurrent PPO learner.  Nothing here synchronises, calls ``nonzero`` or shows the host a count::

    roll = Rollout(log)
    ch = roll.chunker(seed=0)
    batch = roll.gather(128)
    ...                                                              # value, then adv, ret = roll.gae(batch, value, boot_value)
    for epoch in range(4):
        ch.select(batch, 16)                                         # a new shuffle of the chunks
        for first in range(0, N * 8, 256):                           # N * ceil(128 / 16) chunks at the most
            rows = ch.take(batch, first, 256, 16, streams={"adv": adv, "ret": ret, "logp": logp})
            obs = hist.observe(rows["env"].flatten(), rows["obs_index"].flatten())[0]      # index -1: left untouched
            h = stored_state(rows["env"][0], rows["state_index"])    # what the actor kept for (env, state_index)
            for l in range(16):
                h = where(rows["start"][l] & 2, h0, h)               # an episode ended behind the step before: restart
                out, h = rnn(obs[l], h)
            loss = (per_step_loss * rows["mask"]).sum() / rows["mask"].sum().clamp(min=1)

Every ``take`` has the fixed shapes ``[C, S]`` and ``[S]``: positions past the list's end wrap to real, finite chunks with
``valid = 0`` and ``mask = 0``, and a position whose chunk does not exist is the null row (``slot = -1, env = 0``, indices -1,
zeros).  The order of an epoch is the pure integer function of (seed, the number of selects before it, total) the header spells
out; ``tests/chunks_model.py`` restates it in Python ints.

The entry points live in libagx.so, in a header and a binding of their own (active_gym/_native.py is unchanged)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat
from .lifetime import Owner
from .minibatch import INT32_MAX, check_minibatch_size, check_streams as _check_streams
from .rollout import check_rollout_length

_P = C.c_void_p
CHUNK_LIMIT = 256                     # AGX_CHUNK_LIMIT
CHUNK_STREAMS = 8                     # AGX_CHUNK_STREAMS
START_CHUNK, START_EPISODE = 1, 2     # AGX_CHUNK_START_*
RESERVED = ("slot", "env", "obs_index", "next_index", "payload", "ends", "start", "mask", "chunk", "first", "steps", "state_index", "valid")


class ChunkIo(C.Structure):
    """agx_chunks_io."""
    _fields_ = [
        ("d_obs_index", _P), ("d_next_index", _P), ("d_payload", _P), ("payload_bytes", C.c_int32), ("n_f32", C.c_int32),
        ("src_f32", _P * CHUNK_STREAMS), ("d_slot", _P), ("d_env", _P), ("d_obs_index_out", _P), ("d_next_index_out", _P),
        ("d_payload_out", _P), ("dst_f32", _P * CHUNK_STREAMS), ("d_ends_out", _P), ("d_start", _P), ("d_mask", _P),
        ("d_chunk", _P), ("d_first", _P), ("d_steps", _P), ("d_state_index", _P), ("d_valid", _P),
    ]


SIGNATURES = {
    "agx_chunks_create": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "agx_chunks_destroy": (C.c_int, [_P]),
    "agx_chunks_select": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P]),
    "agx_chunks_take": (C.c_int, [_P, C.c_int, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.POINTER(ChunkIo), _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_chunk_length(C_, L) -> int:
    """ValueError, before any GPU work, for a chunk length outside 1 .. min(L, CHUNK_LIMIT); returns C as an int."""
    c, most = int(C_), min(int(L), CHUNK_LIMIT)
    if not 1 <= c <= most:
        raise ValueError(f"C must be 1 .. min(L, {CHUNK_LIMIT}) = {most}, got {c}")
    return c


def check_streams(streams, batch=None) -> dict:
    """minibatch.check_streams, and ValueError for a name a chunk take's dict already holds."""
    streams = _check_streams(streams, batch)
    taken = [k for k in streams if k in RESERVED]
    if taken:
        raise ValueError(f"stream names {taken} are outputs of every take")
    return streams


def check_rows(C_, S):
    """ValueError, before any GPU work, for C * S above INT32_MAX."""
    if int(C_) * int(S) > INT32_MAX:
        raise ValueError(f"C * S = {int(C_) * int(S)} exceeds {INT32_MAX}")


class Chunker(Owner):
    _closed_what = "the chunker or its history"

    def __init__(self, rollout, seed: int = 0):
        """rollout: a Rollout (or VTrace); its history supplies N and the device.  seed: the shuffles' seed (u64)."""
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._lib = lib()
        self.rollout = rollout
        self.history = rollout.history
        self.pipe = rollout.pipe
        self.device = rollout.device
        self.num_envs = rollout.num_envs
        self._c = _P()
        nat.check(self._lib.agx_chunks_create(self.history.handle, self.seed, C.byref(self._c)), self.pipe._ctx)
        # the chunker holds the history's raw handle: it goes before the history does
        self._own(self._c, self._lib.agx_chunks_destroy, (self.history,))
        self._total = torch.zeros((1,), dtype=torch.int32, device=self.device)

    def _check(self, rc):
        nat.check(rc, self.pipe._ctx)

    def _rollout_args(self, batch: dict, C_):
        """(L, C, the checked pointers of len and ends)."""
        L = check_rollout_length(batch["ends"].shape[0], self.num_envs)
        c = check_chunk_length(C_, L)
        n, chk = self.num_envs, self.pipe._chk
        return L, c, chk(batch["len"], (n,), torch.int32, "len"), chk(batch["ends"], (L, n), torch.uint8, "ends")

    def select(self, batch: dict, C_: int) -> torch.Tensor:
        """Start an epoch over the chunks of length ``C_`` of a gathered ``batch``: a new shuffle.  Returns the list's length,
        i32 [1] on the device - the host never waits for it."""
        self._live()
        L, c, pl, _ = self._rollout_args(batch, C_)
        self._check(self._lib.agx_chunks_select(self._c, L, c, pl, _P(self._total.data_ptr()), self.pipe._stream()))
        return self._total

    def total(self) -> torch.Tensor:
        """i32 [1] on the device: the length of the list the last ``select`` made (0 before the first)."""
        return self._total

    def take(self, batch: dict, first: int, S: int, C_: int, permute: bool = True, streams=None, out: Optional[dict] = None) -> dict:
        """Chunks for the positions ``first .. first + S - 1`` of the epoch the last ``select(batch, C_)`` started, as a dict.
        Per step, time-major ``[C, S]``: ``slot`` i32 (t * N + n, -1 where not live), ``env`` i32 (at every step), ``obs_index`` /
        ``next_index`` i64, ``payload`` u8 [C, S, W] (W = 0 for a batch without one), ``ends``, ``start`` (1: the chunk's first
        live step, 2: behind an episode's end) and ``mask`` u8 and, per name in ``streams`` (a dict name -> f32 [L, N], or names
        of entries of ``batch``), f32.  Per chunk, ``[S]``: ``chunk``, ``first``, ``steps`` i32, ``state_index`` i64, ``valid`` u8.
        ``out``: the dict of an earlier take of the same shape to write into, so that a captured graph keeps its addresses."""
        first, S = check_minibatch_size(S, first)
        streams = check_streams(streams, batch)
        self._live()
        L, c, pl, pe = self._rollout_args(batch, C_)
        check_rows(c, S)
        n, chk, new = self.num_envs, self.pipe._chk, self.pipe._out
        out = {} if out is None else out
        io = ChunkIo()
        io.d_obs_index = chk(batch["obs_index"], (L, n), torch.int64, "obs_index")
        io.d_next_index = chk(batch["next_index"], (L, n), torch.int64, "next_index")
        payload = batch.get("payload")
        W = 0 if payload is None else int(payload.shape[-1])
        if W:
            io.d_payload = chk(payload, (L, n, W), torch.uint8, "payload")
        io.payload_bytes, io.n_f32 = W, len(streams)
        for key, shape, dtype, field in (("slot", (c, S), torch.int32, "d_slot"), ("env", (c, S), torch.int32, "d_env"),
                                         ("obs_index", (c, S), torch.int64, "d_obs_index_out"), ("next_index", (c, S), torch.int64, "d_next_index_out"),
                                         ("payload", (c, S, W), torch.uint8, "d_payload_out"), ("ends", (c, S), torch.uint8, "d_ends_out"),
                                         ("start", (c, S), torch.uint8, "d_start"), ("mask", (c, S), torch.uint8, "d_mask"),
                                         ("chunk", (S,), torch.int32, "d_chunk"), ("first", (S,), torch.int32, "d_first"),
                                         ("steps", (S,), torch.int32, "d_steps"), ("state_index", (S,), torch.int64, "d_state_index"),
                                         ("valid", (S,), torch.uint8, "d_valid")):
            out[key], ptr = new(out.get(key), shape, dtype, key)
            setattr(io, field, ptr)
        for k, (name, src) in enumerate(streams.items()):
            io.src_f32[k] = chk(src, (L, n), torch.float32, name).value
            out[name], ptr = new(out.get(name), (c, S), torch.float32, name)
            io.dst_f32[k] = ptr.value
        self._check(self._lib.agx_chunks_take(self._c, int(bool(permute)), L, c, pl, pe, first, S, C.byref(io), self.pipe._stream()))
        return out
