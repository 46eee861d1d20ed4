"""ReplaySampler — ctypes view of include/agx_replay.h: a device-side sampler of (env, index) pairs on the frame history.

A replay buffer on a FrameHistory stores (env, index) instead of observations.  Which pairs are still retained, which belong to
one episode and which have a full glimpse memory depends on state only the device holds; the sampler draws pairs that satisfy
all of it, on the device, without the host seeing a count::

    hist = FrameHistory(pipe, capacity=100_000)
    sampler = ReplaySampler(hist, back=2, forward=1, seed=0)
    ...
    env, index, ok = sampler.sample(256)                    # accepted pairs; (-1, -1, ok = 0) where every attempt failed
    obs, loc, valid = hist.observe(env, index)               # valid == ok
    batch = sampler.transitions(256, glimpses=3)             # obs / next_obs through the glimpse memory, all of them full
    action = my_actions[batch["index"] % hist.capacity, batch["env"].long()]     # the caller's own [T, N] arrays

``(n, k)`` is accepted iff it is valid, the sample ``back`` appends earlier in its episode (or the episode's first) is valid,
and ``k + forward`` was appended in the same episode.  The draw is the pure integer function of (seed, call number) the header
spells out; ``tests/replay_model.py`` restates it in Python ints.

The entry points live in libagx.so, in a header and a binding of their own (active_gym/_native.py is unchanged)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat
from .lifetime import Owner

_P = C.c_void_p
SPAN_LIMIT = 64                       # AGX_REPLAY_SPAN_LIMIT
ATTEMPT_LIMIT = 64                    # AGX_REPLAY_ATTEMPT_LIMIT

SIGNATURES = {
    "agx_replay_create": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "agx_replay_destroy": (C.c_int, [_P]),
    "agx_replay_seed": (C.c_int, [_P, C.c_uint64, _P]),
    "agx_replay_sample": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P]),
    "agx_replay_inspect": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_replay_args(back: int, forward: int, attempts: int):
    """ValueError, before any GPU work, for arguments outside the header's ranges.  Returns them as ints (attempts 0 -> 16)."""
    back, forward, attempts = int(back), int(forward), int(attempts)
    if not 0 <= back <= SPAN_LIMIT:
        raise ValueError(f"back must be 0 .. {SPAN_LIMIT}, got {back}")
    if not 0 <= forward <= SPAN_LIMIT:
        raise ValueError(f"forward must be 0 .. {SPAN_LIMIT}, got {forward}")
    if not 0 <= attempts <= ATTEMPT_LIMIT:
        raise ValueError(f"attempts must be 1 .. {ATTEMPT_LIMIT} (0: 16), got {attempts}")
    return back, forward, attempts or 16


def check_transitions(back: int, forward: int, glimpses) -> None:
    """ValueError, before any GPU work, for a transitions() request the sampler's arguments do not cover."""
    if forward < 1:
        raise ValueError(f"transitions need forward >= 1 (the next observation is index + forward), got forward = {forward}")
    if glimpses is not None and back < int(glimpses) - 1:
        raise ValueError(f"glimpses = {glimpses} needs a sampler with back >= {int(glimpses) - 1} (so that every memory is full), got back = {back}")


class ReplaySampler(Owner):
    _closed_what = "the sampler or its history"

    def __init__(self, history, back: int = 0, forward: int = 1, attempts: int = 16, seed: int = 0):
        """history: a FrameHistory; back: earlier appends of the episode that must be valid too (a glimpse memory of back + 1
        glimpses is then full); forward: later appends of the same episode that must exist (1: transitions); attempts: draws
        per sample before it is given up; seed: the sequence's seed (u64)."""
        self.back, self.forward, self.attempts = check_replay_args(back, forward, attempts)
        self._lib = lib()
        self.history = history
        self.pipe = history.pipe
        self.device = history.device
        self._r = _P()
        nat.check(self._lib.agx_replay_create(history.handle, self.back, self.forward, self.attempts, C.byref(self._r)), self.pipe._ctx)
        # the sampler holds the history's raw handle: it goes before the history does
        self._own(self._r, self._lib.agx_replay_destroy, (history,))
        self._total = torch.zeros((1,), dtype=torch.int64, device=self.device)
        if int(seed):
            self.seed(seed)

    def _check(self, rc):
        nat.check(rc, self.pipe._ctx)

    def seed(self, s: int):
        """Restart the sequence: (seed, calls = 0), on the current stream."""
        self._live()
        self._check(self._lib.agx_replay_seed(self._r, int(s) & 0xFFFFFFFFFFFFFFFF, self.pipe._stream()))

    def sample(self, B: int, env_out: Optional[torch.Tensor] = None, index_out: Optional[torch.Tensor] = None,
               ok_out: Optional[torch.Tensor] = None):
        """Draw B samples on the current stream -> (env i32 [B], index i64 [B], ok u8 [B]).  A sample whose every attempt was
        rejected (or an empty history) is (-1, -1, 0): history.observe leaves its rows untouched."""
        self._live()
        B = int(B)
        if B < 0:
            raise ValueError(f"B must be >= 0, got {B}")
        new = self.pipe._out
        env_out, pe = new(env_out, (B,), torch.int32, "env_out")
        index_out, pi = new(index_out, (B,), torch.int64, "index_out")
        ok_out, po = new(ok_out, (B,), torch.uint8, "ok_out")
        self._check(self._lib.agx_replay_sample(self._r, B, pe, pi, po, _P(self._total.data_ptr()), self.pipe._stream()))
        return env_out, index_out, ok_out

    def total(self) -> torch.Tensor:
        """i64 [1] on the device: the number of candidates the last sample() drew from (0 before the first)."""
        return self._total

    def inspect(self, env: torch.Tensor, index: torch.Tensor):
        """(age i32 [B], ahead i32 [B]) of the samples (env[b], index[b]): the age of a valid sample and the number of later
        appends of its episode already in the history (what an n-step target needs); -1, -1 for an invalid sample."""
        return inspect(self.history, env, index)

    def transitions(self, B: int, glimpses: Optional[int] = None, shift=None):
        """B transitions (index, index + forward) of one episode each, as a dict: env, index, next_index, ok, obs, next_obs and,
        on a fixed pipeline, fov_loc, next_fov_loc.  glimpses = None reads through history.observe; glimpses = P through
        history.memory(P) (fov_loc is then [B, P, 2]) and needs back >= P - 1.  shift: an augment.RandomShift on this history -
        obs and next_obs are read through it, two independent draws, and the dict gains obs_shift and next_obs_shift (not
        together with glimpses).  Rows with ok = 0 are left as allocated."""
        check_transitions(self.back, self.forward, glimpses)
        from .augment import check_shift_read
        check_shift_read(shift, glimpses, self.history)
        env, index, ok = self.sample(B)
        next_index = torch.where(index >= 0, index + self.forward, index)
        if shift is not None:
            read = shift.observe
        else:
            read = self.history.observe if glimpses is None else self.history.memory(glimpses).observe
        out = {"env": env, "index": index, "next_index": next_index, "ok": ok}
        out.update(self.history.transition_obs(read, env, index, next_index, shift))
        return out


def inspect(history, env: torch.Tensor, index: torch.Tensor):
    """agx_replay_inspect on a FrameHistory: needs no sampler."""
    pipe = history.pipe
    b, pe, pi = pipe._pair(env, index)
    age = torch.empty((b,), dtype=torch.int32, device=history.device)
    ahead = torch.empty((b,), dtype=torch.int32, device=history.device)
    nat.check(lib().agx_replay_inspect(history.handle, pe, pi, b, _P(age.data_ptr()), _P(ahead.data_ptr()), pipe._stream()), pipe._ctx)
    return age, ahead
