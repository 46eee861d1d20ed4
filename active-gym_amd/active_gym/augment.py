"""RandomShift — ctypes view of include/agx_augment.h: DrQ's random-shift augmentation folded into the frame history's observe.

A pixel-RL learner pads every replayed observation by ``pad`` pixels with edge replication and crops it back at a random offset,
independently for ``obs`` and ``next_obs``.  In torch that is another read and write of the batch ``FrameHistory.observe`` has
just produced, an index tensor and a host RNG per call; here the observe kernel itself writes the shifted batch, and the shifts
are drawn on the device::

    hist = FrameHistory(pipe, capacity=100_000)
    aug = RandomShift(hist, pad=4, seed=0)
    ...
    obs, loc, valid = aug.observe(env, index)                   # a fresh draw; aug.last_shift is the i32 [B, 2] (dy, dx)
    obs, loc, valid = aug.observe(env, index, shift=my_shifts)  # ... or the caller's shifts, each clamped into 0 .. 2 * pad
    batch = log.batch(sampler, 256, nstep=3, shift=aug)         # obs and next_obs shifted independently, obs_shift / next_obs_shift

Every plane ``U`` of a row becomes ``S[y][x] = U[clamp(y + dy - pad)][clamp(x + dx - pad)]``, one shift for all stacked frames of a
sample: bit for bit the gather of the unshifted output.  ``fov_loc`` and ``valid`` are ``observe``'s.  The draw is the pure
integer function of (seed, call number) the header spells out; ``tests/shift_model.py`` restates it in Python ints.

The entry points live in libagx.so, in a header and a binding of their own (active_gym/_native.py is unchanged)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat
from .history import _WHAT
from .lifetime import Owner

_P = C.c_void_p
PAD_LIMIT = 32                        # AGX_SHIFT_PAD_LIMIT

SIGNATURES = {
    "agx_shift_create": (C.c_int, [_P, C.c_int32, C.POINTER(_P)]),
    "agx_shift_destroy": (C.c_int, [_P]),
    "agx_shift_seed": (C.c_int, [_P, C.c_uint64, _P]),
    "agx_shift_draw": (C.c_int, [_P, C.c_int32, _P, _P]),
    "agx_history_observe_shifted": (C.c_int, [_P, C.c_int, _P, _P, C.c_int32, _P, C.c_int, C.c_int32, _P, _P, _P, _P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_pad(pad) -> int:
    """ValueError, before any GPU work, for a pad outside the header's range."""
    p = int(pad)
    if not 0 <= p <= PAD_LIMIT:
        raise ValueError(f"pad must be 0 .. {PAD_LIMIT}, got {p}")
    return p


def check_no_glimpses(glimpses) -> None:
    """ValueError, before any GPU work, for a shifted read through the glimpse memory."""
    if glimpses is not None:
        raise ValueError("a shift together with glimpses: the glimpse memory is not shifted")


def check_shift_read(shift, glimpses, history) -> None:
    """ValueError, before any GPU work, for a read through ``shift`` (a RandomShift, or None: nothing to check) that is not
    served: together with glimpses, or on another history than the one that is read."""
    if shift is None:
        return
    check_no_glimpses(glimpses)
    if shift.history is not history:
        raise ValueError("the shift is on another history than the one that is read")


class RandomShift(Owner):
    _closed_what = "the shift source or its history"

    def __init__(self, history, pad: int = 4, seed: int = 0):
        """history: a FrameHistory; pad: the replicate padding in pixels (0 .. 32: shifts are 0 .. 2 * pad per axis); seed: the
        sequence's seed (u64)."""
        self.pad = check_pad(pad)
        self._lib = lib()
        self.history = history
        self.pipe = history.pipe
        self.device = history.device
        self._s = _P()
        nat.check(self._lib.agx_shift_create(history.handle, self.pad, C.byref(self._s)), self.pipe._ctx)
        # the source holds the history's raw handle: it goes before the history does
        self._own(self._s, self._lib.agx_shift_destroy, (history,))
        self.last_shift = torch.zeros((0, 2), dtype=torch.int32, device=self.device)     # the shifts of the last observe
        if int(seed):
            self.seed(seed)

    def _check(self, rc):
        nat.check(rc, self.pipe._ctx)

    def seed(self, s: int):
        """Restart the sequence: (seed, calls = 0), on the current stream."""
        self._live()
        self._check(self._lib.agx_shift_seed(self._s, int(s) & 0xFFFFFFFFFFFFFFFF, self.pipe._stream()))

    def draw(self, B: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Draw B shifts on the current stream -> i32 [B, 2] as (dy, dx), each uniform over 0 .. 2 * pad."""
        self._live()
        B = int(B)
        if B < 0:
            raise ValueError(f"B must be >= 0, got {B}")
        out, po = self.pipe._out(out, (B, 2), torch.int32, "out")
        self._check(self._lib.agx_shift_draw(self._s, B, po, self.pipe._stream()))
        return out

    def observe(self, env: torch.Tensor, index: torch.Tensor, action: Optional[torch.Tensor] = None, what: str = "fovea",
                shift: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, loc_out: Optional[torch.Tensor] = None,
                valid_out: Optional[torch.Tensor] = None):
        """``FrameHistory.observe`` with sample b moved by ``shift[b]`` - i32 [B, 2] (dy, dx), clamped into 0 .. 2 * pad on the
        device; None: a fresh ``draw(B)``.  Returns observe's triple (obs, fov_loc, valid) - fov_loc does not reflect the
        shift - and keeps the shifts it used as ``.last_shift``."""
        if what not in _WHAT:
            raise ValueError(f"what must be 'fovea' or 'full', got {what!r}")
        self._live()
        pipe, hist = self.pipe, self.history
        b, pe, pi = pipe._pair(env, index)
        pa, dt = pipe._action(action, b)
        if shift is None:
            shift = self.draw(b)
        ps = pipe._chk(shift, (b, 2), torch.int32, "shift")
        out, po = pipe._out(out, (b,) + hist.obs_row_shape(what), pipe.obs_dtype, "out")
        loc_out, pl = pipe._out(loc_out, (b, 2), torch.int32, "loc_out")
        valid_out, pv = pipe._out(valid_out, (b,), torch.uint8, "valid_out")
        self._check(self._lib.agx_history_observe_shifted(hist.handle, _WHAT[what], pe, pi, b, pa, dt, self.pad, ps, po, pl, pv, pipe._stream()))
        self.last_shift = shift
        return out, loc_out, valid_out
