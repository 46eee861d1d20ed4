"""GlimpseMemory — ctypes view of include/agx_glimpse.h: the elementwise maximum of an env's last P observations (a
persistence-of-vision memory), written by one kernel from the frame history's u8 frames and recorded fov_loc.

    hist = FrameHistory(pipe, capacity=100_000)
    mem = hist.memory(3)                            # the history's one memory of 3 glimpses
    ...
    obs, loc, taken = mem.observe(env, index)       # max over the last up-to-3 observations of the sample's episode

Glimpse ``i`` (0 = newest) of a sample ``(n, k)`` is the observation of ``(n, k - i)`` as ``hist.observe`` re-creates it; it
is taken when no CMD_CLEAR lies between the two appends (same episode) and ``(n, k - i)`` is still a valid sample.  The
result equals, bit for bit, ``torch.maximum`` over the observations the steps returned for the taken glimpses.  Fixed
pipelines in mask-out or resize_to_full mode only.

The entry point lives in libagx.so, in a header and a binding of its own (active_gym/_native.py is unchanged)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat

_P = C.c_void_p
GLIMPSE_LIMIT = 8                     # AGX_GLIMPSE_LIMIT

SIGNATURES = {
    "agx_history_observe_memory": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_glimpse_source(kind: str, out_mode: int) -> None:
    """ValueError, before any GPU work, for what the glimpse memory does not serve."""
    if kind != "fixed":
        raise ValueError(f"a glimpse memory needs kind 'fixed', got {kind!r} (only a fixed fovea leaves glimpses to combine)")
    if out_mode == nat.OUT_RAW:
        raise ValueError("a glimpse memory needs mask_out or resize_to_full mode (a maximum over raw crops at different positions means nothing)")


class GlimpseMemory:
    def __init__(self, history, glimpses: int = 3):
        """history: a FrameHistory of a fixed pipeline in mask-out or resize_to_full mode; glimpses: P, 1 .. 8."""
        self._lib = lib()
        self.history = history
        self.pipe = history.pipe
        self.device = history.device
        self.glimpses = int(glimpses)
        if not 1 <= self.glimpses <= GLIMPSE_LIMIT:
            raise ValueError(f"glimpses must be 1 .. {GLIMPSE_LIMIT}, got {glimpses}")
        check_glimpse_source(self.pipe.kind, self.pipe.out_mode)

    def observe(self, env: torch.Tensor, index: torch.Tensor, out: Optional[torch.Tensor] = None, loc_out: Optional[torch.Tensor] = None,
                taken_out: Optional[torch.Tensor] = None):
        """The memory of the samples (env[b], index[b]) - i32 [B], i64 [B]; any order, repeats allowed.
        Returns (obs [B, ...], fov_loc i32 [B, P, 2], taken u8 [B]).  taken[b] glimpses were combined (0: the sample itself is
        invalid - never issued, or evicted - and its rows are left as they were in `out` / `loc_out`, uninitialised when this
        call allocated them); fov_loc[b, i] is the position of glimpse i for i < taken[b] and left as it was beyond."""
        return observe_memory(self.history, self.glimpses, env, index, out, loc_out, taken_out)


def observe_memory(history, glimpses: int, env, index, out=None, loc_out=None, taken_out=None):
    """agx_history_observe_memory on a FrameHistory (no Python-side refusals: the library's own codes come back as AgxError)."""
    pipe = history.pipe
    b, pe, pi = pipe._pair(env, index)
    p = int(glimpses)
    out, po = pipe._out(out, (b,) + history.obs_row_shape(), pipe.obs_dtype, "out")
    loc_out, pl = pipe._out(loc_out, (b, max(p, 0), 2), torch.int32, "loc_out")
    taken_out, pt = pipe._out(taken_out, (b,), torch.uint8, "taken_out")
    nat.check(lib().agx_history_observe_memory(history.handle, p, pe, pi, b, po, pl, pt, pipe._stream()), pipe._ctx)
    return out, loc_out, taken_out
